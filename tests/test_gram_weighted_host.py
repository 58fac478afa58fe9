"""The host side of the weighted Gram statistics and of the proximal Newton driver (host_route.host_gram(weights=), gram.GramStats.sum_w,
newton.py), without a GPU:

  1. host_gram(weights=) against exact rational arithmetic on a small case, under the bound of section 8.13:
         |got - exact| <= (N + 10) 2^-53 sum_n |w_n a_ni a_nj|
     (N roundings of the running sum, one of each product, one of w a, and slack for the second-order terms);
  2. w = 1 gives the unweighted host_gram bit for bit on integer rows; 0/1 weights give the statistics of the rows kept; G is symmetric
     to the bit with weights of both signs;
  3. GramStats.sum_w, the weighted objective GramLasso evaluates, the refusal of standardized();
  4. logistic_newton(HostRows(A, y), mu) at the three shapes of the lasso-path tests reaches its gap and agrees in objective with a
     plain proximal-gradient solve run to the same gap: both objectives lie within their own certified gap above the minimum, so they
     differ by no more than the larger of the two gaps;
  5. logistic_path warm-starts; the stalled exit on float32 data.
"""
from fractions import Fraction

import numpy as np
import pytest

U53 = 2.0 ** -53
SHAPES = [(6, 3, 2), (200, 50, 5), (300, 130, 7)]
MU_FRACTIONS = (0.5, 0.1)


def logistic_case(N, d, seed, dtype=np.float64):
    """Gaussian rows with labels drawn from a logistic model of a (d / 5)-sparse vector -> (A, y, mu_max): mu_max = ||A'y||_inf / (2 N)
    is the smallest l1 weight at which x = 0 minimises the objective, computed in double from the rows as stored."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, d))
    x_true = np.zeros(d)
    k = max(1, d // 5)
    x_true[rng.choice(d, k, replace=False)] = 2.0 * rng.standard_normal(k)
    y = np.where(rng.random(N) < 1.0 / (1.0 + np.exp(-(A @ x_true))), 1.0, -1.0)
    A, y = A.astype(dtype), y.astype(dtype)
    return A, y, float(np.abs(A.astype(np.float64).T @ y.astype(np.float64)).max()) / (2 * N)


def objective(A, y, x, mu):
    """(1/N) sum log(1 + exp(-t)) + mu ||x||_1 in double, dots included"""
    t = y.astype(np.float64) * (A.astype(np.float64) @ np.asarray(x, np.float64))
    return float(np.mean(np.maximum(-t, 0.0) + np.log1p(np.exp(-np.abs(t))))) + mu * float(np.abs(np.asarray(x, np.float64)).sum())


def weighted_exact(A, b, w):
    """The augmented weighted Gram matrix of [a, b, 1] in Fractions -> ((d + 2) x (d + 2) exact, float64 sums of absolute products)"""
    aug = np.concatenate([A.astype(np.float64), b.astype(np.float64)[:, None], np.ones((A.shape[0], 1))], axis=1)
    cols = [[Fraction(v) for v in aug[:, i].tolist()] for i in range(aug.shape[1])]
    fw = [Fraction(float(v)) for v in w]
    m = aug.shape[1]
    E = [[sum(x * y * z for x, y, z in zip(fw, cols[i], cols[j])) for j in range(m)] for i in range(m)]
    S = np.abs(aug).T @ (np.abs(np.asarray(w, np.float64))[:, None] * np.abs(aug))
    return E, S


def split(E):
    """the augmented matrix of [a, b, 1] -> (G, u, colsum, bsum = [sum w b, sum w b^2, sum w])"""
    E = np.asarray(E, dtype=object)
    d = E.shape[0] - 2
    return E[:d, :d], E[:d, d], E[:d, d + 1], np.array([E[d, d + 1], E[d, d], E[d + 1, d + 1]], dtype=object)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_host_gram_weighted_against_fractions(ciao, dtype):
    from ciaoalgorithms_jl_amd.host_route import host_gram
    rng = np.random.default_rng(5)
    N, d = 40, 5
    A = rng.standard_normal((N, d))
    A[:, 1] += 1e6
    A, b = A.astype(dtype), rng.standard_normal(N).astype(dtype)
    w = rng.standard_normal(N)                     # both signs
    got = host_gram(A, b, w)
    assert len(got[3]) == 3 and all(g.dtype == np.float64 for g in got)
    E, S = weighted_exact(A, b, w)
    for g, e, s, what in zip(got, split(E), split(S), ("G", "u", "colsum", "bsum")):
        g, e, s = np.asarray(g), np.asarray(e, dtype=object), np.asarray(s, dtype=np.float64)
        for idx in np.ndindex(g.shape):
            assert abs(Fraction(float(g[idx])) - e[idx]) <= Fraction((N + 10) * U53) * Fraction(float(s[idx])), (what, idx)
    assert np.array_equal(got[0], got[0].T)


def test_unit_and_indicator_weights_on_integer_rows(ciao):
    from ciaoalgorithms_jl_amd.host_route import host_gram
    i = np.arange(300, dtype=np.int64)
    A = ((7 * i[:, None] + 13 * np.arange(17)[None, :]) % 129 - 64).astype(np.float64)
    b = ((11 * i) % 129 - 64).astype(np.float64)
    plain = host_gram(A, b)
    ones = host_gram(A, b, np.ones(300))
    same = lambda weighted, unweighted: all(np.array_equal(np.ascontiguousarray(p.ravel()[:s.size]).view(np.int64), s.ravel().view(np.int64))
                                            for p, s in zip(weighted, unweighted))     # (bsum: the first two of three)
    assert same(ones, plain) and ones[3][2] == 300.0
    # folds: the five 0/1-weighted results add up exactly to the unweighted one, and each is the statistics of the rows kept
    total = None
    for f in range(5):
        keep = i % 5 == f
        part = host_gram(A, b, keep.astype(np.float64))
        sub = host_gram(A[keep], b[keep])
        assert same(part, sub) and part[3][2] == keep.sum()
        total = part if total is None else [t + p for t, p in zip(total, part)]
    assert same(total, plain) and total[3][2] == 300.0
    # integer weights stay exact
    w = (5 * i) % 9
    got = host_gram(A, b, w)
    Ai, bi = A.astype(np.int64), b.astype(np.int64)
    assert np.array_equal(got[0], (Ai.T @ (w[:, None] * Ai)).astype(np.float64)) and np.array_equal(got[1], (Ai.T @ (w * bi)).astype(np.float64))
    assert np.array_equal(got[2], (Ai.T @ w).astype(np.float64)) and got[3].tolist() == [float((w * bi).sum()), float((w * bi * bi).sum()), float(w.sum())]
    for bad in (np.ones(299), np.ones((300, 1)), np.ones(300) * 1j):
        with pytest.raises(ValueError):
            host_gram(A, b, bad)


def test_gram_stats_sum_w_and_the_weighted_objective(ciao):
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd import gram as GR
    rng = np.random.default_rng(9)
    N, d, lam = 120, 7, 3.0
    A, b, w = rng.standard_normal((N, d)), rng.standard_normal(N), rng.random(N)
    plain, st = GR.host_gram_stats(A, b, lam), GR.host_gram_stats(A, b, lam, weights=w)
    assert plain.sum_w is None and GR.GramStats._fields[-1] == "sum_w" and GR.GramStats._field_defaults["sum_w"] is None
    assert st.N == N and abs(st.sum_w - w.sum()) <= 4 * N * U53 * w.sum()
    assert abs(st.sum_b - (w * b).sum()) <= 4 * N * U53 * np.abs(w * b).sum() and abs(st.sum_bb - (w * b * b).sum()) <= 4 * N * U53 * (w * b * b).sum()
    x = rng.standard_normal(d)
    q = GR.GramLasso(st)
    want = lam / (2 * N) * float(w @ (A @ x - b) ** 2)
    assert abs(q.value(x) - want) <= 8 * q.value_floor(x) + 1e-13 * want
    assert np.allclose(q.gradient(x).numpy(), lam / N * (A.T @ (w * (A @ x - b))), rtol=1e-12, atol=1e-13)
    # lasso_path and mu_max take weighted statistics as they are: the weighted lasso's optimality conditions at the returned point
    mu = 0.3 * GR.mu_max(st)
    path = GR.lasso_path(st, [mu], gap=1e-10)
    assert path.converged[0]
    g = q.gradient(path.x[0]).numpy()
    xs = path.x[0].numpy()
    assert (np.abs(g) <= mu * (1 + 1e-4)).all() and np.allclose(g[xs != 0], -mu * np.sign(xs[xs != 0]), rtol=1e-3)
    with pytest.raises(L.CiaoError) as e:
        st.standardized()
    assert e.value.status == L.ERR_ARG and "weight" in str(e.value)
    assert isinstance(st.to("cpu").G, torch.Tensor) and st.to("cpu").sum_w == st.sum_w


def prox_gradient(A, y, mu, gap, maxit=400000):
    """Plain (accelerated) proximal gradient on the same objective in numpy double, stopped by the same certified gap -> (x, certificate)"""
    from ciaoalgorithms_jl_amd.newton import HostRows
    rows = HostRows(A, y)
    N, d = A.shape
    step = 4.0 * N / float(np.linalg.eigvalsh(A.T @ A)[-1])
    x = z = np.zeros(d)
    t = 1.0
    for it in range(maxit):
        tz = y * (A @ z)
        e = np.exp(-np.abs(tz))
        p = np.where(tz >= 0, e / (1 + e), 1 / (1 + e))
        v = z - step * (-(A.T @ (y * p)) / N)
        xn = np.sign(v) * np.maximum(np.abs(v) - step * mu, 0.0)
        tn = 0.5 * (1 + np.sqrt(1 + 4 * t * t))
        z = xn + (t - 1) / tn * (xn - x)
        x, t = xn, tn
        if it % 20 == 19:
            c = rows.certificate(x, mu, step)
            if c.gap <= gap * max(1.0, c.objective):
                return x, c
    raise AssertionError("the proximal-gradient reference did not reach its gap")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_newton_on_host_rows_reaches_the_gap(ciao, shape):
    from ciaoalgorithms_jl_amd.newton import HostRows, logistic_mu_max, logistic_newton
    N, d, seed = shape
    A, y, mu_max = logistic_case(N, d, seed)
    rows = HostRows(A, y)
    assert abs(logistic_mu_max(rows) - mu_max) <= 1e-12 * mu_max
    for frac in MU_FRACTIONS:
        mu = frac * mu_max
        r = logistic_newton(rows, mu, gap=1e-9)
        c = r.certificate
        print(f"N={N} d={d} mu={frac} mu_max: outer {r.outer} passes {tuple(r.passes)} gap {c.gap:.3e} objective {c.objective:.12f} {r.reason}")
        assert r.converged and r.reason == "gap" and c.gap <= 1e-9 * max(1.0, c.objective)
        assert r.outer <= 16 and r.passes.gram == r.outer and r.passes.first_order >= r.outer + 2
        assert isinstance(r.x, np.ndarray) and r.x.dtype == np.float64 and r.x.shape == (d,)
        assert abs(c.objective - objective(A, y, r.x, mu)) <= 1e-12 * c.objective
        xr, cr = prox_gradient(A, y, mu, 1e-9)
        assert cr.gap >= -1e-13 and c.gap >= -1e-13
        assert abs(c.objective - cr.objective) <= max(c.gap, cr.gap) + 1e-13 * c.objective, (c.objective, cr.objective)
    # above mu_max the zero vector is the answer, certified without a Gram pass
    r0 = logistic_newton(rows, 1.01 * mu_max)
    assert r0.converged and r0.outer == 0 and r0.passes.gram == 0 and not r0.x.any()


def test_path_warm_starts_and_refusals(ciao):
    from ciaoalgorithms_jl_amd.newton import HostRows, logistic_newton, logistic_path
    A, y, mu_max = logistic_case(200, 50, 5)
    rows = HostRows(A, y)
    mus = [0.5 * mu_max, 0.25 * mu_max, 0.125 * mu_max]
    path = logistic_path(rows, mus, gap=1e-9)
    cold = [logistic_newton(rows, m, gap=1e-9) for m in mus]
    assert [r.converged for r in path] == [True] * 3
    assert path[0].outer == cold[0].outer and all(p.outer <= c.outer for p, c in zip(path[1:], cold[1:]))
    for p, c in zip(path, cold):
        assert abs(p.certificate.objective - c.certificate.objective) <= max(p.certificate.gap, c.certificate.gap) + 1e-13
    # a solve started at its own answer stops at once
    again = logistic_newton(rows, mus[-1], x0=path[-1].x, gap=1e-9)
    assert again.converged and again.outer == 0
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            logistic_newton(rows, bad)
    with pytest.raises(ValueError):
        HostRows(A, y[:-1])


def test_the_stalled_exit_on_float32_rows(ciao):
    """Float32 rows: the dots and the gradient carry float32 noise, so a gap far below that noise cannot be certified.  The driver must
    come back -- line search without a decrease -- and not spend its max_outer iterations."""
    from ciaoalgorithms_jl_amd.newton import HostRows, logistic_newton
    A, y, mu_max = logistic_case(200, 50, 5, np.float32)
    rows = HostRows(A, y)
    mu = 0.1 * mu_max
    r = logistic_newton(rows, mu, gap=1e-14, max_outer=60)
    print(f"float32 rows, gap 1e-14 asked: outer {r.outer} reason {r.reason} gap reached {r.certificate.gap:.3e}")
    assert not r.converged and r.reason == "stalled" and r.outer < 60
    assert r.x.dtype == np.float32
    # what it reached is as good as the float64 solve of the same (float32-valued) rows, rounded to float32, up to the noise of float32 dots
    r64 = logistic_newton(HostRows(A.astype(np.float64), y.astype(np.float64)), mu, gap=1e-9)
    x64 = r64.x.astype(np.float32)
    allow = 8 * (50 + 2) * float(np.finfo(np.float32).eps) * float(np.mean(np.abs(A.astype(np.float64)) @ np.abs(x64.astype(np.float64))))
    o32, o64 = rows.loss(rows.dots(r.x))[0] + mu * float(np.abs(r.x.astype(np.float64)).sum()), rows.loss(rows.dots(x64))[0] + mu * float(np.abs(x64.astype(np.float64)).sum())
    print(f"objective float32 solve {o32:.10f}, float64 solve rounded {o64:.10f}, allowance {allow:.3e}, used {(o32 - o64) / allow:.3f}")
    assert o32 <= o64 + allow

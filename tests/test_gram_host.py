"""The host side of the Gram statistics (gram.py, host_route.host_gram), without a GPU: the numpy twin against
exact rational arithmetic, the GramStats algebra (standardized, mu_max, value_floor) on the twin's numbers, lasso_path reaching the known
minimiser under the inequalities the device test uses, the refusal of logistic statistics, and the new prototype.

Bounds.  An entry of G is a sum of N products, each rounded once, added in some order: |G_ij - exact| <= (N + 8) 2^-53 sum_n |a_ni a_nj|
(N roundings of the running sum and one of each product, to first order; the 8 is slack for the second-order terms at these N), u and
colsum alike."""
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U53 = 2.0 ** -53
PATH_SHAPES = [(6, 3, 2), (200, 50, 5), (300, 130, 7)]


def exact_gram(A, b):
    """(G, u, colsum, bsum) as Fractions, and the sums of absolute products that the bounds scale with"""
    N, d = A.shape
    fa = [[Fraction(float(v)) for v in row] for row in A]
    fb = [Fraction(float(v)) for v in b]
    G = [[sum(fa[n][i] * fa[n][j] for n in range(N)) for j in range(d)] for i in range(d)]
    u = [sum(fa[n][j] * fb[n] for n in range(N)) for j in range(d)]
    cs = [sum(fa[n][j] for n in range(N)) for j in range(d)]
    bs = [sum(fb), sum(v * v for v in fb)]
    A64, b64 = np.abs(A.astype(np.float64)), np.abs(b.astype(np.float64))
    return G, u, cs, bs, (A64.T @ A64, A64.T @ b64, A64.sum(axis=0), np.array([b64.sum(), (b64 * b64).sum()]))


def within(got, exact, scale, N):
    """|got - exact| <= (N + 8) 2^-53 scale, the difference taken exactly"""
    got, scale = np.asarray(got, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    ex = np.array(exact, dtype=object).reshape(got.shape)
    for idx in np.ndindex(got.shape):
        if abs(Fraction(float(got[idx])) - ex[idx]) > Fraction((N + 8) * U53) * Fraction(float(scale[idx])):
            return False
    return True


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_gram_against_fractions(ciao, dtype):
    from ciaoalgorithms_jl_amd.host_route import host_gram
    rng = np.random.default_rng(5)
    N, d = 60, 5
    A = rng.standard_normal((N, d))
    A[:, 2] += 1e6
    A, b = A.astype(dtype), rng.standard_normal(N).astype(dtype)
    got = host_gram(A, b)
    assert all(g.dtype == np.float64 for g in got) and got[0].shape == (d, d) and got[1].shape == got[2].shape == (d,) and got[3].shape == (2,)
    *exact, scales = exact_gram(A, b)
    for g, e, s in zip(got, exact, scales):
        assert within(g, e, s, N)
    ints = rng.integers(-64, 65, (300, 7))
    bi = rng.integers(-64, 65, 300)
    G, u, cs, bs = host_gram(ints.astype(dtype), bi.astype(dtype))
    assert np.array_equal(G, ints.T @ ints) and np.array_equal(u, ints.T @ bi) and np.array_equal(cs, ints.sum(axis=0))
    assert bs.tolist() == [bi.sum(), (bi * bi).sum()]
    for bad in (lambda: host_gram(np.zeros((3, 2), np.complex128), np.zeros(3)), lambda: host_gram(np.zeros((3, 2)), np.zeros(4))):
        with pytest.raises(ValueError):
            bad()


def test_standardized_mu_max_and_value_floor_on_the_twin(ciao):
    import torch
    from ciaoalgorithms_jl_amd import gram as GR
    from ciaoalgorithms_jl_amd.host_route import host_gram, host_standardize
    rng = np.random.default_rng(6)
    N, d = 400, 7
    A = rng.standard_normal((N, d)) * np.exp(rng.standard_normal(d)) + 3.0 * rng.standard_normal(d)
    A[:, 4] = 2.5                                    # a constant column: variance 0 in exact arithmetic
    b = rng.standard_normal(N) + 1.5
    st = GR.host_gram_stats(A, b, lam=float(N))
    assert (st.N, st.d, st.kind, st.lam, st.dtype) == (N, d, "ls", float(N), torch.float64)
    assert st.sum_b == float(np.sum(b)) and st.sum_bb == float(np.sum(b * b))

    # standardized() against the Gram statistics of the standardised matrix; tolerance: the reported amplification times the entry's bound
    # (the twin's G and the reference's G_std each carry one bound; the scaled matrix's entries carry a rounding each)
    std, sc = st.standardized()
    A_std, b_std, mean, scale, b_mean = host_standardize(A, b)
    Gr, ur, csr, bsr = host_gram(A_std, b_std)
    amp = sc.amplification.numpy()
    live = [j for j in range(d) if j != 4]
    assert (amp[live] >= 1).all() and (amp[live] < GR.AMPLIFICATION_LIMIT).all() and GR.AMPLIFICATION_LIMIT == 1024.0
    absA = np.abs(A)
    pair = np.sqrt(np.outer(amp, amp))
    tolG = 4 * (N + 8) * U53 * pair * ((absA.T @ absA) * np.outer(scale, scale) + np.abs(A_std).T @ np.abs(A_std))
    Gs = std.G.numpy()
    assert (np.abs(Gs - Gr)[np.ix_(live, live)] <= tolG[np.ix_(live, live)]).all()
    assert np.array_equal(Gs, Gs.T)
    assert (np.abs(np.diag(Gs)[live] - N) <= tolG.diagonal()[live]).all()          # unit population variance
    tolu = 4 * (N + 8) * U53 * np.sqrt(amp) * (absA.T @ np.abs(b) + np.abs(mean) * np.abs(b).sum()) * scale
    assert (np.abs(std.u.numpy() - ur)[live] <= tolu[live]).all()
    assert (np.abs(sc.mean.numpy() - mean)[live] <= 4 * U53 * absA.max(axis=0)[live]).all()
    assert (np.abs(sc.scale.numpy() - scale)[live] <= 4 * (N + 8) * U53 * amp[live] * scale[live]).all()
    assert abs(sc.b_mean - b_mean) <= 4 * U53 * np.abs(b).max() and std.sum_b == 0.0
    assert abs(std.sum_bb - bsr[1]) <= 4 * (N + 8) * U53 * (b * b).sum() and not std.colsum.any()
    # the constant column: its computed variance is rounding noise or zero; either way it is reported, not hidden
    assert amp[4] > GR.AMPLIFICATION_LIMIT
    # center / scale alone; logistic labels stay
    only_c, s2 = st.standardized(scale=False)
    assert (s2.scale == 1).all() and torch.equal(only_c.G, st.G - N * torch.outer(st.colsum / N, st.colsum / N))
    only_s, s3 = st.standardized(center=False)
    assert not s3.mean.any() and s3.b_mean == 0.0 and only_s.sum_b == st.sum_b and only_s.sum_bb == st.sum_bb
    lg, s4 = GR.host_gram_stats(A, np.sign(b), kind="logistic").standardized()
    assert s4.b_mean == 0.0 and lg.sum_bb == float(N) and lg.kind == "logistic" and lg.lam == 1.0

    # mu_max: the gradient at 0 is -lam u / N; at mu_max the certificate of x = 0 has gap 0 and residual 0, just below it it has not
    q = GR.GramLasso(st)
    mm = GR.mu_max(st)
    g0 = q.gradient(torch.zeros(d))
    assert mm == float(N) * float(st.u.abs().max()) / N and torch.equal(g0, -(st.lam / N) * st.u)
    c = q.certificate(torch.zeros(d), mm, 0.1)
    assert c.gap == 0.0 and c.residual == 0.0 and c.F == 0.5 * st.lam * st.sum_bb / N
    assert q.certificate(torch.zeros(d), 0.9 * mm, 0.1).residual > 0
    assert math.isnan(q.certificate(torch.zeros(d), 0.0, 0.1).gap)

    # value and its floor, for one vector and for a matrix of them
    X = torch.from_numpy(rng.standard_normal((d, 3)))
    for k in range(3):
        x = X[:, k].numpy()
        r = A @ x - b
        want = 0.5 * float(r @ r)                    # lam / (2 N) = 1/2
        fl = q.value_floor(X[:, k])
        assert fl == 4 * U53 * 0.5 * (float(X[:, k] @ (st.G @ X[:, k])) + 2 * abs(float(st.u @ X[:, k])) + st.sum_bb)
        assert abs(q.value(X[:, k]) - want) <= fl + 4 * (N + 8) * U53 * want
        assert float(q.value(X)[k]) == q.value(X[:, k]) or abs(float(q.value(X)[k]) - q.value(X[:, k])) <= fl
        assert (q.gradient(X)[:, k] - q.gradient(X[:, k])).abs().max() <= 1e-12 * q.gradient(X[:, k]).abs().max()
    sm = GR.smoothness_exact(st)
    assert abs(sm - float(N) * np.linalg.eigvalsh(A.T @ A)[-1] / N) <= 1e-12 * sm


def data_rounding(A64, b64, A, b, x):
    """|F~(x) - F(x)| for F = 1/2 ||Ax - b||^2 on the float64 data and F~ on the data rounded to float32: at most
    1/2 (||r|| + ||r~||) ||2^-24 (|A| |x| + |b|)||; zero for float64 rows"""
    if A.dtype == np.float64:
        return 0.0
    r, rt = A64 @ x - b64, A.astype(np.float64) @ x - b.astype(np.float64)
    return 0.5 * (np.linalg.norm(r) + np.linalg.norm(rt)) * np.linalg.norm(2.0 ** -24 * (np.abs(A64) @ np.abs(x) + np.abs(b64)))


def check_path(P, GR, st, A64, b64, A, b, x_star, f_star, mus_extra=()):
    """lasso_path at the problem's own weight (and others beside it): the inequalities of weak duality and strong convexity"""
    import torch
    lam_g = 1.0
    path = GR.lasso_path(st, [lam_g, *mus_extra], gap=1e-9, maxit=20000)
    assert path.iterations < 20000 and all(path.converged), (path.iterations, path.converged)
    x, c = path.x[0], path.certificates[0]
    assert x.dtype == (torch.float32 if A.dtype == np.float32 else torch.float64) and x.shape == (A.shape[1],)
    xd = x.double().cpu().numpy()
    q = GR.GramLasso(st)
    floor = q.value_floor(x)
    e_x, e_star = data_rounding(A64, b64, A, b, xd), data_rounding(A64, b64, A, b, x_star)
    sigma = st.lam * float(np.linalg.eigvalsh(A64.T @ A64)[0]) / st.N
    print(f"iterations {path.iterations} gap {c.gap:.3e} objective - f_star {c.objective - f_star:.3e} floor {floor:.3e} "
          f"data {e_x:.3e} |x - x_star|_inf {np.abs(xd - x_star).max():.3e}")
    assert c.gap >= -floor
    assert 0 <= c.objective - f_star + floor + e_x
    assert c.objective - f_star <= c.gap + floor + e_star
    assert float(np.sum((xd - x_star) ** 2)) <= 2 * (c.gap + floor + e_x + e_star) / sigma
    return path


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", PATH_SHAPES)
def test_lasso_path_reaches_the_known_answer_on_the_twin(ciao, shape, dtype):
    import problems as P
    from ciaoalgorithms_jl_amd import gram as GR
    N, n, p = shape
    A64, b64, _, lam, _, x_star, f_star = P.lasso_known_answer(N, n, p)
    A, b = A64.astype(dtype), b64.astype(dtype)
    st = GR.host_gram_stats(A, b, lam=float(N))
    assert lam == 1.0
    path = check_path(P, GR, st, A64, b64, A, b, x_star, f_star, mus_extra=(0.5, 2.0 * GR.mu_max(st)))
    assert not path.x[2].any() and path.certificates[2].gap <= 1e-9 * max(1.0, path.certificates[2].objective)   # beyond mu_max: x = 0
    # a warm start from the answer stops at the first check
    again = GR.lasso_path(st, [1.0], x0=path.x[0], check_every=1)
    assert again.iterations <= 2 or dtype == np.float32


def test_logistic_statistics_are_refused(ciao):
    from ciaoalgorithms_jl_amd import gram as GR
    rng = np.random.default_rng(8)
    A, y = rng.standard_normal((30, 4)), np.sign(rng.standard_normal(30))
    st = GR.host_gram_stats(A, y, kind="logistic")
    for bad in (lambda: GR.GramLasso(st), lambda: GR.lasso_path(st, [0.1]), lambda: GR.mu_max(st)):
        with pytest.raises(ciao._lib.CiaoError) as e:
            bad()
        assert e.value.status == ciao._lib.ERR_ARG
    assert abs(GR.smoothness_exact(st) - np.linalg.eigvalsh(A.T @ A)[-1] / (4 * 30)) <= 1e-12
    with pytest.raises(ValueError):
        GR.host_gram_stats(A, y, kind="hinge")
    ls = GR.host_gram_stats(A, y)
    for bad in (lambda: GR.lasso_path(ls, []), lambda: GR.lasso_path(ls, [0.0]), lambda: GR.lasso_path(ls, [0.1, 0.2], x0=[np.zeros(4)]),
                lambda: GR.GramLasso(ls).certificate(np.zeros(4), 0.1, 0.0)):
        with pytest.raises(ValueError):
            bad()


def test_the_prototype_and_the_module(ciao, tmp_path):
    assert "ciao_gram" in ciao._lib.SIGNATURES and len(ciao._lib.SIGNATURES["ciao_gram"][1]) == 7 and ciao._lib.ABI_VERSION == 3
    src = open(os.path.join(ROOT, "ciaoalgorithms.jl_amd", "solvers.py")).read()
    assert not re.search(r"\bgram\b|ciao_gram|GramStats", src)
    import ciaoalgorithms_jl_amd.gram as GR
    for name in ("GramStats", "gram_stats", "host_gram_stats", "smoothness_exact", "GramLasso", "lasso_path", "mu_max", "LassoPath"):
        assert callable(getattr(GR, name))
    header = open(os.path.join(ROOT, "include", "ciao_hip.h")).read()
    assert re.search(r"/\* EXTENSION(?:(?!\*/).)*\*/\s*CIAO_API int32_t ciao_gram\(", header, re.S)   # marked, in its own comment
    c = tmp_path / "g.c"
    c.write_text('#include <stddef.h>\n#include "ciao_hip.h"\n'
                 "int32_t (*fg)(ciao_ctx *, const ciao_problem *, double *, int64_t, double *, double *, double *) = ciao_gram;\n"
                 "int32_t all(ciao_ctx *c, const ciao_problem *p, double *G, double *v) {\n"
                 "    return ciao_gram(c, p, G, p->d, NULL, NULL, NULL) + ciao_gram(c, p, G, p->d + 3, v, v + p->d, v + 2 * p->d); }\n")
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(c), "-o",
                    str(tmp_path / "g.o")], check=True)

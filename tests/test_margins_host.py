"""The per-sample side of the certificate on the host, no GPU: the logistic gap F + g + E/N against the dual value it abbreviates,
feasibility of the scaled dual point, the gap as a bound at several points of the reference's l1-logistic fixture,
host_certificate(samples=True) and host_score against numpy, solve to tolerance on the host route, and the three new declarations."""
import math
import os
import re
import warnings

import numpy as np
import pytest

import problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeState:
    backend = "host"

    def __init__(self, z):
        self.z = np.asarray(z, dtype=np.float64)


def fixture():
    A, y, L, mu, x0, x_star = P.logistic_fixture(np.float64)
    rng = np.random.default_rng(11)
    noise = rng.standard_normal(A.shape[1])
    points = {"x_star": x_star, "x0": x0, "x_star+1e-3 noise": x_star + 1e-3 * noise, "3 noise": 3 * noise, "40 noise": 40 * noise}
    return A, y, L, mu, x0, x_star, points


def softplus(u):
    return np.maximum(u, 0.0) + np.log1p(np.exp(-np.abs(u)))


def primal(A, y, mu, x):
    return float(np.mean(softplus(-y * (A @ x))) + mu * np.abs(x).sum())


def sigma_neg(t):
    """sigma(-t) = 1 / (1 + exp(t)), stable on both sides"""
    e = np.exp(-np.abs(t))
    return np.where(t >= 0, e / (1 + e), 1 / (1 + e))


def h(u):
    """u log u + (1 - u) log(1 - u) with 0 log 0 = 0"""
    xlogx = lambda v: np.where(v > 0, v * np.log(np.where(v > 0, v, 1.0)), 0.0)
    return xlogx(u) + xlogx(1.0 - u)


def operators(ciao, A, y):
    import ciaoalgorithms_jl_amd.operators as ops
    N, n = A.shape
    return [ops.Precompose(ops.LogisticLoss([y[i]], 1.0), A[i].reshape(1, n), 1.0) for i in range(N)], ops


def test_logistic_gap_is_the_dual_value_and_bounds_the_suboptimality(ciao):
    """D(u) = -(1/N) sum_i h(u_i) on ||(1/N) sum_i u_i y_i a_i||_inf <= mu.  At u' = s sigma(-t), s = min(1, mu / ||grad f||_inf), the
    point is feasible, assemble(entropy=E, n=N).gap = F + g + E/N is P(x) - D(u') to 1e-12, and it is >= 0 and >= P(x) - P(x*)."""
    from ciaoalgorithms_jl_amd.certificate import assemble
    A, y, L, mu, x0, x_star, points = fixture()
    N = A.shape[0]
    for tag, x in points.items():
        t = y * (A @ x)
        u = sigma_neg(t)
        grad = -(A.T @ (u * y)) / N
        M = float(np.abs(grad).max())
        s = 1.0 if M == 0 else min(1.0, mu / M)
        up = s * u
        assert np.abs(A.T @ (up * y) / N).max() <= mu * (1 + 1e-12), tag                     # feasible
        dual = -float(np.mean(h(up)))
        F, g = float(np.mean(softplus(-t))), mu * float(np.abs(x).sum())
        E = float(np.sum(h(up)))
        r = assemble(F, g, 0.0, M, float(x @ grad), 0.0, mu=mu, entropy=E, n=N)
        assert abs(r.gap - (F + g - dual)) <= 1e-12 * max(1.0, F + g), tag
        assert r.gap >= 0 and r.gap >= primal(A, y, mu, x) - primal(A, y, mu, x_star), (tag, r.gap)
        assert r.objective == F + g and r[:7] == assemble(F, g, 0.0, M, float(x @ grad), 0.0, mu=None)[:7]
    # the figures of the derivation's table: the stored x* closes the gap to 5.2e-8, x0 = ones is 7.5 above the optimum
    at = lambda x: assemble(float(np.mean(softplus(-y * (A @ x)))), mu * float(np.abs(x).sum()), 0, 0, 0, 0, mu=mu, n=N,
                            entropy=float(np.sum(h(min(1.0, mu / np.abs(A.T @ (sigma_neg(y * (A @ x)) * y) / N).max()) * sigma_neg(y * (A @ x))))))
    assert 0 <= at(x_star).gap <= 1e-7 and 7.5 <= at(x0).gap <= 8.0
    # NormL1(0) and entropy without mu: no gap
    assert math.isnan(assemble(1.0, 0.0, 0.0, 1.0, 0.0, 0.0, mu=0.0, entropy=-1.0, n=4).gap)
    assert math.isnan(assemble(1.0, 0.0, 0.0, 1.0, 0.0, 0.0, mu=None, entropy=-1.0, n=4).gap)


def test_host_certificate_with_samples_against_numpy(ciao):
    import ciaoalgorithms_jl_amd.host_route as HR
    from ciaoalgorithms_jl_amd.certificate import Certificate
    A, y, L, mu, x0, x_star, points = fixture()
    N = A.shape[0]
    F, ops = operators(ciao, A, y)
    g = ops.NormL1(mu)
    for tag, x in points.items():
        t = y * (A @ x)
        u = sigma_neg(t)
        M = float(np.abs(A.T @ (u * y) / N).max())
        s = min(1.0, mu / M)
        want = primal(A, y, mu, x) + float(np.mean(h(s * u)))
        r = HR.host_certificate(F, g, x, 0.1, N, samples=True)
        assert abs(r.gap - want) <= 1e-12 * max(1.0, primal(A, y, mu, x)), (tag, r.gap, want)
        plain = HR.host_certificate(F, g, x, 0.1, N)
        assert math.isnan(plain.gap) and plain[:7] == r[:7]                                   # without the keyword: as before
        assert Certificate(None, F, g, N, 0.1, samples=True)(FakeState(x)) == r
    # other proxes: no gap, with or without the keyword; LeastSquares rows: the lasso's gap unchanged by the keyword
    assert math.isnan(HR.host_certificate(F, ops.IndBox(-2.0, 2.0), x0, 0.1, N, samples=True).gap)
    assert math.isnan(HR.host_certificate(F, None, x0, 0.1, N, samples=True).gap)
    Al, bl, Ll, lam, xl0, xl_star, _ = P.lasso_known_answer(dtype=np.float64)
    Fl = [ops.LeastSquares(Al[i:i + 1, :], bl[i:i + 1], float(len(bl))) for i in range(len(bl))]
    xl = xl_star + 0.1
    assert HR.host_certificate(Fl, ops.NormL1(lam), xl, 0.1, len(bl), samples=True) == HR.host_certificate(Fl, ops.NormL1(lam), xl, 0.1, len(bl))


def test_host_margin_stats_and_score_against_numpy(ciao):
    import ciaoalgorithms_jl_amd.host_route as HR
    A, y, L, mu, x0, x_star, points = fixture()
    N = A.shape[0]
    F, ops = operators(ciao, A, y)
    for tag, x in points.items():
        t = y * (A @ x)
        for s in (1.0, 0.25, 0.0):
            st = HR.host_margin_stats("logistic", A @ x, y, s)
            want = (np.sum(softplus(-t)), np.sum(h(s * sigma_neg(t))), np.sum(t <= 0), t.min())
            for a, b in zip(st, want):
                assert abs(a - b) <= 1e-12 * max(1.0, abs(b)), (tag, s, st, want)
            assert -N * math.log(2) * (1 + 1e-15) <= st[1] <= 0
        sc = HR.host_score(F, x)
        assert sc.log_loss == pytest.approx(np.mean(softplus(-t)), rel=1e-12) and sc.accuracy == 1 - np.sum(t <= 0) / N and sc.min_margin == t.min()
    assert HR.host_score(F, x_star).accuracy == 1.0 and HR.host_score(F, -x_star).accuracy == 0.0
    Al, bl, Ll, lam, xl0, xl_star, _ = P.lasso_known_answer(dtype=np.float64)
    Fl = [ops.LeastSquares(Al[i:i + 1, :], bl[i:i + 1], 3.0) for i in range(len(bl))]
    x = xl_star + 0.25
    r = Al @ x - bl
    sc = HR.host_score(Fl, x)
    assert sc.mse == pytest.approx(np.mean(r * r), rel=1e-12) and sc.max_abs_residual == np.abs(r).max()
    assert sc.r2 == pytest.approx(1 - np.sum(r * r) / np.sum((bl - bl.mean()) ** 2), rel=1e-10)
    with pytest.raises(TypeError):
        HR.host_score([ops.Zero()] * 3, np.zeros(3))


# the tolerance of the solve-to-tolerance tests, here and on the device (tests/test_gpu_margins.py): the stored x* of the fixture has
# gap 5.2e-8, so 1e-4 is within reach; the host-route run below meets it well before MAXIT
GAP_TOL, MAXIT = 1e-4, 4000


def test_solve_to_tolerance_on_the_host_route(ciao):
    import ciaoalgorithms_jl_amd.solvers as S
    from ciaoalgorithms_jl_amd.certificate import Certificate, stop_when
    A, y, L, mu, x0, x_star, points = fixture()
    N = A.shape[0]
    F, ops = operators(ciao, A, y)
    g = ops.NormL1(mu)
    gamma = float(1 / (7 * np.max(L)))
    stop = stop_when(Certificate(None, F, g, N, gamma, samples=True), gap=GAP_TOL)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x, it = S.SVRG(np.float64, maxit=MAXIT, γ=gamma)(x0.copy(), F=F, g=g, N=N, backend="host", stop=stop, check_every=10)
    print(f"host route: halted after {it} iterations, gap {stop.last.gap:.3e}")
    assert it < MAXIT and 0 <= stop.last.gap <= GAP_TOL
    assert primal(A, y, mu, x) - primal(A, y, mu, x_star) <= GAP_TOL
    # without samples the same stop never fires: the gap is nan there
    blind = stop_when(Certificate(None, F, g, N, gamma), gap=GAP_TOL)
    assert blind(FakeState(x)) is False and math.isnan(blind.last.gap)


def test_header_binding_and_julia_module_name_the_entry_points(ciao):
    hdr = open(os.path.join(ROOT, "include", "ciao_hip.h")).read()
    jl = open(os.path.join(ROOT, "ciaoalgorithms.jl_amd", "julia", "CIAOAlgorithmsAMD", "src", "CIAOAlgorithmsAMD.jl")).read()
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = ciao._lib.load()
    for name, nargs in (("ciao_row_dots", 4), ("ciao_margin_stats", 5), ("ciao_certificate_samples", 6)):
        m = re.search(r"CIAO_API int32_t " + name + r"\(([^;]*)\);", hdr)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in ciao._lib.SIGNATURES and len(ciao._lib.SIGNATURES[name][1]) == nargs
        assert hasattr(lib, name)
        assert f"ccall((:{name}, libciao)" in jl and f":{name}" in md
        assert not name.startswith("ciao_sample")
    assert int(re.search(r"#define CIAO_ABI_VERSION (\d+)", hdr).group(1)) == 3     # additive: the version stays
    # the sample entry points refuse before any launch: a NULL context is an argument error, not a crash
    assert lib.ciao_row_dots(None, None, None, None) == ciao._lib.ERR_ARG
    assert lib.ciao_margin_stats(None, None, None, 1.0, None) == ciao._lib.ERR_ARG
    assert lib.ciao_certificate_samples(None, None, None, None, 1.0, None) == ciao._lib.ERR_ARG

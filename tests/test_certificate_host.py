"""The certificate's host side, no GPU: the gap formula against the dual it abbreviates, stop_when against a fake state, and the
three declarations of ciao_certificate (header, ctypes table, Julia module)."""
import math
import os
import re

import numpy as np
import pytest

import problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeState:
    backend = "host"

    def __init__(self, z):
        self.z = np.asarray(z, dtype=np.float64)


def lasso(ciao):
    import ciaoalgorithms_jl_amd.operators as ops
    A, b, L, lam, x0, x_star, f_star = P.lasso_known_answer(dtype=np.float64)      # 6 x 3
    N = A.shape[0]
    F = [ops.LeastSquares(A[i:i + 1, :], b[i:i + 1], float(N)) for i in range(N)]
    return A, b, N, lam, F, ops.NormL1(lam), x_star


def test_gap_formula_is_the_dual_value_and_bounds_the_suboptimality(ciao):
    """P(x) = c/2 ||Ax - b||^2 + mu ||x||_1 with c = lam_f / N = 1;  D(theta) = -||theta||^2 / (2c) - theta.b on ||A'theta||_inf <= mu.
    At theta = s c (Ax - b) the formula F (2s - s^2) - s x.grad f IS D(theta) (to 1e-12), theta is feasible, the gap is >= 0 and
    >= P(x) - P(x*); a brute-force maximisation of D over the feasible set does not beat P(x*), and at x* the gap closes."""
    from ciaoalgorithms_jl_amd.certificate import Certificate
    A, b, N, mu, F, g, x_star = lasso(ciao)
    c = 1.0
    cert = Certificate(None, F, g, N, 0.01)
    primal = lambda x: P.lasso_cost(A, b, mu, x)
    dual = lambda th: -th @ th / (2 * c) - th @ b
    rng = np.random.default_rng(5)
    points = [np.zeros(3), x_star, x_star + 1e-3, 10 * rng.standard_normal(3)] + [x_star * t for t in (0.5, 0.9, 1.1)]
    for x in points:
        r = cert(FakeState(x))
        res = A @ x - b
        grad = c * A.T @ res
        assert abs(r.F - 0.5 * c * res @ res) <= 1e-12 * max(1.0, r.F) and abs(r.g - mu * np.abs(x).sum()) <= 1e-12 * max(1.0, r.g)
        assert abs(r.grad_inf - np.abs(grad).max()) <= 1e-12 * np.abs(grad).max() and abs(r.x_dot_grad - x @ grad) <= 1e-9
        s = min(1.0, mu / np.abs(grad).max())
        theta = s * c * res
        assert np.abs(A.T @ theta).max() <= mu * (1 + 1e-12)                      # feasible
        direct = primal(x) - dual(theta)
        assert abs(r.gap - direct) <= 1e-12 * max(1.0, abs(primal(x)), abs(dual(theta)))
        assert r.gap >= -1e-12 * max(1.0, primal(x))
        assert r.gap >= primal(x) - primal(x_star) - 1e-12 * max(1.0, primal(x))
        assert r.objective == r.F + r.g and r.box_violation == 0.0
    # brute force: projected ascent on the dual from many feasible starts never exceeds the primal optimum (weak duality), and
    # the certificate's own dual point at x* reaches it
    best = -math.inf
    for _ in range(200):
        th = rng.standard_normal(6)
        th *= min(1.0, mu / np.abs(A.T @ th).max())
        for _ in range(200):
            step = th + 0.05 * (-th / c - b)
            step *= min(1.0, mu / np.abs(A.T @ step).max())                       # scaling keeps A'theta inside the box
            if dual(step) <= dual(th):
                break
            th = step
        best = max(best, dual(th))
    assert best <= primal(x_star) + 1e-12
    at_opt = cert(FakeState(x_star))
    assert abs(at_opt.gap) <= 1e-12 * primal(x_star) and at_opt.residual <= 1e-9
    assert best <= at_opt.objective - at_opt.gap + 1e-12


def test_gap_is_nan_where_it_does_not_apply_and_box_violation_is_reported(ciao):
    import ciaoalgorithms_jl_amd.operators as ops
    from ciaoalgorithms_jl_amd.certificate import Certificate, assemble
    A, y, L, lam, x0, x_star = P.logistic_fixture(np.float64)
    N, n = A.shape
    F = [ops.Precompose(ops.LogisticLoss([y[i]], 1.0), A[i].reshape(1, n), 1.0) for i in range(N)]
    r = Certificate(None, F, ops.NormL1(lam), N, 0.1)(FakeState(x_star))
    assert math.isnan(r.gap) and r.residual < 1e-6 and r.g == pytest.approx(lam * np.abs(x_star).sum())
    r = Certificate(None, F, ops.IndBox(-1.0, 0.5), N, 0.1)(FakeState(np.array([0.0, 0.75, -1.0, 0.0, 0.0])))
    assert r.box_violation == 0.25 and r.g == math.inf and r.objective == math.inf and math.isnan(r.gap)
    assert assemble(2.0, 1.0, 0.0, 0.0, 0.0, 0.0, mu=0.5).gap == 2.0 + 1.0 - 2.0     # zero gradient: s = 1
    assert math.isnan(assemble(2.0, 0.0, 0.0, 1.0, 0.0, 0.0, mu=0.0).gap)            # NormL1(0): no gap
    with pytest.raises(ValueError):
        Certificate(None, F, None, N, 0.0)


def test_stop_when_composes_with_a_state(ciao):
    from ciaoalgorithms_jl_amd.certificate import Certificate, stop_when
    A, b, N, mu, F, g, x_star = lasso(ciao)
    cert = Certificate(None, F, g, N, 0.01)
    far, near = FakeState(np.zeros(3)), FakeState(x_star)
    stop = stop_when(cert, gap=1e-8)
    assert stop(far) is False and stop.last.gap > 1.0
    assert stop(near) is True and stop.last is not None and abs(stop.last.gap) <= 1e-8
    assert stop_when(cert, residual=1e-6)(near) and not stop_when(cert, residual=1e-6)(far)
    assert not stop_when(cert, gap=1e-8, residual=0.0)(FakeState(x_star + 1e-7))    # every bound given must hold
    with pytest.raises(ValueError):
        stop_when(cert)
    # the host route's own states go through the same call: solve to tolerance with the functor's existing stop= keyword
    import warnings
    import ciaoalgorithms_jl_amd.solvers as S
    gamma = float(1 / (7 * np.max(N * np.sum(A ** 2, axis=1))))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x, it = S.SVRG(np.float64, maxit=1000, γ=gamma)(np.zeros(3), F=F, g=g, N=N, backend="host", stop=stop_when(cert, gap=1e-6), check_every=10)
    assert it < 1000 and P.lasso_cost(A, b, mu, x) - P.lasso_cost(A, b, mu, x_star) <= 1e-6


def test_solvers_module_does_not_import_the_certificate():
    src = open(os.path.join(ROOT, "ciaoalgorithms.jl_amd", "solvers.py")).read()
    assert "certificate" not in src


def test_header_binding_and_julia_module_name_the_entry_point(ciao):
    hdr = open(os.path.join(ROOT, "include", "ciao_hip.h")).read()
    m = re.search(r"CIAO_API int32_t ciao_certificate\(([^;]*)\);", hdr)
    assert m and len(m.group(1).split(",")) == 7
    res, args = ciao._lib.SIGNATURES["ciao_certificate"]
    assert len(args) == 7
    assert hasattr(ciao._lib.load(), "ciao_certificate")
    jl = open(os.path.join(ROOT, "ciaoalgorithms.jl_amd", "julia", "CIAOAlgorithmsAMD", "src", "CIAOAlgorithmsAMD.jl")).read()
    assert "ccall((:ciao_certificate, libciao)" in jl and "function certificate(" in jl
    assert ":ciao_certificate" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"#define CIAO_ABI_VERSION (\d+)", hdr).group(1)) == 3     # additive: the version stays

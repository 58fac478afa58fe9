"""Gap-safe screening on the CPU: the radius against hand values, and the safety of the rule's numpy restatement (host_route.host_screen)
along proximal-gradient runs on Gaussian lasso and l1-logistic problems: no coordinate in the support of the 20 000-step solution is
ever discarded -- with the gradient in float64 and rounded to float32 -- and the rule WITHOUT the rounding floor of the radius does
discard one, so the sweep can see that defect."""
import math

import numpy as np
import pytest

STEPS = (1, 4, 11, 31, 101, 301, 1001, 3001, 20000)
SHAPES = ((300, 50), (200, 1000), (64, 257), (1000, 20))
RATIOS = (0.5, 0.1)
# 8 and 12: two seeds (picked by a one-off search; about a quarter of the seeds tried behave so) at which the (64, 257) lasso at 0.5 mu_max reaches a computed gap of exactly 0, where the
# rule without the floor drops support coordinates; the safety assertion holds for whatever seed
SEEDS = (0, 8, 12)


@pytest.fixture(scope="module")
def S(ciao):
    from ciaoalgorithms_jl_amd import screening
    return screening


def _cert(ciao, **kw):
    from ciaoalgorithms_jl_amd.certificate import CertificateResult
    base = dict(F=1.0, g=0.5, objective=1.5, residual=0.0, grad_inf=2.0, x_dot_grad=0.0, box_violation=0.0, gap=1e-3)
    base.update(kw)
    return CertificateResult(**base)


def test_radius_against_hand_values(ciao, S):
    eps = 2.0 ** -52
    # LeastSquares rows: s = mu / grad_inf, G = gap + 64 eps objective, kappa = sqrt(2 lam G / N)
    s, kappa = S.radius("ls", 3.0, 100, _cert(ciao), eps, 0.5)
    assert s == 0.25
    assert kappa == math.sqrt(2.0 * 3.0 * (1e-3 + 64.0 * eps * 1.5) / 100.0)
    # logistic rows: kappa = sqrt(G / (2 N)); the loss may be given as the ABI's constant
    s, kappa = S.radius(ciao._lib.LOSS_LOGISTIC, 1.0, 8, _cert(ciao, grad_inf=0.25), eps, 0.5)
    assert s == 1.0
    assert kappa == math.sqrt((1e-3 + 64.0 * eps * 1.5) / 16.0)
    # grad f = 0: s = 1
    assert S.radius("ls", 1.0, 10, _cert(ciao, grad_inf=0.0), eps, 0.5)[0] == 1.0
    # a negative computed gap counts as 0: the floor alone is left
    s, kappa = S.radius("ls", 1.0, 10, _cert(ciao, gap=-1e-17), eps, 0.5)
    assert kappa == math.sqrt(2.0 * (64.0 * eps * 1.5) / 10.0) and kappa > 0
    # float32 solves have the larger floor
    assert S.radius("ls", 1.0, 10, _cert(ciao, gap=0.0), 2.0 ** -23, 0.5)[1] == math.sqrt(2.0 * (64.0 * 2.0 ** -23 * 1.5) / 10.0)
    # no gap (NaN), or an infinite one: everything is kept
    for gap in (math.nan, math.inf):
        s, kappa = S.radius("ls", 1.0, 10, _cert(ciao, gap=gap), eps, 0.5)
        assert s == 0.25 and kappa == math.inf
    assert S.radius("logistic", 1.0, 10, _cert(ciao, objective=math.nan), eps, 0.5)[1] == math.inf
    with pytest.raises(ValueError):
        S.radius("ls", 1.0, 10, _cert(ciao), eps, 0.0)
    with pytest.raises(ValueError):
        S.radius("zero", 1.0, 10, _cert(ciao), eps, 0.5)


def test_host_screen_keeps_on_nan_and_inf(ciao, S):
    grad = np.array([0.1, np.nan, np.inf, 0.1, 0.1, 0.9])
    colsq = np.array([1.0, 1.0, 1.0, np.nan, np.inf, 1.0])
    keep = S.host_screen(grad, colsq, 1.0, 0.1, 0.5)
    assert keep.tolist() == [False, True, True, True, True, True]
    assert S.host_screen(grad, colsq, 1.0, math.inf, 0.5).all()          # kappa = +inf keeps everything ...
    assert S.host_screen(np.zeros(3), np.zeros(3), 1.0, math.inf, 0.5).all()   # ... also where inf * 0 is NaN


def test_restrict_and_expand_refuse_without_a_device_problem(ciao, S):
    with pytest.raises(ciao._lib.CiaoError):
        S.restrict(object(), [1, 0, 1])
    with pytest.raises(ciao._lib.CiaoError):
        S.gap_safe(None, object(), None, None, 1.0)


# ---- the safety sweep -------------------------------------------------------------------------------------------------------------------
def _problem(loss, N, d, seed):
    rng = np.random.default_rng(1000 * seed + N + d)
    A = rng.standard_normal((N, d))
    x_true = rng.standard_normal(d) * (rng.random(d) < 0.1)
    t = A @ x_true + 0.1 * rng.standard_normal(N)
    return A, (t if loss == "ls" else np.where(t >= 0, 1.0, -1.0))


def _value_grad(loss, A, b, x):
    """F(x) = (1/N) sum f_i(x), grad f(x), and the row dots, in float64 (LeastSquares weight 1)."""
    N = A.shape[0]
    z = A @ x
    if loss == "ls":
        r = z - b
        return 0.5 * float(r @ r) / N, A.T @ r / N, z
    t = b * z
    e = np.exp(-np.abs(t))
    F = float(np.sum(np.maximum(-t, 0.0) + np.log1p(e))) / N
    sig_neg = np.where(t >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
    return F, A.T @ (-b * sig_neg) / N, z


def _certificate(ciao, loss, A, b, x, mu, grad32):
    """What the device certificate would hand to `radius`, in numpy: with grad32 the gradient is rounded to float32 first."""
    from ciaoalgorithms_jl_amd.certificate import assemble
    from ciaoalgorithms_jl_amd.host_route import host_margin_stats
    F, grad, z = _value_grad(loss, A, b, x)
    if grad32:
        grad = grad.astype(np.float32).astype(np.float64)
    grad_inf = float(np.max(np.abs(grad)))
    gval = mu * float(np.abs(x).sum())
    if loss == "ls":
        return assemble(F, gval, 0.0, grad_inf, float(x @ grad), 0.0, mu=mu), grad
    s = 1.0 if grad_inf == 0 else min(1.0, mu / grad_inf)
    return assemble(F, gval, 0.0, grad_inf, float(x @ grad), 0.0, mu=mu, entropy=host_margin_stats("logistic", z, b, s)[1], n=A.shape[0]), grad


def _run(ciao, S, loss, N, d, ratio, seed):
    """(support of the 20 000-step iterate, {(step, grad32, floor): keep mask})"""
    A, b = _problem(loss, N, d, seed)
    colsq = np.sum(A * A, axis=0)
    mu = ratio * float(np.max(np.abs(_value_grad(loss, A, b, np.zeros(d))[1])))
    Lf = np.linalg.norm(A, 2) ** 2 / N * (1.0 if loss == "ls" else 0.25)
    gamma = 1.0 / Lf
    x = np.zeros(d)
    masks = {}
    for k in range(1, STEPS[-1] + 1):
        w = x - gamma * _value_grad(loss, A, b, x)[1]
        x = np.sign(w) * np.maximum(np.abs(w) - gamma * mu, 0.0)
        if k in STEPS:
            for grad32 in (False, True):
                cert, grad = _certificate(ciao, loss, A, b, x, mu, grad32)
                eps = float(np.finfo(np.float32 if grad32 else np.float64).eps)
                for floor in (True, False):
                    s, kappa = S.radius(loss, 1.0, N, cert, eps if floor else 0.0, mu)
                    masks[(k, grad32, floor)] = S.host_screen(grad, colsq, s, kappa, mu)
    return x != 0, masks


@pytest.fixture(scope="module")
def sweep(ciao, S):
    return {(loss, N, d, ratio, seed): _run(ciao, S, loss, N, d, ratio, seed)
            for loss in ("ls", "logistic") for (N, d) in SHAPES for ratio in RATIOS for seed in SEEDS}


def test_the_rule_discards_no_support_coordinate(sweep):
    wrong, dropped, total = [], 0, 0
    for key, (support, masks) in sweep.items():
        for (k, grad32, floor), keep in masks.items():
            if not floor:
                continue
            bad = int(np.sum(support & ~keep))
            if bad:
                wrong.append((key, k, grad32, bad))
            if k == STEPS[-1] and not grad32:
                dropped += int(np.sum(~keep))
                total += keep.size
    print(f"screening sweep: {len(sweep)} problems, {dropped} of {total} coordinates discarded at the last checkpoint (float64)")
    assert not wrong, f"support coordinates discarded (problem, step, float32 gradient, count): {wrong[:10]}"
    assert dropped > 0.5 * total, "the rule discards next to nothing at a converged iterate: the sweep would show no defect either"


def test_without_the_floor_a_support_coordinate_is_discarded(sweep):
    """The defect the floor 64 eps objective is there for, on the (64, 257) lasso at mu = 0.5 mu_max: at a computed gap of 0 the
    support sits on |grad f_j| = mu to rounding."""
    bad = 0
    for (loss, N, d, ratio, seed), (support, masks) in sweep.items():
        if (loss, N, d, ratio) == ("ls", 64, 257, 0.5):
            bad += sum(int(np.sum(support & ~keep)) for (k, grad32, floor), keep in masks.items() if not floor)
    assert bad > 0, "the bare rule discarded no support coordinate: this sweep cannot see the defect the floor guards against"

"""The l1-logistic problem with an unpenalised, bounded intercept on the device (newton.logistic_newton(intercept=True) on DeviceRows,
cv.logistic_cv(intercept=True, score_together=True)), on the seeded offset-1.5 problem of
tests/test_logistic_intercept_host.py, (N, d) = (200, 50).

  * DeviceRows against HostRows, float64, every row and a row list: both converge at gap 1e-9, the objectives agree to
    10 gap max(1, objective), the supports are equal;
  * float32 rows at gap 1e-5 (DESIGN.md section 8.16 has why 1e-6 stalls);
  * logistic_cv(folds=3, three weights, intercept=True) with score_together=True against the default: every held-out loss within
    test_gpu_score_many.general_bounds' law for the pair of device evaluations, the same best, and the scoring call's kernel is the
    row-list mscore kernel."""
import numpy as np
import pytest

from test_gpu_score_many import general_bounds
from test_logistic_intercept_host import problem

pytestmark = pytest.mark.gpu


def packed(A, y):
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    return PackedF.logistic(torch.from_numpy(A).cuda(), torch.from_numpy(y).cuda())


def the_problem(dtype):
    A, y = problem(200, 50, 1.5)
    return A.astype(dtype), y.astype(dtype)


@pytest.mark.parametrize("listed", [False, True], ids=["every-row", "row-list"])
def test_device_rows_against_host_rows(ctx, listed):
    import torch
    from ciaoalgorithms_jl_amd.newton import DeviceRows, HostRows, logistic_mu_max, logistic_newton
    gap = 1e-9
    A, y = the_problem(np.float64)
    F = packed(A, y)
    idx = np.sort(np.random.default_rng(1).choice(200, size=150, replace=False)) if listed else None
    dev_rows = DeviceRows(ctx, F, rows=None if idx is None else torch.from_numpy(idx).cuda())
    host_rows = HostRows(A, y, rows=idx)
    top_d, top_h = logistic_mu_max(dev_rows, intercept=True), logistic_mu_max(host_rows, intercept=True)
    assert abs(top_d - top_h) <= 1e-12 * top_h
    mu = 0.1 * top_h
    dev = logistic_newton(dev_rows, mu, gap=gap, max_outer=30, subproblem="cd", intercept=True)
    host = logistic_newton(host_rows, mu, gap=gap, max_outer=30, subproblem="cd", intercept=True)
    assert dev.converged and host.converged, (dev.reason, host.reason)
    assert dev.x.is_cuda and dev.x.dtype == torch.float64 and dev.certificate.gap >= -1e-12 and abs(dev.intercept) < 32.0
    scale = max(1.0, host.certificate.objective)
    print(f"objective device {dev.certificate.objective!r} host {host.certificate.objective!r} intercept {dev.intercept!r} / {host.intercept!r}")
    assert abs(dev.certificate.objective - host.certificate.objective) <= 10 * gap * scale
    assert np.array_equal(dev.x.cpu().numpy() != 0, np.asarray(host.x) != 0)
    assert dev.passes.gram == dev.outer


def test_float32_rows_converge_at_1e_5(ctx):
    import torch
    from ciaoalgorithms_jl_amd.newton import DeviceRows, HostRows, logistic_mu_max, logistic_newton
    gap = 1e-5
    A, y = the_problem(np.float32)
    F = packed(A, y)
    rows = DeviceRows(ctx, F)
    mu = 0.1 * logistic_mu_max(rows, intercept=True)
    dev = logistic_newton(rows, mu, gap=gap, subproblem="cd", intercept=True)
    host = logistic_newton(HostRows(A, y), mu, gap=gap, subproblem="cd", intercept=True)
    assert dev.converged and host.converged, (dev.reason, dev.certificate.gap, host.reason)
    assert dev.x.dtype == torch.float32 and dev.intercept > 0
    assert abs(dev.certificate.objective - host.certificate.objective) <= 10 * gap * max(1.0, host.certificate.objective)


def test_logistic_cv_scores_a_fold_in_one_pass(ctx, monkeypatch):
    from ciaoalgorithms_jl_amd import cv as CV
    from ciaoalgorithms_jl_amd.newton import HostRows, logistic_mu_max
    A, y = the_problem(np.float64)
    F = packed(A, y)
    top = logistic_mu_max(HostRows(A, y), intercept=True)
    mus = [0.5 * top, 0.2 * top, 0.1 * top]
    seen = []
    inner = ctx.margin_stats_multi

    def spy(F_, xs, s=None, rows=None, offsets=None, check_rows=True):
        out = inner(F_, xs, s, rows=rows, offsets=offsets, check_rows=check_rows)
        seen.append((ctx.last_kernel(), [x.double().cpu().numpy() for x in xs], rows.cpu().numpy(), list(offsets)))
        return out

    monkeypatch.setattr(ctx, "margin_stats_multi", spy)
    together = CV.logistic_cv(ctx, F, mus, folds=3, gap=1e-8, intercept=True, score_together=True)
    monkeypatch.undo()
    assert len(seen) == 3 and all(name.startswith("mscore_partial_kernel<rows,f64,SL4,logistic,") and "K=3" in name for name, *_ in seen)
    apart = CV.logistic_cv(ctx, F, mus, folds=3, gap=1e-8, intercept=True)
    assert bool(together.converged.all()) and bool(apart.converged.all())
    assert together.best == apart.best and together.one_se == apart.one_se
    assert together.intercepts == apart.intercepts == [r.intercept for r in apart.path] and all(c > 0 for c in apart.intercepts)
    A64 = A.astype(np.float64)
    for f, (_, xs, held, cs) in enumerate(seen):
        M = len(held)
        for k in range(3):
            delta, _ = general_bounds("logistic", np.float64, A64[held], y[held], xs[k], M, 50)
            delta = delta + 2.0 ** -53 * (np.abs(A64[held] @ xs[k]) + abs(cs[k]))
            a, b = float(together.loss[f, k]), float(apart.loss[f, k])
            bound = float(np.sum(delta)) / M + 2 * M * 2.0 ** -52 * b
            print(f"fold {f} model {k}: held-out loss together {a!r} apart {b!r} allowed {bound:.3g}")
            assert abs(a - b) <= bound
            t = y[held] * (A64[held] @ xs[k] + cs[k])
            assert abs(float(together.accuracy[f, k]) - float(apart.accuracy[f, k])) * M <= np.count_nonzero(np.abs(t) <= delta)

"""The l1-logistic problem on a row list and its cross-validation on the device (newton.DeviceRows(rows=), scoring.score(rows=),
cv.logistic_cv), on the seeded problem of tests/test_logistic_cv_host.py: (N, d) = (200, 50), 5 folds,
mus = (0.5, 0.25, 0.1, 0.03) logistic_mu_max; float64 rows at gap 1e-8, float32 rows at gap 1e-5.

  * logistic_newton(DeviceRows(ctx, F, rows=train), mu) converges, and its objective lies within 2 gap max(1, objective) of the
    HostRows(A, y, rows=train) solve: each is within gap max(1, objective) of the same minimum;
  * score(ctx, F, x, rows=) and every entry of logistic_cv(ctx, F, ...).loss against direct float64 numpy at the DEVICE's own x, under the
    bound of the CPU test; converged all true; best / one_se are choose() on the device table;
  * DeviceRows(ctx, F) without rows returns the bits it returned before row lists existed (tests/golden/device_rows_full_f64.json: taken
    on the device with the newton.py of the commit before, on this seeded problem)."""
import hashlib
import json
import os

import numpy as np
import pytest

from test_gpu_gram import tname
from test_logistic_cv_host import FRACTIONS, by_definition, cv_problem, direct_loss, mus_of

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_rows_full_f64.json")
CASES = [(np.float64, 1e-8), (np.float32, 1e-5)]


def packed(A, y):
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    return PackedF.logistic(torch.from_numpy(A).cuda(), torch.from_numpy(y).cuda())


@pytest.mark.parametrize("dtype,gap", CASES, ids=["f64", "f32"])
def test_the_fold_problem_on_a_row_list(ctx, dtype, gap):
    import torch
    from ciaoalgorithms_jl_amd import cv as CV
    from ciaoalgorithms_jl_amd.newton import DeviceRows, HostRows, logistic_newton
    from ciaoalgorithms_jl_amd.scoring import score
    A, y = cv_problem(dtype=dtype)
    F = packed(A, y)
    mus = mus_of(A, y)
    lists = CV.fold_lists(200, 5, seed=3, device="cuda")
    train = torch.sort(torch.cat(lists[1:])).values.contiguous()
    rows = DeviceRows(ctx, F, rows=train)
    assert (rows.N, rows.d) == (len(train), 50)
    for mu in (mus[1], mus[3]):
        dev = logistic_newton(rows, mu, gap=gap, subproblem="cd")
        host = logistic_newton(HostRows(A, y, rows=train.cpu().numpy()), mu, gap=gap, subproblem="cd")
        assert dev.converged and dev.reason == "gap" and host.converged, (dev.reason, host.reason)
        assert dev.x.is_cuda and dev.x.dtype == F.dtype
        scale = max(1.0, host.certificate.objective)
        print(f"{tname(dtype)} mu={mu:.4g}: objective device {dev.certificate.objective!r} host {host.certificate.objective!r} allowed {2 * gap * scale:.3g}")
        assert abs(dev.certificate.objective - host.certificate.objective) <= 2 * gap * scale
        assert dev.passes.gram == dev.outer and dev.passes.first_order >= 2 * dev.outer + 2
        # the certificate's loss against direct numpy at the device's x, and the held-out score
        x = dev.x.double().cpu().numpy()
        loss, _, bound = direct_loss(A, y, x, train.cpu().numpy())
        assert abs(dev.certificate.F - loss) <= bound, (dev.certificate.F, loss, bound)
        sc = score(ctx, F, dev.x, rows=lists[0])
        loss, acc, bound = direct_loss(A, y, x, lists[0].cpu().numpy())
        print(f"  held-out log-loss device {sc.log_loss!r} numpy {loss!r} bound {bound:.3g}")
        assert abs(sc.log_loss - loss) <= bound and sc.accuracy == acc
        a = A.astype(np.float64)[lists[0].cpu().numpy()]
        t = y.astype(np.float64)[lists[0].cpu().numpy()] * (a @ x)
        assert abs(sc.min_margin - t.min()) <= float(np.max(2 * (50 + 2) * 2.0 ** -53 * (np.abs(a) @ np.abs(x))))
    # LeastSquares rows through the same list
    from ciaoalgorithms_jl_amd.device import PackedF
    Fl = PackedF.least_squares(F.A, F.b, 1.0)
    sl = score(ctx, Fl, dev.x, rows=lists[0])
    h = lists[0].cpu().numpy()
    r = A.astype(np.float64)[h] @ x - y.astype(np.float64)[h]
    assert abs(sl.mse - float(np.mean(r * r))) <= 1e-12 * float(np.mean(r * r)) and abs(sl.max_abs_residual - np.abs(r).max()) <= 1e-12 * np.abs(r).max()


@pytest.mark.parametrize("dtype,gap", CASES, ids=["f64", "f32"])
def test_logistic_cv_on_the_device(ctx, dtype, gap):
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd import cv as CV
    from ciaoalgorithms_jl_amd.device import PackedF
    from ciaoalgorithms_jl_amd.newton import DeviceRows, logistic_path
    A, y = cv_problem(dtype=dtype)
    F = packed(A, y)
    mus = mus_of(A, y)
    res = CV.logistic_cv(ctx, F, mus, folds=5, seed=3, gap=gap)
    K = len(mus)
    assert res.mus == mus and tuple(res.loss.shape) == tuple(res.accuracy.shape) == tuple(res.converged.shape) == (5, K)
    assert res.loss.device.type == "cpu" and res.loss.dtype == torch.float64
    assert bool(res.converged.all()), res.converged
    lists = CV.fold_lists(200, 5, seed=3, device="cuda")
    worst = 0.0
    for f in range(5):
        train = torch.sort(torch.cat([r for g, r in enumerate(lists) if g != f])).values.contiguous()
        fit = logistic_path(DeviceRows(ctx, F, rows=train), mus, gap=gap, subproblem="cd")           # the same solves again: the same bits
        for k, r in enumerate(fit):
            loss, acc, bound = direct_loss(A, y, r.x.double().cpu().numpy(), lists[f].cpu().numpy())
            worst = max(worst, abs(float(res.loss[f, k]) - loss) / bound)
            assert abs(float(res.loss[f, k]) - loss) <= bound, (f, k, float(res.loss[f, k]), loss, bound)
            assert float(res.accuracy[f, k]) == acc
    print(f"{tname(dtype)}: largest |table - numpy| / bound = {worst:.3g}")
    mean, stderr, best, one_se = by_definition(mus, res.loss.numpy())
    assert (res.best, res.one_se) == (best, one_se) == CV.choose(mus, res.mean.tolist(), res.stderr.tolist())
    assert np.allclose(res.mean.numpy(), mean, rtol=1e-14, atol=0) and np.allclose(res.stderr.numpy(), stderr, rtol=1e-12, atol=0)
    assert len(res.path) == K and all(r.x.is_cuda for r in res.path)
    if dtype == np.float64:
        with pytest.raises(L.CiaoError):
            CV.logistic_cv(ctx, PackedF.least_squares(F.A, F.b, 1.0), mus)
        with pytest.raises(L.CiaoError, match="logistic_cv"):
            CV.lasso_cv(ctx, F, mus)
        with pytest.raises(ValueError):
            CV.logistic_cv(ctx, F, [])
        with pytest.raises(ValueError):
            CV.logistic_cv(ctx, F, mus, folds=201)
        with pytest.raises(ValueError):
            DeviceRows(ctx, F, rows=torch.tensor([0, 200], device="cuda"))
        with pytest.raises(L.CiaoError):
            DeviceRows(ctx, F, rows=torch.empty(0, dtype=torch.int64, device="cuda"))


def device_rows_record(ctx, newton):
    """what DeviceRows(ctx, F) without a list returns on the seeded float64 problem, as hex strings and digests of the bytes"""
    A, y = cv_problem(dtype=np.float64)
    F = packed(A, y)
    rows = newton.DeviceRows(ctx, F)
    mu = FRACTIONS[2] * newton.logistic_mu_max(rows)
    res = newton.logistic_newton(rows, mu, gap=1e-8, subproblem="cd")
    dots = rows.dots(res.x)
    grad = rows.gradient(res.x)
    hess = rows.hessian(dots)
    loss = rows.loss(dots, 0.75)
    cert = rows.certificate(res.x, mu, 1.0)
    raw = lambda t: t.detach().cpu().contiguous().numpy().tobytes()
    return {"mu": float(mu).hex(), "x": raw(res.x).hex(), "gradient": raw(grad).hex(), "dots": hashlib.sha256(raw(dots)).hexdigest(),
            "hessian": hashlib.sha256(raw(hess)).hexdigest(), "loss": [float(v).hex() for v in loss],
            "certificate": [float(v).hex() for v in (cert.objective, cert.gap, cert.residual)], "outer": res.outer, "passes": list(res.passes),
            "reason": res.reason}


def test_device_rows_without_a_list_keep_their_bits(ctx):
    from ciaoalgorithms_jl_amd import newton
    want = json.load(open(GOLDEN))
    got = device_rows_record(ctx, newton)
    for k in want:
        assert got[k] == want[k], k
    assert newton.DeviceRows(ctx, packed(*cv_problem())).list_passes is None

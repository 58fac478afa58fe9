"""cv.logistic_cv on the host route (ctx=None, F = (A, y) numpy arrays: newton.HostRows on gathered copies); DESIGN.md section 8.16.

Gaussian rows, labels from a 6-sparse model with noise 0.5; (N, d) = (200, 50), 5 folds, mus = (0.5, 0.25, 0.1, 0.03) logistic_mu_max.
  * every fold solve ends converged with reason "gap" (float64 at gap 1e-8; float32 at 1e-5: at 1e-6 some float32 solves end "stalled");
  * every table entry against the direct numpy log-loss of the model that produced it on that fold's rows, within
        mean_m(2 (d + 2) 2^-53 |a_m|'|x|) + (M + 4) 2^-53 loss
    (the log-loss is 1-Lipschitz in the margin, a margin is a dot product of d terms -- each side within (d + 2) 2^-53 |a|'|x| of the
    exact one -- and M terms are added);
  * best / one_se from the table by their definitions; a NaN column never wins;
  * the refusals.
cv_problem, direct_loss and loss_bound are shared with tests/test_gpu_logistic_cv.py."""
import math

import numpy as np
import pytest

FRACTIONS = (0.5, 0.25, 0.1, 0.03)


def cv_problem(N=200, d=50, dtype=np.float64, seed=35):
    """Gaussian rows, labels sign(A xt + 0.5 noise) from a model xt of six entries +-1.  The seed is one for which the premise of the
    float32 case holds: logistic_newton on float32 rows stops "stalled" once the gap sits at the noise of float32 dots (newton.py), and
    at gap 1e-5 and the smallest weight that is close: of the seeds 31 .. 36 the EXISTING driver on gathered float32 copies converges
    in every fold for 32 and 35 and ends "stalled" at relative gaps of 2 .. 3e-5 in one to four of the forty fold solves for the others
    (35 has the wider margin, 6.9e-6).  float64 at 1e-8 converges for all of them."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, d)).astype(dtype)
    xt = np.zeros(d)
    xt[:min(6, d)] = rng.choice([-1.0, 1.0], min(6, d))
    y = np.where(A.astype(np.float64) @ xt + 0.5 * rng.standard_normal(N) >= 0, 1.0, -1.0).astype(dtype)
    assert 0.2 < (y > 0).mean() < 0.8
    return A, y


def direct_loss(A, y, x, rows):
    """(mean log-loss, accuracy, the bound on the difference to another float64 evaluation) of x on A[rows], y[rows], in float64 numpy"""
    a = np.asarray(A, np.float64)[rows]
    x = np.asarray(x, np.float64)
    t = np.asarray(y, np.float64)[rows] * (a @ x)
    loss = float(np.mean(np.maximum(-t, 0.0) + np.log1p(np.exp(-np.abs(t)))))
    M, d = a.shape
    bound = float(np.mean(2 * (d + 2) * 2.0 ** -53 * (np.abs(a) @ np.abs(x)))) + (M + 4) * 2.0 ** -53 * loss
    return loss, 1.0 - float(np.sum(t <= 0)) / M, bound


def by_definition(mus, table):
    """(mean, stderr, best, one_se) of a (folds, K) table"""
    nf = table.shape[0]
    mean = table.mean(axis=0)
    stderr = table.std(axis=0, ddof=1) / math.sqrt(nf)
    best = int(np.nanargmin(mean))
    ok = [k for k in range(len(mus)) if mean[k] <= mean[best] + stderr[best]]
    return mean, stderr, best, max(ok, key=lambda k: mus[k])


def mus_of(A, y):
    from ciaoalgorithms_jl_amd.newton import HostRows, logistic_mu_max
    top = logistic_mu_max(HostRows(A, y))
    return [f * top for f in FRACTIONS]


@pytest.mark.parametrize("shape,folds,dtype,gap", [((200, 50), 5, np.float64, 1e-8), ((200, 50), 5, np.float32, 1e-5), ((203, 17), 4, np.float64, 1e-9)],
                         ids=["200x50-f64", "200x50-f32", "203x17-f64"])
@pytest.mark.parametrize("subproblem", ["cd", "fista"])
def test_logistic_cv_on_the_host(ciao, shape, folds, dtype, gap, subproblem):
    import torch
    from ciaoalgorithms_jl_amd import cv as CV
    from ciaoalgorithms_jl_amd.newton import HostRows, logistic_path
    A, y = cv_problem(*shape, dtype=dtype)
    mus = mus_of(A, y)
    res = CV.logistic_cv(None, (A, y), mus, folds=folds, seed=3, gap=gap, subproblem=subproblem)
    assert isinstance(res, CV.LogisticCVResult) and res.mus == mus
    K = len(mus)
    for t in (res.loss, res.accuracy, res.converged):
        assert tuple(t.shape) == (folds, K) and t.device.type == "cpu"
    assert res.loss.dtype == torch.float64 and res.converged.dtype == torch.bool and bool(res.converged.all())
    lists = CV.fold_lists(shape[0], folds, seed=3)
    assert sorted(torch.cat(lists).tolist()) == list(range(shape[0]))
    for f in range(folds):
        train = torch.sort(torch.cat([r for g, r in enumerate(lists) if g != f])).values.numpy()
        fit = logistic_path(HostRows(A[train], y[train]), mus, gap=gap, subproblem=subproblem)       # the existing driver on gathered copies
        assert all(r.converged and r.reason == "gap" for r in fit), (f, [r.reason for r in fit])
        for k, r in enumerate(fit):
            loss, acc, bound = direct_loss(A, y, r.x, lists[f].numpy())
            assert abs(float(res.loss[f, k]) - loss) <= bound, (f, k, float(res.loss[f, k]), loss, bound)
            assert float(res.accuracy[f, k]) == acc
    mean, stderr, best, one_se = by_definition(mus, res.loss.numpy())
    assert np.allclose(res.mean.numpy(), mean, rtol=1e-14, atol=0) and np.allclose(res.stderr.numpy(), stderr, rtol=1e-12, atol=0)
    assert (res.best, res.one_se) == (best, one_se) == CV.choose(mus, res.mean.tolist(), res.stderr.tolist())
    assert mus[res.one_se] >= mus[res.best]
    # the refit: the path on all rows, whatever its solves ended with
    assert len(res.path) == K
    whole = logistic_path(HostRows(A, y), mus, gap=gap, subproblem=subproblem)
    assert all(np.array_equal(np.asarray(a.x), np.asarray(b.x)) for a, b in zip(res.path, whole))


def test_a_nan_column_never_wins(ciao):
    from ciaoalgorithms_jl_amd import cv as CV
    mus = [0.4, 0.2, 0.1, 0.05]
    nan = float("nan")
    assert CV.choose(mus, [nan, 0.6, 0.5, 0.55], [nan, 0.01, 0.2, 0.01]) == (2, 1)
    assert CV.choose(mus, [0.5, nan, 0.4, nan], [0.01, nan, nan, nan]) == (2, 2)
    with pytest.raises(ValueError):
        CV.choose(mus, [nan] * 4, [nan] * 4)


def test_refusals(ciao):
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd import cv as CV
    A, y = cv_problem(40, 5)
    for bad in ([], [0.1, 0.0], [-1.0], [float("inf")], [float("nan")]):
        with pytest.raises(ValueError):
            CV.logistic_cv(None, (A, y), bad)
    for folds in (1, 0, 41):
        with pytest.raises(ValueError):
            CV.logistic_cv(None, (A, y), [0.1], folds=folds)
    with pytest.raises(L.CiaoError):
        CV.logistic_cv(None, A, [0.1])                 # neither a PackedF nor (A, y)
    with pytest.raises(L.CiaoError):
        CV.logistic_cv(None, (A, y, 1.0), [0.1])       # fold_stats' LeastSquares triple: these are not logistic rows

"""K-fold cross-validation of the lasso path in d-space, at ONE pass over A in total.

The statistics of fold f come from a Gram pass over that fold's row list (Context.gram(rows=): the cost of the rows touched, so the folds
together cost one pass); the training statistics of fold f are the sum of the other folds' (gram.add_stats); the K models of a fold come
from gram.lasso_cd / gram.lasso_path on them; the held-out error of a model is a quadratic form in the fold's own statistics (gram.mse).
After the Gram calls nothing reads A.

    res = lasso_cv(ctx, F, mus, folds=5, seed=0)
    res.mse[f, k]; res.mean; res.stderr; mus[res.best]; mus[res.one_se]; res.path.x[res.one_se]

lasso_cv: LeastSquares rows only (logistic statistics are refused, as GramLasso refuses them); the columns are not standardised inside
the folds.

Logistic rows have no sufficient statistics, so their cross-validation reads rows -- but only the rows a fold names (DESIGN.md section
8.16): logistic_cv fits every training fold with newton.logistic_path on DeviceRows(ctx, F, rows=train) (Context.list_dots, list_combine
and gram(weights=, rows=) over the list, no gathered copy) and scores every model on the held-out list (scoring.score(rows=)).

    res = logistic_cv(ctx, F, mus, folds=5, seed=0)
    res.loss[f, k]; res.accuracy[f, k]; res.mean; res.stderr; mus[res.one_se]; res.path[res.one_se].x

solvers.py imports nothing from here.
"""
from __future__ import annotations

import math
from typing import NamedTuple

from . import _lib as L
from .gram import GramStats, _cd_general, _constraints, _need_ls, add_stats, gram_stats, host_gram_stats, lasso_path, mse


class CVResult(NamedTuple):
    mus: list           # the K l1 weights, as given
    mse: object         # (folds, K) float64 CPU tensor: held-out mean squared residual of model k on fold f
    mean: object        # (K,) the mean over the folds
    stderr: object      # (K,) std(ddof=1) / sqrt(folds)
    best: int           # argmin of the mean; a NaN never wins, ties go to the smaller index
    one_se: int         # the index of the largest mu whose mean is <= mean[best] + stderr[best]
    path: object        # gram.LassoPath refitted on the sum of all folds, for every mu
    floor: float        # the largest rounding floor (gram.mse) met in the table: differences of mse below it mean nothing


def fold_lists(N, folds, seed=0, device="cpu"):
    """`folds` sorted int64 lists that partition 0 .. N-1: a seeded torch permutation (drawn on the CPU, so the folds do not depend on the
    device) cut into near-equal parts -- the first N mod folds parts hold one row more -- each sorted ascending for locality."""
    import torch
    N, folds = int(N), int(folds)
    if not 2 <= folds <= N:
        raise ValueError(f"fold_lists needs 2 <= folds <= N (got folds={folds}, N={N})")
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    perm = torch.randperm(N, generator=g, dtype=torch.int64)
    base, extra = divmod(N, folds)
    out, lo = [], 0
    for f in range(folds):
        hi = lo + base + (1 if f < extra else 0)
        out.append(torch.sort(perm[lo:hi]).values.contiguous().to(device))
        lo = hi
    return out


def fold_stats(ctx, F, lists):
    """One GramStats per list: len(lists) calls of gram_stats(ctx, F, rows=list).  With ctx=None and F = (A, b) numpy arrays (optionally
    (A, b, lam)) the statistics come from host_route.host_gram instead, as CPU tensors."""
    if ctx is None:
        import numpy as np
        A, b = F[0], F[1]
        lam = float(F[2]) if len(F) > 2 else 1.0
        return [host_gram_stats(A, b, lam=lam, rows=np.asarray(r.cpu() if hasattr(r, "cpu") else r, dtype=np.int64)) for r in lists]
    return [gram_stats(ctx, F, rows=r) for r in lists]


def choose(mus, mean, stderr):
    """(best, one_se) from the table's column means by their definitions."""
    best, val = -1, math.inf
    for k, v in enumerate(mean):
        if v == v and (best < 0 or v < val):
            best, val = k, v
    if best < 0:
        raise ValueError("lasso_cv: every model's mean error is NaN")
    se = stderr[best]
    bound = val + (se if se == se else 0.0)
    one_se = best
    for k, v in enumerate(mean):
        if v == v and v <= bound and mus[k] > mus[one_se]:
            one_se = k
    return best, one_se


def lasso_cv_from_stats(stats_f, mus, gap=1e-6, method="cd", ctx=None, fused=False, penalty_factor=None, lower=None, upper=None,
                        ridge=0.0) -> CVResult:
    """Cross-validation from the folds' statistics alone: pure d-space, on whatever device the statistics live (device statistics with
    method="cd" need the Context to launch on, as gram.lasso_cd).  For each fold f: the training statistics are add_stats of the other
    folds in fold order, the K models come from lasso_path(method=) on them with the gap asked for, and the held-out errors from
    mse(stats_f[f], X).  The table itself is formed on the HOST in float64 (a d x d x K product per fold), so that it does not depend on
    the device the statistics live on.

    penalty_factor, lower, upper, ridge: gram.lasso_cd's, for every fold and the refit (method="cd").  fused=True (method="cd"; DESIGN.md
    section 8.17): the folds' training statistics and the all-rows statistics are stacked and all (folds + 1) K models go through ONE
    driver loop, one Context.gram_cd_general launch per round, each model on its own fold's Gram matrix, u and tol schedule and frozen
    on its own gap.  A model's bits do not depend on its neighbours in a launch, so where no model runs into the sweep budget the
    result is bit for bit that of fused=False."""
    import torch
    stats_f = list(stats_f)
    if len(stats_f) < 2:
        raise ValueError("lasso_cv_from_stats needs at least two folds")
    for s in stats_f:
        if not isinstance(s, GramStats):
            raise TypeError("lasso_cv_from_stats takes a list of gram.GramStats")
        _need_ls(s, "lasso_cv")
    mus = [float(m) for m in mus]
    K = len(mus)
    if K < 1 or any(not (m > 0 and math.isfinite(m)) for m in mus):
        raise ValueError("lasso_cv needs at least one l1 weight, every one > 0 and finite")
    nf = len(stats_f)
    table = torch.empty((nf, K), dtype=torch.float64)
    floor = 0.0
    kw = dict(penalty_factor=penalty_factor, lower=lower, upper=upper, ridge=ridge)
    fits = None
    if fused:
        if method != "cd":
            raise ValueError("fused=True needs method='cd': the folds share one coordinate-descent launch")
        s0 = stats_f[0]
        pf, lo, hi, rdg, general = _constraints(s0.d, s0.G.device, penalty_factor, lower, upper, ridge)
        groups = [add_stats([s for g, s in enumerate(stats_f) if g != f]) for f in range(nf)] + [add_stats(stats_f)]
        fits = _cd_general(groups, mus, None, gap, 2000, ctx, None, pf, lo, hi, rdg, general)
    for f in range(nf):
        if fits is not None:
            fit = fits[f]
        else:
            fit = lasso_path(add_stats([s for g, s in enumerate(stats_f) if g != f]), mus, gap=gap, method=method, ctx=ctx, **kw)
        X = torch.stack([x.double().cpu() for x in fit.x], dim=1)
        v, fl = mse(stats_f[f].to("cpu"), X)
        table[f] = v
        fl = fl[fl == fl]
        if fl.numel():
            floor = max(floor, float(fl.max()))
    mean = table.mean(0)
    stderr = table.std(0, unbiased=True) / math.sqrt(nf)
    best, one_se = choose(mus, mean.tolist(), stderr.tolist())
    path = fits[nf] if fits is not None else lasso_path(add_stats(stats_f), mus, gap=gap, method=method, ctx=ctx, **kw)
    return CVResult(mus, table, mean, stderr, best, one_se, path, floor)


def lasso_cv(ctx, F, mus, folds=5, seed=0, gap=1e-6, method="cd", fused=False, penalty_factor=None, lower=None, upper=None, ridge=0.0) -> CVResult:
    """K-fold cross-validation of the lasso path over the rows of F at one pass over A in total: fold_lists(F.N, folds, seed), then
    fold_stats (one Gram pass per fold over that fold's row list), then lasso_cv_from_stats (fused and the four constraint keywords are
    its).  F: a device.PackedF of LeastSquares rows."""
    from .device import PackedF
    if not isinstance(F, PackedF) or F.loss != L.LOSS_LS:
        raise L.CiaoError(L.ERR_ARG, "lasso_cv covers device.PackedF problems of LeastSquares rows (logistic cross-validation is not built "
                                     "here: cv.logistic_cv)")
    lists = fold_lists(F.N, folds, seed, device=F.A.device)
    return lasso_cv_from_stats(fold_stats(ctx, F, lists), mus, gap=gap, method=method, ctx=ctx, fused=fused, penalty_factor=penalty_factor,
                               lower=lower, upper=upper, ridge=ridge)


class LogisticCVResult(NamedTuple):
    mus: list           # the K l1 weights, as given
    loss: object        # (folds, K) float64 CPU tensor: held-out mean log-loss of model k on fold f
    accuracy: object    # (folds, K) held-out accuracy, 1 - #{y a'x <= 0} / M
    mean: object        # (K,) the mean of loss over the folds
    stderr: object      # (K,) std(ddof=1) / sqrt(folds)
    best: int           # argmin of the mean; a NaN never wins, ties go to the smaller index
    one_se: int         # the index of the largest mu whose mean is <= mean[best] + stderr[best]
    path: list          # K newton.NewtonResult: the refit on all rows, for every mu
    converged: object   # (folds, K) bool: the fold solve ended converged
    intercepts: list = None   # logistic_cv(intercept=True): the refit's K intercepts (zeros without one)


def logistic_cv(ctx, F, mus, folds=5, seed=0, gap=1e-6, subproblem="cd", max_outer=30, intercept=False, intercept_bound=32.0,
                score_together=False) -> LogisticCVResult:
    """K-fold cross-validation of the l1-logistic path without copying rows: fold_lists(F.N, folds, seed); for
    fold f the training list is the other folds' lists concatenated in fold order and sorted, the K models come from
    newton.logistic_path(DeviceRows(ctx, F, rows=train), mus, ...) -- in the order given, each solve warm-started from the last -- and
    the held-out mean log-loss and accuracy of every model from scoring.score(ctx, F, x, rows=lists[f]); the refit on all rows uses
    DeviceRows(ctx, F).  The table is formed on the host in float64; best / one_se are choose() on the loss means.  Every pass reads
    only the rows its list names (M / N of a pass over A each); the columns are not standardised inside the folds.

    F: a device.PackedF of logistic rows.  With ctx=None and F = (A, y) numpy arrays the same driver runs on the host: newton.HostRows
    on gathered copies, the scores from host_route.host_margin_stats.

    intercept, intercept_bound: every fit, the refit included, carries an unpenalised intercept
    (newton.logistic_newton's keywords) and every score is that of a_i'x + c; the result's intercepts are the refit's.
    score_together=True: the K models of a fold are scored by ONE scoring.score_many(rows=lists[f], intercepts=) call -- one pass over
    the held-out rows (ciao_margin_stats_multi_rows) instead of K; the scores agree with the default's to rounding (another order of
    addition).  The host route takes the same keywords (host_route.host_margin_stats_multi(rows=, offsets=))."""
    import torch
    from .host_route import _score, host_margin_stats, host_margin_stats_multi
    from .newton import DeviceRows, HostRows, logistic_path
    host = ctx is None
    ikw = dict(intercept=True, intercept_bound=intercept_bound) if intercept else {}
    if host:
        import numpy as np
        if not (isinstance(F, (tuple, list)) and len(F) == 2):
            raise L.CiaoError(L.ERR_ARG, "logistic_cv without a Context takes F = (A, y) numpy arrays")
        A, y = np.asarray(F[0]), np.asarray(F[1])
        N = int(A.shape[0])
    else:
        from .device import PackedF
        if not isinstance(F, PackedF) or F.loss != L.LOSS_LOGISTIC:
            raise L.CiaoError(L.ERR_ARG, "logistic_cv covers device.PackedF problems of logistic rows (LeastSquares rows: cv.lasso_cv)")
        N = int(F.N)
    mus = [float(m) for m in mus]
    K = len(mus)
    if K < 1 or any(not (m > 0 and math.isfinite(m)) for m in mus):
        raise ValueError("logistic_cv needs at least one l1 weight, every one > 0 and finite")
    lists = fold_lists(N, folds, seed, device="cpu" if host else F.A.device)
    nf = len(lists)
    loss = torch.empty((nf, K), dtype=torch.float64)
    acc = torch.empty((nf, K), dtype=torch.float64)
    conv = torch.empty((nf, K), dtype=torch.bool)
    for f in range(nf):
        train = torch.sort(torch.cat([r for g, r in enumerate(lists) if g != f])).values.contiguous()
        rows = HostRows(A, y, rows=train.numpy()) if host else DeviceRows(ctx, F, rows=train)
        fit = logistic_path(rows, mus, gap=gap, max_outer=max_outer, subproblem=subproblem, **ikw)
        together = None
        if score_together:
            cs = [r.intercept for r in fit] if intercept else None
            if host:
                held = lists[f].numpy()
                st = host_margin_stats_multi("logistic", A, [np.asarray(r.x, dtype=np.float64) for r in fit], y, rows=held, offsets=cs)
                together = [_score("logistic", s4, len(held)) for s4 in st]
            else:
                from .scoring import score_many
                together = score_many(ctx, F, [r.x for r in fit], rows=lists[f], intercepts=cs)
        for k, r in enumerate(fit):
            if together is not None:
                sc = together[k]
            elif host:
                held = lists[f].numpy()
                x = np.asarray(r.x, dtype=np.float64)
                dots = A[held].astype(np.float64) @ x
                if intercept:
                    dots = dots + r.intercept
                sc = _score("logistic", host_margin_stats("logistic", dots, y[held], 1.0), len(held))
            else:
                from .scoring import score
                sc = score(ctx, F, r.x, rows=lists[f], intercept=r.intercept)
            loss[f, k], acc[f, k], conv[f, k] = sc.log_loss, sc.accuracy, bool(r.converged)
    mean = loss.mean(0)
    stderr = loss.std(0, unbiased=True) / math.sqrt(nf)
    best, one_se = choose(mus, mean.tolist(), stderr.tolist())
    path = logistic_path(HostRows(A, y) if host else DeviceRows(ctx, F), mus, gap=gap, max_outer=max_outer, subproblem=subproblem, **ikw)
    return LogisticCVResult(mus, loss, acc, mean, stderr, best, one_se, path, conv, [r.intercept for r in path])

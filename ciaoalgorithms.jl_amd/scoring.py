"""Scores of a fitted model on device rows: predictions never leave the GPU.

    score(ctx, F, x)    F: device.PackedF -- the training rows, or NEW rows with the same d (the prediction path)

One full pass gives the row dots a_i'x (Context.row_dots), one reduction over the N samples the sums (Context.margin_stats, s = 1);
the fields below are formed from those four doubles on the host.  For operator objects on the host route: host_route.host_score.
"""
from __future__ import annotations

from typing import NamedTuple


class LeastSquaresScore(NamedTuple):
    mse: float                # (1/N) sum_i (a_i'x - b_i)^2
    r2: float                 # 1 - sum_i (a_i'x - b_i)^2 / sum_i (b_i - mean b)^2   (nan where b is constant)
    max_abs_residual: float   # max_i |a_i'x - b_i|


class LogisticScore(NamedTuple):
    log_loss: float           # (1/N) sum_i log(1 + exp(-y_i a_i'x))
    accuracy: float           # 1 - #{i: y_i a_i'x <= 0} / N
    min_margin: float         # min_i y_i a_i'x


def margin_stats_torch(kind, dots, b, s=1.0):
    """The four numbers of ciao_margin_stats from float64 torch vectors (dots, and b = the targets / labels, of one length), by the same
    stable evaluation as host_route.host_margin_stats: the statistics of a row LIST, whose dots are an M-vector (Context.list_dots).
    The order of addition is torch's.  Synchronises."""
    import torch
    dots, b = dots.double(), b.double()
    if kind == "ls":
        r = dots - b
        return float((r * r).sum()), float(b.sum()), float((b * b).sum()), float(r.abs().max())
    t = b * dots
    e = torch.exp(-t.abs())
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    v = s * torch.where(t >= 0, small, big)
    w = (1.0 - s) + s * torch.where(t >= 0, big, small)
    xlogx = lambda u: torch.where(u > 0, u * torch.log(torch.where(u > 0, u, torch.ones_like(u))), torch.zeros_like(u))
    return (float((torch.clamp(-t, min=0.0) + torch.log1p(e)).sum()), float((xlogx(v) + xlogx(w)).sum()), float((t <= 0).sum()), float(t.min()))


def score(ctx, F, x, rows=None, intercept=0.0):
    """LeastSquaresScore or LogisticScore of x on the rows of F (a device.PackedF of LeastSquares or logistic rows); synchronises.

    rows: a contiguous int64 device vector of M >= 1 row numbers in [0, N), any order, repeats allowed -> the score over A[rows],
    b[rows] (held-out rows, a fold) at the cost of the rows touched: Context.list_dots, then float64 torch operations on the
    M-vector.

    intercept: a finite number c -> the score of the predictions a_i'x + c (newton.logistic_newton(intercept=True); DESIGN.md section
    8.18): the list route (rows=None: every row), c added to the float64 dots.  0.0 adds nothing and keeps the calls above."""
    from . import _lib as L
    from .host_route import _score
    kind = "logistic" if F.loss == L.LOSS_LOGISTIC else "ls"
    intercept = float(intercept)
    if intercept - intercept != 0.0:
        raise ValueError("score: the intercept must be finite")
    if rows is None and intercept == 0.0:
        stats = ctx.margin_stats(F, ctx.row_dots(F, x), 1.0)
        return _score(kind, tuple(stats), F.N)
    from .stepsize import _on_stream
    with _on_stream(ctx):
        dots = ctx.list_dots(F, x, rows=rows)
        if dots.numel() < 1:
            raise ValueError("score: rows must name at least one row")
        if intercept != 0.0:
            dots = dots + intercept
        stats = margin_stats_torch(kind, dots, F.b if rows is None else F.b[rows], 1.0)
    return _score(kind, stats, int(dots.numel()))


def score_many(ctx, F, xs, rows=None, intercepts=None):
    """[score(ctx, F, x) for x in xs] from ONE pass over the rows of F (Context.margin_stats_multi: up to 256 models a call; the
    N x K predictions never exist): the scores of a regularisation path, of folds or of restarts on held-out rows.  Each agrees with
    its own score() to rounding (another order of addition).  Synchronises.

    rows, intercepts: [score(ctx, F, x, rows=rows, intercept=c) for x, c in zip(xs, intercepts)] from one pass over the rows the list
    names (Context.margin_stats_multi(rows=, offsets=)); the score's n is the length of the list."""
    from . import _lib as L
    from .host_route import _score
    kind = "logistic" if F.loss == L.LOSS_LOGISTIC else "ls"
    n = F.N if rows is None else int(rows.shape[0])
    return [_score(kind, tuple(st), n) for st in ctx.margin_stats_multi(F, xs, rows=rows, offsets=intercepts)]


def best(scores):
    """The index of the score with the smallest log_loss (LogisticScore) or mse (LeastSquaresScore).  A NaN never wins; ties go to the
    smaller index.  ValueError on an empty list or where every score is NaN."""
    arg, val = -1, float("inf")
    for k, sc in enumerate(scores):
        v = sc.log_loss if hasattr(sc, "log_loss") else sc.mse
        if v == v and (arg < 0 or v < val):
            arg, val = k, v
    if arg < 0:
        raise ValueError("best: no score to choose from (an empty list, or every score is NaN)")
    return arg

"""Column standardisation of a matrix that is already packed on the device.

One l1 weight mu on columns of different scale penalises units, not features, and LeastSquares rows have no intercept unless A and b are
centred: every l1 problem these solvers are used for assumes comparable columns.  These functions make them so where the matrix lies,
from one pass for the moments (ciao_col_moments) and one for the scaling (ciao_scale_columns), both in csrc/colmom_kernels.h:

    F = PackedF.least_squares(A_dev, b_dev, lam)
    F_std, sc = standardize(ctx, F)                        # inplace=True: over F.A, no second matrix
    x_std, it = SVRG(np.float64)(x0, F=F_std, g=g, N=N)
    x, intercept = sc.coefficients(x_std)                  # the model on the ORIGINAL columns: a_i'x + intercept
    score(ctx, sc.transform(ctx, F_validation), x_std)     # other rows, the same centre and scale

Nothing here is called by solvers.py.  The numpy twins: host_route.host_col_moments / host_standardize, host_column_moments below.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import _lib as L
from .stepsize import _on_stream

REFINE_RATIO = 2.0 ** 10     # s2 / M2 beyond this: the first pass lost more than ten bits of M2, a second one is made


class ColumnMoments(NamedTuple):
    mean: object      # d-vector of doubles (device tensor; numpy array from the host twin)
    var: object       # population variance, max(M2, 0) / N
    n: int            # rows
    passes: int       # passes over A made: 1 or 2


def _needs_refinement(s1, s2, n):
    """The rule, on numpy arrays or torch tensors alike -> a boolean d-vector.  M2 = s2 - s1^2 / N carries a relative error of at most
    2 (N + 3) 2^-53 s2 / M2: refine where that amplification exceeds 2^10, or where cancellation left M2 <= 0 under a positive s2."""
    m2 = s2 - s1 * s1 / n
    return ((m2 > 0) & (s2 > REFINE_RATIO * m2)) | ((m2 <= 0) & (s2 > 0))


def _check(ctx, F, what):
    from .device import PackedF
    if not isinstance(F, PackedF) or F.loss not in (L.LOSS_LS, L.LOSS_LOGISTIC):
        raise L.CiaoError(L.ERR_ARG, f"{what} covers device.PackedF problems of real LeastSquares or logistic rows: complex rows, the sharing "
                                     "family and Zero terms are not standardised")
    if ctx.is_row_sharded() or F.N_total != F.N:
        raise L.CiaoError(L.ERR_ARG, f"{what} on a row-sharded context (all-reduce hook, shard table, peers or a row shard): the column "
                                     "moments would need an all-reduce of their own")
    if F.N < 1:
        raise L.CiaoError(L.ERR_ARG, f"{what} needs at least one row (N = 0: the columns have no mean)")


def _refine_arg(refine):
    if refine not in ("auto", True, False):
        raise ValueError(f"refine must be 'auto', True or False (got {refine!r})")
    return refine


def column_moments(ctx, F, shift=None, refine="auto") -> ColumnMoments:
    """Mean and population variance of every column of F.A -> ColumnMoments(mean, var, n, passes), mean and var device float64 d-vectors.

    One pass of shifted sums (Context.col_moments) about c = shift (a float64 device d-vector) or the first row: mean = c + s1 / N,
    var = max(s2 - s1^2 / N, 0) / N.  refine="auto" makes a second pass about the computed mean where the first one's own output shows
    that cancellation cost more than ten bits in some column (s2 / M2 > 2^10, or M2 <= 0 < s2): one small device reduction and one
    synchronisation decide.  refine=True always makes it, refine=False never (and does not synchronise)."""
    import torch
    _check(ctx, F, "column_moments")
    refine = _refine_arg(refine)
    n = F.N
    with _on_stream(ctx):
        c = F.A[0].double() if shift is None else shift
        s1, s2 = ctx.col_moments(F, shift)
        mean = c + s1 / n
        passes = 1
        if refine is True or (refine == "auto" and bool(_needs_refinement(s1, s2, n).any())):
            mean = mean.contiguous()
            s1, s2 = ctx.col_moments(F, mean)
            mean = mean + s1 / n
            passes = 2
        var = torch.clamp(s2 - s1 * s1 / n, min=0.0) / n
    return ColumnMoments(mean, var, n, passes)


def host_column_moments(A, shift=None, refine="auto") -> ColumnMoments:
    """column_moments in numpy (float64) on a host matrix: the same shift, the same rule, the same second pass."""
    from .host_route import host_col_moments
    refine = _refine_arg(refine)
    A = np.asarray(A)
    n = A.shape[0]
    if n < 1:
        raise ValueError("column moments need at least one row")
    c = A[0].astype(np.float64) if shift is None else np.asarray(shift, dtype=np.float64)
    s1, s2 = host_col_moments(A, shift)
    mean = c + s1 / n
    passes = 1
    if refine is True or (refine == "auto" and bool(_needs_refinement(s1, s2, n).any())):
        s1, s2 = host_col_moments(A, mean)
        mean = mean + s1 / n
        passes = 2
    return ColumnMoments(mean, np.maximum(s2 - s1 * s1 / n, 0.0) / n, n, passes)


class Scaler:
    """What standardize did, to undo it on a solution and to repeat it on other rows.

    mean, scale: device float64 d-vectors (mean = 0 where the columns were not centred, scale = 1 where they were not scaled, and where a
    column is constant); b_mean: the mean taken off LeastSquares targets, 0.0 for logistic rows and without centring."""

    def __init__(self, mean, scale, b_mean, centered, scaled):
        self.mean, self.scale, self.b_mean = mean, scale, float(b_mean)
        self.centered, self.scaled = bool(centered), bool(scaled)

    def _like(self, x):
        """mean and scale as x's kind of array, in float64"""
        import torch
        if isinstance(x, torch.Tensor):
            return x.double(), self.mean.to(x.device), self.scale.to(x.device), lambda v: v.to(x.dtype)
        x = np.asarray(x)
        return x.astype(np.float64), self.mean.cpu().numpy(), self.scale.cpu().numpy(), lambda v: v.astype(x.dtype)

    def coefficients(self, x_std):
        """A solution on the standardised columns -> (x, intercept) on the original ones: x_j = x_std_j scale_j and
        intercept = b_mean - mean . x, so that a_std_i'x_std + b_mean = a_i'x + intercept for every row.  x has x_std's type and dtype (the
        products are formed in float64, the intercept from the rounded x); intercept is a float."""
        xs, mean, scale, back = self._like(x_std)
        x = back(xs * scale)
        return x, self.b_mean - float((mean * self._like(x)[0]).sum())

    def to_standardized(self, x):
        """The inverse of the coefficient map, for warm starts: x_std_j = x_j / scale_j."""
        xo, _, scale, back = self._like(x)
        return back(xo / scale)

    def transform(self, ctx, F_new, inplace=False):
        """The same centre and scale on other rows with the same d (validation rows for scoring.score) -> a PackedF; LeastSquares targets
        have b_mean taken off.  inplace=True writes over F_new.A."""
        _check(ctx, F_new, "Scaler.transform")
        if F_new.d != self.mean.numel():
            raise ValueError(f"the scaler was fitted on {self.mean.numel()} columns, F_new has {F_new.d}")
        return _apply(ctx, F_new, self, inplace)


def _apply(ctx, F, sc, inplace):
    from .device import PackedF
    with _on_stream(ctx):
        out = ctx.scale_columns(F, sc.mean if sc.centered else None, sc.scale if sc.scaled else None, inplace=inplace)
        b = F.b
        if F.loss == L.LOSS_LS and sc.centered:
            b = (F.b.double() - sc.b_mean).to(F.dtype)
            if ctx.stream is not None:
                b.record_stream(ctx.stream)
    G = PackedF(F.loss, out, b, F.lam, N_total=F.N_total, row0=F.row0, cyclic=F.cyclic)
    G.padded_from = F.padded_from
    return G


def standardize(ctx, F, center=True, scale=True, inplace=False, refine=True):
    """Centre every column of F.A at its mean and scale it to unit population variance -> (F_std, Scaler).

    scale_j = 1 / sqrt(var_j), and 1 where var_j = 0: a constant column centred comes out exactly zero (its mean is the column's own
    value, (double)a - mean = 0).  With center=False the columns are only scaled (by the same 1 / sqrt(var_j)), with scale=False only
    centred.  For LeastSquares rows with `center` the targets are centred too, b - mean(b) in a fresh N-vector (float64 arithmetic,
    rounded once); logistic labels stay as they are.  F_std keeps loss, lam, N_total, row ownership and padded_from.  inplace=True writes
    over F.A (no second matrix; F itself then sees the standardised rows too, with its old b).

    refine=True: the moments are always taken a second time about the computed mean (column_moments), three passes over A in all.  The
    scale divides every entry, so an error of k units in var_j shows as k / 2 units in every entry of the column and as k units in
    its sum of squares: about the first row the amplification s2 / M2 = 1 + (a_0j - mean_j)^2 / var_j is 2 on average and 10 for one
    column in a few hundred, about the mean it is 1 and the columns come out with sum of squares N to a few units of F's type.
    refine="auto" spares that pass where no column lost more than ten bits.  Synchronises."""
    import torch
    _check(ctx, F, "standardize")
    m = column_moments(ctx, F, refine=refine)
    with _on_stream(ctx):
        mean = m.mean.contiguous() if center else torch.zeros_like(m.mean)
        sd = torch.sqrt(m.var)
        sc = torch.where(m.var > 0, 1.0 / sd, torch.ones_like(sd)).contiguous() if scale else torch.ones_like(m.var)
        b_mean = float(F.b.double().mean()) if (center and F.loss == L.LOSS_LS) else 0.0
    scaler = Scaler(mean, sc, b_mean, center, scale)
    return _apply(ctx, F, scaler, inplace), scaler

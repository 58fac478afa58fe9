"""Step sizes from the data, for a matrix that is already packed on the device.

Every solver here takes its step from the per-sample smoothness constants L_i of the f_i: L_i = lam ||a_i||^2 for
LeastSquares(a_i, b_i, lam) rows (test_lasso.jl:52-56) and L_i = ||a_i||^2 / 4 for logistic rows (test_logistic_l1.jl:39).  The
reference's tests form them on the host from the rows; these functions form them from one pass over the device rows
(ciao_row_sqnorms, csrc/rowsq_kernels.h):

    F = PackedF.least_squares(A_dev, b_dev, lam)
    x, it = SAGA(np.float64)(x0, F=F, g=g, L=lipschitz_max(ctx, F), N=N)      # gamma = 1 / (3 max L): one float, no N-vector
    x, it = Finito(np.float64)(x0, F=F, g=g, L=lipschitz(ctx, F), N=N)        # gamma_i = alpha N / L_i, formed on the device
    est, upper = smoothness(ctx, F); ctx.proxgrad_step(F, g, 1.0 / upper, x, av, y)

Nothing here is called by solvers.py: the solvers' `L=` takes a scalar, a numpy array or a device tensor as before.
The numpy twins: host_route.host_row_sqnorms / host_lipschitz, and host_smoothness below.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from . import _lib as L


class LipschitzRange(NamedTuple):
    max: float      # max_i L_i
    argmax: int     # the smallest i that attains it
    min: float      # min_i L_i


def _on_stream(ctx):
    """torch's own operations on the library's results run on the context's stream, behind the kernels that produced them (a Context
    made on a stream of its own is not torch's current stream)."""
    import contextlib
    import torch
    return torch.cuda.stream(ctx.stream) if ctx.stream is not None else contextlib.nullcontext()


def _scale(F) -> float:
    """c with L_i = c ||a_i||^2."""
    from .device import PackedF
    if not isinstance(F, PackedF) or F.loss not in (L.LOSS_LS, L.LOSS_LOGISTIC, L.LOSS_LS_COMPLEX):
        raise L.CiaoError(L.ERR_ARG, "smoothness constants exist for device.PackedF problems of LeastSquares (real or complex) or logistic "
                                     "rows: the sharing family and Zero terms have no data rows")
    return 0.25 if F.loss == L.LOSS_LOGISTIC else float(F.lam)


def lipschitz(ctx, F):
    """L_i of every local row of F -> a device N-vector of F's real dtype: F.lam ||a_i||^2 for LeastSquares rows (real and complex),
    ||a_i||^2 / 4 for logistic rows.  The norms are summed in double (Context.row_sqnorms), the product is formed in double and
    rounded to the dtype once.  Pass it as `L=` to Finito (the step sizes alpha N / L_i are then formed on the device, without a
    host copy) or to SVRG / SAGA / SAG (which take its maximum; lipschitz_max gives that without the vector).  Does not synchronise.

    A row of zeros has L_i = 0: see lipschitz_range."""
    c = _scale(F)
    with _on_stream(ctx):
        return (ctx.row_sqnorms(F) * c).to(F.dtype)


def lipschitz_range(ctx, F) -> LipschitzRange:
    """LipschitzRange(max, argmax, min) of the L_i of F's local rows, from the summary of the row pass alone (Context.row_sqnorm_stats):
    no N-vector is written or copied.  Synchronises.

    min == 0 means that some row is all zeros: its f_i is constant along every direction, L_i = 0, and Finito's per-sample step
    alpha N / L_i is +inf for that sample.  Nothing here hides that: the caller decides (drop the row, or pass a floored vector such
    as lipschitz(ctx, F).clamp_min(tiny) as `L=`).  A NaN anywhere in A makes max and min NaN, a step size derived from them NaN, and
    the solvers' own `assert gamma > 0` stops the run."""
    c = _scale(F)
    st = ctx.row_sqnorm_stats(F)
    return LipschitzRange(c * st.max, st.argmax, c * st.min)


def lipschitz_max(ctx, F) -> float:
    """max_i L_i as a float: the scalar `L=` of SAGA / SAG (gamma = 1 / (3 L), 1 / (16 L): SAGA_basic.jl:35) and of SVRG (with mu=),
    or an explicit gamma = 1 / (7 L) as test_lasso.jl:164 sets it.  From the summary of the row pass: 32 bytes cross to the host, not
    the 8 N of taking the maximum of lipschitz(ctx, F) there.  lipschitz_range(ctx, F) also has the minimum -- 0 where a row is all
    zeros, see there.  Synchronises."""
    return lipschitz_range(ctx, F).max


def _power(apply, v, iters, rtol, dot):
    """Power iteration on a symmetric positive semi-definite operator: (Rayleigh quotient of the last unit iterate, iterations made).
    Per iteration one application, one dot product (the quotient: v is a unit vector) and one norm (the next iterate).  Stops where two
    successive quotients differ by at most rtol of the later one."""
    if iters < 1:
        raise ValueError("iters must be >= 1")
    v = v / math.sqrt(dot(v, v))
    rho, prev = 0.0, None
    for k in range(int(iters)):
        w = apply(v)
        rho = dot(v, w)
        nrm = math.sqrt(dot(w, w))
        if not nrm > 0.0 or (prev is not None and abs(rho - prev) <= rtol * abs(rho)):
            return rho, k + 1
        prev = rho
        v = w / nrm
    return rho, int(iters)


def smoothness(ctx, F, iters=50, rtol=1e-6, seed=0):
    """(estimate, upper) of the smoothness constant of the AVERAGE function f = (1/N) sum_i f_i:  L_f = (c / N) lambda_max(A'A) with
    lipschitz's c: F.lam (LeastSquares rows) or 1/4 (logistic rows: sigma' <= 1/4).  This is the constant a full proximal-gradient step
    needs (Context.proxgrad_step converges for gamma < 2 / L_f), not the per-sample max_i L_i of the stochastic solvers.

    estimate: power iteration on A'A through Context.full_gradient on a LeastSquares view of the same rows with b = 0 (its gradient at
        v is A'A v / N); at most `iters` passes over A, fewer once two successive values agree to rtol; the start vector is drawn on the
        host from numpy's default_rng(seed).  It is a Rayleigh quotient, so it approaches L_f FROM BELOW: 1 / estimate may be too long
        a step.  Use it to see how loose `upper` is, or with a margin of your own.
    upper: (c / N) sum_i ||a_i||^2 = (c / N) trace(A'A) >= L_f, from the summary of the row pass (Context.row_sqnorm_stats; one more
        pass over A).  It always holds: THIS is the one that is safe to divide by (gamma = 1 / upper); it exceeds L_f by at most the
        factor rank(A).

    Real dtypes only; refused on a row-sharded context (the quotient would need all-reduces of its own).  Synchronises."""
    import torch
    from .device import PackedF
    c = _scale(F)
    if F.loss == L.LOSS_LS_COMPLEX:
        raise L.CiaoError(L.ERR_ARG, "smoothness covers real problems only (complex T: the power iteration runs on the real full-gradient pass)")
    if ctx.is_row_sharded() or F.N_total != F.N:
        raise L.CiaoError(L.ERR_ARG, "smoothness on a row-sharded context (all-reduce hook, shard table or peers): the Rayleigh quotient and "
                                     "the trace would need all-reduces of their own")
    def apply(v):
        w = torch.empty_like(v)
        ctx.full_gradient(view, v.contiguous(), w)
        return w

    with _on_stream(ctx):
        view = PackedF(L.LOSS_LS, F.A, torch.zeros(F.N, dtype=F.dtype, device=F.device), 1.0)
        v0 = torch.from_numpy(np.random.default_rng(seed).standard_normal(F.d)).to(device=F.device, dtype=F.dtype)
        rho, _ = _power(apply, v0, iters, rtol, lambda a, b: float(torch.dot(a.double(), b.double())))
    # rho estimates lambda_max(A'A) / N
    return c * rho, (c / F.N) * ctx.row_sqnorm_stats(F).sum


def host_smoothness(kind, A, lam=1.0, iters=50, rtol=1e-6, seed=0):
    """smoothness in numpy (float64) on a host matrix: the same start vector, the same iteration and stopping rule, the same trace
    bound.  kind: "ls" or "logistic"."""
    from .host_route import host_row_sqnorms
    if kind not in ("ls", "logistic"):
        raise ValueError(f"kind must be 'ls' or 'logistic' (got {kind!r})")
    A = np.asarray(A, dtype=np.float64)
    N, d = A.shape
    cN = float(lam) if kind == "ls" else 0.25
    rho, _ = _power(lambda v: A.T @ (A @ v) / N, np.random.default_rng(seed).standard_normal(d), iters, rtol, lambda a, b: float(a @ b))
    return cN * rho, (cN / N) * float(np.sum(host_row_sqnorms(A)))

"""Gap-safe feature screening for l1 problems on device rows.

For  min_x (1/N) sum_i f_i(x) + mu ||x||_1  with LeastSquares or logistic rows, the duality gap the certificate already computes
(certificate.py) bounds the distance from the dual point it uses to the dual optimum, and the optimum's column correlations decide
which coordinates are zero there.  With s and kappa from the gap,

    s |grad f(x)_j| + kappa ||A_j|| < mu      implies      x*_j = 0

for ANY x: those columns can be dropped and the problem solved on the rest.

    colsq = ctx.col_sqnorms(F)                           # one pass over A, once per dataset
    res = gap_safe(ctx, F, g, x, gamma, colsq=colsq)     # two passes over A: grad f(x), and the certificate's own pass
    F_red = restrict(F, res.keep)                        # a PackedF over the kept columns
    x_red, it = SVRG(...)(x[res.keep.bool()], F=F_red, g=g, N=N)
    x_full = expand(x_red, res.keep)

Cost of one screening: two passes over A (2 N d sizeof(T) bytes) and two d-vector reductions; the column pass (N d sizeof(T) bytes,
`tools/colsq_time.py`) is skipped with a cached `colsq`.  Nothing here is called by solvers.py; single-device contexts only.
The rule alone in numpy: host_route.host_screen.
"""
from __future__ import annotations

import math
from typing import Any, NamedTuple

from . import _lib as L


class ScreenResult(NamedTuple):
    keep: Any             # uint8 device d-vector: 0 = proven zero at the optimum
    n_kept: int
    d: int
    s: float              # the dual point's scaling, the certificate's own
    kappa: float          # the radius in front of ||A_j||
    certificate: Any      # certificate.CertificateResult at x


def _is_ls(loss):
    if loss in (L.LOSS_LS, "ls"):
        return True
    if loss in (L.LOSS_LOGISTIC, "logistic"):
        return False
    raise ValueError(f"screening covers LeastSquares and logistic rows (got loss {loss!r})")


def radius(loss, lam, N_total, cert, eps_T, mu):
    """(s, kappa) of the rule from a certificate.CertificateResult at x; host arithmetic only.

    s = 1 where grad f(x) = 0, else min(1, mu / ||grad f(x)||_inf): the scaling that makes the certificate's dual point feasible, so
    that s grad f(x)_j is column j's value AT that point.  G = max(gap, 0) + 64 eps_T objective: the gap, floored by a multiple of the
    rounding of the objective it was subtracted from -- at a computed gap of exactly 0 the support sits on |grad f_j| = mu to rounding
    and the bare rule would drop it.  LeastSquares rows (lam its weight): the dual is N / lam strongly concave,
    kappa = sqrt(2 lam G / N_total).  Logistic rows: h'' >= 4 on [0, 1], kappa = sqrt(G / (2 N_total)).  A gap that is NaN or +inf
    (no gap for this pair of f and g, F(x) unknown) gives kappa = +inf: everything is kept."""
    ls = _is_ls(loss)
    mu = float(mu)
    if not (mu > 0 and math.isfinite(mu)):
        raise ValueError("mu must be > 0 and finite")
    s = 1.0 if cert.grad_inf == 0 else min(1.0, mu / cert.grad_inf)
    G = max(cert.gap, 0.0) + 64.0 * float(eps_T) * cert.objective if not math.isnan(cert.gap) else math.nan
    if not (G < math.inf):
        return s, math.inf
    kappa = math.sqrt(2.0 * float(lam) * G / float(N_total)) if ls else math.sqrt(G / (2.0 * float(N_total)))
    return s, kappa


def _l1(ctx, F, g):
    """The device ProxG of g = NormL1(mu > 0) (packed here from an operators.NormL1), or the refusal."""
    from . import operators as Op
    from .device import PackedF, ProxG
    if not isinstance(F, PackedF) or F.loss not in (L.LOSS_LS, L.LOSS_LOGISTIC):
        raise L.CiaoError(L.ERR_ARG, "gap-safe screening covers device.PackedF problems of LeastSquares or logistic rows (no sharing family, "
                                     "no complex rows, no Zero terms)")
    if isinstance(g, Op.NormL1):
        g = Op.pack_g(g, F.d, F.dtype, F.device)
    if not isinstance(g, ProxG) or g.kind != L.PROX_L1 or not (g.lam > 0 and math.isfinite(g.lam)):
        raise L.CiaoError(L.ERR_ARG, "gap-safe screening needs g = NormL1(mu) with mu > 0 (IndBox, Zero and the complex NormL1 have no rule here)")
    if ctx.is_row_sharded() or F.N_total != F.N:
        raise L.CiaoError(L.ERR_ARG, "gap-safe screening on a row-sharded context (all-reduce hook, shard table or peers): the column "
                                     "norms and the per-sample sums would need all-reduces of their own")
    return g


def gap_safe(ctx, F, g, x, gamma, colsq=None) -> ScreenResult:
    """Screen at x: ScreenResult(keep, n_kept, d, s, kappa, certificate).  F: device.PackedF of LeastSquares or logistic rows;
    g: NormL1(mu), mu > 0 (device.ProxG or operators.NormL1); gamma: the certificate's prox-gradient step (any gamma > 0).  Two passes
    over A (grad f(x); the certificate, with its per-sample terms for logistic rows) unless colsq is None, which adds the column
    pass: cache ctx.col_sqnorms(F) per dataset.  Synchronises."""
    import torch
    g = _l1(ctx, F, g)
    grad = torch.empty(F.d, dtype=F.dtype, device=F.device)
    ctx.full_gradient(F, x, grad)
    cert = ctx.certificate(F, g, x, gamma, samples=(F.loss == L.LOSS_LOGISTIC))
    s, kappa = radius(F.loss, F.lam, F.N_total, cert, torch.finfo(F.dtype).eps, g.lam)
    if colsq is None:
        colsq = ctx.col_sqnorms(F)
    keep, n_kept = ctx.screen(grad, colsq, s, kappa, g.lam)
    return ScreenResult(keep, n_kept, F.d, s, kappa, cert)


def mu_max(ctx, F) -> float:
    """||grad f(0)||_inf: for mu at or above it the solution of the l1 problem is x = 0.  One full pass; synchronises."""
    import torch
    from .device import ProxG
    _l1(ctx, F, ProxG(L.PROX_L1, lam=1.0))
    x0 = torch.zeros(F.d, dtype=F.dtype, device=F.device)
    return ctx.certificate(F, ProxG(L.PROX_L1, lam=1.0), x0, 1.0).grad_inf


def restrict(F, keep):
    """The problem over the kept columns: a device.PackedF with A[:, keep] (a torch column gather into a fresh row-major matrix,
    ld = the kept count, as operators.pack_rows_from_host lays rows out) and F's b, lam, N_total, row ownership.  A problem whose rows
    the host mirror padded (operators.pack_F(pad_to=...): padded_from set) is padded again, with zero columns up to whole 16-byte
    chunks of the kept count.  keep: d flags (device uint8 / bool, or anything torch.as_tensor takes); at least one must be set."""
    import torch
    from .device import PackedF
    if not isinstance(F, PackedF) or F.loss not in (L.LOSS_LS, L.LOSS_LOGISTIC):
        raise L.CiaoError(L.ERR_ARG, "restrict covers device.PackedF problems of LeastSquares or logistic rows")
    real = F.padded_from if F.padded_from is not None else F.d
    k = torch.as_tensor(keep, device=F.device).reshape(-1)
    if k.numel() not in (real, F.d):
        raise ValueError(f"keep has {k.numel()} flags, the problem {real} coordinates")
    idx = torch.nonzero(k[:real] != 0).reshape(-1)
    n = int(idx.numel())
    if n < 1:
        raise ValueError("restrict needs at least one kept coordinate (an all-zero solution needs no solve)")
    vec = 16 // F.A.element_size()
    dp = (n + vec - 1) // vec * vec if F.padded_from is not None else n
    if dp == n:
        A = F.A.index_select(1, idx).contiguous()
    else:
        A = torch.zeros((F.N, dp), dtype=F.dtype, device=F.device)
        A[:, :n] = F.A.index_select(1, idx)
    out = PackedF(F.loss, A, F.b, F.lam, N_total=F.N_total, row0=F.row0, cyclic=F.cyclic)
    out.padded_from = n if dp != n else None
    return out


def expand(x_red, keep):
    """The d-vector with x_red in the kept places (in order) and zeros in the dropped ones."""
    import torch
    k = torch.as_tensor(keep, device=x_red.device).reshape(-1) != 0
    n = int(k.sum().item())
    if x_red.numel() < n:
        raise ValueError(f"x_red has {x_red.numel()} coordinates, keep has {n} set")
    out = torch.zeros(k.numel(), dtype=x_red.dtype, device=x_red.device)
    out[k] = x_red.reshape(-1)[:n]
    return out


def host_screen(grad, colsq, s, kappa, mu):
    """The rule in numpy (float64) -> a boolean keep mask: host_route.host_screen."""
    from .host_route import host_screen as _hs
    return _hs(grad, colsq, s, kappa, mu)

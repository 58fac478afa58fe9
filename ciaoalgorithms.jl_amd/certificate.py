"""Optimality certificate and solve-to-tolerance: how far is a solver's iterate from the optimum?

Every solver here runs exactly `maxit` iterations; `state.objective` tells the value reached, not its distance from the minimum.
`Context.certificate` (include/ciao_hip.h: ciao_certificate) answers with two numbers computed on the device in one pass over A and
one reduction over the d coordinates:

    residual = || x - prox_{gamma g}(x - gamma grad f(x)) || / gamma     zero exactly at a minimiser, for every loss and prox here
    gap      = F(x) + g(x) - D(theta)                                    lasso only: objective(x) - min <= gap for ANY x (weak duality)

The gap exists for LeastSquares rows with g = NormL1(mu), mu > 0: the dual point theta = s (lam/N)(Ax - b),
s = min(1, mu / ||grad f(x)||_inf), is feasible by construction and b'r = x'A'r - ||r||^2 removes every per-row quantity, so that
D = F (2s - s^2) - s x.grad f(x) needs only the numbers the d-vector reduction leaves.  For the logistic loss the dual value needs
the per-sample terms (an entropy of every margin): without them `gap` is nan and `residual` is the certificate.  With
`samples=True` the call keeps the row dots of its pass and a second reduction, over the N samples, adds them:

    gap      = F(x) + g(x) + (1/N) sum_i h(s sigma(-y_i a_i'x))         logistic rows with g = NormL1(mu), mu > 0

with h(u) = u log u + (1 - u) log(1 - u) and the lasso's s: the dual point u_i = s sigma(-t_i) is feasible by the same scaling.

    cert = Certificate(ctx, F, g, N, gamma)
    x, it = SVRG(...)(x0, F=F, g=g, N=N, stop=stop_when(cert, gap=1e-8), check_every=k)

`solvers.py` does not import this module: `stop_when` returns a plain callable for the functors' existing `stop=` keyword.
"""
from __future__ import annotations

import math
from typing import NamedTuple


class CertificateResult(NamedTuple):
    F: float               # (1/N) sum_i f_i(x)
    g: float               # g(x): NormL1's value, 0 for Zero / a feasible Box point, +inf for an infeasible one
    objective: float       # F + g
    residual: float        # || x - prox_{gamma g}(x - gamma grad f(x)) ||_2 / gamma
    grad_inf: float        # || grad f(x) ||_inf
    x_dot_grad: float      # x . grad f(x)
    box_violation: float   # max_k max(lo_k - x_k, x_k - hi_k, 0)
    gap: float             # lasso duality gap (nan where it does not apply)


def assemble(F, g_value, residual, grad_inf, x_dot_grad, box_violation, mu=None, entropy=None, n=None) -> CertificateResult:
    """The named result from the six numbers of ciao_certificate, in double.  mu: NormL1's weight when the gap applies, else None:
    for LeastSquares rows the lasso's gap; for logistic rows give also entropy = E(s), the per-sample reduction's sum of
    h(s sigma(-t_i)) at s = min(1, mu / grad_inf), and n = the number of samples: gap = F + g + E / n."""
    g = math.inf if box_violation > 0 else g_value
    gap = math.nan
    if entropy is not None:
        if mu is not None and mu > 0:
            gap = F + g + entropy / n
    elif mu is not None and mu > 0:
        s = 1.0 if grad_inf == 0 else min(1.0, mu / grad_inf)
        dual = F * (2 * s - s * s) - s * x_dot_grad
        gap = F + g - dual
    return CertificateResult(F, g, F + g, residual, grad_inf, x_dot_grad, box_violation, gap)


class Certificate:
    """cert(state) -> CertificateResult at solution(state).

    F, g, N: what the solver call takes (operator objects, or device.PackedF / device.ProxG); gamma: the prox-gradient step of the
    residual (any gamma > 0 certifies; 1 / L_max is the natural scale).  On a device state whose F came as operator objects the
    iterable's own packing of them is used (no second copy of A on the device); a host-route state (backend == "host") is answered
    in numpy by host_route.host_certificate.  ctx=None: the state's context.  samples=True: the per-sample terms too -- the duality
    gap of logistic rows with NormL1 (Context.certificate's keyword)."""

    def __init__(self, ctx, F, g, N, gamma, samples=False):
        if not (gamma > 0 and math.isfinite(gamma)):
            raise ValueError("gamma must be > 0 and finite")
        self.ctx, self.F, self.g, self.N, self.gamma, self.samples = ctx, F, g, int(N), float(gamma), bool(samples)

    def __call__(self, state) -> CertificateResult:
        from .solvers import solution
        x = solution(state)
        if getattr(state, "backend", None) == "host":
            from . import host_route as HR
            return HR.host_certificate(self.F, self.g, x, self.gamma, self.N, samples=self.samples)
        from .device import PackedF
        it = state._it
        F, g = (self.F, self.g) if isinstance(self.F, PackedF) else (it.F, it.g)
        return (self.ctx if self.ctx is not None else it.ctx).certificate(F, g, x, self.gamma, samples=self.samples)


def gaps_together(ctx, F, gs, xs, gamma):
    """[Certificate(ctx, F, g_k, N, gamma, samples=True) at x_k for k < K] from TWO passes over A in all, whatever K is: the K
    certificates of a regularisation path (one g per model: gs is a list of K device.ProxG, or one for all).

    Pass 1, Context.full_gradient_multi: the K gradients.  Then, per model and without a pass, the reduction over the d coordinates
    (ciao_certificate with av given) for the residual, ||grad f(x_k)||_inf and x_k . grad f(x_k).  Pass 2,
    Context.margin_stats_multi at s_k = min(1, mu_k / ||grad f(x_k)||_inf): F(x_k) -- the log-loss sum / N, or lam sum r^2 / (2 N)
    -- and the entropy of the logistic dual.  The gap is the lasso's (LeastSquares rows) or F + g + E / N (logistic rows) for
    g_k = NormL1(mu_k), mu_k > 0, and nan elsewhere.  Each result agrees with its single-model certificate to rounding (other orders
    of addition in both passes), not bitwise.  F: a device.PackedF; refused on a row-sharded context and for the sharing problem, as
    Certificate(samples=True) is.  Synchronises."""
    import torch
    from . import _lib as L
    from .device import PackedF
    if not isinstance(F, PackedF):
        raise L.CiaoError(L.ERR_ARG, "gaps_together covers finite sums of LeastSquares / logistic rows packed for the device (device.PackedF)")
    if ctx.is_row_sharded():
        raise L.CiaoError(L.ERR_ARG, "gaps_together on a row-sharded context: the per-sample sums would need an all-reduce of their own")
    if not (gamma > 0 and math.isfinite(gamma)):
        raise L.CiaoError(L.ERR_ARG, "gaps_together: gamma must be > 0 and finite")
    xs = list(xs)
    K = len(xs)
    gs = list(gs) if isinstance(gs, (list, tuple)) else [gs] * K
    if K < 1 or len(gs) != K:
        raise L.CiaoError(L.ERR_ARG, f"gaps_together: {K} iterates and {len(gs)} regularisers (one g per model, at least one model)")
    avs = [torch.empty_like(x) for x in xs]
    ctx.full_gradient_multi(F, xs, avs)
    parts, scal, mus = [], [], []
    for g, x, av in zip(gs, xs, avs):
        c = ctx.certificate(F, g, x, gamma, av=av)
        mu = g.lam if (g is not None and g.kind == L.PROX_L1 and g.lam > 0) else None
        parts.append(c)
        mus.append(mu)
        scal.append(1.0 if (mu is None or c.grad_inf == 0 or not c.grad_inf == c.grad_inf) else min(1.0, mu / c.grad_inf))
    stats = ctx.margin_stats_multi(F, xs, scal)
    out = []
    for c, mu, st in zip(parts, mus, stats):
        if F.loss == L.LOSS_LOGISTIC:
            out.append(assemble(st.loss_sum / F.N_total, c.g, c.residual, c.grad_inf, c.x_dot_grad, c.box_violation, mu=mu,
                                entropy=st.entropy, n=F.N_total))
        else:
            out.append(assemble(0.5 * F.lam * st.sum_r2 / F.N_total, c.g, c.residual, c.grad_inf, c.x_dot_grad, c.box_violation, mu=mu))
    return out


def stop_when(cert, gap=None, residual=None):
    """A callable for the functors' `stop=` keyword: true at the first checked state whose certificate meets EVERY bound given
    (gap <= gap, residual <= residual).  The last certificate is kept in `.last`."""
    if gap is None and residual is None:
        raise ValueError("give a bound: gap=, residual= or both")

    def stop(state):
        c = stop.last = cert(state)
        return (gap is None or c.gap <= gap) and (residual is None or c.residual <= residual)

    stop.last = None
    return stop

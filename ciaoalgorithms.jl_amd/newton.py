"""A proximal Newton method for l1-regularised logistic rows with N >> d, on the weighted Gram pass.

    minimise  Phi(x) = (1/N) sum_i log(1 + exp(-y_i a_i'x)) + mu ||x||_1

One outer iteration, everything in double:

    t = y o (A x)      p = sigma(-t)      w = p (1 - p)                  N-vector torch ops (numpy on the host): off the hot path
    H = A' diag(w) A / N                                                  ONE weighted Gram pass (ciao_gram_weighted)
    u = (N H) x - N grad f(x)                                             grad f from the existing full-gradient pass: no division by w,
                                                                          so saturated samples (w = 0) are harmless
    x^ = argmin_z (1/2N)(z'(N H) z - 2 u'z) + mu ||z||_1                  gram.lasso_path on GramStats(G = N H, u), warm-started at x, to
                                                                          a gap INNER_FACTOR below the outer one: d-space, A is not read
    Delta = x^ - x;  backtracking: the first s in 1, 1/2, 1/4 ... with
        Phi(x + s Delta) <= Phi(x) + 1e-4 s (grad f'Delta + mu ||x^||_1 - mu ||x||_1)        (Lee, Sun, Saunders 2014)
                                                                          one row_dots pass + one margin_stats reduction per trial

and stops when the logistic duality gap of section 8.7 is <= gap * max(1, objective) (converged), when the line search finds no
decrease -- no trial passes the test, or the accepted one lowered Phi by less than Phi resolves in the rows' precision (RESOLUTION)
without halving the gap either -- (converged = False, reason = "stalled": float32 rows end this way once the gap sits at the noise of
float32 dots; so does a solve whose own evaluation of the gap meets the bound while the returned certificate, another order of
addition over the same vector, does not), or after max_outer iterations (reason = "max_outer").  Per outer iteration: one weighted Gram pass, one full-gradient pass and one row-dots
pass per line-search trial (the accepted trial's dots are the next iteration's); one certificate pass at the end.

`rows` is a small protocol (vector, as64, dots, loss, gradient, hessian, certificate, stream) with two implementations: DeviceRows(ctx, F) -- Context.full_gradient, row_dots, margin_stats,
certificate(samples=True) and gram(weights=) -- and HostRows(A, y) -- numpy and host_route -- so that the driver runs end to end
without a GPU.  Both take rows=, a list of row numbers: the same problem on A[rows], y[rows] -- on the device without a gathered copy,
through Context.list_dots, list_combine and gram(rows=).  solvers.py imports nothing of this module.
"""
from __future__ import annotations

import math
from typing import NamedTuple

from . import _lib as L
from .certificate import CertificateResult, assemble
from .gram import GramStats, lasso_cd, lasso_path

INNER_FACTOR = 0.1        # the subproblem is solved to INNER_FACTOR * gap (relative to max(1, model value), as lasso_path measures it)
INNER_FORCING = 1e-3      # (intercept=True) ... and to at most this fraction of the outer iterate's own relative gap
ARMIJO = 1e-4
MAX_HALVINGS = 30
RESOLUTION = 8.0          # a decrease of Phi below RESOLUTION * eps(rows' dtype) * max(1, Phi) cannot be told from the rounding of the row
                          # dots Phi is evaluated from.  Such a step still counts while it halves the duality gap (the last steps of a
                          # float64 solve do: the gap is first-order in the distance, Phi second-order); one that does neither is no
                          # decrease the line search found, and the solve has stalled
HOST_SUBPROBLEM_D = 2048  # up to this d the d x d subproblem is solved on the host (thousands of tiny products: launch-bound on a GPU)


class Passes(NamedTuple):
    gram: int          # weighted Gram passes (N d^2 flops each)
    first_order: int   # full-gradient, row-dots and certificate passes (N d elements read each); for DeviceRows(rows=) the list passes
                       # made (Context.list_dots / list_combine): M d elements each, M / N of a pass over A; and the Gram passes likewise


class NewtonResult(NamedTuple):
    x: object                       # the iterate, in the rows' own form: a device d-vector of F's dtype / a numpy d-vector of A's dtype
    certificate: CertificateResult  # rows.certificate at exactly that vector
    outer: int                      # outer iterations made (weighted Gram passes)
    passes: Passes
    converged: bool                 # certificate.gap <= gap * max(1, certificate.objective)
    reason: str                     # "gap", "stalled" or "max_outer"
    intercept: float = 0.0          # logistic_newton(intercept=True): the unpenalised intercept c; 0.0 without one


def _sigmoid_weights(t):
    """w = sigma(-t) (1 - sigma(-t)) without overflow, for a float64 torch vector t"""
    import torch
    e = torch.exp(-t.abs())
    return e / ((1.0 + e) * (1.0 + e))


class DeviceRows:
    """Logistic rows packed for the device: F = device.PackedF.logistic(A, y) on ctx (float32 or float64 rows, d <= 4096); refused on
    a row-sharded context.

    rows: None (every row of F: the calls, and the bits, of the full passes), or a contiguous int64 device vector of M >= 1 row numbers
    in [0, N) -- any order, repeats allowed (a training fold, a bootstrap resample): the logistic problem on A[rows], y[rows] WITHOUT a
    gathered copy.  Then N = M; dots is Context.list_dots (a float64 M-vector); gradient(x) is
    Context.list_combine(c) / M with c_m = -y_m sigma(-y_m dots_m) formed in float64 torch on the M-vector, as the weights of hessian
    are; hessian is Context.gram(weights=, rows=); loss is the four logistic numbers of host_route.host_margin_stats by the same stable
    evaluation in float64 torch against F.b[rows]; certificate is _certificate from one gradient and one dots pass.  The list is
    checked against [0, N) once, here.  The row dots of the vector last passed to dots() are kept, so that gradient() and
    certificate() at that same (unmodified) tensor do not read the rows again; list_passes counts the list passes made
    (Passes.first_order reports them: each costs M / N of a pass over A)."""

    def __init__(self, ctx, F, rows=None):
        from .device import PackedF
        if not isinstance(F, PackedF) or F.loss != L.LOSS_LOGISTIC:
            raise L.CiaoError(L.ERR_ARG, "DeviceRows takes a device.PackedF of logistic rows (PackedF.logistic)")
        if ctx.is_row_sharded() or F.N_total != F.N:
            raise L.CiaoError(L.ERR_ARG, "DeviceRows on a row-sharded context: the ranks' weighted Gram matrices are not combined")
        if F.N < 1:
            raise L.CiaoError(L.ERR_ARG, "DeviceRows needs at least one row (N = 0)")
        self.ctx, self.F = ctx, F
        self.N, self.d, self.dtype, self.device = int(F.N), int(F.d), F.dtype, F.A.device
        self.rows, self.list_passes = None, None
        if rows is not None:
            rows, M = ctx._row_list(F, rows, True, "DeviceRows")
            if M < 1:
                raise L.CiaoError(L.ERR_ARG, "DeviceRows needs at least one row (an empty list)")
            self.rows, self.N, self.list_passes = rows, M, 0
            with self.stream():
                self.y = F.b[rows].double()
            self._kept = None   # (x, its version, its row dots)

    def stream(self):
        """torch's own operations on these rows' vectors run inside this: on the context's stream, behind the kernels that produced
        their inputs and ahead of the kernels that read their results (a Context made on a stream of its own is not torch's current
        stream).  Every method below enters it itself; the driver keeps it for its whole iteration."""
        import torch
        from .stepsize import _on_stream
        if self.ctx.stream is not None and torch.cuda.current_stream(self.device) != self.ctx.stream:
            self.ctx.stream.wait_stream(torch.cuda.current_stream(self.device))   # what the caller queued (an x0) comes first
        return _on_stream(self.ctx)

    def vector(self, x64):
        with self.stream():
            return x64.to(device=self.device, dtype=self.dtype).contiguous()

    def as64(self, x):
        import torch
        with self.stream():
            return torch.as_tensor(x).to(device=self.device, dtype=torch.float64)

    def dots(self, x):
        if self.rows is None:
            return self.ctx.row_dots(self.F, x)
        kept = self._kept
        if kept is not None and kept[0] is x and kept[1] == x._version:
            return kept[2]
        with self.stream():
            out = self.ctx.list_dots(self.F, x, rows=self.rows, check_rows=False)
        self.list_passes += 1
        self._kept = (x, x._version, out)
        return out

    def loss(self, dots, s=1.0):
        if self.rows is None:
            st = self.ctx.margin_stats(self.F, dots, s)
            return st.loss_sum / self.N, st.entropy
        from .scoring import margin_stats_torch
        with self.stream():
            st = margin_stats_torch("logistic", dots, self.y, s)
        return st[0] / self.N, st[1]

    def gradient(self, x):
        import torch
        if self.rows is None:
            with self.stream():                    # (av is allocated on the stream that writes and reads it)
                av = torch.empty_like(x)
                self.ctx.full_gradient(self.F, x, av)
                return av.double()
        dots = self.dots(x)
        with self.stream():
            t = self.y * dots
            e = torch.exp(-t.abs())
            p = torch.where(t >= 0, e / (1.0 + e), 1.0 / (1.0 + e))           # sigma(-t)
            g = self.ctx.list_combine(self.F, -self.y * p, rows=self.rows, check_rows=False)
            self.list_passes += 1
            return g / self.N

    def hessian(self, dots):
        with self.stream():
            if self.rows is None:
                w = _sigmoid_weights(self.F.b.double() * dots.double())
                return self.ctx.gram(self.F, u=None, colsum=None, bsum=None, weights=w)[0]
            w = _sigmoid_weights(self.y * dots)
            return self.ctx.gram(self.F, u=None, colsum=None, bsum=None, weights=w, rows=self.rows, check_rows=False)[0]

    def certificate(self, x, mu, gamma):
        if self.rows is None:
            from .device import ProxG
            return self.ctx.certificate(self.F, ProxG(L.PROX_L1, lam=mu), x, gamma, samples=True)
        with self.stream():
            return _certificate(self, self.as64(x), self.gradient(x), self.dots(x), mu, gamma)

    # -- the intercept route: the list-route formulation for rows=None too -- float64 vectors by list position
    def labels64(self):
        if self.rows is not None:
            return self.y
        if getattr(self, "_y64", None) is None:      # (one float64 copy of the labels, made once: loss64 asks for it at every trial)
            with self.stream():
                self._y64 = self.F.b.double()
        return self._y64

    def dots64(self, x):
        with self.stream():
            return self.ctx.list_dots(self.F, x, rows=self.rows, check_rows=False)

    def combine64(self, coeff):
        with self.stream():
            return self.ctx.list_combine(self.F, coeff.contiguous(), rows=self.rows, check_rows=False)

    def loss64(self, margins, s=1.0):
        from .scoring import margin_stats_torch
        with self.stream():
            st = margin_stats_torch("logistic", margins, self.labels64(), s)
        return st[0] / self.N, st[1]

    def hessian_aug(self, w):
        """(A'diag(w)A, A'w, sum w) from ONE weighted Gram pass: its colsum and the third element of its bsum"""
        with self.stream():
            G, _, colsum, bsum = self.ctx.gram(self.F, u=None, colsum=True, bsum=True, weights=w.contiguous(), rows=self.rows, check_rows=False)
            return G, colsum, bsum[2]


class HostRows:
    """The same rows on the host: A a real N x d numpy matrix (float32 or float64), y its N labels (+-1).  Row dots and the gradient
    are formed in A's dtype, as the device forms them; the statistics and the weighted Gram matrix (host_route.host_gram) in double.

    rows: None, or an integer vector of M >= 1 row numbers in [0, N), any order, repeats allowed: the problem on the gathered copies
    A[rows], y[rows] -- bit for bit HostRows(A[rows], y[rows])."""

    def __init__(self, A, y, rows=None):
        import numpy as np
        import torch
        A, y = np.asarray(A), np.asarray(y)
        if A.ndim != 2 or A.dtype not in (np.float32, np.float64) or y.shape != (A.shape[0],) or A.shape[0] < 1:
            raise ValueError("HostRows: A must be a float32 / float64 N x d matrix with N >= 1 and y an N-vector")
        if rows is not None:
            rows = np.asarray(rows.cpu() if hasattr(rows, "cpu") else rows)
            if rows.ndim != 1 or not np.issubdtype(rows.dtype, np.integer) or rows.size < 1:
                raise ValueError("HostRows: rows must be an integer vector of at least one row number")
            if rows.min() < 0 or rows.max() >= A.shape[0]:
                raise ValueError(f"rows: entries must lie in [0, {A.shape[0]})")
            A, y = A[rows], y[rows]
        self.A, self.y = A, y.astype(A.dtype)
        self.N, self.d = A.shape
        self.dtype, self.device = (torch.float32 if A.dtype == np.float32 else torch.float64), torch.device("cpu")

    def stream(self):
        import contextlib
        return contextlib.nullcontext()

    def vector(self, x64):
        return x64.detach().cpu().numpy().astype(self.A.dtype)

    def as64(self, x):
        import numpy as np
        import torch
        return torch.from_numpy(np.array(x.detach().cpu() if hasattr(x, "detach") else x, dtype=np.float64).reshape(-1))

    def dots(self, x):
        return self.A @ x

    def loss(self, dots, s=1.0):
        from .host_route import host_margin_stats
        st = host_margin_stats("logistic", dots, self.y, s)
        return st[0] / self.N, st[1]

    def gradient(self, x):
        import numpy as np
        import torch
        t = (self.y * (self.A @ x)).astype(np.float64)
        e = np.exp(-np.abs(t))
        p = np.where(t >= 0, e / (1.0 + e), 1.0 / (1.0 + e))           # sigma(-t)
        c = (-(self.y.astype(np.float64)) * p / self.N).astype(self.A.dtype)
        return torch.from_numpy((self.A.T @ c).astype(np.float64))

    def hessian(self, dots):
        import numpy as np
        import torch
        from .host_route import host_gram
        t = self.y.astype(np.float64) * np.asarray(dots, np.float64)
        w = _sigmoid_weights(torch.from_numpy(t)).numpy()
        return torch.from_numpy(host_gram(self.A, self.y, w)[0])

    def certificate(self, x, mu, gamma):
        return _certificate(self, self.as64(x), self.gradient(x), self.dots(x), mu, gamma)

    # -- the intercept route, as DeviceRows: float64 CPU tensors
    def labels64(self):
        import numpy as np
        import torch
        return torch.from_numpy(self.y.astype(np.float64))

    def dots64(self, x):
        import numpy as np
        import torch
        return torch.from_numpy((self.A @ x).astype(np.float64))

    def combine64(self, coeff):
        import numpy as np
        import torch
        return torch.from_numpy(self.A.astype(np.float64).T @ coeff.numpy())

    def loss64(self, margins, s=1.0):
        import numpy as np
        from .host_route import host_margin_stats
        st = host_margin_stats("logistic", margins.numpy(), self.y.astype(np.float64), s)
        return st[0] / self.N, st[1]

    def hessian_aug(self, w):
        import torch
        from .host_route import host_gram
        G, _, colsum, bsum = host_gram(self.A, self.y, w.numpy())
        return torch.from_numpy(G), torch.from_numpy(colsum), torch.as_tensor(bsum[2], dtype=torch.float64)


def _certificate(rows, x64, grad, dots, mu, gamma):
    """The certificate of section 8.7 at x from its gradient (float64 d-vector) and its row dots: one margin_stats reduction at
    s = min(1, mu / ||grad||_inf), no pass over A."""
    import torch
    ginf = float(grad.abs().max())
    s = 1.0 if ginf == 0 else min(1.0, mu / ginf)
    F, entropy = rows.loss(dots, s)
    v = x64 - gamma * grad
    res = x64 - torch.sign(v) * torch.clamp(v.abs() - gamma * mu, min=0.0)
    return assemble(F, mu * float(x64.abs().sum()), float(res.norm()) / gamma, ginf, float(x64 @ grad), 0.0, mu=mu,
                    entropy=entropy, n=rows.N)


def _model_stats(rows, G, u, device):
    """GramStats of the quadratic model (1/2N)(z'G z - 2 u'z + c) as a least-squares problem: c = u'G^+ u, the smallest constant for
    which [[G, u], [u', c]] is positive semidefinite, so that lasso_path's duality gap is a gap of this model (u lies in the range of G up
    to the samples whose weight underflowed; components of u along eigenvalues below 2^-40 lambda_max are left out of c)."""
    import torch
    G, u = G.to(device), u.to(device)
    lam, Q = torch.linalg.eigh(G)
    keep = lam > lam[-1] * 2.0 ** -40
    c = float((((Q.T @ u)[keep]) ** 2 / lam[keep]).sum()) if bool(keep.any()) else 0.0
    return GramStats(rows.N, rows.d, G, u, torch.zeros_like(u), 0.0, c, 1.0, "ls", torch.float64)


def _start_intercept(y, bound=math.inf) -> float:
    """log(n+ / n-) of the labels y (a float64 vector of +-1), clipped to +-bound: the intercept that minimises the loss at x = 0"""
    n_pos = int((y > 0).sum())
    n_neg = int(y.numel()) - n_pos
    if n_pos == 0 or n_neg == 0:
        raise ValueError("an intercept needs both classes among the labels (all labels are equal: the loss has no minimiser in c)")
    return max(-bound, min(bound, math.log(n_pos / n_neg)))


def _sigma_neg(t):
    """sigma(-t) without overflow, for a float64 torch vector t"""
    import torch
    e = torch.exp(-t.abs())
    return torch.where(t >= 0, e / (1.0 + e), 1.0 / (1.0 + e))


def _refine_intercept(y, dots, c, bound, iters=8) -> float:
    """The minimiser over |c| <= bound of the loss at fixed row dots, from c, by Newton's method in one variable on the float64
    M-vectors (no pass over A): a step is kept only while the loss does not rise.  The gap's box term is bound * s * |g_c|, so the
    unpenalised coordinate is worth solving to the rounding of its own gradient, which the d-space subproblem's gap does not ask for."""
    import torch

    def loss(cc):
        t = y * (dots + cc)
        return float((torch.clamp(-t, min=0.0) + torch.log1p(torch.exp(-t.abs()))).mean())

    f = loss(c)
    for _ in range(iters):
        theta = _sigma_neg(y * (dots + c))
        g, h = -float((y * theta).mean()), float((theta * (1.0 - theta)).mean())
        if not h > 0:
            break
        cn = max(-bound, min(bound, c - g / h))
        if cn == c:
            break
        fn = loss(cn)
        if not fn <= f:
            break
        c, f = cn, fn
    return c


def logistic_mu_max(rows, intercept=False) -> float:
    """||grad f(0)||_inf = ||A'y||_inf / (2 N): the smallest l1 weight at which x = 0 minimises Phi.  One full-gradient pass.

    intercept=True: ||A'(y o sigma(-y c0))||_inf / N at c0 = log(n+ / n-), the l1 weight from which on x = 0, c = c0 minimises the
    problem with an intercept.  One list_combine pass."""
    import torch
    with rows.stream():
        if intercept:
            y = rows.labels64()
            c0 = _start_intercept(y)
            return float(rows.combine64(y * _sigma_neg(y * c0)).abs().max()) / rows.N
        return float(rows.gradient(rows.vector(torch.zeros(rows.d, dtype=torch.float64))).abs().max())


def _newton_intercept(rows, mu, x0, c_start, gap, max_outer, gamma, bound) -> NewtonResult:
    """logistic_newton(intercept=True): the iteration of this module's header on (x, c), |c| <= bound, c unpenalised (DESIGN.md section
    8.18).  Margins dots(x) + c, the gradient as list_combine of the float64 coefficients -y o theta and their sum, the model matrix
    [[G, A'w], [w'A, sum w]] from one weighted Gram pass, the subproblem by gram.lasso_cd with penalty factor 0 and the box on the last
    coordinate.  After an accepted step c is minimised exactly at the new row dots (_refine_intercept: M-vector operations, no pass).
    The certificate is section 8.7's plus bound * s * |g_c|; it is formed at every iterate, so the returned one costs no further pass."""
    import types
    import torch
    C = float(bound)
    with rows.stream():
        y = rows.labels64()
        N, d = rows.N, rows.d
        c = _start_intercept(y, C) if c_start is None else max(-C, min(C, float(c_start)))
        x = rows.vector(torch.zeros(d, dtype=torch.float64) if x0 is None else rows.as64(x0))
        eps = float(torch.finfo(rows.dtype).eps)
        n_gram = n_first = outer = 0
        dots = rows.dots64(x)
        n_first += 1
        dev = dots.device
        pf = torch.ones(d + 1, dtype=torch.float64, device=dev)
        pf[d] = 0.0
        lo = torch.full((d + 1,), -math.inf, dtype=torch.float64, device=dev)
        hi = torch.full((d + 1,), math.inf, dtype=torch.float64, device=dev)
        lo[d], hi[d] = -C, C
        shape = types.SimpleNamespace(N=N, d=d + 1)
        last, reason = None, "max_outer"
        while True:
            x64 = rows.as64(x)
            margins = dots + c
            theta = _sigma_neg(y * margins)
            coeff = -y * theta
            grad = rows.combine64(coeff) / N
            n_first += 1
            g_c = float(coeff.sum()) / N
            ginf = float(grad.abs().max())
            s = 1.0 if ginf == 0 else min(1.0, mu / ginf)
            F, entropy = rows.loss64(margins, s)
            v = x64 - gamma * grad
            res = x64 - torch.sign(v) * torch.clamp(v.abs() - gamma * mu, min=0.0)
            res_c = c - max(-C, min(C, c - gamma * g_c))
            cert = assemble(F, mu * float(x64.abs().sum()), math.hypot(float(res.norm()), res_c) / gamma, ginf, float(x64 @ grad), 0.0, mu=mu,
                            entropy=entropy, n=N)
            cert = cert._replace(gap=cert.gap + C * s * abs(g_c))
            if cert.gap <= gap * max(1.0, cert.objective):
                reason = "gap"
                break
            if last is not None and last.objective - cert.objective <= RESOLUTION * eps * max(1.0, abs(last.objective)) and not cert.gap <= 0.5 * last.gap:
                reason = "stalled"
                break
            last = cert
            if outer >= max_outer:
                break
            G, colsum, sw = rows.hessian_aug(_sigmoid_weights(y * margins))
            n_gram += 1
            outer += 1
            Ga = torch.empty((d + 1, d + 1), dtype=torch.float64, device=dev)
            Ga[:d, :d] = G
            Ga[:d, d] = colsum
            Ga[d, :d] = colsum
            Ga[d, d] = sw
            z64 = torch.cat([x64, torch.tensor([c], dtype=torch.float64, device=dev)])
            ga = torch.cat([grad, torch.tensor([g_c], dtype=torch.float64, device=dev)])
            u = Ga @ z64 - N * ga
            model = _model_stats(shape, Ga, u, dev)
            # the subproblem's gap: INNER_FACTOR * gap, and never above INNER_FORCING of the relative gap the iterate has now -- the model's
            # certificate and this one are formed at different dual points, and over the last steps the first is all that is left of the second
            inner = min(INNER_FACTOR * gap, INNER_FORCING * cert.gap / max(1.0, cert.objective))
            zhat = lasso_cd(model, [mu], x0=z64, gap=inner, ctx=getattr(rows, "ctx", None), dtype=torch.float64, penalty_factor=pf,
                            lower=lo, upper=hi).x[0]
            delta = zhat - z64
            dx, dc = delta[:d], float(delta[d])
            decrease = float(grad @ dx) + g_c * dc + mu * (float(zhat[:d].abs().sum()) - float(x64.abs().sum()))
            accepted = False
            # Phi is evaluated to RESOLUTION * eps * max(1, Phi) at best: a trial within that of the Armijo bound passes it (the last steps
            # of a solve lower Phi by less than it resolves and still halve the gap; the stall rule above judges the step that does not)
            slack = RESOLUTION * eps * max(1.0, abs(cert.objective))
            if decrease < slack:      # (the predicted decrease of such a last step is itself a difference below what its terms resolve)
                step = 1.0
                for _ in range(MAX_HALVINGS):
                    xt = rows.vector(x64 + step * dx)
                    ct = max(-C, min(C, c + step * dc))
                    dt = rows.dots64(xt)
                    n_first += 1
                    phi = rows.loss64(dt + ct)[0] + mu * float(rows.as64(xt).abs().sum())
                    if phi <= cert.objective + ARMIJO * step * decrease + slack:
                        x, c, dots, accepted = xt, _refine_intercept(y, dt, ct, C), dt, True
                        break
                    step *= 0.5
            if not accepted:
                reason = "stalled"
                break
        converged = reason == "gap"
    return NewtonResult(x, cert, outer, Passes(n_gram, n_first), converged, reason, c)


def logistic_newton(rows, mu, x0=None, gap=1e-9, max_outer=30, gamma=1.0, subproblem_device=None, subproblem="fista", intercept=False,
                    intercept_bound=32.0, intercept0=None) -> NewtonResult:
    """Minimise (1/N) sum_i log(1 + exp(-y_i a_i'x)) + mu ||x||_1 over rows (DeviceRows or HostRows) by the proximal Newton
    iteration of this module's header -> NewtonResult.  mu > 0; x0: None (zeros) or a d-vector; gap: the relative duality gap asked
    for; gamma: the step of the certificate's prox residual (reported only); subproblem_device: where the d x d lasso is solved
    (None: the host up to d = 2048, the rows' device beyond).

    subproblem: "fista" (the default: gram.lasso_path) or "cd": gram.lasso_cd, coordinate descent on the model's Gram matrix (DESIGN.md
    section 8.14) -- on the device kernel, where G already lies, when the rows are DeviceRows (subproblem_device is then not used), and
    in numpy for HostRows.

    intercept=True: minimise over x and an unpenalised intercept c, |c| <= intercept_bound (finite: an
    unbounded unpenalised coordinate has no finite dual point in general),
        (1/N) sum_i log(1 + exp(-y_i (a_i'x + c))) + mu ||x||_1
    -> NewtonResult.intercept = c; the certificate's gap carries the box's term intercept_bound * s * |g_c|, its residual the
    projected-gradient residual of c, its grad_inf and x_dot_grad are statistics of x alone.  The subproblem is gram.lasso_cd with
    penalty factor 0 on c (subproblem="cd"; "fista" takes no penalty factors and is refused), so d + 1 <= 4096.  The start is x0 (None:
    zeros) and intercept0 (None: log(n+ / n-)), clipped into the bound; labels that are all equal are refused.  With intercept=False
    nothing changes and the result's intercept is 0.0; intercept0 without intercept=True is refused.  subproblem_device is not used on
    the intercept route (the subproblem runs where lasso_cd runs it: the device kernel for DeviceRows, numpy for HostRows)."""
    import torch
    mu = float(mu)
    if not (mu > 0 and math.isfinite(mu)):
        raise ValueError("logistic_newton needs an l1 weight mu > 0 and finite")
    if subproblem not in ("fista", "cd"):
        raise ValueError(f"subproblem must be 'fista' or 'cd' (got {subproblem!r})")
    if not (gap > 0 and max_outer >= 0):
        raise ValueError("gap must be > 0 and max_outer >= 0")
    if intercept0 is not None and not intercept:
        raise ValueError("intercept0 is the start of the intercept: it needs intercept=True")
    if intercept:
        if subproblem != "cd":
            raise ValueError("intercept=True needs subproblem='cd': FISTA takes no penalty factors, and the intercept is unpenalised")
        if not (intercept_bound > 0 and math.isfinite(intercept_bound)):
            raise ValueError("intercept_bound must be > 0 and finite (an unbounded unpenalised coordinate has no finite dual point)")
        if rows.d + 1 > 4096:
            raise ValueError(f"intercept=True needs d + 1 <= 4096 coordinates in the subproblem (got d = {rows.d})")
        return _newton_intercept(rows, mu, x0, intercept0, gap, max_outer, gamma, intercept_bound)
    sub = torch.device(subproblem_device) if subproblem_device is not None else (torch.device("cpu") if rows.d <= HOST_SUBPROBLEM_D else rows.device)
    # every torch operation of the iteration -- the vectors between the library's calls, G x, the line search's trial points -- runs on
    # the rows' stream (DeviceRows.stream): in order with the kernels on either side of it, whatever torch's current stream is
    with rows.stream():
        x = rows.vector(torch.zeros(rows.d, dtype=torch.float64) if x0 is None else rows.as64(x0))
        eps = float(torch.finfo(rows.dtype).eps)
        n_gram = n_first = outer = 0
        list_passes0 = getattr(rows, "list_passes", None)
        last = None
        dots = rows.dots(x)
        n_first += 1
        reason = "max_outer"
        while True:
            x64 = rows.as64(x)
            grad = rows.gradient(x)
            n_first += 1
            cert = _certificate(rows, x64, grad, dots, mu, gamma)
            if cert.gap <= gap * max(1.0, cert.objective):
                reason = "gap"
                break
            if last is not None and last.objective - cert.objective <= RESOLUTION * eps * max(1.0, abs(last.objective)) and not cert.gap <= 0.5 * last.gap:
                reason = "stalled"
                break
            last = cert
            if outer >= max_outer:
                break
            G = rows.hessian(dots)
            n_gram += 1
            outer += 1
            u = G @ x64 - rows.N * grad
            if subproblem == "cd":
                model = _model_stats(rows, G, u, G.device)
                xhat = lasso_cd(model, [mu], x0=x64, gap=INNER_FACTOR * gap, ctx=getattr(rows, "ctx", None), dtype=torch.float64).x[0]
            else:
                model = _model_stats(rows, G, u, sub)
                xhat = lasso_path(model, [mu], x0=x64.to(sub), gap=INNER_FACTOR * gap, dtype=torch.float64).x[0].to(x64.device)
            delta = xhat - x64
            decrease = float(grad @ delta) + mu * (float(xhat.abs().sum()) - float(x64.abs().sum()))
            accepted = False
            if decrease < 0:
                s = 1.0
                for _ in range(MAX_HALVINGS):
                    xt = rows.vector(x64 + s * delta)
                    dt = rows.dots(xt)
                    n_first += 1
                    phi = rows.loss(dt)[0] + mu * float(rows.as64(xt).abs().sum())
                    if phi <= cert.objective + ARMIJO * s * decrease:
                        x, dots, accepted = xt, dt, True
                        break
                    s *= 0.5
            if not accepted:
                reason = "stalled"
                break
        final = rows.certificate(x, mu, gamma)
        n_first += 1
        if list_passes0 is not None:   # rows over a list count their own passes (a gradient at a new vector is two, at a kept one one)
            n_first = rows.list_passes - list_passes0
        converged = bool(final.gap <= gap * max(1.0, final.objective))
        if reason == "gap" and not converged:
            # the iteration's own evaluation of the gap (full gradient + margin statistics) met the bound and the certificate's pass over the
            # same vector does not: two orders of addition differ by more than the gap asked for -- it lies below the noise of the rows' type
            reason = "stalled"
    return NewtonResult(x, final, outer, Passes(n_gram, n_first), converged, reason)


def logistic_path(rows, mus, x0=None, gap=1e-9, max_outer=30, gamma=1.0, subproblem_device=None, subproblem="fista", intercept=False,
                  intercept_bound=32.0) -> list:
    """logistic_newton for every l1 weight of `mus`, in the given order, each solve warm-started from the one before (the first from
    x0) -> a list of NewtonResult.  A decreasing sequence from logistic_mu_max(rows) down is the regularisation path.  intercept,
    intercept_bound: logistic_newton's; the warm starts carry the intercept too."""
    out = []
    c0 = None
    for mu in mus:
        r = logistic_newton(rows, mu, x0=x0, gap=gap, max_outer=max_outer, gamma=gamma, subproblem_device=subproblem_device, subproblem=subproblem,
                            intercept=intercept, intercept_bound=intercept_bound, intercept0=c0)
        out.append(r)
        x0 = r.x
        c0 = r.intercept if intercept else None
    return out

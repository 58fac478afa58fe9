"""Second-order statistics of a packed matrix, and what follows from them without reading the matrix again.

One pass over the rows on the matrix cores (include/ciao_hip.h: ciao_gram; csrc/gram_kernels.h) leaves G = A'A, u = A'b, A'1, sum b and
sum b^2 in double.  From these d x d numbers alone:

    st = gram_stats(ctx, F)                                  # the one pass over A
    L_f = smoothness_exact(st)                               # lam lambda_max(G) / N: the constant stepsize.smoothness brackets
    q = GramLasso(st)                                        # LeastSquares rows: grad f(x) = lam (G x - u) / N, F(x), certified gaps
    path = lasso_path(st, [mu_max(st) * 0.5 ** k for k in range(1, 9)])
    solve_together(..., x0=path.x)                           # exact warm starts; score_many(ctx, F_val, path.x) takes them as they are
    st_std, sc = st.standardized()                           # the statistics of the standardised columns, A untouched

Everything past gram_stats works on torch tensors of ANY device (GramStats.to moves them): a d x d problem is often best solved on
the host, and the CPU tests feed these functions host_route.host_gram's numbers.  Nothing here is called by solvers.py.
"""
from __future__ import annotations

import math
from typing import NamedTuple

from . import _lib as L
from .certificate import CertificateResult, assemble

AMPLIFICATION_LIMIT = 2.0 ** 10   # standardize.REFINE_RATIO: beyond it, standardise the matrix itself
EPS = 2.0 ** -53


class GramStats(NamedTuple):
    N: int            # rows summed
    d: int
    G: object         # (d, d) float64 tensor, A'A, symmetric to the bit
    u: object         # (d,) float64, A'b (b: LeastSquares targets, logistic labels)
    colsum: object    # (d,) float64, A'1
    sum_b: float
    sum_bb: float
    lam: float        # LeastSquares(a, b, lam)'s lam; 1.0 for logistic rows
    kind: str         # "ls" or "logistic"
    dtype: object = None   # the dtype of the rows the statistics came from (lasso_path returns iterates in it); None: float64
    sum_w: float = None    # weighted statistics (gram_stats(weights=)): sum of the weights; None: unweighted, to be read as N

    def to(self, device):
        """The same statistics with their tensors on another device."""
        return self._replace(G=self.G.to(device), u=self.u.to(device), colsum=self.colsum.to(device))

    def standardized(self, center=True, scale=True):
        """The statistics the standardised matrix WOULD have -> (GramStats, standardize.Scaler), from G, A'1 and N alone:

            mean_j = colsum_j / N        var_j = G_jj / N - mean_j^2        scale_j = 1 / sqrt(var_j), and 1 where var_j = 0
            G_std = D (G - N mean mean') D        u_std = D (u - mean sum_b)        D = diag(scale)

        (center=False: no mean is taken off; scale=False: D = I).  LeastSquares targets are centred with the columns, as
        standardize.standardize centres them: sum_b becomes 0 and sum_bb loses sum_b^2 / N; logistic labels stay.  The Scaler maps
        solutions back (Scaler.coefficients) and carries `amplification`, a float64 d-vector: G_jj / (N var_j) = 1 + mean_j^2 / var_j,
        the factor by which the subtraction G_jj - N mean_j^2 magnifies G's own rounding.  A column whose mean is a
        thousand standard deviations loses twenty bits here.  Where the amplification of some column exceeds 2^10
        (AMPLIFICATION_LIMIT, the rule of section 8.10), standardise the matrix itself -- standardize.standardize, which subtracts the
        mean from every entry before anything is squared -- and take gram_stats of the result.

        Weighted statistics (sum_w is not None) are REFUSED: weighted column moments would divide by sum w where N stands here, and
        with weights of both signs that variance has no sign; standardise the matrix itself (standardize.standardize), or take the
        statistics of the standardised rows with the same weights."""
        import torch
        from .standardize import Scaler
        if self.sum_w is not None:
            raise L.CiaoError(L.ERR_ARG, "standardized() is defined for unweighted statistics only: these carry a weight per row "
                                         "(sum_w is set); standardise the matrix itself and take its weighted statistics")
        n = float(self.N)
        G, u = self.G, self.u
        mean = self.colsum / n
        diag = torch.diagonal(G)
        var = torch.clamp(diag / n - mean * mean, min=0.0)
        amp = torch.where(var > 0, diag / (n * var), torch.where(diag > 0, torch.full_like(var, math.inf), torch.ones_like(var)))
        sc = torch.where(var > 0, 1.0 / torch.sqrt(var), torch.ones_like(var)) if scale else torch.ones_like(var)
        sum_b, sum_bb, colsum = self.sum_b, self.sum_bb, self.colsum
        b_mean = 0.0
        if center:
            G = G - n * torch.outer(mean, mean)   # (outer's products commute: still symmetric to the bit)
            u = u - mean * sum_b
            colsum = torch.zeros_like(colsum)
            if self.kind == "ls":
                b_mean = sum_b / n
                sum_bb = max(sum_bb - sum_b * sum_b / n, 0.0)
                sum_b = 0.0
        else:
            mean = torch.zeros_like(mean)
        G = G * torch.outer(sc, sc)               # (one product per entry, with a symmetric factor: symmetric to the bit)
        scaler = Scaler(mean, sc, b_mean, center, scale)
        scaler.amplification = amp
        return self._replace(G=G, u=sc * u, colsum=sc * colsum, sum_b=sum_b, sum_bb=sum_bb), scaler


def gram_stats(ctx, F, weights=None, rows=None) -> GramStats:
    """One pass over the rows of F (Context.gram) -> GramStats on F's device.  F: a device.PackedF of real LeastSquares or logistic rows
    with d <= 4096; refused on a row-sharded context (the ranks' matrices would have to be added).  Synchronises (the two sums of b
    cross to the host).

    weights: a float64 device N-vector w (Context.gram(weights=)) -> the weighted statistics: G = A'diag(w)A,
    u = A'(w b), colsum = A'w, sum_b = sum w b, sum_bb = sum w b^2, sum_w = sum w.  N stays the row count, so the objective GramLasso
    evaluates is lam / (2 N) sum_i w_i (a_i'x - b_i)^2; GramLasso, lasso_path and mu_max take such statistics as they are (sample
    weights; with 0/1 weights a fold of a cross-validation without copying rows).  Weights of both signs are summed faithfully, but the
    lasso functions assume G positive semidefinite.

    rows: a contiguous int64 device vector of M >= 1 row numbers (Context.gram(rows=)) -> the statistics of
    A[rows], b[rows] at the cost of the rows touched, with N = M; weights then has M elements."""
    from .device import PackedF
    from .stepsize import _on_stream
    if not isinstance(F, PackedF) or F.loss not in (L.LOSS_LS, L.LOSS_LOGISTIC):
        raise L.CiaoError(L.ERR_ARG, "gram_stats covers device.PackedF problems of real LeastSquares or logistic rows: complex rows, the "
                                     "sharing family and Zero terms have no Gram statistics here")
    if ctx.is_row_sharded() or F.N_total != F.N:
        raise L.CiaoError(L.ERR_ARG, "gram_stats on a row-sharded context (all-reduce hook, shard table, peers or a row shard): the ranks' "
                                     "Gram matrices are not combined")
    if F.N < 1:
        raise L.CiaoError(L.ERR_ARG, "gram_stats needs at least one row (N = 0)")
    if rows is not None and int(rows.shape[0]) < 1:
        raise L.CiaoError(L.ERR_ARG, "gram_stats needs at least one row (an empty list)")
    G, u, colsum, bsum = ctx.gram(F, weights=weights, rows=rows)
    with _on_stream(ctx):
        sb = bsum.cpu()
    ls = F.loss == L.LOSS_LS
    return GramStats(int(F.N) if rows is None else int(rows.shape[0]), int(F.d), G, u, colsum, float(sb[0]), float(sb[1]), float(F.lam) if ls else 1.0, "ls" if ls else "logistic",
                     F.dtype, None if weights is None else float(sb[2]))


def host_gram_stats(A, b, lam=1.0, kind="ls", weights=None, rows=None) -> GramStats:
    """GramStats from host_route.host_gram on a host matrix (numpy), as CPU torch tensors.  weights: a real N-vector (gram_stats);
    rows: an integer list of row numbers (gram_stats): the statistics of A[rows], b[rows], N = len(rows)."""
    import numpy as np
    import torch
    from .host_route import host_gram
    if kind not in ("ls", "logistic"):
        raise ValueError(f"kind must be 'ls' or 'logistic' (got {kind!r})")
    A = np.asarray(A)
    G, u, colsum, bsum = host_gram(A, b, weights, rows)
    dt = torch.float32 if A.dtype == np.float32 else torch.float64
    return GramStats(A.shape[0] if rows is None else len(rows), A.shape[1], torch.from_numpy(G), torch.from_numpy(u), torch.from_numpy(colsum), float(bsum[0]), float(bsum[1]),
                     float(lam) if kind == "ls" else 1.0, kind, dt, None if weights is None else float(bsum[2]))


def add_stats(stats) -> GramStats:
    """The statistics of the rows of several disjoint sets together: G, u, colsum, the two sums of b and N added in list order (the
    training statistics of a cross-validation fold are the sum of the other folds').  The same d, lam, kind and device throughout;
    weighted statistics are refused (their N is not the weight they carry).  The sums are floating-point sums of the parts: exact where
    the parts are (integer rows), otherwise within the parts' own rounding."""
    stats = list(stats)
    if not stats:
        raise ValueError("add_stats needs at least one GramStats")
    s0 = stats[0]
    for s in stats:
        if s.sum_w is not None:
            raise L.CiaoError(L.ERR_ARG, "add_stats takes unweighted statistics (sum_w is set on one of them)")
        if (s.d, s.lam, s.kind) != (s0.d, s0.lam, s0.kind):
            raise L.CiaoError(L.ERR_ARG, f"add_stats needs the same d, lam and kind throughout (got {(s.d, s.lam, s.kind)} beside "
                                         f"{(s0.d, s0.lam, s0.kind)})")
    G, u, colsum, N, sb, sbb = s0.G, s0.u, s0.colsum, s0.N, s0.sum_b, s0.sum_bb
    for s in stats[1:]:
        G, u, colsum, N, sb, sbb = G + s.G, u + s.u, colsum + s.colsum, N + s.N, sb + s.sum_b, sbb + s.sum_bb
    if len(stats) == 1:
        G, u, colsum = G.clone(), u.clone(), colsum.clone()
    return s0._replace(N=N, G=G, u=u, colsum=colsum, sum_b=sb, sum_bb=sbb)


def mse(stats: GramStats, X):
    """(mse, floor): the mean squared residual (1/N) sum_i (a_i'x_k - b_i)^2 = (x_k'G x_k - 2 u'x_k + sum b^2) / N of the K columns of X
    (d x K, or one d-vector) over the rows `stats` were taken from, as one d x d x K product and without a pass over A: the held-out
    error of a model on a fold.  floor: GramLasso.value_floor on the same scale, 4 * 2^-53 (x'Gx + 2 |u'x| + sum b^2) / N -- what the
    rounding of the three terms can amount to; differences of mse below it mean nothing.  LeastSquares statistics, unweighted."""
    import torch
    _need_ls(stats, "mse")
    if stats.sum_w is not None:
        raise L.CiaoError(L.ERR_ARG, "mse takes unweighted statistics")
    if not isinstance(X, torch.Tensor):
        X = torch.as_tensor(X)
    X = X.to(device=stats.G.device, dtype=torch.float64)
    one = X.dim() == 1
    if one:
        X = X[:, None]
    q = (X * (stats.G @ X)).sum(0)
    l = (stats.u[:, None] * X).sum(0)
    v = (q - 2.0 * l + stats.sum_bb) / stats.N
    fl = 4.0 * EPS * (q + 2.0 * l.abs() + stats.sum_bb) / stats.N
    return (float(v[0]), float(fl[0])) if one else (v, fl)


def smoothness_exact(stats: GramStats) -> float:
    """The smoothness constant of f = (1/N) sum_i f_i, exactly: lam lambda_max(G) / N for LeastSquares rows, lambda_max(G) / (4 N) for
    logistic rows (sigma' <= 1/4), from one torch.linalg.eigvalsh of the d x d matrix.  stepsize.smoothness brackets this number
    (estimate <= it <= upper) with up to fifty passes over A."""
    import torch
    c = stats.lam if stats.kind == "ls" else 0.25
    return c * float(torch.linalg.eigvalsh(stats.G)[-1]) / stats.N


def mu_max(stats: GramStats) -> float:
    """lam ||u||_inf / N = ||grad f(0)||_inf: the smallest l1 weight at which x = 0 minimises the lasso (LeastSquares rows)."""
    _need_ls(stats, "mu_max")
    return stats.lam * float(stats.u.abs().max()) / stats.N


def _need_ls(stats, what):
    if stats.kind != "ls":
        raise L.CiaoError(L.ERR_ARG, f"{what} needs the statistics of LeastSquares rows: the logistic loss is not a function of A'A and A'b "
                                     "(newton.logistic_newton is the Gram route for logistic rows)")


def _soft(v, tau):
    import torch
    return torch.sign(v) * torch.clamp(v.abs() - tau, min=0.0)


class GramLasso:
    """f(x) = (1/N) sum_i (lam / 2)(a_i'x - b_i)^2 in d-space, from GramStats of LeastSquares rows (logistic stats are refused):

        gradient(x) = lam (G x - u) / N                    value(x) = lam (x'G x - 2 u'x + sum_bb) / (2 N)

    x: a float64-convertible d-vector, or a d x K matrix of K iterates (K values / K gradient columns), on G's device.  value is a
    difference of large terms: value_floor(x) = 4 * 2^-53 lam (x'Gx + 2 |u'x| + sum_bb) / (2 N) is what their rounding can amount to, and
    a gap below it means nothing."""

    def __init__(self, stats: GramStats):
        _need_ls(stats, "GramLasso")
        self.stats = stats

    def _x(self, x):
        import torch
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(x)
        return x.to(device=self.stats.G.device, dtype=torch.float64)

    def gradient(self, x):
        s = self.stats
        x = self._x(x)
        return (s.lam / s.N) * (s.G @ x - (s.u if x.dim() == 1 else s.u[:, None]))

    def _terms(self, x):
        s = self.stats
        x = self._x(x)
        Gx = s.G @ x
        return (x * Gx).sum(0), (s.u if x.dim() == 1 else s.u[:, None]).mul(x).sum(0)

    def value(self, x):
        s = self.stats
        q, l = self._terms(x)
        v = (s.lam / (2.0 * s.N)) * (q - 2.0 * l + s.sum_bb)
        return float(v) if v.dim() == 0 else v

    def value_floor(self, x):
        s = self.stats
        q, l = self._terms(x)
        v = 4.0 * EPS * (s.lam / (2.0 * s.N)) * (q + 2.0 * l.abs() + s.sum_bb)
        return float(v) if v.dim() == 0 else v

    def certificate(self, x, mu, gamma) -> CertificateResult:
        """Context.certificate(F, NormL1(mu), x, gamma) without a pass over A: the same eight numbers through certificate.assemble.  mu: the
        l1 weight (mu = 0 or None: g = Zero, the gap is nan); gamma: the step of the prox residual."""
        if not (gamma > 0 and math.isfinite(gamma)):
            raise ValueError("gamma must be > 0 and finite")
        x = self._x(x)
        if x.dim() != 1:
            raise ValueError("certificate takes one iterate (a d-vector)")
        mu_ = float(mu) if mu else 0.0
        grad = self.gradient(x)
        res = x - _soft(x - gamma * grad, gamma * mu_)
        return assemble(self.value(x), mu_ * float(x.abs().sum()), float(res.norm()) / gamma, float(grad.abs().max()), float(x @ grad), 0.0,
                        mu=mu_ if mu_ > 0 else None)

    def as_certificate(self, mu, gamma):
        """A callable state -> CertificateResult for certificate.stop_when: the stop check of a solve over the same rows then costs a
        d x d product instead of a pass over A."""
        def cert(state):
            from .solvers import solution
            return self.certificate(solution(state), mu, gamma)
        return cert


class LassoPath(NamedTuple):
    x: list               # K d-vectors in the rows' dtype, on G's device
    certificates: list    # K CertificateResult, taken AT those (rounded) vectors
    iterations: int       # FISTA iterations made (lasso_path) / sweeps made, over all models (lasso_cd)
    converged: list       # K booleans: the model met its gap before maxit


def _path_gaps(q, mu, X):
    """(gap_k, objective_k) of the K columns of X (d x K, float64) for the l1 weights mu (a K-vector on X's device): the certified duality
    gap of certificate.assemble's lasso formula, all K at once.  lasso_path and lasso_cd stop on it."""
    import torch
    s = q.stats
    c = s.lam / s.N
    grad = c * (s.G @ X - s.u[:, None])
    Fv = q.value(X)
    gv = mu * X.abs().sum(0)
    ginf = grad.abs().amax(0)
    sc = torch.where(ginf > 0, torch.clamp(mu / ginf, max=1.0), torch.ones_like(ginf))
    dual = Fv * (2 * sc - sc * sc) - sc * (X * grad).sum(0)
    return Fv + gv - dual, Fv + gv


def lasso_path(stats: GramStats, mus, x0=None, gap=1e-9, maxit=20000, check_every=10, dtype=None, method="fista", ctx=None, penalty_factor=None,
               lower=None, upper=None, ridge=0.0) -> LassoPath:
    """The lasso min_x f(x) + mu_k ||x||_1 for every mu_k of `mus`, in d-space: FISTA with the step 1 / smoothness_exact(stats), all K
    models as one d x K matrix (one d x d x K product per iteration; A is never read).  Model k stops -- its column is frozen -- at the
    first check (every `check_every` iterations) with gap_k <= gap * max(1, objective_k), the gap being the certified duality gap of
    certificate.assemble.  x0: None (zeros), a d-vector for all, or K of them.  Returns LassoPath: the K iterates in the rows' dtype
    (stats.dtype; dtype= overrides), ready for solve_together and score_many, with the certificates of exactly those vectors (rounding
    an iterate to float32 moves its gap: the certificate says what was reached, `converged` what the float64 iteration met).
    LeastSquares statistics only.

    method: "fista" (the default: the iteration above) or "cd": lasso_cd(stats, mus, x0, gap, ctx=ctx, dtype=dtype) -- coordinate descent,
    on the device kernel where stats.G is on the GPU and a Context is given (maxit and check_every belong to FISTA and are not used).
    penalty_factor, lower, upper, ridge: lasso_cd's, forwarded with method="cd"; FISTA here solves the plain lasso only and refuses them."""
    import torch
    if method == "cd":
        return lasso_cd(stats, mus, x0=x0, gap=gap, ctx=ctx, dtype=dtype, penalty_factor=penalty_factor, lower=lower, upper=upper, ridge=ridge)
    if method != "fista":
        raise ValueError(f"method must be 'fista' or 'cd' (got {method!r})")
    if not (penalty_factor is None and lower is None and upper is None and ridge == 0.0):
        raise ValueError("penalty_factor, lower, upper and ridge need method='cd': the FISTA path solves the plain lasso")
    q = GramLasso(stats)
    s = stats
    mus = [float(m) for m in mus]
    K = len(mus)
    if K < 1 or any(not (m > 0 and math.isfinite(m)) for m in mus):
        raise ValueError("lasso_path needs at least one l1 weight, every one > 0 and finite")
    dev = s.G.device
    mu = torch.tensor(mus, dtype=torch.float64, device=dev)
    if x0 is None:
        X = torch.zeros((s.d, K), dtype=torch.float64, device=dev)
    elif isinstance(x0, (list, tuple)):
        if len(x0) != K:
            raise ValueError(f"{len(x0)} starting points for {K} models")
        X = torch.stack([q._x(v) for v in x0], dim=1)
    else:
        X = q._x(x0)[:, None].repeat(1, K)
    Lf = smoothness_exact(s)
    if not Lf > 0:
        raise ValueError("the Gram matrix is zero: every x minimises f")
    step = 1.0 / Lf
    c = s.lam / s.N
    Y, t = X.clone(), 1.0
    active = torch.ones(K, dtype=torch.bool, device=dev)
    it = 0

    def gaps(X):
        return _path_gaps(q, mu, X)

    while it < maxit:
        grad = c * (s.G @ Y - s.u[:, None])
        Xn = _soft(Y - step * grad, step * mu[None, :])
        tn = 0.5 * (1.0 + math.sqrt(1.0 + 4.0 * t * t))
        Yn = Xn + ((t - 1.0) / tn) * (Xn - X)
        X = torch.where(active[None, :], Xn, X)
        Y = torch.where(active[None, :], Yn, X)
        t = tn
        it += 1
        if it % check_every == 0 or it == maxit:
            gp, obj = gaps(X)
            active = active & ~(gp <= gap * torch.clamp(obj, min=1.0))
            if not bool(active.any()):
                break
    out_dtype = dtype or s.dtype or torch.float64
    xs = [X[:, k].to(out_dtype).contiguous() for k in range(K)]
    done = (~active).tolist()
    return LassoPath(xs, [q.certificate(x, m, step) for x, m in zip(xs, mus)], it, done)


CD_FIRST_TOL = 1e-7       # lasso_cd's first sweep tolerance, times sum b^2 (the change G_jj delta^2 has the units of x'G x)
CD_TOL_DROP = 100.0       # ... divided by this for every model that has not met its gap
CD_MAX_LAUNCH = 1024      # sweeps one launch may make (ciao_gram_cd's bound)


def lasso_cd(stats: GramStats, mus, x0=None, gap=1e-9, max_sweeps=2000, ctx=None, dtype=None, penalty_factor=None, lower=None, upper=None,
             ridge=0.0) -> LassoPath:
    """lasso_path's problem by cyclic coordinate descent with covariance updates: an update reads one row of G, a
    coordinate that stays at zero reads none.  With stats.G on the GPU and a device.Context `ctx` the sweeps run in ONE kernel launch for
    all models (Context.gram_cd: a workgroup per model); otherwise in numpy (host_route.host_gram_cd).  The two give the same bits.

    The driver: launch with the sweep tolerance tol = 1e-7 sum b^2 on the largest change G_jj delta^2 of a sweep; take the certified
    duality gaps of all K models (lasso_path's formula); freeze the models with gap_k <= gap max(1, objective_k); relaunch the rest,
    warm, with tol / 100; until all have met the gap or a model has made max_sweeps sweeps.  A model whose launch moved no coordinate
    at all is at a fixed point of the update in floating point and is frozen as it is (converged = False unless its gap is met).
    x0, dtype and the returned LassoPath are lasso_path's; iterations = the sweeps made, summed over the models.  LeastSquares
    statistics only, weighted ones included.

    penalty_factor, lower, upper (a number or a d-vector each), ridge: the problem becomes
        min_x f(x) + sum_j mu_k penalty_factor_j |x_j| + (ridge / 2) ||x||^2     over  lower_j <= x_j <= upper_j
    (non-negative and box-constrained lasso; adaptive lasso, unpenalised coordinates with factor 0, excluded ones with +inf; elastic
    net), with lower <= 0 <= upper.  With all four at their defaults nothing changes; otherwise the same driver runs on
    Context.gram_cd_general / host_route.host_gram_cd_general and stops on constrained_gaps, and the certificates carry that objective
    and gap (residual: NaN).  A factor of 0 on a coordinate with an infinite bound is refused without a ridge: no duality gap can stop
    that solve."""
    import numpy as np
    import torch
    pf, lo, hi, ridge, general = _constraints(stats.d, stats.G.device, penalty_factor, lower, upper, ridge)
    if general:
        return _cd_general([stats], mus, x0, gap, max_sweeps, ctx, dtype, pf, lo, hi, ridge, True)[0]
    q = GramLasso(stats)
    s = stats
    mus = [float(m) for m in mus]
    K = len(mus)
    if K < 1 or any(not (m > 0 and math.isfinite(m)) for m in mus):
        raise ValueError("lasso_cd needs at least one l1 weight, every one > 0 and finite")
    if not (gap > 0 and max_sweeps >= 1):
        raise ValueError("gap must be > 0 and max_sweeps >= 1")
    dev = s.G.device
    on_device = dev.type == "cuda" and ctx is not None
    if dev.type == "cuda" and ctx is None:
        raise L.CiaoError(L.ERR_ARG, "lasso_cd on device statistics needs the Context to launch on (ctx=); stats.to('cpu') runs the numpy twin")
    if on_device:
        from .stepsize import _on_stream
        stream = lambda: _on_stream(ctx)   # noqa: E731
    else:
        import contextlib
        stream = contextlib.nullcontext
    with stream():
        mu = torch.tensor(mus, dtype=torch.float64, device=dev)
        if x0 is None:
            X = torch.zeros((K, s.d), dtype=torch.float64, device=dev)
        elif isinstance(x0, (list, tuple)):
            if len(x0) != K:
                raise ValueError(f"{len(x0)} starting points for {K} models")
            X = torch.stack([q._x(v) for v in x0], dim=0).contiguous()
        else:
            X = q._x(x0)[None, :].repeat(K, 1)
        c = s.lam / s.N
        tau = torch.tensor([m / c for m in mus], dtype=torch.float64, device=dev)
        diag = torch.diagonal(s.G)
        inv = torch.where(diag > 0, 1.0 / diag, torch.zeros_like(diag)).contiguous()
        G = s.G if s.G.stride(1) == 1 or s.d == 1 else s.G.contiguous()
        u = s.u.contiguous()
        tol = CD_FIRST_TOL * float(s.sum_bb)
        if not (tol >= 0 and math.isfinite(tol)):
            raise ValueError("sum_bb must be finite and >= 0")
        used = [0] * K
        done = [False] * K
        live = list(range(K))
        while live:
            budget = min(CD_MAX_LAUNCH, max_sweeps - max(used[k] for k in live))
            if budget < 1:
                break
            idx = torch.tensor(live, dtype=torch.long, device=dev)
            Xl = X.index_select(0, idx).contiguous()
            if on_device:
                _, _, st = ctx.gram_cd(G, u, inv, tau.index_select(0, idx).contiguous(), Xl, tol, budget, R=None)
                st = st.cpu().numpy()
            else:
                Xn, _, st = _host_cd(G, u, inv, tau.index_select(0, idx), Xl, tol, budget)
                Xl = torch.from_numpy(Xn)
            X.index_copy_(0, idx, Xl)
            gp, obj = _path_gaps(q, mu.index_select(0, idx), Xl.t())
            met = (gp <= gap * torch.clamp(obj, min=1.0)).tolist()
            nxt = []
            for pos, k in enumerate(live):
                used[k] += int(st[pos, 0])
                if met[pos]:
                    done[k] = True
                elif st[pos, 3] != 2 and st[pos, 1] > 0:
                    nxt.append(k)
            live = nxt
            tol /= CD_TOL_DROP
        out_dtype = dtype or s.dtype or torch.float64
        xs = [X[k].to(out_dtype).contiguous() for k in range(K)]
        gamma = 1.0 / float(diag.max()) / c if float(diag.max()) > 0 else 1.0
        certs = [q.certificate(x, m, gamma) for x, m in zip(xs, mus)]
    return LassoPath(xs, certs, int(np.sum(used)), done)


def _host_cd(G, u, inv, tau, X, tol, max_sweeps):
    """host_route.host_gram_cd on CPU torch tensors (G may have any strides)."""
    from .host_route import host_gram_cd
    return host_gram_cd(G.numpy(), u.numpy(), inv.numpy(), tau.numpy(), X.numpy(), tol, max_sweeps)


def _constraints(d, dev, penalty_factor, lower, upper, ridge):
    """(pf, lo, hi, ridge, general): the three per-coordinate vectors as float64 d-vectors on `dev` (None where left at the default) and
    whether any of the four leaves the plain lasso.  Refuses what ciao_gram_cd_general would answer with state 3."""
    import torch

    def vec(v, name):
        if v is None:
            return None
        v = torch.as_tensor(v, dtype=torch.float64).to(dev)
        v = v.expand(d) if v.dim() == 0 else v
        if tuple(v.shape) != (d,):
            raise ValueError(f"{name} must be a number or a vector of d = {d} elements")
        return v.contiguous()

    pf, lo, hi = vec(penalty_factor, "penalty_factor"), vec(lower, "lower"), vec(upper, "upper")
    ridge = float(ridge)
    if pf is not None and not bool((pf >= 0).all()):
        raise ValueError("penalty_factor must be >= 0 everywhere (+inf excludes a coordinate) and not NaN")
    if lo is not None and not bool((lo <= 0).all()):
        raise ValueError("lower must be <= 0 everywhere (-inf: no bound) and not NaN: x = 0 has to be feasible")
    if hi is not None and not bool((hi >= 0).all()):
        raise ValueError("upper must be >= 0 everywhere (+inf: no bound) and not NaN: x = 0 has to be feasible")
    if not (ridge >= 0 and math.isfinite(ridge)):
        raise ValueError("ridge must be >= 0 and finite")
    return pf, lo, hi, ridge, not (pf is None and lo is None and hi is None and ridge == 0.0)


def constrained_gaps(stats: GramStats, X, mus, penalty_factor=None, lower=None, upper=None, ridge=0.0):
    """(gap_k, objective_k) of the K columns of X (d x K) for the problems

        min_x  F(x) + g(x),   F(x) = (c/2)(x'G x - 2 u'x + sum b^2),  c = lam / N,
        g(x) = sum_j mu_k pf_j |x_j| + (ridge / 2) x_j^2   over  lower_j <= x_j <= upper_j   (+inf outside)

    by Fenchel duality, all K at once on X's device: with grad = c (G x - u) and v = -s grad,

        dual = F (2 s - s^2) - s x'grad - sum_j g*_j(v_j),      gap = F + g(x) - dual >= objective - optimum,
        g*_j(v) = v xh - mu_j |xh| - (ridge / 2) xh^2  at  xh = clamp(soft(v, mu_j) / ridge, lower_j, upper_j)        (ridge > 0)
                                                           xh = upper_j if v > mu_j, lower_j if v < -mu_j, else 0     (ridge = 0)

    s = 1 with a ridge; otherwise the largest s <= 1 with v_j <= mu_j wherever upper_j = +inf and -v_j <= mu_j wherever lower_j = -inf
    (those terms are then 0: the scaling lasso_path's gap uses, restricted to the sides that are open to infinity).  An unpenalised
    coordinate with an infinite side and no ridge forces s = 0 and a gap that never closes.  penalty_factor, lower, upper: a number or
    a d-vector, None: 1, -inf, +inf.  With the defaults this is the gap lasso_path and lasso_cd stop on, up to rounding."""
    import torch
    q = GramLasso(stats)
    s_ = stats
    X = q._x(X)
    if X.dim() == 1:
        X = X[:, None]
    dev = X.device
    d, K = X.shape
    mu = torch.as_tensor(mus, dtype=torch.float64).to(dev).reshape(-1)
    if mu.shape[0] != K:
        raise ValueError(f"{mu.shape[0]} l1 weights for {K} columns")
    pf, lo, hi, nu, _ = _constraints(d, dev, penalty_factor, lower, upper, ridge)
    pf = torch.ones(d, dtype=torch.float64, device=dev) if pf is None else pf
    lo = torch.full((d,), -math.inf, dtype=torch.float64, device=dev) if lo is None else lo
    hi = torch.full((d,), math.inf, dtype=torch.float64, device=dev) if hi is None else hi
    c = s_.lam / s_.N
    grad = c * (s_.G @ X - s_.u[:, None])
    Fv = q.value(X)
    if not isinstance(Fv, torch.Tensor):
        Fv = torch.as_tensor([Fv], dtype=torch.float64, device=dev)
    muj = mu[None, :] * pf[:, None]                                   # d x K; +inf where a coordinate is excluded
    zero = torch.zeros_like(X)
    ax = X.abs()
    gv = torch.where(ax > 0, muj * ax, zero).sum(0) + 0.5 * nu * (X * X).sum(0)
    outside = ((X > hi[:, None]) | (X < lo[:, None])).any(0)
    gv = torch.where(outside, torch.full_like(gv, math.inf), gv)
    LO, HI = lo[:, None].expand(d, K), hi[:, None].expand(d, K)
    if nu > 0:
        sc = torch.ones(K, dtype=torch.float64, device=dev)
        v = -grad
        xh = torch.minimum(torch.maximum(torch.sign(v) * torch.clamp(v.abs() - muj, min=0.0) / nu, LO), HI)
    else:
        # the sides open to infinity bound s: s (-grad_j) <= mu_j where upper_j = +inf, s grad_j <= mu_j where lower_j = -inf
        inf = torch.full_like(grad, math.inf)
        need = torch.minimum(torch.where(torch.isinf(HI) & (grad < 0), muj / -grad, inf), torch.where(torch.isinf(LO) & (grad > 0), muj / grad, inf))
        sc = torch.clamp(need.amin(0), max=1.0)
        v = -sc[None, :] * grad
        xh = torch.where((v > muj) & torch.isfinite(HI), HI, torch.where((v < -muj) & torch.isfinite(LO), LO, zero))
    axh = xh.abs()
    conj = (v * xh - torch.where(axh > 0, muj * axh, zero) - 0.5 * nu * xh * xh).sum(0)
    dual = Fv * (2 * sc - sc * sc) - sc * (X * grad).sum(0) - conj
    return Fv + gv - dual, Fv + gv


CD_UNBOUNDED_FREE = ("lasso_cd: penalty_factor is 0 on a coordinate with an infinite bound and there is no ridge: the dual problem has no "
                     "finite point in general, so no duality gap can stop the solve.  Bound the coordinate (lower= / upper=), add a ridge, "
                     "or centre the columns and targets (GramStats.standardized) and leave the coordinate out")


def _cd_general(groups, mus, x0, gap, max_sweeps, ctx, dtype, pf, lo, hi, ridge, general):
    """lasso_cd's driver over SEVERAL statistics at once -> one LassoPath per group: the models of every group go through ONE
    Context.gram_cd_general launch per round (host_route.host_gram_cd_general without a context), model (g, k) on Gram matrix g with
    group g's u, its inv = 1 / (G_jj + ridge N / lam), its own tol schedule (1e-7 sum b^2 of the group, divided by 100 per round) and
    frozen on its own gap.  A model's bits do not depend on the others in the launch, so a group's path is what the driver gives the
    group alone -- up to the sweep budget, which one launch shares.  general: stop on constrained_gaps and certify with it; otherwise
    (the plain lasso, all constraints None) on lasso_path's gap, with lasso_cd's certificates."""
    import numpy as np
    import torch
    from .host_route import host_gram_cd_general
    s0 = groups[0]
    for s in groups:
        _need_ls(s, "lasso_cd")
        if s.d != s0.d or s.G.device != s0.G.device:
            raise ValueError("the statistics must share d and the device")
    mus = [float(m) for m in mus]
    K, S, d = len(mus), len(groups), s0.d
    if K < 1 or any(not (m > 0 and math.isfinite(m)) for m in mus):
        raise ValueError("lasso_cd needs at least one l1 weight, every one > 0 and finite")
    if not (gap > 0 and max_sweeps >= 1):
        raise ValueError("gap must be > 0 and max_sweeps >= 1")
    if S * K > 4096:
        raise ValueError(f"{S} x {K} models exceed one launch (4096)")
    dev = s0.G.device
    on_device = dev.type == "cuda" and ctx is not None
    if dev.type == "cuda" and ctx is None:
        raise L.CiaoError(L.ERR_ARG, "lasso_cd on device statistics needs the Context to launch on (ctx=); stats.to('cpu') runs the numpy twin")
    if general and ridge == 0.0 and pf is not None:
        open_side = torch.ones(d, dtype=torch.bool, device=dev)
        if lo is not None and hi is not None:
            open_side = torch.isinf(lo) | torch.isinf(hi)
        if bool(((pf == 0) & open_side).any()):
            raise ValueError(CD_UNBOUNDED_FREE)
    if on_device:
        from .stepsize import _on_stream
        stream = lambda: _on_stream(ctx)   # noqa: E731
    else:
        import contextlib
        stream = contextlib.nullcontext
    qs = [GramLasso(s) for s in groups]
    with stream():
        mu = torch.tensor(mus, dtype=torch.float64, device=dev)
        if x0 is None:
            X = torch.zeros((S * K, d), dtype=torch.float64, device=dev)
        elif isinstance(x0, (list, tuple)):
            if len(x0) != K:
                raise ValueError(f"{len(x0)} starting points for {K} models")
            X = torch.stack([qs[0]._x(v) for v in x0], dim=0).repeat(S, 1).contiguous()
        else:
            X = qs[0]._x(x0)[None, :].repeat(S * K, 1)
        Gs = torch.stack([s.G for s in groups], dim=0)
        Us = torch.stack([s.u for s in groups], dim=0)
        cs = [s.lam / s.N for s in groups]
        tau = torch.tensor([m / c for c in cs for m in mus], dtype=torch.float64, device=dev)
        diags = [torch.diagonal(s.G) for s in groups]
        if general:
            dens = [dg + ridge / c for dg, c in zip(diags, cs)]
        else:
            dens = diags
        INVs = torch.stack([torch.where(dn > 0, 1.0 / dn, torch.zeros_like(dn)) for dn in dens], dim=0)
        tols = [CD_FIRST_TOL * float(s.sum_bb) for s in groups]
        if any(not (t >= 0 and math.isfinite(t)) for t in tols):
            raise ValueError("sum_bb must be finite and >= 0")
        used = [0] * (S * K)
        done = [False] * (S * K)
        live = list(range(S * K))
        while live:
            budget = min(CD_MAX_LAUNCH, max_sweeps - max(used[m] for m in live))
            if budget < 1:
                break
            idx = torch.tensor(live, dtype=torch.long, device=dev)
            gidx = torch.tensor([m // K for m in live], dtype=torch.long, device=dev)
            Xl = X.index_select(0, idx).contiguous()
            tol = torch.tensor([tols[m // K] for m in live], dtype=torch.float64, device=dev)
            taul = tau.index_select(0, idx).contiguous()
            Ul, Il = Us.index_select(0, gidx).contiguous(), INVs.index_select(0, gidx).contiguous()
            if on_device:
                _, _, st = ctx.gram_cd_general(Gs, Ul, Il, taul, Xl, tol, budget, gsel=gidx.to(torch.int32), pf=pf, lo=lo, hi=hi, R=None)
                st = st.cpu().numpy()
            else:
                npv = lambda t: None if t is None else t.numpy()   # noqa: E731
                Xn, _, st = host_gram_cd_general(Gs.numpy(), Ul.numpy(), Il.numpy(), taul.numpy(), Xl.numpy(), tol.numpy(), budget,
                                                 gsel=gidx.numpy(), pf=npv(pf), lo=npv(lo), hi=npv(hi))
                Xl = torch.from_numpy(Xn)
            X.index_copy_(0, idx, Xl)
            met = {}
            for g in sorted({m // K for m in live}):
                pos = [p for p, m in enumerate(live) if m // K == g]
                ks = torch.tensor([live[p] % K for p in pos], dtype=torch.long, device=dev)
                Xg = Xl.index_select(0, torch.tensor(pos, dtype=torch.long, device=dev)).t()
                if general:
                    gp, obj = constrained_gaps(groups[g], Xg, mu.index_select(0, ks), pf, lo, hi, ridge)
                else:
                    gp, obj = _path_gaps(qs[g], mu.index_select(0, ks), Xg)
                for p, ok in zip(pos, (gp <= gap * torch.clamp(obj, min=1.0)).tolist()):
                    met[p] = ok
            nxt = []
            for pos, m in enumerate(live):
                used[m] += int(st[pos, 0])
                if met[pos]:
                    done[m] = True
                elif st[pos, 3] not in (2, 3) and st[pos, 1] > 0:
                    nxt.append(m)
            live = nxt
            tols = [t / CD_TOL_DROP for t in tols]
        out = []
        for g, s in enumerate(groups):
            out_dtype = dtype or s.dtype or torch.float64
            xs = [X[g * K + k].to(out_dtype).contiguous() for k in range(K)]
            if general:
                Xr = torch.stack([x.double() for x in xs], dim=1)
                gp, obj = constrained_gaps(s, Xr, mu, pf, lo, hi, ridge)
                grad = qs[g].gradient(Xr)
                Fv = qs[g].value(Xr)
                viol = torch.zeros_like(Xr)
                if lo is not None:
                    viol = torch.maximum(viol, lo[:, None] - Xr)
                if hi is not None:
                    viol = torch.maximum(viol, Xr - hi[:, None])
                nan = math.nan
                # (the prox residual is NormL1's: it has no meaning under bounds, factors or a ridge)
                certs = [CertificateResult(float(Fv[k]), float(obj[k] - Fv[k]), float(obj[k]), nan, float(grad[:, k].abs().max()),
                                           float(Xr[:, k] @ grad[:, k]), float(viol[:, k].max()), float(gp[k])) for k in range(K)]
            else:
                dmax = float(diags[g].max())
                gamma = 1.0 / dmax / cs[g] if dmax > 0 else 1.0
                certs = [qs[g].certificate(x, m, gamma) for x, m in zip(xs, mus)]
            out.append(LassoPath(xs, certs, int(np.sum(used[g * K:(g + 1) * K])), done[g * K:(g + 1) * K]))
    return out

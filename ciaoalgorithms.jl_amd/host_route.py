"""The explicit HOST route of the solvers: `solver(x0; F, g, ..., fallback="host")`.

The device path packs five operator families (operators.py) and refuses everything else; the reference accepts any
ProximalOperators object (SVRG.jl:46-58, SAGA.jl:44-58, Finito.jl:66-116).  With `fallback="host"` a problem whose F / g
cannot be packed runs here instead: the same iterables (SVRG_basic.jl:30-96, SAGA_basic.jl:26-68, Finito_basic.jl:44-121,
Finito_LFinito.jl:40-103), one `gradient` / `prox` call per sample on the host (host_ops.py, numpy), the same injected
sampling stream, the same iteration protocol and `solution(state)` identity.  It is slow (an interpreted loop over samples),
it is announced with a warning, every state carries `backend == "host"`, and nothing in it touches the GPU, the library or
oracle/ -- it is a convenience for operators that have no device form, not a second implementation of the hot path, and no
performance or parity statement of this repo is about it.  `backend="host"` forces it for a problem that WOULD pack (tests
compare the two routes on such problems).
"""
from __future__ import annotations

import warnings

import numpy as np

from . import host_ops as H
from .sampling import IndexStream


class HostState:
    backend = "host"
    _it = None

    @property
    def objective(self):
        return self._it.objective(self)


class _HostIterable:
    backend = "host"
    _chunkable = True
    monitor = False

    def __init__(self, R, F, g, x0, N, stream):
        if N is None:
            raise TypeError("N (number of terms in the finite sum) is required")
        self.R = np.dtype(R)
        self.x0 = x0                                     # not copied: iter.x0 === x0 (test/test_lasso.jl:182)
        self.N = int(N)
        x = np.asarray(x0.detach().cpu() if hasattr(x0, "detach") else x0)
        want = np.result_type(self.R, x.dtype) if np.iscomplexobj(x) else self.R
        if x.dtype != want and not (np.iscomplexobj(x) and x.real.dtype == self.R):
            raise TypeError(f"x0 has dtype {x.dtype} but the solver's real type is {self.R} (no silent promotion)")
        self._x = x.reshape(-1)
        self._numpy, self._complex = True, False
        self.F = [None] * self.N if F is None else list(F)
        if len(self.F) != self.N:
            raise ValueError(f"F has {len(self.F)} terms but N={self.N}")
        self.g = g
        self.stream = stream if stream is not None else IndexStream(0)
        self._state, self._started = None, False

    class _NoCtx:                                        # the functor's loop synchronises its context: nothing to wait for here
        @staticmethod
        def synchronize():
            return None

    ctx = _NoCtx()

    def grad(self, i, x):
        return H.gradient(self.F[i], x)[0]

    def prox(self, x, gamma):
        return H.prox(self.g, x, self.R.type(gamma))[0]

    def objective(self, state):
        """(1/N) sum_i f_i(x) + g(x) at solution(state): one pass of `gradient` values."""
        x = host_solution(state)
        return float(sum(np.real(H.gradient(f, x)[1]) for f in self.F) / max(self.N, 1) + _gval(self.g, x))

    def __iter__(self):
        self._state, self._started = None, False
        return self

    def __next__(self):
        if not self._started:
            self._started = True
            self._state = self._init()
            if self._state is None:
                raise StopIteration
            return self._state
        if self._state is None:
            raise StopIteration
        self._step(self._state, 1)
        return self._state


def _gval(g, x):
    """g(x) (for the objective): the value `prox` reports at a point is g(prox) -- evaluate at x itself where g is finite."""
    from . import operators as Op
    if g is None or isinstance(g, Op.Zero) or isinstance(g, Op.IndBox):
        return 0.0
    if isinstance(g, Op.NormL1):
        return float(g.lam * np.sum(np.abs(x)))
    if hasattr(g, "value") and callable(g.value):
        return float(g.value(x))
    return float("nan")


def _maxL(Lc):
    return float(np.max(np.asarray(Lc.detach().cpu() if hasattr(Lc, "detach") else Lc)))


def _gammas(it):
    """Finito_basic.jl:61-74 / Finito_LFinito.jl:51-63."""
    R, N = it.R.type, it.N
    if it.γ is None:
        if it.L is None:
            warnings.warn("--> smoothness parameter absent")
            return None
        if np.ndim(it.L) == 0:
            return np.full(N, R(it.α) * R(N) / R(it.L), dtype=it.R)
        return (R(it.α) * R(N) / np.asarray(it.L, dtype=it.R)).astype(it.R)
    if np.ndim(it.γ) == 0:
        return np.full(N, R(it.γ), dtype=it.R)
    return np.asarray(it.γ, dtype=it.R)


# ---- SVRG (SVRG_basic.jl) ------------------------------------------------------------------------------------------------
class HostSVRGState(HostState):
    def __init__(self, γ, m, av, z, z_full, w):
        self.γ, self.m, self.av, self.z, self.z_full, self.w = γ, m, av, z, z_full, w

    gamma = property(lambda self: self.γ)


class HostSVRG(_HostIterable):
    _chunkable = False

    def __init__(self, R, F, g, x0, N, L, μ, γ, m, plus, stream=None):
        super().__init__(R, F, g, x0, N, stream)
        self.L, self.μ, self.γ, self.m, self.plus = L, μ, γ, m, plus

    def _init(self):                                                       # :30-69
        N = self.N
        m = N if self.m is None else self.m
        if self.γ is None:
            if self.plus:
                warnings.warn("provide a stepsize γ")
                return None
            if self.L is None or self.μ is None:
                warnings.warn("smoothness or convexity parameter absent")
                return None
            L_M, μ_M = _maxL(self.L), _maxL(self.μ)
            γ = 1 / (10 * L_M)
            rho = (1 + 4 * L_M * γ ** 2 * μ_M * (N + 1)) / (μ_M * γ * N * (1 - 4 * L_M * γ))
            if rho >= 1:
                warnings.warn("convergence condition violated...provide a stepsize!")
        else:
            γ = self.γ
        av = np.zeros_like(self._x)
        for i in range(N):                                                 # :58-63
            av += self.grad(i, self._x) / N
        st = HostSVRGState(float(γ), int(m), av, np.zeros_like(av), self._x.copy(), self._x.copy())
        st._it = self
        return st

    def _step(self, st, n):                                                # :71-96
        γ = self.R.type(st.γ)
        for _ in range(n):
            for i in self.stream.rand_indices(self.N, st.m):               # :73
                temp = self.grad(int(i), st.z_full)
                temp = temp - self.grad(int(i), st.w)
                temp -= st.av
                temp *= γ
                temp += st.w
                st.w = self.prox(temp, st.γ)
                st.z += st.w
            st.z_full[...] = st.z / st.m
            if not self.plus:
                st.w = st.z_full.copy()
            st.z = np.zeros_like(st.z)
            st.av[...] = 0
            for i in range(self.N):
                st.av += self.grad(i, st.z_full) / self.N
            if self.plus:
                st.m *= 2


# ---- SAGA / SAG (SAGA_basic.jl) ------------------------------------------------------------------------------------------
class HostSAGAState(HostState):
    def __init__(self, s, γ, av, z):
        self.s, self.γ, self.av, self.z, self.ind = s, γ, av, z, 0

    gamma = property(lambda self: self.γ)


class HostSAGA(_HostIterable):
    def __init__(self, R, F, g, x0, N, L, γ, SAG, stream=None):
        super().__init__(R, F, g, x0, N, stream)
        self.L, self.γ, self.SAG = L, γ, SAG

    def _init(self):                                                       # :26-51
        if self.γ is None:
            if self.L is None:
                warnings.warn("smoothness parameter absent")
                return None
            L_M = _maxL(self.L)
            γ = 1 / (16 * L_M) if self.SAG else 1 / (3 * L_M)
        else:
            γ = self.γ
        s = [self.grad(i, self._x) for i in range(self.N)]
        av = sum(s) / self.N if self.N else np.zeros_like(self._x)
        z = self.prox((1 - self.R.type(γ)) * self._x, γ)                   # :48 (sic)
        st = HostSAGAState(s, float(γ), av, z)
        st._it = self
        return st

    def _step(self, st, n):                                                # :53-68
        γ = self.R.type(st.γ)
        for i in self.stream.rand_indices(self.N, n):
            i = int(i)
            gn = self.grad(i, st.z)
            if self.SAG:
                st.av += (gn - st.s[i]) / self.N
                w = st.z - γ * st.av
            else:
                w = st.z - γ * (gn - st.s[i] + st.av)
                st.av += (gn - st.s[i]) / self.N
            st.z[...] = self.prox(w, st.γ)
            st.s[i] = gn
            st.ind = i + 1


# ---- Finito / MISO (Finito_basic.jl) and LFinito (Finito_LFinito.jl) ---------------------------------------------------------
class HostFinitoState(HostState):
    def __init__(self, s, γ, hat_γ, av, z, d):
        self.s, self.γ, self.hat_γ, self.av, self.z, self.d = s, γ, hat_γ, av, z, d
        self.idxr, self.idx, self.inds = 1, 0, np.arange(d, dtype=np.int64)

    hat_gamma = property(lambda self: self.hat_γ)


def _static(N, r, j):
    lo = r * j
    return range(lo, min(lo + r, N))


class HostFinito(_HostIterable):
    def __init__(self, R, F, g, x0, N, L, γ, sweeping, batch, α, stream=None):
        super().__init__(R, F, g, x0, N, stream)
        self.L, self.γ, self.sweeping, self.batch, self.α = L, γ, int(sweeping), int(batch), α
        if self.batch < 1:
            raise ValueError("batch size must be >= 1")

    def _init(self):                                                       # :44-89
        N, r = self.N, self.batch
        gam = _gammas(self)
        if gam is None:
            return None
        s = [self._x - gam[i] / N * self.grad(i, self._x) for i in range(N)]
        hat_γ = 1 / np.sum(1 / gam)
        av = hat_γ * sum(s[i] / gam[i] for i in range(N))
        z = self.prox(av, hat_γ)
        st = HostFinitoState(s, gam, float(hat_γ), av, z, -(-N // r) if N > 0 else 0)
        st._it = self
        return st

    def _next_batch(self, st):                                             # :95-108
        N, r = self.N, self.batch
        if self.sweeping == 1:
            return [int(i) for i in self.stream.sample_without_replacement(N, r)]
        if self.sweeping == 2:
            j = st.idxr % st.d                                             # idxr is 1-based: mod(idxr, d) + 1, then 0-based
            st.idxr = j + 1
            return _static(N, r, j)
        if st.idx == st.d:
            st.inds = self.stream.randperm(st.d)
            st.idx = 0
        j = int(st.inds[st.idx])
        st.idx += 1
        st.idxr = j + 1
        return _static(N, r, j)

    def _step(self, st, n):                                                # :109-118
        hg = self.R.type(st.hat_γ)
        for _ in range(n):
            for i in self._next_batch(st):
                t = st.z - (st.γ[i] / self.N) * self.grad(i, st.z)
                st.av += (t - st.s[i]) * (hg / st.γ[i])
                st.s[i] = t
            st.z[...] = self.prox(st.av, st.hat_γ)


class HostLFinitoState(HostState):
    def __init__(self, γ, hat_γ, av, d, z, z_full):
        self.γ, self.hat_γ, self.av, self.d, self.z, self.z_full = γ, hat_γ, av, d, z, z_full
        self.inds = np.arange(d, dtype=np.int64)

    hat_gamma = property(lambda self: self.hat_γ)


class HostLFinito(_HostIterable):
    _chunkable = False

    def __init__(self, R, F, g, x0, N, L, γ, sweeping, batch, α, stream=None):
        super().__init__(R, F, g, x0, N, stream)
        self.L, self.γ, self.sweeping, self.batch, self.α = L, γ, int(sweeping), int(batch), α
        if self.batch < 1:
            raise ValueError("batch size must be >= 1")

    def _init(self):                                                       # :40-76
        N, r = self.N, self.batch
        gam = _gammas(self)
        if gam is None:
            return None
        hat_γ = 1 / np.sum(1 / gam)
        av = self._x.copy()
        for i in range(N):
            av -= (hat_γ / N) * self.grad(i, self._x)
        st = HostLFinitoState(gam, float(hat_γ), av, -(-N // r) if N > 0 else 0, np.zeros_like(av), np.zeros_like(av))
        st._it = self
        return st

    def _step(self, st, n):                                                # :78-103
        N, r = self.N, self.batch
        hg = self.R.type(st.hat_γ)
        for _ in range(n):
            st.z_full[...] = self.prox(st.av, st.hat_γ)
            st.av[...] = st.z_full
            for i in range(N):
                st.av -= (hg / N) * self.grad(i, st.z_full)
            if self.sweeping == 3:
                st.inds = self.stream.randperm(st.d)
            for j in st.inds:
                st.z[...] = self.prox(st.av, st.hat_γ)
                for i in _static(N, r, int(j)):
                    st.av += (hg / N) * self.grad(i, st.z_full)
                    st.av -= (hg / N) * self.grad(i, st.z)
                    st.av += (hg / st.γ[i]) * (st.z - st.z_full)


def host_solution(state):
    return state.z_full if isinstance(state, HostSVRGState) else state.z


def _rows(F):
    """("ls" | "logistic", A, b) in float64 when every f_i is a one-row LeastSquares / Precompose(LogisticLoss) term; else None."""
    from . import operators as Op
    if F and all(isinstance(f, Op.LeastSquares) and not np.iscomplexobj(f.A) for f in F):
        return ("ls", np.concatenate([f.A for f in F], axis=0).astype(np.float64), np.concatenate([f.b for f in F]).astype(np.float64))
    if F and all(isinstance(f, Op.Precompose) and isinstance(f.f, Op.LogisticLoss) and f.f.mu == 1.0 and not np.any(np.asarray(f.b) != 0) for f in F):
        return ("logistic", np.concatenate([f.L for f in F], axis=0).astype(np.float64), np.concatenate([f.f.y for f in F]).astype(np.float64))
    return None


def host_margin_stats(kind, dots, b, s=1.0):
    """The four numbers of ciao_margin_stats in numpy (float64), by the same stable evaluation (csrc/mstat_kernels.h)."""
    dots, b = np.asarray(dots, np.float64), np.asarray(b, np.float64)
    if kind == "ls":
        r = dots - b
        return float(np.sum(r * r)), float(np.sum(b)), float(np.sum(b * b)), float(np.max(np.abs(r)))
    t = b * dots
    e = np.exp(-np.abs(t))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    v = s * np.where(t >= 0, small, big)
    w = (1.0 - s) + s * np.where(t >= 0, big, small)
    xlogx = lambda u: np.where(u > 0, u * np.log(np.where(u > 0, u, 1.0)), 0.0)
    return (float(np.sum(np.maximum(-t, 0.0) + np.log1p(e))), float(np.sum(xlogx(v) + xlogx(w))), float(np.sum(t <= 0)), float(np.min(t)))


def host_margin_stats_multi(kind, A, xs, b, s=None, rows=None, offsets=None):
    """ciao_margin_stats_multi in numpy (float64): K calls of host_margin_stats on the row dots A @ x_k, at s_k (None: 1).

    rows, offsets (ciao_margin_stats_multi_rows): gather, then add -- the statistics of A[rows], b[rows] for the dots
    A[rows] @ x_k + offsets[k]; rows: integer row numbers in [0, N), any order, repeats allowed; offsets: K numbers (None: nothing is
    added)."""
    A, b = np.asarray(A, np.float64), np.asarray(b, np.float64)
    if rows is not None:
        rows = np.asarray(rows)
        if rows.ndim != 1 or not np.issubdtype(rows.dtype, np.integer) or rows.size < 1:
            raise ValueError("host_margin_stats_multi: rows must be an integer vector of at least one row number")
        if rows.min() < 0 or rows.max() >= A.shape[0]:
            raise ValueError(f"rows: entries must lie in [0, {A.shape[0]})")
        A, b = A[rows], b[rows]
    if offsets is not None and len(offsets) != len(xs):
        raise ValueError(f"host_margin_stats_multi: {len(offsets)} offsets for {len(xs)} iterates")
    out = []
    for k, x in enumerate(xs):
        dots = A @ np.asarray(x, np.float64).reshape(-1)
        if offsets is not None:
            dots = dots + float(offsets[k])
        out.append(host_margin_stats(kind, dots, b, 1.0 if s is None else float(s[k])))
    return out


def _score(kind, stats, n):
    """scoring.score's fields from the four statistics."""
    from .scoring import LeastSquaresScore, LogisticScore
    if kind == "ls":
        sum_r2, sum_b, sum_b2, max_abs_r = stats
        tss = sum_b2 - sum_b * sum_b / n
        return LeastSquaresScore(sum_r2 / n, 1.0 - sum_r2 / tss if tss > 0 else float("nan"), max_abs_r)
    loss_sum, _, errors, min_margin = stats
    return LogisticScore(loss_sum / n, 1.0 - errors / n, min_margin)


def host_score(F, x):
    """scoring.score in numpy for operator objects (one-row LeastSquares or Precompose(LogisticLoss) terms): the same fields."""
    x = np.asarray(x.detach().cpu() if hasattr(x, "detach") else x).reshape(-1).astype(np.float64)
    rows = _rows(list(F))
    if rows is None:
        raise TypeError("host_score needs F as one-row LeastSquares terms or Precompose(LogisticLoss) terms")
    kind, A, b = rows
    return _score(kind, host_margin_stats(kind, A @ x, b, 1.0), len(b))


def host_certificate(F, g, x, gamma, N, samples=False):
    """certificate.CertificateResult at x in numpy (float64): the quantities of ciao_certificate for operator objects -- the host
    route's answer to certificate.Certificate.  The gap applies when every f_i is a LeastSquares and g = NormL1(mu), mu > 0; with
    samples=True also when every f_i is a Precompose(LogisticLoss) row (the per-sample entropy, as ciao_certificate_samples)."""
    from . import operators as Op
    from .certificate import assemble
    x = np.asarray(x.detach().cpu() if hasattr(x, "detach") else x).reshape(-1).astype(np.float64)
    F = [None] * int(N) if F is None else list(F)
    av, fsum = np.zeros_like(x), 0.0
    for f in F:
        y, fx = H.gradient(f, x)
        av += y
        fsum += float(np.real(fx))
    av /= max(len(F), 1)
    r = x - H.prox(g, x - gamma * av, gamma)[0]
    viol = 0.0
    if isinstance(g, Op.IndBox):
        lo, hi = np.asarray(g.lo, dtype=np.float64), np.asarray(g.hi, dtype=np.float64)
        viol = float(max(np.max(lo - x), np.max(x - hi), 0.0))
    rows = _rows(F) if (samples and isinstance(g, Op.NormL1)) else None
    if rows is not None and rows[0] == "logistic":
        grad_inf = float(np.max(np.abs(av))) if x.size else 0.0
        mu = float(g.lam)
        s = 1.0 if (grad_inf == 0 or mu <= 0) else min(1.0, mu / grad_inf)
        entropy = host_margin_stats("logistic", rows[1] @ x, rows[2], s)[1]
        return assemble(fsum / len(F), _gval(g, x), float(np.linalg.norm(r)) / gamma, grad_inf, float(x @ av), viol, mu=mu, entropy=entropy,
                        n=len(F))
    lasso = isinstance(g, Op.NormL1) and len(F) > 0 and all(isinstance(f, Op.LeastSquares) for f in F)
    return assemble(fsum / max(len(F), 1), _gval(g, x), float(np.linalg.norm(r)) / gamma, float(np.max(np.abs(av))) if x.size else 0.0,
                    float(x @ av), viol, mu=float(g.lam) if lasso else None)


def host_screen(grad, colsq, s, kappa, mu):
    """The gap-safe screening rule of ciao_screen in numpy (float64): keep[j] = not (s |grad_j| + kappa sqrt(colsq_j) < mu), a boolean
    d-vector; a NaN anywhere keeps the coordinate.  The same operations in the same order as csrc/colsq_kernels.h: screen_kernel (numpy
    contracts nothing either), so the two masks differ only where the left side is within rounding of mu (a device sqrt or a
    float32 -> float64 conversion cannot differ: both are exact / correctly rounded)."""
    g = np.abs(np.asarray(grad).astype(np.float64))
    with np.errstate(invalid="ignore"):
        lhs = float(s) * g + float(kappa) * np.sqrt(np.asarray(colsq, dtype=np.float64))
        return ~(lhs < float(mu))


def host_row_sqnorms(A):
    """The row sums of squares of ciao_row_sqnorms in numpy (float64): out[i] = sum_j |A[i,j]|^2, a complex row as its 2n reals.  The
    squares are what the device forms ((double)a * (double)a); the order of addition is numpy's, so the two agree to
    (d + 2) 2^-53 relative, not bitwise."""
    A = np.asarray(A)
    if np.iscomplexobj(A):
        A = np.ascontiguousarray(A).view(A.real.dtype).reshape(A.shape[0], -1)
    A = A.astype(np.float64)
    return np.sum(A * A, axis=1)


def host_lipschitz(kind, A, lam=1.0):
    """The per-sample smoothness constants of stepsize.lipschitz in numpy (float64): lam ||a_i||^2 for LeastSquares(a_i, b_i, lam) rows
    (kind "ls", real or complex; test_lasso.jl:52-56), ||a_i||^2 / 4 for logistic rows (kind "logistic"; test_logistic_l1.jl:39)."""
    if kind not in ("ls", "logistic"):
        raise ValueError(f"kind must be 'ls' or 'logistic' (got {kind!r})")
    return (float(lam) if kind == "ls" else 0.25) * host_row_sqnorms(A)


def host_col_moments(A, shift=None):
    """The shifted column sums of ciao_col_moments in numpy (float64) -> (s1, s2): s1[j] = sum_i (A[i,j] - c_j), s2[j] = sum_i
    (A[i,j] - c_j)^2 with c = shift or (None) the first row.  The differences and squares are what the device forms; the order of addition
    is numpy's, so the two agree to (N + 2) 2^-53 sum|a - c| and (N + 3) 2^-53 sum (a - c)^2, and bitwise where every sum is exact."""
    A = np.asarray(A)
    if A.ndim != 2 or np.iscomplexobj(A):
        raise ValueError("A must be a real N x d matrix")
    A = A.astype(np.float64)
    c = A[0] if shift is None else np.asarray(shift, dtype=np.float64)
    t = A - c[None, :]
    return np.sum(t, axis=0), np.sum(t * t, axis=0)


def host_gram(A, b, weights=None, rows=None):
    """The Gram statistics of ciao_gram in numpy (float64) -> (G, u, colsum, bsum): G = A'A, u = A'b, colsum = A'1, bsum = [sum b,
    sum b^2].  The products are what the device forms (float32 data is exact in float64, and so is every product of two of them); the
    order of addition is numpy's, so the two agree to (N + 8) 2^-53 sum_n |a_ni a_nj| per entry, and bitwise where every sum is exact.

    weights: a real N-vector w (ciao_gram_weighted) -> G = A'diag(w)A, u = A'(w b), colsum = A'w, bsum = [sum w b, sum w b^2, sum w].
    As on the device ONE operand of every product carries the weight, rounded once: G[i][j] = sum_n a_ni (w_n a_nj) for i <= j and the
    other triangle is its mirror; u[j] = sum_n a_nj (w_n b_n); colsum[j] = sum_n a_nj w_n; sum w b^2 = sum_n b_n (w_n b_n).  No square
    root of w: any finite weight, w = 1 gives the unweighted result bit for bit, a zero weight does not mask a non-finite element.
    The bound grows to (N + 10) 2^-53 sum_n |w_n a_ni a_nj|.

    rows: an integer M-vector of row numbers in [0, N), any order, repeats allowed (ciao_gram_rows) -> the statistics of the gathered
    copy A[rows], b[rows]; weights then has M elements, one per list position.  An empty list gives zeros."""
    A, b = np.asarray(A), np.asarray(b)
    if A.ndim != 2 or np.iscomplexobj(A) or np.iscomplexobj(b) or b.shape != (A.shape[0],):
        raise ValueError("A must be a real N x d matrix and b a real N-vector")
    if rows is not None:
        rows = np.asarray(rows)
        if rows.ndim != 1 or not np.issubdtype(rows.dtype, np.integer):
            raise ValueError("rows must be an integer vector of row numbers")
        if rows.size and (rows.min() < 0 or rows.max() >= A.shape[0]):
            raise ValueError(f"rows: entries must lie in [0, {A.shape[0]})")
        A, b = A[rows], b[rows]
    A, b = A.astype(np.float64), b.astype(np.float64)
    if weights is None:
        return A.T @ A, A.T @ b, np.sum(A, axis=0), np.array([np.sum(b), np.sum(b * b)])
    w = np.asarray(weights)
    if np.iscomplexobj(w) or w.shape != (A.shape[0],):
        raise ValueError("weights must be a real N-vector")
    w = w.astype(np.float64)
    WA, wb = w[:, None] * A, w * b
    G = np.triu(A.T @ WA)
    G = G + np.triu(G, 1).T
    return G, A.T @ wb, A.T @ w, np.array([np.sum(wb), b @ wb, np.sum(w)])


def _list_rows(A, rows):
    """A (a real N x d matrix) gathered over `rows` as float64, by host_gram's validation of the list; rows=None: every row in order."""
    A = np.asarray(A)
    if A.ndim != 2 or np.iscomplexobj(A):
        raise ValueError("A must be a real N x d matrix")
    if rows is not None:
        rows = np.asarray(rows)
        if rows.ndim != 1 or not np.issubdtype(rows.dtype, np.integer):
            raise ValueError("rows must be an integer vector of row numbers")
        if rows.size and (rows.min() < 0 or rows.max() >= A.shape[0]):
            raise ValueError(f"rows: entries must lie in [0, {A.shape[0]})")
        A = A[rows]
    return A.astype(np.float64)


def host_list_dots(A, x, rows=None):
    """ciao_list_dots in numpy (float64): out[m] = a_{rows[m]}'x, an M-vector (rows=None: every row in order).  The products are what
    the device forms ((double)a * (double)x: exact for float32 data); the order of addition is numpy's, so the two agree to
    (d + 2) 2^-53 sum_j |a_j x_j| each from the exact value, and bitwise where every sum is exact.  An empty list gives an empty vector."""
    A = _list_rows(A, rows)
    x = np.asarray(x)
    if np.iscomplexobj(x) or x.shape != (A.shape[1],):
        raise ValueError("x must be a real d-vector")
    return A @ x.astype(np.float64)


def host_list_combine(A, c, rows=None):
    """ciao_list_combine in numpy (float64): out[j] = sum_m c[m] A[rows[m], j], a d-vector (rows=None: every row in order; c has one
    element per list position).  The products are what the device forms (c * (double)a, rounded once); the order of addition is numpy's,
    so the two agree to (M + 3) 2^-53 sum_m |c_m a_mj| each from the exact value, and bitwise where every sum is exact.  An empty list
    gives zeros."""
    A = _list_rows(A, rows)
    c = np.asarray(c)
    if np.iscomplexobj(c) or c.shape != (A.shape[0],):
        raise ValueError("c must be a real vector with one element per list position")
    return A.T @ c.astype(np.float64)


def host_gram_cd(G, u, inv, tau, X, tol, max_sweeps):
    """ciao_gram_cd in numpy (float64) -> (X, R, stat): cyclic coordinate descent with covariance updates on a Gram matrix, the
    SPECIFICATION of the device kernel (csrc/gramcd_kernels.h) and its CPU twin -- the two agree bit for bit.
    G: d x d (only row j is read for coordinate j); u, inv: d (inv_j = 1 / G_jj where G_jj > 0, else 0); tau: K; X: K x d warm starts
    (not modified; the results are returned); tol >= 0; 1 <= max_sweeps.  R: the final r = u - G x as accumulated; stat: K x 4 =
    {sweeps, non-zero updates, largest change of the last completed full sweep, state (1 converged, 0 budget spent, 2 not finite)}.
    Row-vector operations only, so every product is rounded before it is added, as in the kernel."""
    G, u, inv = np.asarray(G, np.float64), np.asarray(u, np.float64), np.asarray(inv, np.float64)
    tau = np.asarray(tau, np.float64).reshape(-1)
    X = np.array(X, dtype=np.float64, ndmin=2)
    K, d = X.shape
    if G.shape != (d, d) or u.shape != (d,) or inv.shape != (d,) or tau.shape != (K,):
        raise ValueError("host_gram_cd: G must be d x d, u and inv d-vectors, tau a K-vector and X K x d")
    if not (tol >= 0) or max_sweeps < 1:
        raise ValueError("host_gram_cd: tol must be >= 0 and max_sweeps >= 1")
    R = np.empty((K, d))
    stat = np.zeros((K, 4))
    diag = np.diagonal(G).copy()
    with np.errstate(all="ignore"):
        for k in range(K):
            x, t = X[k], tau[k]
            r = u.copy()
            for j in np.flatnonzero(x != 0):
                r -= x[j] * G[j]
            sweeps, nupd, last_full, state, active = 0, 0, 0.0, 0, False
            while True:
                if sweeps >= max_sweeps:
                    state = 0
                    break
                sweeps += 1
                big, support, bad = 0.0, False, False
                for j in range(d):
                    xj = x[j]
                    if active and xj == 0:
                        continue
                    rho = r[j] + diag[j] * xj
                    a = abs(rho) - t
                    if a <= 0 and xj == 0:
                        continue                      # x+ = 0 = x_j: nothing moves
                    xp = 0.0 if a <= 0 else np.copysign(a, rho) * inv[j]
                    delta = xp - xj
                    if not np.isfinite(delta):
                        bad = True
                        break
                    if delta != 0:
                        r -= delta * G[j]
                        x[j] = xp
                        nupd += 1
                        ch = diag[j] * (delta * delta)
                        if ch > big:
                            big = ch
                        if (xj == 0) != (xp == 0):
                            support = True
                if bad:
                    state = 2
                    break
                if not active:
                    last_full = big
                    if big <= tol and not support:
                        state = 1
                        break
                    active = True
                elif big <= tol:
                    active = False
            R[k] = r
            stat[k] = (sweeps, nupd, last_full, state)
    return X, R, stat


def host_gram_cd_general(G, u, inv, tau, X, tol, max_sweeps, gsel=None, pf=None, lo=None, hi=None):
    """ciao_gram_cd_general in numpy (float64) -> (X, R, stat): host_gram_cd with bounds lo <= x <= hi, a penalty factor per coordinate,
    a ridge term (through inv alone) and a Gram matrix, u and tol per model; the SPECIFICATION of the device kernel
    (csrc/gramcdg_kernels.h) -- the two agree bit for bit.  Model k minimises over lo_kj <= x_j <= hi_kj
        1/2 x'G x - u_k'x + sum_j t_kj |x_j| + (ridge_k / 2) sum_j x_j^2,     G = G[gsel[k]],   t_kj = tau_k pf_kj (one rounded product)
    G: d x d or S x d x d; gsel: K set numbers (None: set 0); u, inv, pf, lo, hi: d (shared) or K x d; inv_kj = 1 / (G_jj + ridge_k)
    where that is > 0, else 0; pf, lo, hi None: 1, -inf, +inf; tol: a number or K of them; tau: K; X: K x d warm starts (not modified).
    update(j) is host_gram_cd's with a = |rho| - t_kj and, after x+ is formed, `if x+ > hi: x+ = hi; if x+ < lo: x+ = lo` (comparisons,
    so a NaN goes through to state 2).  A model that cannot run -- gsel[k] outside [0, S); tol_k < 0 or NaN; a pf_kj < 0 or NaN; a t_kj
    NaN; lo_kj > 0, hi_kj < 0 or either NaN -- ends with state 3: stat = (0, 0, 0, 3), its row of X as given, its row of R NaN (the
    device leaves that row of R unwritten).  With the defaults the results are host_gram_cd's bit for bit."""
    G = np.asarray(G, np.float64)
    if G.ndim == 2:
        G = G[None]
    tau = np.asarray(tau, np.float64).reshape(-1)
    X = np.array(X, dtype=np.float64, ndmin=2)
    K, d = X.shape
    if G.ndim != 3 or G.shape[1:] != (d, d) or G.shape[0] < 1 or tau.shape != (K,):
        raise ValueError("host_gram_cd_general: G must be d x d or S x d x d, tau a K-vector and X K x d")
    S = G.shape[0]

    def vec(v, name, default):
        if v is None:
            return np.full((K, d), default)
        v = np.asarray(v, np.float64)
        if v.shape == (d,):
            return np.broadcast_to(v, (K, d))
        if v.shape != (K, d):
            raise ValueError(f"host_gram_cd_general: {name} must be a d-vector (shared) or K x d")
        return v

    if u is None or inv is None:
        raise ValueError("host_gram_cd_general: u and inv are needed")
    U, INV = vec(u, "u", 0.0), vec(inv, "inv", 0.0)
    PF, LO, HI = vec(pf, "pf", 1.0), vec(lo, "lo", -np.inf), vec(hi, "hi", np.inf)
    tol = np.asarray(tol, np.float64)
    tol = np.full(K, float(tol)) if tol.ndim == 0 else tol.reshape(-1)
    sel = np.zeros(K, np.int64) if gsel is None else np.asarray(gsel).astype(np.int64).reshape(-1)
    if tol.shape != (K,) or sel.shape != (K,) or max_sweeps < 1:
        raise ValueError("host_gram_cd_general: tol and gsel must have K elements and max_sweeps must be >= 1")
    R = np.full((K, d), np.nan)
    stat = np.zeros((K, 4))
    with np.errstate(all="ignore"):
        for k in range(K):
            t = tau[k] * PF[k]
            if (not 0 <= sel[k] < S or not tol[k] >= 0 or not (PF[k] >= 0).all() or np.isnan(t).any()
                    or not (LO[k] <= 0).all() or not (HI[k] >= 0).all()):
                stat[k] = (0, 0, 0, 3)
                continue
            Gk = G[sel[k]]
            diag = np.diagonal(Gk).copy()
            x, inv_k, lo_k, hi_k, tol_k = X[k], INV[k], LO[k], HI[k], tol[k]
            r = U[k].copy()
            for j in np.flatnonzero(x != 0):
                r -= x[j] * Gk[j]
            sweeps, nupd, last_full, state, active = 0, 0, 0.0, 0, False
            while True:
                if sweeps >= max_sweeps:
                    state = 0
                    break
                sweeps += 1
                big, support, bad = 0.0, False, False
                for j in range(d):
                    xj = x[j]
                    if active and xj == 0:
                        continue
                    rho = r[j] + diag[j] * xj
                    a = abs(rho) - t[j]
                    if a <= 0 and xj == 0:
                        continue                      # x+ = 0 = x_j: nothing moves
                    xp = 0.0 if a <= 0 else np.copysign(a, rho) * inv_k[j]
                    if xp > hi_k[j]:
                        xp = hi_k[j]
                    if xp < lo_k[j]:
                        xp = lo_k[j]
                    delta = xp - xj
                    if not np.isfinite(delta):
                        bad = True
                        break
                    if delta != 0:
                        r -= delta * Gk[j]
                        x[j] = xp
                        nupd += 1
                        ch = diag[j] * (delta * delta)
                        if ch > big:
                            big = ch
                        if (xj == 0) != (xp == 0):
                            support = True
                if bad:
                    state = 2
                    break
                if not active:
                    last_full = big
                    if big <= tol_k and not support:
                        state = 1
                        break
                    active = True
                elif big <= tol_k:
                    active = False
            R[k] = r
            stat[k] = (sweeps, nupd, last_full, state)
    return X, R, stat


def host_standardize(A, b=None, center=True, scale=True, refine=True):
    """standardize.standardize in numpy on a host matrix -> (A_std, b_std, mean, scale, b_mean).  The moments are
    standardize.host_column_moments' (the same shift, the same refinement rule, the same default: always refined); scale_j = 1 / sqrt(var_j) with the population variance, 1
    where var_j = 0; A_std = ((float64(A) - mean) * scale) rounded to A's dtype once, which is bitwise what ciao_scale_columns computes
    from the same mean and scale.  b (LeastSquares targets) is centred when `center`; pass None for logistic labels: b_std = None,
    b_mean = 0.  center=False / scale=False leave mean = 0 / scale = 1."""
    from .standardize import host_column_moments
    A = np.asarray(A)
    m = host_column_moments(A, refine=refine)
    d = A.shape[1]
    mean = m.mean if center else np.zeros(d)
    sc = np.ones(d)
    if scale:
        nz = m.var > 0
        sc[nz] = 1.0 / np.sqrt(m.var[nz])
    A_std = ((A.astype(np.float64) - mean[None, :]) * sc[None, :]).astype(A.dtype)
    b_mean, b_std = 0.0, None
    if b is not None:
        b = np.asarray(b)
        if center:
            b_mean = float(np.mean(b.astype(np.float64)))
            b_std = (b.astype(np.float64) - b_mean).astype(b.dtype)
        else:
            b_std = b.copy()
    return A_std, b_std, mean, sc, b_mean


def announce(why):
    warnings.warn("CIAOAlgorithms (AMD): this problem runs on the HOST route -- numpy, one operator call per sample, no GPU -- "
                  f"because {why}.  It is orders of magnitude slower than the device path and none of this package's "
                  "performance or parity statements apply to it.", RuntimeWarning, stacklevel=3)

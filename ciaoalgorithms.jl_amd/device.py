"""Device-side plumbing: a `Context` (ciao_ctx handle bound to a torch HIP stream) and typed wrappers that pass torch
device tensors to the C ABI.  PyTorch is used here only for device memory, streams and (in parallel.py)
torch.distributed -- all arithmetic happens in libciao_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L

_DT = {torch.float32: L.F32, torch.float64: L.F64}
_NP2T = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}


def torch_dtype(R) -> torch.dtype:
    """Map the reference's real type parameter `R` (numpy/torch dtype or python float) to a torch dtype."""
    if isinstance(R, torch.dtype):
        if R not in _DT:
            raise TypeError(f"only float32/float64 are supported on the device path, got {R}")
        return R
    if R is float:
        return torch.float64
    return _NP2T[np.dtype(R)]


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class PackedF:
    """F = [f_1 .. f_N] packed for the device: row-major A (N x d), b (targets or labels), loss kind, LeastSquares λ.

    Replaces the reference's Vector of N one-row operator objects (test/test_lasso.jl:50-58).  `N_total` is the global
    sample count when A holds only this rank's row shard (parallel.py); `row0` is the global index of local row 0.
    """

    def __init__(self, loss: int, A: torch.Tensor | None, b: torch.Tensor | None, lam: float = 1.0, N_total: int | None = None,
                 row0: int = 0, d: int | None = None, dtype: torch.dtype | None = None, N: int | None = None,
                 cyclic: tuple[int, int] | None = None):
        self.loss = int(loss)
        # row ownership of a shard: contiguous block [row0, row0+N) (default), or cyclic=(rank, world): this rank owns the
        # global rows i with i % world == rank, stored in order (local row = i // world).  Cyclic ownership spreads every
        # static contiguous Finito batch (Finito_basic.jl:52-58) evenly over the ranks.
        self.cyclic = cyclic
        if A is not None:
            assert A.is_cuda and A.dim() == 2 and A.stride(1) == 1, "A must be a row-major device matrix"
            assert A.dtype in _DT, f"unsupported dtype {A.dtype}"
            self.N, self.d = int(A.shape[0]), int(A.shape[1])
            self.ld = int(A.stride(0)) if self.N > 1 else self.d
            self.dtype = A.dtype
            self.device = A.device
        else:  # F = fill(Zero(), N): no data at all (SVRG.jl:58)
            assert loss == L.LOSS_ZERO and d is not None and dtype is not None and N is not None
            self.N, self.d, self.ld, self.dtype = int(N), int(d), int(d), dtype
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.complex = (self.loss == L.LOSS_LS_COMPLEX)   # vectors are (re, im) pairs of the real dtype: d counts reals
        if self.complex:
            assert self.d % 2 == 0 and self.ld % 2 == 0, "complex rows are (re, im) pairs: an even number of reals"
        if b is not None:
            assert b.is_cuda and b.dtype == self.dtype and b.is_contiguous() and b.shape == ((2 if self.complex else 1) * self.N,)
        elif loss != L.LOSS_ZERO:
            raise ValueError("b (targets / labels) is required for LeastSquares and logistic F")
        self.A, self.b, self.lam = A, b, float(lam)
        # Feature padding (operators.pack_F(pad_to=...)): the rows carry self.d - padded_from zero columns, and the solver's state
        # vectors are length-padded_from VIEWS of length-self.d buffers.  None: every vector must have exactly self.d elements.
        self.padded_from: int | None = None
        self.N_total = int(N_total) if N_total is not None else self.N
        self.row0 = int(row0)
        self._c = L.Problem(self.loss, _DT[self.dtype], self.N, self.d, max(self.ld, self.d), self.N_total,
                            A.data_ptr() if (A is not None and self.N > 0) else None,
                            b.data_ptr() if (b is not None and self.N > 0) else None, self.lam)

    @property
    def ref(self):
        return C.byref(self._c)

    def localise(self, idx):
        """Global sample indices -> the local row indices of the members this shard owns (order preserved)."""
        import numpy as _np
        idx = _np.asarray(idx, dtype=_np.int64)
        if self.N == self.N_total and self.cyclic is None:
            return idx
        if self.cyclic is not None:
            rank, world = self.cyclic
            return idx[idx % world == rank] // world
        sel = idx[(idx >= self.row0) & (idx < self.row0 + self.N)]
        return sel - self.row0

    def local_blocks(self, lo, hi):
        """Global row blocks [lo[t], hi[t]) -> (first, length) of the LOCAL rows this shard owns of each: again contiguous
        blocks, under both ownership rules (block: clip to [row0, row0+N); cyclic: local row = i // world for i % world == rank)."""
        import numpy as _np
        lo = _np.asarray(lo, dtype=_np.int64)
        hi = _np.asarray(hi, dtype=_np.int64)
        if self.N == self.N_total and self.cyclic is None:
            return lo, hi - lo
        if self.cyclic is not None:
            rank, world = self.cyclic
            f = (lo - rank + world - 1) // world          # first local row whose global index is >= lo
            e = (hi - rank + world - 1) // world          # first local row whose global index is >= hi
            f = _np.maximum(f, 0)
            return f, _np.maximum(e - f, 0)
        f = _np.clip(lo, self.row0, self.row0 + self.N) - self.row0
        e = _np.clip(hi, self.row0, self.row0 + self.N) - self.row0
        return f, e - f

    def local_slice(self, vec):
        """The entries of a global N_total-vector (L, gamma) that belong to this shard's rows."""
        if self.N == self.N_total and self.cyclic is None:
            return vec
        if self.cyclic is not None:
            rank, world = self.cyclic
            return vec[rank::world]
        return vec[self.row0:self.row0 + self.N]

    # reference-style constructors --------------------------------------------------------------------------------
    @staticmethod
    def least_squares(A, b, lam=1.0, **kw):
        """f_i = LeastSquares(A[i:i,:], b[i:i], lam)  (test/test_lasso.jl:52-54)"""
        return PackedF(L.LOSS_LS, A, b, lam, **kw)

    @staticmethod
    def least_squares_complex(A_pairs, b_pairs, lam=1.0, **kw):
        """Complex T (CIAOAlgorithms.jl:3; test_lasso.jl:3): f_i = LeastSquares(A[i:i,:], b[i:i], lam) with complex A, b given as
        interleaved (re, im) pairs of the real dtype: A_pairs is N x 2n, b_pairs has 2N entries (torch.view_as_real)."""
        return PackedF(L.LOSS_LS_COMPLEX, A_pairs, b_pairs, lam, **kw)

    @staticmethod
    def logistic(A, y, **kw):
        """f_i = Precompose(LogisticLoss([y_i], 1.0), A[i:i,:], 1.0)  (test/test_logistic_l1.jl:36)"""
        return PackedF(L.LOSS_LOGISTIC, A, y, 1.0, **kw)

    @staticmethod
    def zero(N, d, dtype):
        return PackedF(L.LOSS_ZERO, None, None, 0.0, d=d, dtype=dtype, N=N)


class PackedSepQuad:
    """F = [f_1..f_N] with f_i = Sum(Quadratic(diagm(Q_i), q_i), SqrDistL2(IndBox(lo, hi), eta)) packed for the device
    (the operator family of test/test_sharing.jl:16-25): q row-major N x d; Q the N x d diagonals, or N x d x d dense blocks."""

    def __init__(self, Q: torch.Tensor, q: torch.Tensor, eta: float = 0.0, lo: float = 0.0, hi: float = 0.0,
                 N_total: int | None = None, row0: int = 0):
        assert Q.is_cuda and q.is_cuda and q.dim() == 2 and Q.dtype == q.dtype and Q.dtype in _DT
        assert Q.is_contiguous() and q.is_contiguous()
        # Q of shape N x d: the diagonals (the reference test's diagm); N x d x d: one dense matrix per agent
        self.dense = Q.dim() == 3
        assert (Q.shape == (q.shape[0], q.shape[1], q.shape[1])) if self.dense else (Q.shape == q.shape)
        self.Q, self.q, self.eta, self.lo, self.hi = Q, q, float(eta), float(lo), float(hi)
        self.N, self.d = int(q.shape[0]), int(q.shape[1])
        self.dtype, self.device = Q.dtype, Q.device
        self.N_total = int(N_total) if N_total is not None else self.N
        self.row0, self.cyclic = int(row0), None
        self._c = L.SepQuad(_DT[self.dtype], int(self.dense), self.N, self.d, self.d, self.N_total, Q.data_ptr() if self.N else None,
                            q.data_ptr() if self.N else None, self.eta, self.lo, self.hi)

    @property
    def ref(self):
        return C.byref(self._c)

    localise = PackedF.localise
    local_slice = PackedF.local_slice
    local_blocks = PackedF.local_blocks


class ProxG:
    """g packed for the device: Zero / NormL1(λ) / IndBox(lo, hi)."""

    def __init__(self, kind=L.PROX_ZERO, lam=0.0, lo=-float("inf"), hi=float("inf"), lo_vec=None, hi_vec=None):
        self.kind, self.lam, self.lo, self.hi = int(kind), float(lam), float(lo), float(hi)
        self.lo_vec, self.hi_vec = lo_vec, hi_vec  # keep the device tensors alive
        self._c = L.ProxDesc(self.kind, 0, self.lam, self.lo, self.hi,
                             lo_vec.data_ptr() if lo_vec is not None else None,
                             hi_vec.data_ptr() if hi_vec is not None else None)

    @property
    def ref(self):
        return C.byref(self._c)


class LogisticStats(NamedTuple):
    """Context.margin_stats on logistic rows, t_i = y_i a_i'x."""
    loss_sum: float     # sum_i log(1 + exp(-t_i))
    entropy: float      # E(s) = sum_i h(s sigma(-t_i)), h(u) = u log u + (1 - u) log(1 - u)
    errors: float       # the number of samples with t_i <= 0
    min_margin: float   # min_i t_i


class LeastSquaresStats(NamedTuple):
    """Context.margin_stats on LeastSquares rows, r_i = a_i'x - b_i."""
    sum_r2: float       # sum_i r_i^2
    sum_b: float        # sum_i b_i
    sum_b2: float       # sum_i b_i^2
    max_abs_r: float    # max_i |r_i|


class RowNormStats(NamedTuple):
    """Context.row_sqnorm_stats: the summary of the row sums of squares ||a_i||^2 over the N local rows."""
    max: float          # max_i ||a_i||^2 (NaN where any row holds a NaN)
    argmax: int         # the smallest row index that attains it
    min: float          # min_i ||a_i||^2
    sum: float          # sum_i ||a_i||^2 = ||A||_F^2 = trace(A'A)


class _ChainBatch:
    """Context manager of Context.chain_batch()."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        L.check(self.ctx.lib.ciao_ctx_chain_batch_begin(self.ctx._h))
        self.ctx._batch_keep = []
        return self.ctx

    def __exit__(self, et, ev, tb):
        keep, self.ctx._batch_keep = self.ctx._batch_keep, None
        st = self.ctx.lib.ciao_ctx_chain_batch_end(self.ctx._h, 1 if et is None else 0)
        self.ctx._batch_last_idx = keep      # (the launch reads them: alive until the next batch or the ctx goes)
        if et is None:
            L.check(st)
        return False


class Context:
    """One device + one HIP stream + the library's private workspace (ciao_ctx).  Not thread-safe."""

    def __init__(self, device: int | None = None, stream: "torch.cuda.Stream | None" = None):
        self.lib = L.load()  # raises if the extension is not built
        if device is None:
            device = torch.cuda.current_device() if torch.cuda.is_available() else 0
        self.device = int(device)
        self._h = C.c_void_p()
        if stream is None and torch.cuda.is_available():
            stream = torch.cuda.current_stream(self.device)
        self.stream = stream
        handle = C.c_void_p(stream.cuda_stream) if stream is not None else None
        L.check(self.lib.ciao_ctx_create(self.device, handle, C.byref(self._h)))
        self._hook_keepalive = None
        self._rccl_keepalive = None
        self._peers_keepalive = None
        self._batch_keep = None        # index tensors of an open chain batch (kept alive until its launch is enqueued)
        self.shards = None

    # -- lifetime ----------------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.ciao_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        """Wait for the stream and surface a sticky device-side error (an out-of-range sample index)."""
        L.check(self.lib.ciao_ctx_synchronize(self._h))

    def set_option(self, key: str, value: int):
        L.check(self.lib.ciao_ctx_set_option(self._h, key.encode(), int(value)))

    def timing_enable(self, on: bool = True):
        L.check(self.lib.ciao_ctx_timing_enable(self._h, 1 if on else 0))

    def timing_read(self) -> tuple[float, int]:
        """(summed device ms of the dominant-kernel launches since the last read, their count); synchronises."""
        ms, n = C.c_double(0.0), C.c_int64(0)
        L.check(self.lib.ciao_ctx_timing_read(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def last_kernel(self) -> str:
        return self.lib.ciao_ctx_last_kernel(self._h).decode()

    def set_allreduce(self, fn):
        """fn(buf_ptr:int, count:int, dtype:int, stream_ptr:int) -> int (0 = ok); None clears the hook."""
        if fn is None:
            self._hook_keepalive = None
            L.check(self.lib.ciao_ctx_set_allreduce(self._h, L.ALLREDUCE_FN(0), None))
            return

        def _tramp(_user, buf, count, dtype, stream):
            try:
                return int(fn(buf, count, dtype, stream))
            except Exception as e:  # never let a Python exception unwind through C
                import sys
                print(f"[ciao] all-reduce hook raised: {e!r}", file=sys.stderr)
                return 1

        cb = L.ALLREDUCE_FN(_tramp)
        self._hook_keepalive = cb
        L.check(self.lib.ciao_ctx_set_allreduce(self._h, cb, None))

    def set_monitor(self, g: "ProxG | None", obj: "torch.Tensor | None"):
        """Objective monitor (include/ciao_hip.h: ciao_ctx_set_monitor): `obj` is a device float64[3] that every full pass
        fills with {F(x), (1/N) sum f_i(x), g(x)}; obj=None switches it off."""
        if obj is None:
            self._monitor_keepalive = None
            L.check(self.lib.ciao_ctx_set_monitor(self._h, None, None))
            return
        assert obj.is_cuda and obj.dtype == torch.float64 and obj.is_contiguous() and obj.numel() >= 3
        self._monitor_keepalive = (g, obj)
        L.check(self.lib.ciao_ctx_set_monitor(self._h, g.ref if g is not None else None, _ptr(obj)))

    def set_shards(self, table: "L.ShardTable | None"):
        """Row-sharded problem for the sequential chains (include/ciao_hip.h: ciao_ctx_set_shards); None removes it."""
        L.check(self.lib.ciao_ctx_set_shards(self._h, C.byref(table) if table is not None else None))
        self.shards = table

    def set_peers(self, group: "parallel.PeerGroup | None"):
        """One-shot peer all-reduce (include/ciao_hip.h: ciao_ctx_set_peers): `group` is a parallel.PeerGroup whose mailboxes are
        exchanged and mapped; None turns it off."""
        if group is None:
            self._peers_keepalive = None
            L.check(self.lib.ciao_ctx_set_peers(self._h, 0, 0, None, 0))
            return
        self._peers_keepalive = group
        arr = (C.c_void_p * group.world)(*group.mailboxes)
        L.check(self.lib.ciao_ctx_set_peers(self._h, group.rank, group.world, arr, group.max_elems))

    def peer_allreduce(self, t: torch.Tensor):
        """In-place sum over the ranks of a float32 / float64 device tensor through the peer mailboxes (bench / tests)."""
        assert t.is_cuda and t.is_contiguous() and t.dtype in (torch.float32, torch.float64)
        L.check(self.lib.ciao_peer_allreduce(self._h, L.F64 if t.dtype == torch.float64 else L.F32, t.numel(), C.c_void_p(t.data_ptr())))

    def set_rccl(self, comm):
        """Native all-reduce: `comm` is a parallel.RcclComm (or None to clear).  The library then calls ncclAllReduce itself on
        its stream -- no Python callback per reduction (include/ciao_hip.h: ciao_ctx_set_rccl)."""
        if comm is None:
            self._rccl_keepalive = None
            L.check(self.lib.ciao_ctx_set_rccl(self._h, None, None))
            return
        self._rccl_keepalive = comm
        self._hook_keepalive = None
        L.check(self.lib.ciao_ctx_set_rccl(self._h, comm.handle, comm.lib_path.encode()))

    def is_row_sharded(self) -> bool:
        """True while this context sums over other ranks' rows: an all-reduce hook (set_allreduce), an RCCL communicator (set_rccl),
        a shard table (set_shards) or peer mailboxes (set_peers) is set."""
        return (self._hook_keepalive is not None or self._rccl_keepalive is not None or self.shards is not None
                or self._peers_keepalive is not None)

    # -- helpers -------------------------------------------------------------------------------------------------------
    def _vec(self, t: torch.Tensor, p: PackedF, name: str, n: int | None = None):
        n = p.d if n is None else n
        # A length-padded_from VIEW of a longer buffer is taken for the p.d-vector it heads -- only for a problem whose rows the host
        # mirror padded itself (PackedF.padded_from, set by operators.pack_F(pad_to=...): solvers._Iterable owns those buffers and
        # made them p.d long).  For every other problem the length must be exact: the kernels read and write all p.d coordinates,
        # and a caller's big[:d-1] would be written one element past its end.
        ok = isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == p.dtype and t.is_contiguous()
        if ok and t.numel() != n:
            es = t.element_size()
            ok = (n == p.d and getattr(p, "padded_from", None) is not None and t.numel() == p.padded_from and
                  t.untyped_storage().nbytes() >= (t.storage_offset() + n) * es)
        if not ok:
            raise ValueError(f"{name}: need a contiguous {p.dtype} device vector of length {n}, got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', '?')}")
        return _ptr(t)

    def _idx(self, idx) -> torch.Tensor:
        if isinstance(idx, torch.Tensor):
            assert idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous()
            return idx
        t = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(f"cuda:{self.device}", non_blocking=False)
        # The (synchronous) upload ran on torch's current stream; the kernels that read `t` run on the ctx's stream and may
        # still be running when the caller drops `t`: tell the caching allocator, or it hands the block out again too early.
        if self.stream is not None:
            t.record_stream(self.stream)
        return t

    def sample_uniform(self, seed: int, pos: int, N: int, m: int) -> torch.Tensor:
        """m uniform draws from 0..N-1 of the injected index stream (outputs pos .. pos+m-1), generated on the device
        (ciao_sample_uniform): the values sampling.IndexStream.rand_indices produces on the host."""
        out = torch.empty(int(m), dtype=torch.int64, device=f"cuda:{self.device}")
        L.check(self.lib.ciao_sample_uniform(self._h, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint64(int(pos)), int(N), int(m),
                                             C.c_void_p(out.data_ptr())))
        if self.stream is not None:
            out.record_stream(self.stream)
        return out

    # -- L1 plugin API ----------------------------------------------------------------------------------------------
    def gradient(self, p: PackedF, i: int, x, y, fval=None):
        L.check(self.lib.ciao_gradient(self._h, p.ref, int(i), self._vec(x, p, "x"), self._vec(y, p, "y"), _ptr(fval)))

    def prox(self, g: ProxG, x: torch.Tensor, gamma: float, y: torch.Tensor):
        assert x.is_cuda and y.is_cuda and x.dtype == y.dtype and x.is_contiguous() and y.is_contiguous()
        L.check(self.lib.ciao_prox(self._h, _DT[x.dtype], x.numel(), g.ref, _ptr(x), float(gamma), _ptr(y)))

    # -- sweep -------------------------------------------------------------------------------------------------------------
    def full_gradient(self, p: PackedF, x, av):
        L.check(self.lib.ciao_full_gradient(self._h, p.ref, self._vec(x, p, "x"), self._vec(av, p, "av")))

    def proxgrad_step(self, p: PackedF, g: ProxG, gamma: float, x, av, y):
        L.check(self.lib.ciao_proxgrad_step(self._h, p.ref, g.ref, float(gamma), self._vec(x, p, "x"), self._vec(av, p, "av"),
                                            self._vec(y, p, "y")))

    def objective(self, p: PackedF, g: ProxG, x) -> float:
        out = C.c_double(0.0)
        L.check(self.lib.ciao_objective(self._h, p.ref, g.ref, self._vec(x, p, "x"), C.byref(out)))
        return out.value

    def certificate(self, F, g, x, gamma: float, av=None, fval: float | None = None, samples: bool = False):
        """Optimality certificate at x (include/ciao_hip.h: ciao_certificate) -> certificate.CertificateResult; synchronises.

        av=None: one full pass is made (F(x) and grad f(x) together).  av = the caller's grad f(x) (SVRG: state.av where
        x = z_full): no pass over A; F(x) is then `fval` where the caller knows it and nan otherwise -- and with it `objective`
        and `gap`.  The gap is the lasso's (LeastSquares rows, NormL1(mu), mu > 0) and nan elsewhere: the logistic dual needs
        per-sample terms.  Real problems only; the sharing family has no certificate.

        samples=True (ciao_certificate_samples): the call's own pass also keeps the row dots and a second reduction, over the N
        samples, adds those terms: for logistic rows with NormL1(mu), mu > 0 the gap is F + g + E / N; the
        other fields, and the lasso's gap, are bitwise what samples=False gives.  av / fval must then be None; not on a row-sharded
        context."""
        from .certificate import assemble
        if isinstance(F, PackedSepQuad):
            raise L.CiaoError(L.ERR_ARG, "the certificate covers finite sums of LeastSquares / logistic rows, not the sharing problem")
        if samples:
            if av is not None or fval is not None:
                raise L.CiaoError(L.ERR_ARG, "certificate(samples=True) makes its own pass (it needs the row dots): av= and fval= must be None")
            return self.certificate_samples(F, g, x, gamma)[0]
        out = (C.c_double * 6)(float("nan") if fval is None else float(fval))
        L.check(self.lib.ciao_certificate(self._h, F.ref, g.ref if g is not None else None, self._vec(x, F, "x"),
                                          None if av is None else self._vec(av, F, "av"), float(gamma), out))
        mu = g.lam if (g is not None and F.loss == L.LOSS_LS and g.kind == L.PROX_L1) else None
        return assemble(*out, mu=mu)

    def certificate_samples(self, F, g, x, gamma: float):
        """certificate(samples=True) together with the per-sample statistics it rests on (include/ciao_hip.h:
        ciao_certificate_samples) -> (certificate.CertificateResult, LogisticStats | LeastSquaresStats): the statistics are
        margin_stats of the pass's own row dots at s = min(1, mu / grad_inf) for g = NormL1(mu), mu > 0 (s = 1 where grad f = 0 and
        for every other g); synchronises."""
        from .certificate import assemble
        if isinstance(F, PackedSepQuad):
            raise L.CiaoError(L.ERR_ARG, "the certificate covers finite sums of LeastSquares / logistic rows, not the sharing problem")
        out = (C.c_double * 10)()
        L.check(self.lib.ciao_certificate_samples(self._h, F.ref, g.ref if g is not None else None, self._vec(x, F, "x"), float(gamma), out))
        l1 = g is not None and g.kind == L.PROX_L1
        if F.loss == L.LOSS_LOGISTIC:
            return assemble(*out[:6], mu=g.lam if l1 else None, entropy=out[7], n=F.N_total), LogisticStats(*out[6:])
        return assemble(*out[:6], mu=g.lam if l1 else None), LeastSquaresStats(*out[6:])

    def row_dots(self, F, x, out=None):
        """out[i] = a_i'x for the N local rows of F (include/ciao_hip.h: ciao_row_dots) -> a device N-vector of F's dtype: the
        per-sample predictions (LeastSquares) or scores (logistic: the margin is y_i a_i'x).  One full pass; does not synchronise."""
        if isinstance(F, PackedSepQuad):
            raise L.CiaoError(L.ERR_ARG, "row dots exist for LeastSquares / logistic rows, not for the sharing problem")
        if out is None:
            out = torch.empty(F.N, dtype=F.dtype, device=f"cuda:{self.device}")
            if self.stream is not None:
                out.record_stream(self.stream)
        self._vec(out, F, "out", F.N)
        L.check(self.lib.ciao_row_dots(self._h, F.ref, self._vec(x, F, "x"), _ptr(out) if F.N > 0 else None))
        return out

    def margin_stats(self, F, dots, s: float = 1.0):
        """The per-sample reduction of `dots` (a device N-vector, e.g. row_dots(F, x)) against F's targets / labels
        (include/ciao_hip.h: ciao_margin_stats) -> LogisticStats or LeastSquaresStats; synchronises."""
        if isinstance(F, PackedSepQuad):
            raise L.CiaoError(L.ERR_ARG, "margin statistics exist for LeastSquares / logistic rows, not for the sharing problem")
        out = (C.c_double * 4)()
        L.check(self.lib.ciao_margin_stats(self._h, F.ref, self._vec(dots, F, "dots", F.N), float(s), out))
        return (LogisticStats if F.loss == L.LOSS_LOGISTIC else LeastSquaresStats)(*out)

    def margin_stats_multi(self, F, xs, s=None, rows=None, offsets=None, check_rows=True):
        """margin_stats of the row dots a_i'x_k for K iterates in ONE pass over A, without the N x K dots (include/ciao_hip.h:
        ciao_margin_stats_multi) -> a list of K LogisticStats or LeastSquaresStats.  xs: a list of 1..256 device d-vectors; s: None
        (= 1 for every model), one number, or K numbers in [0, 1].  Synchronises.

        rows: a contiguous int64 device vector of M >= 1 local row numbers, any order, repeats allowed -> the statistics over A[rows],
        b[rows] at the cost of the rows touched (include/ciao_hip.h: ciao_margin_stats_multi_rows), BIT FOR BIT
        what the call without a list gives on that gathered copy.  offsets: K finite numbers, model k's statistics are those of the dots
        a_i'x_k + offsets[k] (one float64 addition: a fitted intercept); None adds nothing.  check_rows: as Context.gram(rows=); with
        False an entry outside [0, N) is skipped (its sample is not counted).  With rows and offsets both None the call, and its bits,
        are the ones above.  Where the one-pass kernel does not take the problem (d in 1025..4096, or an iterate that is not 16-byte
        aligned) every model is scored on its own: list_dots, the offset added in float64, scoring.margin_stats_torch -- with
        check_rows=False over the entries that name a row, so that both routes skip the others."""
        if isinstance(F, PackedSepQuad):
            raise L.CiaoError(L.ERR_ARG, "margin statistics exist for LeastSquares / logistic rows, not for the sharing problem")
        xs = list(xs)
        K = len(xs)
        if s is None:
            sv = None
        else:
            vals = [float(s)] * K if isinstance(s, (int, float)) else [float(v) for v in s]
            if len(vals) != K:
                raise L.CiaoError(L.ERR_ARG, f"margin_stats_multi: {len(vals)} scalings for {K} iterates")
            sv = (C.c_double * max(K, 1))(*vals)
        out = (C.c_double * (4 * max(K, 1)))()
        kind = LogisticStats if F.loss == L.LOSS_LOGISTIC else LeastSquaresStats
        if rows is None and offsets is None:
            L.check(self.lib.ciao_margin_stats_multi(self._h, F.ref, K, self._ptr_table(xs, F, "x"), sv, out))
            return [kind(*out[4 * k:4 * k + 4]) for k in range(K)]
        rows, M = self._row_list(F, rows, check_rows, "margin_stats_multi")
        if M < 1:
            raise L.CiaoError(L.ERR_ARG, "margin_stats_multi: rows must name at least one row")
        ov = None
        if offsets is not None:
            ov = [float(v) for v in offsets]
            if len(ov) != K:
                raise L.CiaoError(L.ERR_ARG, f"margin_stats_multi: {len(ov)} offsets for {K} iterates")
            if any(v - v != 0.0 for v in ov):
                raise L.CiaoError(L.ERR_ARG, "margin_stats_multi: every offset must be finite")
        table = self._ptr_table(xs, F, "x")
        if F.d > 1024 or any(x.data_ptr() % 16 for x in xs):
            from .scoring import margin_stats_torch
            from .stepsize import _on_stream
            if not 1 <= K <= 256:
                raise L.CiaoError(L.ERR_ARG, f"margin_stats_multi: K must be in 1..256 (got {K})")
            name, res = ("logistic" if F.loss == L.LOSS_LOGISTIC else "ls"), []
            with _on_stream(self):
                if rows is not None and not check_rows:   # the kernel skips an entry that names no row: so does this route
                    rows = rows[(rows >= 0) & (rows < F.N)].contiguous()
                    if rows.numel() == 0:                  # the statistics of no sample, as the kernel leaves them
                        return [kind(0.0, 0.0, 0.0, float("inf") if F.loss == L.LOSS_LOGISTIC else 0.0) for _ in xs]
                b = F.b if rows is None else F.b[rows]
                for k, x in enumerate(xs):
                    dots = self.list_dots(F, x, rows=rows, check_rows=False)
                    if ov is not None and ov[k] != 0.0:   # (as scoring.score: a zero intercept adds nothing, not even +0.0)
                        dots = dots + ov[k]
                    res.append(kind(*margin_stats_torch(name, dots, b, 1.0 if sv is None else sv[k])))
            return res
        op = None if ov is None else (C.c_double * max(K, 1))(*ov)
        L.check(self.lib.ciao_margin_stats_multi_rows(self._h, F.ref, None if rows is None else _ptr(rows), M, K, table, op, sv, out))
        return [kind(*out[4 * k:4 * k + 4]) for k in range(K)]

    # -- gap-safe screening (screening.py) ----------------------------------------------------------
    def col_sqnorms(self, F, out=None):
        """out[j] = sum_i A[i,j]^2 over the N local rows of F (include/ciao_hip.h: ciao_col_sqnorms) -> a device float64 d-vector
        whatever F's dtype is.  One pass over A, paid once per dataset; bitwise reproducible.  Does not synchronise, except where the
        workspace of partial sums has to grow (the first call at a larger N x d)."""
        if isinstance(F, PackedSepQuad):
            raise L.CiaoError(L.ERR_ARG, "column norms exist for LeastSquares / logistic rows, not for the sharing problem")
        if out is None:
            out = torch.empty(F.d, dtype=torch.float64, device=f"cuda:{self.device}")
            if self.stream is not None:
                out.record_stream(self.stream)
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == F.d):
            raise ValueError(f"out: need a contiguous float64 device vector of length {F.d}")
        L.check(self.lib.ciao_col_sqnorms(self._h, F.ref, _ptr(out)))
        return out

    def screen(self, grad, colsq, s: float, kappa: float, mu: float):
        """The screening rule keep[j] = !(s |grad_j| + kappa sqrt(colsq_j) < mu) on the device (include/ciao_hip.h: ciao_screen) ->
        (keep, n_kept): keep a uint8 device d-vector, n_kept the number of ones.  grad: a float32 / float64 device d-vector;
        colsq: col_sqnorms' float64 d-vector.  Synchronises."""
        if not (isinstance(grad, torch.Tensor) and grad.is_cuda and grad.dtype in _DT and grad.is_contiguous() and grad.dim() == 1):
            raise ValueError("grad: need a contiguous float32 / float64 device vector")
        d = grad.numel()
        if not (isinstance(colsq, torch.Tensor) and colsq.is_cuda and colsq.dtype == torch.float64 and colsq.is_contiguous() and colsq.numel() == d):
            raise ValueError(f"colsq: need a contiguous float64 device vector of length {d} (Context.col_sqnorms)")
        keep = torch.empty(d, dtype=torch.uint8, device=grad.device)
        if self.stream is not None:
            keep.record_stream(self.stream)
        n = C.c_int64(-1)
        L.check(self.lib.ciao_screen(self._h, _DT[grad.dtype], d, _ptr(grad) if d else None, _ptr(colsq) if d else None, float(s), float(kappa),
                                     float(mu), _ptr(keep) if d else None, C.byref(n)))
        return keep, n.value

    # -- step sizes from the data (stepsize.py) ---------------------------------------------------------
    def _row_sqnorms(self, F, out, stats):
        if isinstance(F, PackedSepQuad):
            raise L.CiaoError(L.ERR_ARG, "row norms exist for LeastSquares / logistic rows, not for the sharing problem")
        L.check(self.lib.ciao_row_sqnorms(self._h, F.ref, _ptr(out), stats))

    def row_sqnorms(self, F, out=None):
        """out[i] = sum_j A[i,j]^2 = ||a_i||^2 for the N local rows of F (include/ciao_hip.h: ciao_row_sqnorms) -> a device float64
        N-vector whatever F's dtype is (a complex row: the sum over its 2n reals).  One pass over A; bitwise reproducible.  Does not
        synchronise."""
        if out is None and not isinstance(F, PackedSepQuad):
            out = torch.empty(F.N, dtype=torch.float64, device=f"cuda:{self.device}")
            if self.stream is not None:
                out.record_stream(self.stream)
        if not isinstance(F, PackedSepQuad) and not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64
                                                     and out.is_contiguous() and out.numel() == F.N):
            raise ValueError(f"out: need a contiguous float64 device vector of length {F.N}")
        self._row_sqnorms(F, out, None)
        return out

    def row_sqnorm_stats(self, F) -> RowNormStats:
        """The summary of row_sqnorms(F) without its N-vector: RowNormStats(max, argmax, min, sum) from the same pass over A (no
        N-vector is allocated or written).  Bitwise the numbers row_sqnorms' vector has; synchronises."""
        stats = (C.c_double * 4)()
        self._row_sqnorms(F, None, stats)
        return RowNormStats(stats[0], int(stats[1]), stats[2], stats[3])

    # -- column standardisation (standardize.py) -------------------------------------------------------
    def _dvec(self, t, name, d):
        """a float64 device d-vector, or None -> its pointer (None: NULL)"""
        if t is None:
            return None
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == d):
            raise ValueError(f"{name}: need a contiguous float64 device vector of length {d}")
        return _ptr(t)

    def col_moments(self, F, shift=None, s1=None, s2=None):
        """(s1, s2) with s1[j] = sum_i (A[i,j] - c_j) and s2[j] = sum_i (A[i,j] - c_j)^2 over the N local rows of F (include/ciao_hip.h:
        ciao_col_moments) -> two device float64 d-vectors whatever F's dtype is.  c = shift, a float64 device d-vector, or (None) the
        first local row.  One pass over A; bitwise reproducible.  Does not synchronise, except where the workspace of partial sums has
        to grow."""
        if isinstance(F, PackedSepQuad):
            raise L.CiaoError(L.ERR_ARG, "column moments exist for LeastSquares / logistic rows, not for the sharing problem")
        for v in (s1, s2):
            if v is None:
                continue
            self._dvec(v, "s1 / s2", F.d)
        if s1 is None or s2 is None:
            both = torch.empty((2, F.d), dtype=torch.float64, device=f"cuda:{self.device}")
            if self.stream is not None:
                both.record_stream(self.stream)
            s1 = both[0] if s1 is None else s1
            s2 = both[1] if s2 is None else s2
        L.check(self.lib.ciao_col_moments(self._h, F.ref, self._dvec(shift, "shift", F.d), _ptr(s1), _ptr(s2)))
        return s1, s2

    def scale_columns(self, F, center=None, scale=None, out=None, inplace=False):
        """out[i,j] = T((float64(A[i,j]) - center_j) * scale_j) for the N local rows of F (include/ciao_hip.h: ciao_scale_columns) -> out.
        center / scale: float64 device d-vectors; None means 0 / 1.  out: a row-major (N, d) device matrix of F's dtype (any row stride; its
        padding columns are not written), a fresh one by default; inplace=True writes over F.A.  One pass: N d read, N d written.  Does not
        synchronise."""
        if isinstance(F, PackedSepQuad):
            raise L.CiaoError(L.ERR_ARG, "columns are scaled for LeastSquares / logistic rows, not for the sharing problem")
        if inplace:
            if out is not None and out is not F.A:
                raise ValueError("inplace=True writes over F.A: out must be None")
            out = F.A
        elif out is None and F.A is not None:
            out = torch.empty((F.N, F.d), dtype=F.dtype, device=f"cuda:{self.device}")
            if self.stream is not None:
                out.record_stream(self.stream)
        if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == F.dtype and out.dim() == 2
                                    and tuple(out.shape) == (F.N, F.d) and (out.stride(1) == 1 or F.d == 1)):
            raise ValueError(f"out: need a row-major device matrix of shape ({F.N}, {F.d}) and dtype {F.dtype}")
        ld_out = F.d if out is None else (int(out.stride(0)) if F.N > 1 else F.d)
        L.check(self.lib.ciao_scale_columns(self._h, F.ref, self._dvec(center, "center", F.d), self._dvec(scale, "scale", F.d),
                                            _ptr(out) if out is not None else None, ld_out))
        return out

    # -- Gram statistics (gram.py) -------------------------------------------------------------------
    def gram(self, F, G=None, u=True, colsum=True, bsum=True, weights=None, rows=None, check_rows=True):
        """(G, u, colsum, bsum) with G = A'A (d x d), u = A'b, colsum = A'1 and bsum = (sum b, sum b^2) over the N local rows of F
        (include/ciao_hip.h: ciao_gram) -> device float64 tensors whatever F's dtype is; fp32 rows give the bits their .double() copy
        gives.  G: a row-major float64 device matrix of d rows (any row stride >= d; columns beyond d are not written), a fresh one by
        default; both triangles are written with the same bits.  u / colsum / bsum: a float64 device vector (d, d, 2 elements) to write
        into, True for a fresh one, or None / False to leave it out (NULL: the others' bits do not change).  One pass over A on the
        matrix cores, paid once per dataset; bitwise reproducible.  d <= 4096.  Does not synchronise, except where the workspace of
        partial tiles has to grow.

        weights: a contiguous float64 device N-vector w, one weight per local row (include/ciao_hip.h: ciao_gram_weighted; DESIGN.md
        section 8.13) -> G = A'diag(w)A, u = A'(w b), colsum = A'w and bsum = (sum w b, sum w b^2, sum w): THREE elements then.  One
        operand of every product is w_n times an element, rounded once, the other the raw element: any finite weight, negative ones
        included; w = 1 gives the unweighted bits; 0/1 weights the statistics of a row subset.  A zero weight does not mask a
        non-finite element (0 inf = NaN).

        rows: a contiguous int64 device vector of M local row numbers, at any 8-byte alignment (a slice of a longer tensor works), in
        any order, repeats allowed (include/ciao_hip.h: ciao_gram_rows) -> the statistics of A[rows], b[rows] at
        the cost of the M rows touched, BIT FOR BIT what gram() gives on that gathered copy.  weights then has M elements, one per list
        position.  check_rows: take min and max of the list on the device and raise ValueError before any launch where an entry lies
        outside [0, N) (one synchronisation); False skips it (the kernel then treats such an entry as a row of zeros)."""
        if isinstance(F, PackedSepQuad):
            raise L.CiaoError(L.ERR_ARG, "the Gram matrix exists for LeastSquares / logistic rows, not for the sharing problem")
        dev = f"cuda:{self.device}"
        d = F.d
        if rows is not None and not (isinstance(rows, torch.Tensor) and rows.is_cuda and rows.device.index == self.device
                                     and rows.dtype == torch.int64 and rows.dim() == 1 and rows.is_contiguous()):
            raise ValueError(f"rows: need a contiguous int64 vector of row numbers on cuda:{self.device}")
        nw = F.N if rows is None else int(rows.shape[0])
        if weights is not None and not (isinstance(weights, torch.Tensor) and weights.is_cuda and weights.device.index == self.device
                                        and weights.dtype == torch.float64 and weights.dim() == 1 and weights.shape[0] == nw
                                        and weights.is_contiguous()):
            raise ValueError(f"weights: need a contiguous float64 vector of {nw} elements on cuda:{self.device}")
        if rows is not None and check_rows and nw > 0:
            lo, hi = (int(v) for v in torch.aminmax(rows))
            if lo < 0 or hi >= F.N:
                raise ValueError(f"rows: entries must lie in [0, {F.N}) (got min {lo}, max {hi})")
        nb = 2 if weights is None else 3

        def fresh(*shape):
            t = torch.empty(shape, dtype=torch.float64, device=dev)
            if self.stream is not None:
                t.record_stream(self.stream)
            return t

        if G is None:
            G = fresh(d, d)
        if not (isinstance(G, torch.Tensor) and G.is_cuda and G.dtype == torch.float64 and G.dim() == 2 and tuple(G.shape) == (d, d)
                and (G.stride(1) == 1 or d == 1)):
            raise ValueError(f"G: need a row-major float64 device matrix of shape ({d}, {d})")
        ldg = int(G.stride(0)) if d > 1 else d
        outs = []
        for v, name, n in ((u, "u", d), (colsum, "colsum", d), (bsum, "bsum", nb)):
            if v is None or v is False:
                outs.append(None)
            elif v is True:
                outs.append(fresh(n))
            else:
                self._dvec(v, name, n)
                outs.append(v)
        outp = [None if v is None else _ptr(v) for v in outs]
        if rows is not None:
            # (an empty weight vector has no address: any aligned non-NULL one says "weighted", three sums; with M = 0 nothing is read)
            wp = None if weights is None else (_ptr(weights) if nw > 0 else _ptr(G))
            L.check(self.lib.ciao_gram_rows(self._h, F.ref, _ptr(rows), nw, wp, _ptr(G), ldg, *outp))
        elif weights is None:
            L.check(self.lib.ciao_gram(self._h, F.ref, _ptr(G), ldg, *outp))
        else:
            L.check(self.lib.ciao_gram_weighted(self._h, F.ref, _ptr(weights), _ptr(G), ldg, *outp))
        return (G, *outs)

    # -- first-order passes over a list of rows (newton.DeviceRows(rows=), scoring.score(rows=), cv.logistic_cv) --
    def _row_list(self, F, rows, check_rows, what):
        """Context.gram's checks of a row list -> (its pointer or None, M)"""
        if isinstance(F, PackedSepQuad):
            raise L.CiaoError(L.ERR_ARG, f"{what} exists for LeastSquares / logistic rows, not for the sharing problem")
        if rows is not None and not (isinstance(rows, torch.Tensor) and rows.is_cuda and rows.device.index == self.device
                                     and rows.dtype == torch.int64 and rows.dim() == 1 and rows.is_contiguous()):
            raise ValueError(f"rows: need a contiguous int64 vector of row numbers on cuda:{self.device}")
        M = F.N if rows is None else int(rows.shape[0])
        if rows is not None and check_rows and M > 0:
            lo, hi = (int(v) for v in torch.aminmax(rows))
            if lo < 0 or hi >= F.N:
                raise ValueError(f"rows: entries must lie in [0, {F.N}) (got min {lo}, max {hi})")
        return rows, M

    def _list_out(self, out, n):
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=f"cuda:{self.device}")
            if self.stream is not None:
                out.record_stream(self.stream)
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device.index == self.device and out.dtype == torch.float64
                and out.dim() == 1 and out.is_contiguous() and out.numel() == n):
            raise ValueError(f"out: need a contiguous float64 vector of {n} elements on cuda:{self.device}")
        return out

    def list_dots(self, F, x, rows=None, out=None, check_rows=True):
        """out[m] = a_{rows[m]}'x for the M list positions (include/ciao_hip.h: ciao_list_dots) -> a device
        float64 M-vector whatever F's dtype is: A[rows] @ x at the cost of the rows touched, BIT FOR BIT what list_dots gives without a
        list on the gathered copy A[rows]; one row has one bit pattern at every position of every list.  x: a device d-vector of F's
        dtype.  rows: a contiguous int64 device vector of M local row numbers at any 8-byte alignment, any order, repeats allowed;
        None: every row in order (M = N).  check_rows: as Context.gram(rows=) -- min and max of the list are taken on the device and
        an entry outside [0, N) raises ValueError before any launch (one synchronisation); False skips it (the kernel then writes 0 at
        such a position).  d <= 4096.  Does not synchronise otherwise."""
        rows, M = self._row_list(F, rows, check_rows, "list_dots")
        out = self._list_out(out, M)
        xp = self._vec(x, F, "x")
        if M == 0:
            # (an empty list and an empty output have no address: any aligned non-NULL one says "a list"; with M = 0 nothing is read or written)
            pad = torch.empty(1, dtype=torch.int64, device=f"cuda:{self.device}")
            L.check(self.lib.ciao_list_dots(self._h, F.ref, None if rows is None else _ptr(pad), 0, xp, _ptr(pad)))
            return out
        L.check(self.lib.ciao_list_dots(self._h, F.ref, _ptr(rows), M, xp, _ptr(out)))
        return out

    def list_combine(self, F, c, rows=None, out=None, check_rows=True):
        """out[j] = sum_m c[m] A[rows[m], j] (include/ciao_hip.h: ciao_list_combine) -> a device float64
        d-vector whatever F's dtype is: A[rows]' c at the cost of the rows touched, BIT FOR BIT what list_combine gives without a list
        on the gathered copy A[rows].  c: a contiguous float64 device M-vector, one coefficient per list position.  rows, check_rows:
        as list_dots (an entry outside [0, N) contributes no term where the check is skipped).  d <= 4096.  Does not synchronise,
        except for that check and where the workspace of partial sums has to grow."""
        rows, M = self._row_list(F, rows, check_rows, "list_combine")
        if not (isinstance(c, torch.Tensor) and c.is_cuda and c.device.index == self.device and c.dtype == torch.float64 and c.dim() == 1
                and c.shape[0] == M and c.is_contiguous()):
            raise ValueError(f"c: need a contiguous float64 vector of {M} elements on cuda:{self.device}")
        out = self._list_out(out, F.d)
        # (an empty list / coefficient vector has no address: any aligned non-NULL one will do, with M = 0 nothing is read)
        L.check(self.lib.ciao_list_combine(self._h, F.ref, _ptr(rows) if (rows is None or M > 0) else _ptr(out), M,
                                           _ptr(c) if M > 0 else _ptr(out), _ptr(out)))
        return out

    def gram_cd(self, G, u, inv, tau, X, tol, max_sweeps, R=True, stat=None):
        """(X, R, stat): cyclic coordinate descent with covariance updates on a Gram matrix, K models in one launch (include/ciao_hip.h:
        ciao_gram_cd; DESIGN.md section 8.14, with the method to the bit and its numpy mirror).  All float64 device tensors: G (d, d)
        row-major with any row stride >= d; u, inv d-vectors (inv_j = 1 / G_jj where G_jj > 0, else 0); tau a K-vector (mu_k N / lam);
        X (K, d) with any row stride >= d: the warm starts, OVERWRITTEN with the results.  R: a (K, d) matrix to receive the final
        r = u - G x, True for a fresh one, None / False to leave it out; stat: a contiguous (K, 4) matrix, fresh by default: sweeps,
        non-zero updates, largest change of the last full sweep, state (1 converged, 0 sweep budget spent, 2 not finite).
        0 <= tol; 1 <= max_sweeps <= 1024; d, K <= 4096.  Does not synchronise."""
        dev = f"cuda:{self.device}"

        def fresh(*shape):
            t = torch.empty(shape, dtype=torch.float64, device=dev)
            if self.stream is not None:
                t.record_stream(self.stream)
            return t

        def mat(t, name, rows, cols):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.device and t.dtype == torch.float64 and t.dim() == 2
                    and tuple(t.shape) == (rows, cols) and (t.stride(1) == 1 or cols == 1) and (rows == 1 or t.stride(0) >= cols)):
                raise ValueError(f"{name}: need a row-major float64 matrix of shape ({rows}, {cols}) on {dev}")
            return int(t.stride(0)) if rows > 1 else cols

        if not (isinstance(X, torch.Tensor) and X.dim() == 2):
            raise ValueError("X: need a (K, d) float64 device matrix")
        K, d = int(X.shape[0]), int(X.shape[1])
        ldx = mat(X, "X", K, d)
        ldg = mat(G, "G", d, d)
        self._dvec(u, "u", d)
        self._dvec(inv, "inv", d)
        self._dvec(tau, "tau", K)
        if R is True:
            R = fresh(K, d)
        elif R is None or R is False:
            R = None
        ldr = mat(R, "R", K, d) if R is not None else 0
        if stat is None:
            stat = fresh(K, 4)
        elif not (isinstance(stat, torch.Tensor) and stat.is_cuda and stat.dtype == torch.float64 and tuple(stat.shape) == (K, 4) and stat.is_contiguous()):
            raise ValueError(f"stat: need a contiguous float64 device matrix of shape ({K}, 4)")
        L.check(self.lib.ciao_gram_cd(self._h, d, K, _ptr(G), ldg, _ptr(u), _ptr(inv), _ptr(tau), _ptr(X), ldx, float(tol), int(max_sweeps),
                                      _ptr(R), ldr, _ptr(stat)))
        return X, R, stat

    def gram_cd_general(self, G, u, inv, tau, X, tol, max_sweeps, gsel=None, pf=None, lo=None, hi=None, R=True, stat=None):
        """(X, R, stat): gram_cd with bounds lo <= x <= hi, a penalty factor per coordinate, a ridge term and a Gram matrix, u and tol
        per model, K models in one launch (include/ciao_hip.h: ciao_gram_cd_general; DESIGN.md section 8.17, with the method to the bit
        and its numpy mirror).  All float64 device tensors.  G: (d, d) or (S, d, d), row-major with any
        row stride >= d and any set stride that keeps the sets apart; gsel: an int32 K-vector of set numbers, None: set 0; u, inv, pf,
        lo, hi: (d,) shared by all models or (K, d) with any row stride >= d; inv_kj = 1 / (G_jj + ridge_k) where that is > 0, else 0;
        pf, lo, hi None: 1, -inf, +inf; tau: a K-vector; tol: a number (broadcast to a device K-vector) or a device K-vector; X, R,
        stat, max_sweeps: as gram_cd.  stat's state 3: the model could not run (a gsel outside [0, S), a negative or NaN tol or pf,
        lo > 0, hi < 0, a NaN bound or tau pf) and its rows of X and R are untouched.  Does not synchronise."""
        dev = f"cuda:{self.device}"

        def fresh(*shape):
            t = torch.empty(shape, dtype=torch.float64, device=dev)
            if self.stream is not None:
                t.record_stream(self.stream)
            return t

        def f64(t, name, dim):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.device and t.dtype == torch.float64 and t.dim() in dim):
                raise ValueError(f"{name}: need a float64 tensor on {dev} with {' or '.join(str(n) for n in dim)} dimensions")

        def mat(t, name, rows, cols):
            f64(t, name, (2,))
            if not (tuple(t.shape) == (rows, cols) and (t.stride(1) == 1 or cols == 1) and (rows == 1 or t.stride(0) >= cols)):
                raise ValueError(f"{name}: need a row-major float64 matrix of shape ({rows}, {cols}) on {dev}")
            return int(t.stride(0)) if rows > 1 else cols

        def per_model(t, name):
            """a (d,) vector shared by all models -> stride 0; a (K, d) matrix -> its row stride"""
            if t is None:
                return 0
            f64(t, name, (1, 2))
            if t.dim() == 1:
                if not (t.shape[0] == d and (t.stride(0) == 1 or d == 1)):
                    raise ValueError(f"{name}: need a contiguous vector of {d} elements, or a ({K}, {d}) matrix")
                return 0
            return mat(t, name, K, d)

        if not (isinstance(X, torch.Tensor) and X.dim() == 2):
            raise ValueError("X: need a (K, d) float64 device matrix")
        K, d = int(X.shape[0]), int(X.shape[1])
        ldx = mat(X, "X", K, d)
        f64(G, "G", (2, 3))
        if G.dim() == 2:
            S, sg, ldg = 1, 0, mat(G, "G", d, d)
        else:
            S = int(G.shape[0])
            if S < 1:
                raise ValueError("G: need at least one Gram matrix")
            ldg = mat(G[0], "G[s]", d, d)
            sg = int(G.stride(0)) if S > 1 else 0
            if S > 1 and sg < (d - 1) * ldg + d:
                raise ValueError("G: the Gram matrices overlap (the set stride is below (d - 1) ldg + d)")
        if u is None or inv is None:
            raise ValueError("u and inv are needed")
        ldu, ldinv, ldpf, ldlo, ldhi = (per_model(t, n) for t, n in ((u, "u"), (inv, "inv"), (pf, "pf"), (lo, "lo"), (hi, "hi")))
        self._dvec(tau, "tau", K)
        if isinstance(tol, torch.Tensor):
            self._dvec(tol, "tol", K)
        else:
            tol = torch.full((K,), float(tol), dtype=torch.float64, device=dev)
            if self.stream is not None:
                tol.record_stream(self.stream)
        if gsel is not None and not (isinstance(gsel, torch.Tensor) and gsel.is_cuda and gsel.device.index == self.device and gsel.dtype == torch.int32
                                     and gsel.dim() == 1 and gsel.shape[0] == K and gsel.is_contiguous()):
            raise ValueError(f"gsel: need a contiguous int32 vector of {K} elements on {dev}")
        if R is True:
            R = fresh(K, d)
        elif R is None or R is False:
            R = None
        ldr = mat(R, "R", K, d) if R is not None else 0
        if stat is None:
            stat = fresh(K, 4)
        elif not (isinstance(stat, torch.Tensor) and stat.is_cuda and stat.dtype == torch.float64 and tuple(stat.shape) == (K, 4) and stat.is_contiguous()):
            raise ValueError(f"stat: need a contiguous float64 device matrix of shape ({K}, 4)")
        L.check(self.lib.ciao_gram_cd_general(self._h, d, K, _ptr(G), ldg, sg, S, _ptr(gsel), _ptr(u), ldu, _ptr(inv), ldinv, _ptr(tau),
                                              _ptr(pf), ldpf, _ptr(lo), ldlo, _ptr(hi), ldhi, _ptr(X), ldx, _ptr(tol), int(max_sweeps),
                                              _ptr(R), ldr, _ptr(stat)))
        return X, R, stat

    # -- SVRG ------------------------------------------------------------------------------------------------------------
    def svrg_init(self, p, x0, av, z, z_full, w):
        L.check(self.lib.ciao_svrg_init(self._h, p.ref, self._vec(x0, p, "x0"), self._vec(av, p, "av"), self._vec(z, p, "z"),
                                        self._vec(z_full, p, "z_full"), self._vec(w, p, "w")))

    def chain_batch(self):
        """`with ctx.chain_batch(): ...` -- the svrg_inner / saga_steps / small-batch finito_steps calls inside are recorded and launched TOGETHER on leaving
        the block, one workgroup per chain (include/ciao_hip.h: ciao_ctx_chain_batch_begin / _end): several independent solves
        over the same rows (a regularisation path, folds, restarts) on as many compute units.  The chains must own their state
        vectors / tables; each one's results are bitwise those of the same call made alone.  An exception inside the block
        drops the records."""
        return _ChainBatch(self)

    def svrg_inner(self, p, g, gamma, idx, av, z, z_full, w):
        idx = self._idx(idx)
        if self._batch_keep is not None:
            self._batch_keep.append(idx)
        L.check(self.lib.ciao_svrg_inner(self._h, p.ref, g.ref, float(gamma), idx.numel(), _ptr(idx), self._vec(av, p, "av"),
                                         self._vec(z, p, "z"), self._vec(z_full, p, "z_full"), self._vec(w, p, "w")))
        return idx

    def svrg_iterate(self, p, g, gamma, idx, plus, av, z, z_full, w, reuse_rowdots: bool = False):
        """reuse_rowdots=True: the caller vouches that A, b and z_full are exactly what the previous svrg_init /
        svrg_iterate on this context left (include/ciao_hip.h: ciao_svrg_iterate); the inner cycle then reuses the
        a_i'z_full of that full pass.  The default never reads anything cached."""
        idx = self._idx(idx)
        L.check(self.lib.ciao_svrg_iterate(self._h, p.ref, g.ref, float(gamma), idx.numel(), _ptr(idx), 1 if plus else 0,
                                           1 if reuse_rowdots else 0, self._vec(av, p, "av"), self._vec(z, p, "z"),
                                           self._vec(z_full, p, "z_full"), self._vec(w, p, "w")))
        return idx

    def svrg_epoch_tail(self, p, m, plus, av, z, z_full, w):
        """SVRG_basic.jl:84-92 on their own: z_full = z / m; w = z_full unless plus; z = 0; av = full gradient at z_full."""
        L.check(self.lib.ciao_svrg_epoch_tail(self._h, p.ref, int(m), 1 if plus else 0, self._vec(av, p, "av"), self._vec(z, p, "z"),
                                              self._vec(z_full, p, "z_full"), self._vec(w, p, "w")))

    def _ptr_table(self, vecs, p, name):
        arr = (C.c_void_p * len(vecs))(*[self._vec(v, p, f"{name}[{k}]") for k, v in enumerate(vecs)])
        return arr

    def full_gradient_multi(self, p, xs, avs):
        """av_k = (1/N) sum_i grad f_i(x_k) for K iterates in ONE pass over A (ciao_full_gradient_multi: matrix cores where the shape
        allows, K single sweeps otherwise).  xs, avs: lists of K device d-vectors."""
        assert len(xs) == len(avs) and len(xs) >= 1
        L.check(self.lib.ciao_full_gradient_multi(self._h, p.ref, len(xs), self._ptr_table(xs, p, "x"), self._ptr_table(avs, p, "av")))

    def svrg_epoch_tail_multi(self, p, m, plus, avs, zs, z_fulls, ws):
        """SVRG_basic.jl:84-92 for K solves over the same rows: every solve's tail, then the K full passes as one pass over A."""
        K = len(avs)
        assert K >= 1 and len(zs) == K and len(z_fulls) == K and len(ws) == K
        L.check(self.lib.ciao_svrg_epoch_tail_multi(self._h, p.ref, K, int(m), 1 if plus else 0, self._ptr_table(avs, p, "av"),
                                                    self._ptr_table(zs, p, "z"), self._ptr_table(z_fulls, p, "z_full"),
                                                    self._ptr_table(ws, p, "w")))

    # -- SAGA / SAG ----------------------------------------------------------------------------------------------------
    def saga_init(self, p, g, gamma, x0, table, av, z):
        L.check(self.lib.ciao_saga_init(self._h, p.ref, g.ref, float(gamma), self._vec(x0, p, "x0"),
                                        self._vec(table, p, "table", p.N * p.d), self._vec(av, p, "av"), self._vec(z, p, "z")))

    def saga_steps(self, p, g, gamma, sag, idx, table, av, z):
        idx = self._idx(idx)
        if self._batch_keep is not None:
            self._batch_keep.append(idx)
        L.check(self.lib.ciao_saga_steps(self._h, p.ref, g.ref, float(gamma), 1 if sag else 0, idx.numel(), _ptr(idx),
                                         self._vec(table, p, "table", p.N * p.d), self._vec(av, p, "av"), self._vec(z, p, "z")))
        return idx

    # -- Finito / LFinito -------------------------------------------------------------------------------------------
    def hat_gamma(self, gam: torch.Tensor) -> float:
        out = C.c_double(0.0)
        L.check(self.lib.ciao_hat_gamma(self._h, _DT[gam.dtype], gam.numel(), _ptr(gam), C.byref(out)))
        return out.value

    def finito_init(self, p, g, gam, hat_gamma, x0, table, av, z):
        L.check(self.lib.ciao_finito_init(self._h, p.ref, g.ref, self._vec(gam, p, "gam", p.N), float(hat_gamma),
                                          self._vec(x0, p, "x0"), self._vec(table, p, "table", p.N * p.d),
                                          self._vec(av, p, "av"), self._vec(z, p, "z")))

    def finito_steps(self, p, g, gam, hat_gamma, bptr: np.ndarray, bidx, table, av, z):
        bptr = np.ascontiguousarray(bptr, dtype=np.int64)
        bidx = self._idx(bidx)
        if self._batch_keep is not None:
            self._batch_keep.append(bidx)
        assert bptr[0] == 0 and bptr[-1] == bidx.numel()
        L.check(self.lib.ciao_finito_steps(self._h, p.ref, g.ref, self._vec(gam, p, "gam", p.N), float(hat_gamma),
                                           len(bptr) - 1, C.c_void_p(bptr.ctypes.data), _ptr(bidx),
                                           self._vec(table, p, "table", p.N * p.d), self._vec(av, p, "av"),
                                           self._vec(z, p, "z")))
        return bidx

    @staticmethod
    def _blocks(first, length):
        first = np.ascontiguousarray(first, dtype=np.int64)
        length = np.ascontiguousarray(length, dtype=np.int64)
        assert first.shape == length.shape and first.ndim == 1
        return first, length

    def finito_steps_blocks(self, p, g, gam, hat_gamma, first, length, table, av, z):
        """Batches given as contiguous local row blocks [first[t], first[t] + length[t]) -- no index array (ciao_finito_steps_blocks)."""
        first, length = self._blocks(first, length)
        L.check(self.lib.ciao_finito_steps_blocks(self._h, p.ref, g.ref, self._vec(gam, p, "gam", p.N), float(hat_gamma), first.size,
                                                  C.c_void_p(first.ctypes.data), C.c_void_p(length.ctypes.data),
                                                  self._vec(table, p, "table", p.N * p.d), self._vec(av, p, "av"), self._vec(z, p, "z")))

    def lfinito_iterate_blocks(self, p, g, gam, hat_gamma, first, length, av, z, z_full):
        first, length = self._blocks(first, length)
        L.check(self.lib.ciao_lfinito_iterate_blocks(self._h, p.ref, g.ref, self._vec(gam, p, "gam", p.N), float(hat_gamma), first.size,
                                                     C.c_void_p(first.ctypes.data), C.c_void_p(length.ctypes.data),
                                                     self._vec(av, p, "av"), self._vec(z, p, "z"), self._vec(z_full, p, "z_full")))

    def proshi_steps_blocks(self, f, g, gam, hat_gamma, first, length, table, av, z):
        first, length = self._blocks(first, length)
        L.check(self.lib.ciao_proshi_steps_blocks(self._h, f.ref, g.ref, self._vec(gam, f, "gam", f.N), float(hat_gamma), first.size,
                                                  C.c_void_p(first.ctypes.data), C.c_void_p(length.ctypes.data),
                                                  self._vec(table, f, "table", f.N * f.d), self._vec(av, f, "av"), self._vec(z, f, "z")))

    def lfinito_init(self, p, hat_gamma, x0, av, z, z_full):
        L.check(self.lib.ciao_lfinito_init(self._h, p.ref, float(hat_gamma), self._vec(x0, p, "x0"), self._vec(av, p, "av"),
                                           self._vec(z, p, "z"), self._vec(z_full, p, "z_full")))

    def lfinito_iterate(self, p, g, gam, hat_gamma, bptr: np.ndarray, bidx, av, z, z_full):
        bptr = np.ascontiguousarray(bptr, dtype=np.int64)
        bidx = self._idx(bidx)
        assert bptr[0] == 0 and bptr[-1] == bidx.numel()
        L.check(self.lib.ciao_lfinito_iterate(self._h, p.ref, g.ref, self._vec(gam, p, "gam", p.N), float(hat_gamma),
                                              len(bptr) - 1, C.c_void_p(bptr.ctypes.data), _ptr(bidx), self._vec(av, p, "av"),
                                              self._vec(z, p, "z"), self._vec(z_full, p, "z_full")))
        return bidx

    # -- adaptive Finito -------------------------------------------------------------------------------------------------
    def afinito_init(self, p, g, alpha, x0, table, meta, av, z, hat_gamma_dev, gam_override=None):
        L.check(self.lib.ciao_afinito_init(self._h, p.ref, g.ref, float(alpha), self._vec(x0, p, "x0"),
                                           self._vec(table, p, "table", p.N * p.d), self._vec(meta, p, "meta", p.N * 16),
                                           self._vec(av, p, "av"), self._vec(z, p, "z"), self._vec(hat_gamma_dev, p, "hat_gamma", 1),
                                           None if gam_override is None else self._vec(gam_override, p, "gam_override", p.N)))

    def afinito_probe(self, p, i: int, x0, signs, t: float) -> float:
        """One retry of the Lipschitz probe for sample i at x0 + t*signs (Finito_adaptive.jl:80-82); synchronises."""
        out = C.c_double(0.0)
        n_signs = p.d // 2 if getattr(p, "complex", False) else p.d     # complex T: one real draw per complex entry
        L.check(self.lib.ciao_afinito_probe(self._h, p.ref, int(i), self._vec(x0, p, "x0"), self._vec(signs, p, "signs", n_signs),
                                            float(t), C.byref(out)))
        return out.value

    def afinito_steps(self, p, g, alpha, tol_b, idx, table, meta, av, z, hat_gamma_dev) -> tuple[int, int]:
        """-> (steps completed, backtracking trials); synchronises."""
        idx = self._idx(idx)
        done, trials = C.c_int64(0), C.c_int64(0)
        L.check(self.lib.ciao_afinito_steps(self._h, p.ref, g.ref, float(alpha), float(tol_b), idx.numel(), _ptr(idx),
                                            self._vec(table, p, "table", p.N * p.d), self._vec(meta, p, "meta", p.N * 16),
                                            self._vec(av, p, "av"), self._vec(z, p, "z"), self._vec(hat_gamma_dev, p, "hat_gamma", 1),
                                            C.byref(done), C.byref(trials)))
        return done.value, trials.value

    # -- ProShI ------------------------------------------------------------------------------------------------------------
    def proshi_init(self, f, g, gam, x0, table, av, z, hat_gamma_dev):
        L.check(self.lib.ciao_proshi_init(self._h, f.ref, g.ref, self._vec(gam, f, "gam", f.N), self._vec(x0, f, "x0"),
                                          self._vec(table, f, "table", f.N * f.d), self._vec(av, f, "av"), self._vec(z, f, "z"),
                                          self._vec(hat_gamma_dev, f, "hat_gamma", 1)))

    def proshi_steps(self, f, g, gam, hat_gamma, bptr: np.ndarray, bidx, table, av, z):
        bptr = np.ascontiguousarray(bptr, dtype=np.int64)
        bidx = self._idx(bidx)
        assert bptr[0] == 0 and bptr[-1] == bidx.numel()
        L.check(self.lib.ciao_proshi_steps(self._h, f.ref, g.ref, self._vec(gam, f, "gam", f.N), float(hat_gamma), len(bptr) - 1,
                                           C.c_void_p(bptr.ctypes.data), _ptr(bidx), self._vec(table, f, "table", f.N * f.d),
                                           self._vec(av, f, "av"), self._vec(z, f, "z")))

    def proshi_solution(self, f, gam, z, table):
        L.check(self.lib.ciao_proshi_solution(self._h, f.ref, self._vec(gam, f, "gam", f.N), self._vec(z, f, "z"),
                                              self._vec(table, f, "table", f.N * f.d)))

    # -- synthetic data -------------------------------------------------------------------------------------------------
    def synth_normal(self, out: torch.Tensor, row0: int, seed: int, scale: float):
        assert out.is_cuda and out.dim() == 2 and out.stride(1) == 1
        L.check(self.lib.ciao_synth_normal(self._h, _DT[out.dtype], _ptr(out), out.shape[0], out.shape[1],
                                           out.stride(0) if out.shape[0] > 1 else out.shape[1], int(row0), int(seed), float(scale)))

    def synth_targets(self, p: PackedF, x_true, noise: float, labels: bool, seed: int, b_out):
        L.check(self.lib.ciao_synth_targets(self._h, p.ref, self._vec(x_true, p, "x_true"), float(noise), 1 if labels else 0,
                                            int(p.row0), int(seed), self._vec(b_out, p, "b_out", p.N)))


_default_ctx: dict[int, Context] = {}


def _close_default_contexts():
    # destroy the library workspaces while the HIP runtime is still alive (not from __del__ during interpreter teardown)
    for c in list(_default_ctx.values()):
        try:
            c.close()
        except Exception:
            pass
    _default_ctx.clear()


import atexit  # noqa: E402

atexit.register(_close_default_contexts)


def default_context() -> Context:
    """A per-device Context bound to torch's current stream at first use."""
    dev = torch.cuda.current_device()
    ctx = _default_ctx.get(dev)
    if ctx is None:
        ctx = Context(dev)
        _default_ctx[dev] = ctx
    return ctx

"""mrhs_kernel (csrc/mrhs_kernels.h) at every tile count, block map and layout its plan can produce; beside
tests/test_gpu_multi_rhs.py, whose eight shapes leave seven of the nine instantiations with one or two tiles per partition.

  0. the plan: tests/test_multi_rhs_host.py restates launch_mrhs (`plan`, `report`, `classes`); the CU count comes from the device.  Every
     kernel call is held to the launch report the plan predicts, and every parametrised case asserts that its (N, K) list reaches the
     classes it is there for ON THIS DEVICE: another CU count fails loudly instead of passing on shallower partitions;
  1. integer rows, exactly: least squares on a in {-1, 0, 1}, x, b in {-2 .. 2}, lam in {1, 1/2}; every partial sum is an integer (or a
     half-integer) below 2^24, so any order of addition gives T(lam S) * (T(1) / T(N)) with S = A'(A X - b) in int64 -- compared in bits,
     for the nine instantiations, over partitions of 1, 2, 3 and 5 whole tiles, short last tiles of 1 and 13 rows alone and behind
     steady steps, empty trailing partitions, N = 1, both block maps with several column blocks, K in {2, 3, 16, 17, 256, 257, 512,
     528}; in five layouts (tight; a padded, poisoned row stride of one and of five 16-byte units; outputs at a poisoned stride between
     guard bands; outputs one element off 16-byte alignment), with the guards, the inputs and a second call checked after every call;
  2. both losses against the oracle and against the library's own single sweeps on the deep partitions (the only cover of the logistic
     link and of the label loads in the steady step), under the scales of test_gpu_multi_rhs.py;
  3. every conjunct of mrhs_supported false in turn: bitwise K single sweeps, no mrhs_kernel in the report;
  4. ciao_svrg_epoch_tail_multi against K calls of ciao_svrg_epoch_tail: both types, both losses, plus and basic, a kernel shape with
     three tiles per partition and a fallback shape, the four state vectors of every solve in guarded buffers; once exactly on integers;
     and solvers.solve_together(one_pass=True) with SVRG++.

The K iterates of a call are the rows of ONE guarded (K, d) buffer and so are the K outputs: two buffers, not 2 K."""
import numpy as np
import pytest

import problems as P
import test_multi_rhs_host as H
from layouts import Guarded, bits, has_poison, poison_bits
from test_gpu_parity import EPS, close, make

pytestmark = pytest.mark.gpu

VARIANT_IDS = [pytest.param(dt, d, id=f"{'f64' if dt == np.float64 else 'f32'}-{d}") for dt, d in H.VARIANTS]
BOTH = [pytest.param(np.float64, id="f64"), pytest.param(np.float32, id="f32")]


def vec(dtype):
    """elements of a 16-byte unit"""
    return 16 // np.dtype(dtype).itemsize


@pytest.fixture(scope="module")
def num_cu(ctx):
    import torch
    return int(torch.cuda.get_device_properties(ctx.device).multi_processor_count)


def rows(g, K=None):
    """the rows of a guarded (K, d) buffer as the list of d-vectors a call takes"""
    return [g.view[k] for k in range(g.shape[0] if K is None else K)]


def repoison(g):
    bits(g.flat).fill_(poison_bits(g.flat.dtype))


def same_bits(a, b):
    import torch
    return torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def worst_solve(got, ref, dtype):
    """(k, ratio): the solve whose error, in close()'s own units eps |ref_k|_inf, is largest -- close() on that solve passes exactly when
    it passes on every solve"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    unit = EPS[dtype] * np.maximum(np.abs(ref).max(axis=1), 1e-30)
    ratio = np.abs(got - ref).max(axis=1) / unit
    k = int(np.argmax(ratio))
    return k, float(ratio[k])


def single_sweeps(ctx, F, xs):
    """K calls of ctx.full_gradient -> (K, d) tensor"""
    import torch
    out = torch.full((len(xs), F.d), float("nan"), dtype=xs[0].dtype, device="cuda")
    for k, x in enumerate(xs):
        ctx.full_gradient(F, x, out[k])
    return out


# ---- 1. integer rows, exactly -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", VARIANT_IDS)
def test_integer_rows_exactly(ctx, num_cu, dtype, d):
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    reached = H.classes(H.CASES, num_cu)
    assert H.REQUIRED <= reached, f"{num_cu} compute units: the (N, K) list does not reach {sorted(H.REQUIRED - reached)}"
    A, X, b = H.int_data(d)
    v = vec(dtype)
    tA, tX, tb = (torch.from_numpy(a.astype(dtype)) for a in (A, X, b[:H.NMAX]))
    want = {c: torch.from_numpy(H.expected(H.int_reference(d, *c)[0], H.lam_of(c), c[0], dtype)).cuda() for c in H.CASES}
    Gb = Guarded(tb, device="cuda", name="b")
    GXs = {ld: Guarded(tX, ld=ld, device="cuda", name=f"iterates (stride {ld})") for ld in (d, d + v)}
    Xrows = {ld: rows(g) for ld, g in GXs.items()}
    ran = []
    # (name, row stride of A, stride of the iterates and of the outputs, outputs' offset from 16-byte alignment)
    for name, lda, ldv, off in (("tight", d, d, 0), ("A at d + 16 bytes", d + v, d + v, 0), ("A at d + 80 bytes", d + 5 * v, d + v, 0),
                                ("outputs at a poisoned stride", d, d + v, 0), ("outputs one element off alignment", d, d + v, 1)):
        GA = Guarded(tA, ld=lda, device="cuda", name=f"A ({name})")
        GX, xall = GXs[ldv], Xrows[ldv]
        for N, K in H.call_order(H.CASES):
            what = f"{name}, N = {N}, K = {K}"
            F = PackedF.least_squares(GA.view[:N], Gb.view[:N], H.lam_of((N, K)))
            out = Guarded(shape=(K, d), dtype=dtype, ld=ldv, off=off, device="cuda", name="outputs")
            xs, avs = xall[:K], rows(out)
            assert all(x.data_ptr() % 16 == 0 for x in xs[:2]) and (avs[0].data_ptr() % 16 != 0) == bool(off) and F.ld == (lda if N > 1 else d)
            for rep in range(2):
                ctx.full_gradient_multi(F, xs, avs)
                assert ctx.last_kernel() == H.report(dtype, d, N, K, num_cu), (what, ctx.last_kernel())
                out.check_outside(what)
                for g in (GA, Gb, GX):
                    g.check_unchanged(what)
                assert not has_poison(out.view), what
                bad = (bits(out.view.contiguous()) != bits(want[(N, K)])).any(dim=1).nonzero().flatten().tolist()
                assert not bad, f"{what}, call {rep}: {len(bad)} solve(s) differ from the exact result, the first solve {bad[0]}"
                repoison(out)                                                  # the second call starts from poison again
            if name == "tight" and N & (N - 1) == 0:                           # 1 / N a power of two: every placement of it is exact
                assert same_bits(single_sweeps(ctx, F, xs), want[(N, K)]), f"{what}: the single sweeps"
            ran.append((N, K))
    assert H.REQUIRED <= H.classes(ran, num_cu) and len(ran) == 5 * len(H.CASES)
    ctx.synchronize()


# ---- 2. both losses against the oracle ------------------------------------------------------------------------------------------------
# 8 x 16 + 1 rows under the plain map with two column blocks; 48 rows a partition: one steady step; 15 x 80 + 77: three steady steps and a
# 13-row tile behind two.  The last one runs on rows at a padded, poisoned stride.
GAUSS_CASES = [(129, 17), (768, 256), (1277, 256)]
GAUSS_NEED = {"3 whole tiles", ">= 5 whole tiles", ">= 3 steady steps", ">= 3 steady steps, xcd map, nkb > 1", "13-15-row tile after steady steps",
              "1-row tile alone", "plain map, nkb > 1"}


def gauss_iterates(d, K, dtype, seed):
    """every solve its own iterate, scales 0.3 .. 2.2 in turn: the range tests/test_gpu_multi_rhs.py's scales were set on (its K <= 48
    reach 5; the logistic link is the same function at every scale)"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((K, d)) * (0.3 + 0.1 * (np.arange(K) % 20))[:, None]).astype(dtype)


@pytest.mark.parametrize("loss", ["ls", "logistic"])
@pytest.mark.parametrize("dtype,d", VARIANT_IDS)
def test_both_losses_against_the_oracle_on_deep_partitions(ctx, num_cu, dtype, d, loss):
    import torch
    from oracle import oracle as O
    assert GAUSS_NEED <= H.classes(GAUSS_CASES, num_cu), f"{num_cu} compute units: {sorted(GAUSS_NEED - H.classes(GAUSS_CASES, num_cu))}"
    for N, K in GAUSS_CASES:
        A, b, _ = P.synthetic(loss, N, d, dtype, seed=d + K)
        op, dp = make(loss, A, b, float(N) if loss == "ls" else 1.0, dtype, pad=vec(dtype) if N == 1277 else 0)
        assert dp.ld == d + (vec(dtype) if N == 1277 else 0)
        xs_h = gauss_iterates(d, K, dtype, seed=K)
        GX = Guarded(xs_h, ld=d + vec(dtype), device="cuda", name="iterates")
        out = Guarded(shape=(K, d), dtype=dtype, ld=d + vec(dtype), device="cuda", name="outputs")
        xs = rows(GX)
        ctx.full_gradient_multi(dp, xs, rows(out))
        assert ctx.last_kernel() == H.report(dtype, d, N, K, num_cu), ctx.last_kernel()
        out.check_outside(ctx.last_kernel())
        GX.check_unchanged(ctx.last_kernel())
        got = out.view.cpu().numpy()
        assert not np.isnan(got).any() and not has_poison(dp.A) and not has_poison(dp.b)
        ref = np.stack([O.full_pass(op, xs_h[k]) for k in range(K)])
        k, r = worst_solve(got, ref, dtype)
        close(got[k], ref[k], dtype, scale={64: 670, 32: 650}, what=f"multi-rhs pass on deep partitions vs the oracle ({loss}, d={d}, N={N}, K={K}, solve {k})")
        solo = single_sweeps(ctx, dp, xs).cpu().numpy()
        k2, r2 = worst_solve(got, solo, dtype)
        close(got[k2], solo[k2], dtype, scale={64: 44, 32: 48}, what=f"multi-rhs pass on deep partitions vs its own single sweeps ({loss}, d={d}, N={N}, K={K}, solve {k2})")
        print(f"{loss} {np.dtype(dtype).name} d={d} N={N} K={K}: worst solve vs the oracle {r:.2f} eps (solve {k}), vs its single sweep {r2:.2f} eps (solve {k2})")
    ctx.synchronize()


# ---- 3. every reason not to take the kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", BOTH)
def test_every_reason_not_to_take_the_kernel(ctx, ciao, num_cu, dtype):
    """One matrix that takes the kernel (d = 256, the integer rows of part 1) and, one at a time, what mrhs_supported refuses beyond
    the five cases of tests/test_gpu_multi_rhs.py: each runs as K single sweeps, bitwise what K calls of ctx.full_gradient give on the
    same problem (made with no monitor set), and the launch report names no mrhs_kernel."""
    import torch
    import ciaoalgorithms_jl_amd._lib as L
    from ciaoalgorithms_jl_amd.device import PackedF, ProxG
    N, K, v = 512, 17, vec(dtype)

    def data(d, n=N):
        if d in (128, 256):
            A, X, b = H.int_data(d)
        else:                                                                  # (one generator: three independent draws)
            rng = np.random.default_rng(d)
            A, X, b = rng.integers(-1, 2, (n, d)), rng.integers(-2, 3, (K, d)), rng.integers(-2, 3, n)
        return tuple(torch.from_numpy(np.ascontiguousarray(a).astype(dtype)) for a in (A[:n], X[:K], b[:n]))

    def run(A, X, b, a_off=0, x_off=None, monitor=False):
        """-> (report, outputs, K single sweeps); x_off: the one iterate that is shifted one element"""
        d = A.shape[1]
        GA, Gb = Guarded(A, off=a_off, device="cuda", name="A"), Guarded(b, device="cuda", name="b")
        GX = Guarded(X, ld=d + v, device="cuda", name="iterates")
        xs = rows(GX)
        shifted = None
        if x_off is not None:
            shifted = Guarded(X[x_off], off=1, device="cuda", name="the shifted iterate")
            xs[x_off] = shifted.view
        assert [x.data_ptr() % 16 != 0 for x in xs] == [k == x_off for k in range(K)] and (GA.view.data_ptr() % 16 != 0) == bool(a_off)
        F = PackedF.least_squares(GA.view, Gb.view, 0.5)
        out = Guarded(shape=(K, d), dtype=dtype, ld=d + v, device="cuda", name="outputs")
        obj = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
        if monitor:
            ctx.set_monitor(ProxG(L.PROX_L1, lam=0.02), obj)
        try:
            ctx.full_gradient_multi(F, xs, rows(out))
            report = ctx.last_kernel()
        finally:
            ctx.set_monitor(None, None)
        out.check_outside(report)
        for g in (GA, Gb, GX) + ((shifted,) if shifted is not None else ()):
            g.check_unchanged(report)
        assert not has_poison(out.view) and bool(torch.isnan(obj).any()) != monitor
        return report, out.view.contiguous(), single_sweeps(ctx, F, xs)

    base = data(256)
    report, got, solo = run(*base)                                             # the control: nothing shifted
    assert report == H.report(dtype, 256, N, K, num_cu), report
    want = torch.from_numpy(H.expected(H.int_reference(256, N, K)[0], 0.5, N, dtype)).cuda()
    assert same_bits(got, want) and same_bits(solo, want)                       # (N a power of two: the sweeps are exact too)
    cases = [("the objective monitor", base, dict(monitor=True)), ("A one element off alignment", base, dict(a_off=1)),
             ("the last iterate one element off alignment", base, dict(x_off=K - 1)), ("the first iterate one element off alignment", base, dict(x_off=0)),
             ("d = 1040", data(1040, 64), {}), ("d = 2048", data(2048, 64), {})]
    if dtype == np.float32:
        cases.append(("fp32 d = 128", data(128), {}))
    for what, dat, kw in cases:
        report, got, solo = run(*dat, **kw)
        assert "mrhs_kernel" not in report, (what, report)
        assert same_bits(got, solo), what
        if dat is base:
            assert same_bits(got, want), what
    if dtype == np.float64:                                                    # the same 128 columns in fp64 do take the kernel
        assert run(*data(128))[0] == H.report(dtype, 128, N, K, num_cu)
    ctx.synchronize()


# ---- 4. the epoch tail of K solves -----------------------------------------------------------------------------------------------------
def tail_states(arrays, ld, what=""):
    """(av, z, z_full, w) of K solves: four guarded (K, d) buffers"""
    return [Guarded(a, ld=ld, device="cuda", name=f"{nm}{what}") for a, nm in zip(arrays, ("av", "z", "z_full", "w"))]


@pytest.mark.parametrize("shape", ["kernel", "fallback"])
@pytest.mark.parametrize("plus", [False, True], ids=["basic", "plus"])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
@pytest.mark.parametrize("dtype", BOTH)
def test_epoch_tails_of_K_solves(ctx, num_cu, dtype, loss, plus, shape):
    """ciao_svrg_epoch_tail_multi against K calls of ciao_svrg_epoch_tail: z, z_full and w in bits (the tail is elementwise), av in bits
    where the call runs K single sweeps (d = 100) and within the single-sweep scales of part 2 on the kernel (d = 256, K = 256, N = 768:
    three tiles a partition, one steady step)."""
    import torch
    N, d, K = (768, 256, 256) if shape == "kernel" else (300, 100, 5)
    m = 17
    if shape == "kernel":
        assert "3 whole tiles" in H.classes([(N, K)], num_cu)
    A, b, _ = P.synthetic(loss, N, d, dtype, seed=5)
    _, dp = make(loss, A, b, float(N) if loss == "ls" else 1.0, dtype)
    rng = np.random.default_rng(K + d)
    start = [(rng.standard_normal((K, d)) * (0.3 + 0.1 * (np.arange(K) % 20))[:, None]).astype(dtype) for _ in range(4)]
    G = tail_states(start, d + vec(dtype))
    solo = [torch.from_numpy(a.copy()).cuda() for a in start]
    ctx.svrg_epoch_tail_multi(dp, m, plus, *(rows(g) for g in G))
    report = ctx.last_kernel()
    assert report == H.report(dtype, d, N, K, num_cu) if shape == "kernel" else "mrhs_kernel" not in report, report
    for g in G:
        g.check_outside(report)
        assert not has_poison(g.view)
    for k in range(K):
        ctx.svrg_epoch_tail(dp, m, plus, *(s[k] for s in solo))
    for g, s, nm in list(zip(G, solo, ("av", "z", "z_full", "w")))[1:]:
        assert same_bits(g.view, s), f"{nm} of the K tails in one call differs from the K single tails"
    assert not bool(solo[1].any()) and same_bits(solo[3], solo[2] if not plus else torch.from_numpy(start[3]).cuda())
    if shape == "fallback":
        assert same_bits(G[0].view, solo[0]), "av: K single sweeps inside the call against K calls"
    else:
        got, ref = G[0].view.cpu().numpy(), solo[0].cpu().numpy()
        k, r = worst_solve(got, ref, dtype)
        print(f"{loss} {np.dtype(dtype).name} plus={plus}: av of the worst solve ({k}) {r:.2f} eps from its single sweep")
        close(got[k], ref[k], dtype, scale={64: 44, 32: 48}, what=f"epoch tails of K solves: av vs the single tail ({loss}, plus={plus}, solve {k})")
    ctx.synchronize()


@pytest.mark.parametrize("dtype", BOTH)
def test_epoch_tail_on_integer_rows_exactly(ctx, num_cu, dtype):
    """z = 16 X with m = 16 on the integer rows of part 1: z_full = z / m is the integer iterate X exactly, so av is part 1's exact result
    (d = 256, N = 768, K = 256), w = z_full and z = 0 -- all in bits."""
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    d, N, K = 256, 768, 256
    A, X, b = H.int_data(d)
    lam = H.lam_of((N, K))
    F = PackedF.least_squares(torch.from_numpy(A[:N].astype(dtype)).cuda(), torch.from_numpy(b[:N].astype(dtype)).cuda(), lam)
    G = [Guarded(shape=(K, d), dtype=dtype, ld=d + vec(dtype), device="cuda", name=nm) for nm in ("av", "z", "z_full", "w")]   # outputs: poison
    G[1] = Guarded((16 * X[:K]).astype(dtype), ld=d + vec(dtype), device="cuda", name="z")
    ctx.svrg_epoch_tail_multi(F, 16, False, *(rows(g) for g in G))
    assert ctx.last_kernel() == H.report(dtype, d, N, K, num_cu), ctx.last_kernel()
    for g in G:
        g.check_outside(ctx.last_kernel())
    Xd = torch.from_numpy(X[:K].astype(dtype)).cuda()
    want = torch.from_numpy(H.expected(H.int_reference(d, N, K)[0], lam, N, dtype)).cuda()
    assert same_bits(G[2].view, Xd) and same_bits(G[3].view, Xd) and not bool(G[1].view.any())
    assert same_bits(G[0].view, want)
    ctx.synchronize()


def test_lockstep_solves_with_one_pass_svrg_plus(ctx, ciao):
    """solvers.solve_together(one_pass=True) with SVRG++ (plus=True: w is kept, m doubles every outer step) on the problem and under the
    bound of tests/test_gpu_multi_rhs.py::test_svrg_epoch_tails_of_K_solves_in_one_pass."""
    import ciaoalgorithms_jl_amd._lib as L
    from ciaoalgorithms_jl_amd.device import PackedF, ProxG
    from ciaoalgorithms_jl_amd import solvers as S
    dtype, N, d = np.float64, 3000, 1024
    A, b, _ = P.synthetic("ls", N, d, dtype, seed=3)
    _, dp = make("ls", A, b, float(N), dtype)
    F = PackedF.least_squares(dp.A, dp.b, float(N))
    gamma = 1.0 / (7 * float((float(N) * np.sum(A * A, axis=1)).max()))
    lams = [0.01 * (1 + k) for k in range(6)]

    def solve(one_pass):
        ctx.set_option("svrg_cache_rowdots", 0)
        try:
            its = [S.iterator(S.SVRG(np.float64, γ=gamma, plus=True), np.zeros(d), F=F, g=ProxG(L.PROX_L1, lam=lam), N=N, ctx=ctx,
                              stream=ciao.IndexStream(100 + k)) for k, lam in enumerate(lams)]
            xs, it = S.solve_together(its, 5, one_pass=one_pass)
            return xs, it, ctx.last_kernel()
        finally:
            ctx.set_option("svrg_cache_rowdots", 1)

    xs0, it0, _ = solve(False)
    xs1, it1, _ = solve(True)
    assert it0 == it1 == 5
    worst = max(np.abs(u - v).max() / max(np.abs(u).max(), 1e-30) for u, v in zip(xs0, xs1))
    print(f"SVRG++ in lockstep, one pass against K sweeps per outer step: worst relative difference {worst:.3e}")
    for u, v in zip(xs0, xs1):
        assert np.abs(u - v).max() <= 1e-11 * max(np.abs(u).max(), 1e-30)
    ctx.synchronize()

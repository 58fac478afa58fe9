"""GPU parity tests proper: every C-ABI entry point of libciao_hip.so against the CPU oracle on the same seeded
inputs (sizes the oracle finishes in seconds), through the ctypes binding (the same ABI a Julia ccall binds).

Stated tolerance (north_star: "iterates matching the CPU reference to a stated fp64 tolerance"), in units of the
rounding unit of the real type R (eps = 2.2e-16 for fp64, 1.2e-7 for fp32):

        | device - oracle |_inf  <=  scale * eps(R) * | oracle |_inf

with `scale` written at every comparison.  The scales are not guesses: every comparison logs its observed error in
these units (gpurun_out/parity_observed.json, written by conftest.py at the end of a GPU run; the committed copy is
profiles/r02_parity_observed.json) and tools/retune_scales.py sets each `scale=` to 10x the largest value observed at
that call site over both dtypes, rounded up to 1-2-5 (floor 8).  What to expect (DESIGN.md section 5 has the law):
one sweep over N rows is a sum of N terms in a fixed tree order against the oracle's sequential order, 2-20 eps
observed; a dependent chain grows about linearly in the number of steps (a few hundred eps after 3 000 SVRG steps).
Bitwise equality is not attainable: the reference sums sequentially (SVRG_basic.jl:59-63) while the device sums
in a fixed tree order; the device result is bitwise reproducible run to run (tested below).
"""
import os

import numpy as np
import pytest

import problems as P

pytestmark = pytest.mark.gpu

EPS = {np.float64: float(np.finfo(np.float64).eps), np.float32: float(np.finfo(np.float32).eps)}
CALIBRATE = os.environ.get("CIAO_PARITY_CALIBRATE") == "1"   # log only (tools/retune_scales.py reads the log)


# iterates match the reference to 1e-10 (Float64) / 1e-4 (Float32) relative.  In units of eps(R) that is 4.5e5 and
# 840: no `scale` below may exceed them, and tests/test_gpu_parity.py::test_stated_tolerances_stay_inside_the_baseline checks that
# none does.  The statement is two-sided for Float32:
#   (i)  ACCURACY: the device's Float32 result against the oracle run in FLOAT64 on the same Float32 data (oracle/twin.py keeps a
#        Float64 twin of every Float32 oracle state; `ref64=` overrides), in eps32 units --
#        at most 840, set from measurement.  This is the statement about the device;
#   (ii) the Float32 oracle itself (`ref`): the reference's own arithmetic in Float32 -- sequential left folds `av += delta` whose every
#        addend is a fraction of an ulp of the sum -- is often the LESS accurate of the two (test_C5...: 2932 eps32 from the Float64
#        value where the device is 0.7 away), so this bound says how far two Float32 evaluations of the same formula drift apart.
# `scale` is a number (one bound for both types) or {64: a, 32: b}; tools/retune_scales.py writes them from a calibration run
# (10 x the largest error observed at the call site and type, two significant digits, floor 8).
BASELINE_EPS = {np.dtype(np.float64): 1e-10 / np.finfo(np.float64).eps, np.dtype(np.float32): 1e-4 / np.finfo(np.float32).eps}


def _scale_for(scale, dtype):
    if isinstance(scale, dict):
        return float(scale[64 if np.dtype(dtype) == np.float64 else 32])
    return float(scale)


def close(dev, ref, dtype, scale=8, what="", ref64=None, scale64=None, size=None):
    """size: the magnitude one rounding unit is taken at, where it is not the result's own -- a result formed as a DIFFERENCE of
    larger quantities (ProShI's z = (prox(av) - av) / hat_gamma) carries their rounding"""
    dev = dev.detach().cpu().numpy() if hasattr(dev, "detach") else np.asarray(dev)
    import inspect
    fr = inspect.stack()[1]

    def one(ref, scale, form):
        ref = np.asarray(ref)
        unit = EPS[dtype] * max(np.abs(ref).max(initial=0.0) if size is None else float(size), 1e-30)     # one rounding unit at the size of the reference
        bound = scale * unit
        err = np.abs(dev.astype(np.float64) - ref.astype(np.float64)).max(initial=0.0)
        # every comparison is logged as (error in eps units, scale allowed); conftest.py writes gpurun_out/parity_observed.json
        P.PARITY_LOG.append({"file": os.path.basename(fr.filename), "test": fr.function, "line": fr.lineno, "what": what + form, "dtype": np.dtype(dtype).name,
                             "ratio": float(err / unit), "scale": float(scale), "form": "f64 oracle" if form else "oracle"})
        if not CALIBRATE:
            assert err <= bound, f"{what}{form}: max abs err {err:.3e} = {err / unit:.1f} eps > {scale} eps ({bound:.3e})"

    one(ref, _scale_for(scale, dtype), "")
    if ref64 is None and np.dtype(dtype) == np.float32:
        # form (i) comes by itself wherever `ref` is a result of the twinned oracle (oracle/twin.py: every Float32 oracle call is
        # repeated in Float64 on the same data, state for state); ref64=False switches it off (a site must say why)
        from oracle import twin
        ref64 = twin.twin_of(ref)
    if ref64 is not None and ref64 is not False:   # Float32 runs only: form (i)
        assert np.dtype(dtype) == np.float32 and np.asarray(ref64).dtype == np.float64
        one(ref64, float(scale64 if scale64 is not None else BASELINE_EPS[np.dtype(np.float32)]), " [vs the Float64 oracle on the Float32 data]")


def make(loss, A, b, lam_f, dtype, pad=0):
    """(oracle Problem, device PackedF) over the same data; pad > 0 gives the device copy a row stride d+pad, the padding columns
    poisoned (tests/layouts.py): what a row's padding holds is unspecified input and must stay out of every result."""
    import torch
    from oracle import twin as O
    from ciaoalgorithms_jl_amd.device import PackedF
    import ciaoalgorithms_jl_amd._lib as L
    import layouts
    op = O.Problem(loss, A, b, lam_f)
    N, d = A.shape
    tA = torch.from_numpy(A).cuda()
    if pad:
        buf = layouts.poisoned((N, d + pad), tA.dtype, "cuda")
        buf[:, :d] = tA
        tA = buf[:, :d]
    tb = torch.from_numpy(b).cuda()
    kind = {"ls": L.LOSS_LS, "logistic": L.LOSS_LOGISTIC}[loss]
    return op, PackedF(kind, tA, tb, lam_f)


def make_g(kind, dtype, d, lam=0.05, data_dtype=None):
    """(oracle Prox, device ProxG).  data_dtype=np.float32 with dtype=np.float64: the Float64 oracle on the Float32 run's bounds."""
    import torch
    from oracle import twin as O
    from ciaoalgorithms_jl_amd.device import ProxG
    import ciaoalgorithms_jl_amd._lib as L
    if kind == "zero":
        return O.Prox("zero"), ProxG(L.PROX_ZERO)
    if kind == "l1":
        return O.Prox("l1", lam=lam), ProxG(L.PROX_L1, lam=lam)
    if kind == "box":
        return O.Prox("box", lo=-0.2, hi=0.3, dtype=dtype), ProxG(L.PROX_BOX, lo=-0.2, hi=0.3)
    lo = np.linspace(-0.3, 0.0, d).astype(data_dtype or dtype).astype(dtype)
    hi = np.linspace(0.05, 0.4, d).astype(data_dtype or dtype).astype(dtype)
    return (O.Prox("box", lo=lo, hi=hi, dtype=dtype),
            ProxG(L.PROX_BOX, lo_vec=torch.from_numpy(lo).cuda(), hi_vec=torch.from_numpy(hi).cuda()))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


SHAPES = [(1, 1), (6, 3), (8, 5), (37, 50), (200, 64), (129, 128), (300, 256), (64, 1024), (33, 1000), (16, 2048), (5, 4096),
          (40, 1536), (12, 3000), (9, 8192), (700, 1100), (25, 1001), (7, 3001), (300, 257)]


# ----------------------------------------------------------------------------------------------------------------------
# L1 plugin API
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
def test_gradient_single_sample(ctx, dtype, loss):
    import torch
    from oracle import twin as O
    A, b, x = P.synthetic(loss, 9, 70, dtype)
    op, dp = make(loss, A, b, 9.0, dtype)
    y = torch.empty(70, dtype=dev(x).dtype, device="cuda")
    fv = torch.empty(1, dtype=y.dtype, device="cuda")
    for i in (0, 4, 8):
        ctx.gradient(dp, i, dev(x), y, fv)
        gy, f = O.gradient(op.loss, A[i], b[i], 9.0, x)
        close(y, gy, dtype, scale={64: 500, 32: 240}, what=f"gradient i={i}", scale64=40)
        close(fv, [f], dtype, scale={64: 1000, 32: 500}, what="f_i value")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("gk", ["zero", "l1", "box", "boxvec"])
def test_prox(ctx, dtype, gk):
    import torch
    from oracle import twin as O
    rng = np.random.default_rng(3)
    for d in (1, 5, 257, 1024):
        x = rng.standard_normal(d).astype(dtype)
        og, dg = make_g(gk, dtype, d)
        y = torch.empty(d, dtype=dev(x).dtype, device="cuda")
        ctx.prox(dg, dev(x), 0.7, y)
        assert np.array_equal(y.cpu().numpy(), O.prox(og, x, dtype(0.7))), "prox is elementwise: must be bit-exact"
        xin = dev(x)
        ctx.prox(dg, xin, 0.7, xin)  # in place
        assert np.array_equal(xin.cpu().numpy(), O.prox(og, x, dtype(0.7)))


# ----------------------------------------------------------------------------------------------------------------------
# the sweep: S2 / S4 (full gradient), fused prox-gradient step, objective
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
@pytest.mark.parametrize("shape", SHAPES)
def test_full_gradient(ctx, dtype, loss, shape):
    import torch
    from oracle import twin as O
    N, d = shape
    A, b, x = P.synthetic(loss, N, d, dtype, seed=N + d)
    op, dp = make(loss, A, b, float(N), dtype)
    av = torch.empty(d, dtype=dev(x).dtype, device="cuda")
    ctx.full_gradient(dp, dev(x), av)
    ref = O.full_pass(op, x)
    ref64 = O.full_pass(O.Problem(loss, A.astype(np.float64), b.astype(np.float64), float(N)), x.astype(np.float64))
    # judge against the fp64 oracle so that the fp32 oracle's own sequential-sum error does not enter
    close(av, ref64, dtype, scale={64: 81, 32: 15}, what=f"full_gradient {ctx.last_kernel()}")
    close(av, ref, dtype, scale={64: 81, 32: 100}, what="full_gradient vs same-precision oracle", scale64=15)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_full_gradient_generic_equals_fast(ctx, dtype):
    """Same rows through the LDS-accumulator generic kernel and through the register fast path."""
    import torch
    A, b, x = P.synthetic("ls", 500, 512, dtype)
    _, dp = make("ls", A, b, 500.0, dtype)
    av1 = torch.empty(512, dtype=dev(x).dtype, device="cuda")
    av2 = torch.empty_like(av1)
    ctx.full_gradient(dp, dev(x), av1)
    assert "rows_fast_kernel" in ctx.last_kernel() or "rows_multi_kernel" in ctx.last_kernel()
    ctx.set_option("force_generic", 1)
    try:
        ctx.full_gradient(dp, dev(x), av2)
        assert "rows_generic_kernel" in ctx.last_kernel()
    finally:
        ctx.set_option("force_generic", 0)
    close(av2, av1.cpu().numpy(), dtype, scale={64: 10, 32: 8}, what="generic vs fast")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_full_gradient_padded_rows_and_prefetch_variants(ctx, dtype):
    import torch
    from oracle import twin as O
    A, b, x = P.synthetic("logistic", 1000, 256, dtype)
    op, dp = make("logistic", A, b, 1.0, dtype, pad=64)   # ld = 320: still 16-byte aligned rows -> fast path
    assert dp.ld == 320
    ref = O.full_pass(op, x)
    outs = []
    for pf in (1, 0):
        ctx.set_option("sweep_prefetch", pf)
        av = torch.empty(256, dtype=dev(x).dtype, device="cuda")
        ctx.full_gradient(dp, dev(x), av)
        assert "rows_fast_kernel" in ctx.last_kernel() or "rows_multi_kernel" in ctx.last_kernel()
        close(av, ref, dtype, scale={64: 79, 32: 46}, what=f"padded rows prefetch={pf}", scale64=8)
        outs.append(av.cpu().numpy())
    ctx.set_option("sweep_prefetch", -1)
    # the two pipelining flavours assign the same rows to the same waves: identical summation order
    assert np.array_equal(outs[0], outs[1])
    op2, dp2 = make("logistic", A, b, 1.0, dtype, pad=3)    # ld = 259: rows with no 16-byte alignment -> element-wise chunks
    av = torch.empty(256, dtype=dev(x).dtype, device="cuda")
    ctx.full_gradient(dp2, dev(x), av)
    assert "rows_split_kernel" in ctx.last_kernel() and "scalar" in ctx.last_kernel(), ctx.last_kernel()
    close(av, ref, dtype, scale={64: 79, 32: 37}, what="unaligned rows", scale64=8)
    ctx.set_option("force_generic", 1)
    try:
        ctx.full_gradient(dp2, dev(x), av)
        assert "rows_generic_kernel" in ctx.last_kernel()
    finally:
        ctx.set_option("force_generic", 0)
    close(av, ref, dtype, scale={64: 84, 32: 42}, what="unaligned rows, generic kernel", scale64=8)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d", [256, 512, 1024])
def test_multi_row_sweep_matches_single_row_sweep(ctx, dtype, d):
    """Short rows go through rows_multi_kernel (R rows per wave per iteration); same result as one row per wave, also
    when the row count is not a multiple of R and with an index list (LFinito-style two-point batch)."""
    import torch
    from oracle import twin as O
    N = 1003
    A, b, x = P.synthetic("logistic", N, d, dtype, seed=d)
    op, dp = make("logistic", A, b, 1.0, dtype)
    outs = {}
    for multi in (1, 0):
        ctx.set_option("sweep_multi", multi)
        av = torch.empty(d, dtype=dev(x).dtype, device="cuda")
        ctx.full_gradient(dp, dev(x), av)
        outs[multi] = (av.cpu().numpy(), ctx.last_kernel())
    ctx.set_option("sweep_multi", 1)
    if d * np.dtype(dtype).itemsize in (2048, 4096):
        assert "rows_multi_kernel" in outs[1][1] and "rows_fast_kernel" in outs[0][1]
    ref = O.full_pass(op, x)
    close(outs[1][0], ref, dtype, scale={64: 61, 32: 73}, what="multi-row sweep", scale64=8.9)
    close(outs[0][0], ref, dtype, scale={64: 61, 32: 73}, what="single-row sweep", scale64=8)


def test_full_gradient_empty_problem(ctx):
    """N = 0 (empty input): the sum over no samples is the zero vector."""
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    import ciaoalgorithms_jl_amd._lib as L
    A = torch.zeros((0, 16), dtype=torch.float64, device="cuda")
    b = torch.zeros((0,), dtype=torch.float64, device="cuda")
    dp = PackedF(L.LOSS_LS, A, b, 1.0, N_total=1)
    av = torch.full((16,), 7.0, dtype=torch.float64, device="cuda")
    ctx.full_gradient(dp, torch.ones(16, dtype=torch.float64, device="cuda"), av)
    assert torch.count_nonzero(av).item() == 0


def test_zero_loss(ctx):
    """F = fill(Zero(), N) (SVRG.jl:58): every gradient is zero, SVRG reduces to repeated prox."""
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    for tdt in (torch.float64, torch.float32):   # (rows of 17 .. 255 elements WITH data run the LDS-DMA kernel: not these, there is no A)
        dp = PackedF.zero(10, 33, tdt)
        av = torch.full((33,), 7.0, dtype=tdt, device="cuda")
        ctx.full_gradient(dp, torch.ones(33, dtype=tdt, device="cuda"), av)
        assert torch.count_nonzero(av).item() == 0 and "rows_smallm" not in ctx.last_kernel(), ctx.last_kernel()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("gk", ["zero", "l1", "boxvec"])
def test_proxgrad_step_and_objective(ctx, dtype, gk):
    import torch
    from oracle import twin as O
    for loss, (N, d) in (("ls", (300, 1024)), ("logistic", (77, 50))):
        A, b, x = P.synthetic(loss, N, d, dtype)
        op, dp = make(loss, A, b, float(N), dtype)
        og, dg = make_g(gk, dtype, d, lam=0.01)
        gamma = 0.05
        av = torch.empty(d, dtype=dev(x).dtype, device="cuda")
        y = torch.empty_like(av)
        ctx.proxgrad_step(dp, dg, gamma, dev(x), av, y)
        rav = O.full_pass(op, x)
        ry = O.prox(og, (x - dtype(gamma) * rav).astype(dtype), dtype(gamma))
        close(av, rav, dtype, scale={64: 36, 32: 50}, what="proxgrad av", scale64=8.9)
        close(y, ry, dtype, scale=8, what="proxgrad y", scale64=8)
        obj = ctx.objective(dp, dg, dev(x))
        robj = O.objective(op, og, x)
        assert abs(obj - robj) <= (1e-9 if dtype == np.float64 else 2e-4) * max(1.0, abs(robj))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(300, 1024), (77, 50), (40, 1536)])
def test_objective_monitor_rides_on_the_full_pass(ctx, ciao, dtype, shape):
    """ciao_ctx_set_monitor: with a monitor set, the full passes that SVRG / LFinito / the prox-gradient
    step make anyway also leave (1/N) sum f_i(x) + g(x), the value `gradient!` returns and the reference discards
    (SVRG_basic.jl:89, test_lasso.jl:45-47) -- checked against orc_objective at the point of the pass."""
    import torch
    from oracle import twin as O
    N, d = shape
    rtol = 1e-11 if dtype == np.float64 else 5e-5
    for loss in ("ls", "logistic"):
        A, b, x = P.synthetic(loss, N, d, dtype, seed=5)
        op, dp = make(loss, A, b, float(N) if loss == "ls" else 1.0, dtype)
        og, dg = make_g("l1", dtype, d, lam=0.02)
        obj = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
        tdt = dev(x).dtype
        ctx.set_monitor(dg, obj)
        try:
            av = torch.empty(d, dtype=tdt, device="cuda")
            ctx.full_gradient(dp, dev(x), av)
            ctx.synchronize()
            o = obj.cpu().numpy()
            ref = O.objective(op, og, x)
            assert abs(o[0] - ref) <= rtol * max(1.0, abs(ref)), (o, ref)
            assert abs(o[0] - (o[1] + o[2])) <= 1e-15 * max(1.0, abs(o[0]))
            assert abs(o[2] - 0.02 * np.abs(x.astype(np.float64)).sum()) <= (1e-12 if dtype == np.float64 else 1e-6) * max(1.0, o[2])
            close(av, O.full_pass(op, x), dtype, scale={64: 65, 32: 39}, what="the gradient is unchanged by the monitor", scale64=9.8)
            # prox-gradient step IN PLACE: the monitored point is the x the pass read, not the y it wrote
            xin = dev(x).clone()
            ctx.proxgrad_step(dp, dg, 0.01, xin, av, xin)
            ctx.synchronize()
            assert abs(obj[0].item() - ref) <= rtol * max(1.0, abs(ref))
            # SVRG: the tail pass of an epoch is taken at the new z_full = solution(state)
            gamma = 0.5 if loss == "logistic" else 1.0 / (7 * N * float(np.max(np.sum(A.astype(np.float64) ** 2, axis=1))))
            z, zf, w = (torch.empty(d, dtype=tdt, device="cuda") for _ in range(3))
            ctx.svrg_init(dp, dev(x), av, z, zf, w)
            ctx.synchronize()
            assert abs(obj[0].item() - ref) <= rtol * max(1.0, abs(ref))
            idx = ciao.IndexStream(2).rand_indices(N, N)
            ctx.svrg_iterate(dp, dg, gamma, idx, False, av, z, zf, w)
            ctx.synchronize()
            ref_zf = O.objective(op, og, zf.cpu().numpy())
            assert abs(obj[0].item() - ref_zf) <= rtol * max(1.0, abs(ref_zf))
            # LFinito: the full pass is taken at z_full = prox(av)
            gam = torch.full((N,), 0.3, dtype=tdt, device="cuda")
            hg = ctx.hat_gamma(gam)
            ctx.lfinito_init(dp, hg, dev(x), av, z, zf)
            bptr = np.arange(0, N + 1, 7, dtype=np.int64)
            bptr = np.append(bptr, N) if bptr[-1] != N else bptr
            ctx.lfinito_iterate(dp, dg, gam, hg, bptr, np.arange(N, dtype=np.int64), av, z, zf)
            ctx.synchronize()
            ref_zf = O.objective(op, og, zf.cpu().numpy())
            assert abs(obj[0].item() - ref_zf) <= rtol * max(1.0, abs(ref_zf))
        finally:
            ctx.set_monitor(None, None)
        # switched off: nothing is written any more
        obj.fill_(-1.0)
        ctx.full_gradient(dp, dev(x), av)
        ctx.synchronize()
        assert obj[0].item() == -1.0


def test_sweep_is_bitwise_reproducible(ctx):
    import torch
    A, b, x = P.synthetic("ls", 5000, 1024, np.float64)
    _, dp = make("ls", A, b, 5000.0, np.float64)
    outs = []
    for _ in range(3):
        av = torch.empty(1024, dtype=torch.float64, device="cuda")
        ctx.full_gradient(dp, dev(x), av)
        outs.append(av.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


# ----------------------------------------------------------------------------------------------------------------------
# SVRG
# ----------------------------------------------------------------------------------------------------------------------
# d*sizeof(T) a multiple of 4096 B selects the LDS-DMA chain (f64: 512, 1024, 2048, 4096; f32: 1024, 2048, 4096);
# everything else (and every shape again with chain_no_dma=1) runs the register-ring chain
CHAIN_SHAPES = [(6, 3), (8, 5), (50, 50), (40, 256), (30, 300), (12, 512), (64, 1024), (20, 1500), (9, 2048), (10, 4096), (15, 1001), (11, 1501)]


@pytest.fixture(params=[0, 1], ids=["dma", "regring"])
def chain_variant(request, ctx):
    ctx.set_option("chain_no_dma", request.param)
    yield request.param
    ctx.set_option("chain_no_dma", 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
@pytest.mark.parametrize("shape", CHAIN_SHAPES)
def test_svrg_epochs(ctx, ciao, chain_variant, dtype, loss, shape):
    """init + 3 x Base.iterate (inner cycle m = 2N, tail, full pass) vs the oracle, same index stream."""
    import torch
    from oracle import twin as O
    N, d = shape
    A, b, x0 = P.synthetic(loss, N, d, dtype, seed=7)
    lam_f = float(N) if loss == "ls" else 1.0
    op, dp = make(loss, A, b, lam_f, dtype)
    og, dg = make_g("l1", dtype, d, lam=0.01)
    Lmax = (lam_f if loss == "ls" else 0.25) * np.max(np.sum(A.astype(np.float64) ** 2, axis=1))
    gamma = 1.0 / (7 * Lmax)
    st = ciao.IndexStream(5)
    tdt = dev(x0).dtype
    av, z, zf, w = (torch.empty(d, dtype=tdt, device="cuda") for _ in range(4))
    ctx.svrg_init(dp, dev(x0), av, z, zf, w)
    rav, rz, rzf, rw = O.svrg_init(op, x0)
    close(av, rav, dtype, scale={64: 67, 32: 69}, what="svrg_init av", scale64=15)
    assert np.array_equal(zf.cpu().numpy(), x0) and np.array_equal(w.cpu().numpy(), x0) and not z.any().item()
    m = 2 * N
    for ep in range(3):
        idx = st.rand_indices(N, m)
        ctx.svrg_iterate(dp, dg, gamma, idx, False, av, z, zf, w)
        O.svrg_iterate(op, og, dtype(gamma), idx, False, rav, rz, rzf, rw)
        close(zf, rzf, dtype, scale={64: 610, 32: 410}, what=f"svrg epoch {ep} z_full ({ctx.last_kernel()})", scale64=840)
        close(w, rw, dtype, scale={64: 610, 32: 410}, what=f"svrg epoch {ep} w", scale64=840)
        close(av, rav, dtype, scale={64: 160, 32: 170}, what=f"svrg epoch {ep} av", scale64=290)
        assert not z.any().item()
    ctx.synchronize()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d,expect", [(1024, "chain_dma_kernel<{t},J{j},alg0>"), (1000, "chain_dma_kernel<{t},J{j},alg0,masked>"),
                                      (1500, "chain_dma_kernel<{t},J{jj},alg0,masked>"), (7, "chain_kernel<")])
def test_chain_path_selection(ctx, ciao, dtype, d, expect):
    """Which kernel runs the SVRG inner cycle: the LDS-DMA ring for every row of whole 16-byte chunks up to 32 KiB (dead
    chunks masked when the row is not J*4096 bytes), the register ring otherwise -- and each against the oracle with
    per-coordinate box bounds, which the dead chunks must not read."""
    import torch
    from oracle import twin as O
    N = 40
    A, b, x0 = P.synthetic("ls", N, d, dtype, seed=d)
    op, dp = make("ls", A, b, float(N), dtype)
    og, dg = make_g("boxvec", dtype, d)
    tdt = dev(x0).dtype
    av, z, zf, w = (torch.empty(d, dtype=tdt, device="cuda") for _ in range(4))
    ctx.svrg_init(dp, dev(x0), av, z, zf, w)
    rav, rz, rzf, rw = O.svrg_init(op, x0)
    idx = ciao.IndexStream(3).rand_indices(N, 3000)   # three chunks of the staged index stream
    gamma = 0.02
    ctx.svrg_inner(dp, dg, gamma, idx, av, z, zf, w)
    es = np.dtype(dtype).itemsize
    j = 1
    while j * 4096 < d * es:
        j *= 2
    name = expect.format(t="f64" if es == 8 else "f32", j=j, jj=j)
    assert name in ctx.last_kernel(), ctx.last_kernel()
    O.svrg_inner(op, og, dtype(gamma), idx, rav, rz, rzf, rw)
    close(w, rw, dtype, scale={64: 3700, 32: 3300}, what=f"svrg_inner w ({ctx.last_kernel()})", scale64=840)
    close(z, rz, dtype, scale={64: 2300, 32: 1900}, what="svrg_inner z (sum of 3000 iterates)", scale64=840)
    ctx.synchronize()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_svrg_plus_and_inner_only(ctx, ciao, dtype):
    import torch
    from oracle import twin as O
    N, d = 25, 130
    A, b, x0 = P.synthetic("logistic", N, d, dtype, seed=2)
    op, dp = make("logistic", A, b, 1.0, dtype)
    og, dg = make_g("boxvec", dtype, d)
    gamma = 0.3
    tdt = dev(x0).dtype
    av, z, zf, w = (torch.empty(d, dtype=tdt, device="cuda") for _ in range(4))
    ctx.svrg_init(dp, dev(x0), av, z, zf, w)
    rav, rz, rzf, rw = O.svrg_init(op, x0)
    st = ciao.IndexStream(11)
    m = 3
    for ep in range(4):   # SVRG++: w is not reset, m doubles (SVRG_basic.jl:85,93)
        idx = st.rand_indices(N, m)
        ctx.svrg_iterate(dp, dg, gamma, idx, True, av, z, zf, w)
        O.svrg_iterate(op, og, dtype(gamma), idx, True, rav, rz, rzf, rw)
        m *= 2
        close(zf, rzf, dtype, scale={64: 82, 32: 9.600000000000001}, what=f"svrg++ epoch {ep} z_full", scale64=27)
        close(w, rw, dtype, scale={64: 100, 32: 15}, what=f"svrg++ epoch {ep} w", scale64=38)
    # inner cycle alone accumulates into z
    idx = st.rand_indices(N, 17)
    ctx.svrg_inner(dp, dg, gamma, idx, av, z, zf, w)
    O.svrg_inner(op, og, dtype(gamma), idx, rav, rz, rzf, rw)
    close(z, rz, dtype, scale={64: 95, 32: 14}, what="svrg_inner z", scale64=45)
    close(w, rw, dtype, scale={64: 100, 32: 15}, what="svrg_inner w", scale64=44)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_svrg_rowdot_cache(ctx, ciao, dtype):
    """ciao_svrg_iterate may reuse a_i'z_full from the full pass (one dot per step) when the caller vouches for the state
    (reuse_rowdots).  It must (a) agree with the recomputing kernel and the oracle, (b) never be read without that flag,
    (c) be dropped by the library when another entry point ran in between, whatever the flag says."""
    import torch
    from oracle import twin as O
    N, d = 300, 1024
    A, b, x0 = P.synthetic("logistic", N, d, dtype, seed=13)
    op, dp = make("logistic", A, b, 1.0, dtype)
    og, dg = make_g("l1", dtype, d, lam=0.01)
    gamma = 0.5
    tdt = dev(x0).dtype
    outs = {}
    for reuse in (True, False):
        av, z, zf, w = (torch.empty(d, dtype=tdt, device="cuda") for _ in range(4))
        ctx.svrg_init(dp, dev(x0), av, z, zf, w)
        st = ciao.IndexStream(3)
        for ep in range(3):
            ctx.svrg_iterate(dp, dg, gamma, st.rand_indices(N, 2 * N), False, av, z, zf, w, reuse_rowdots=reuse)
        outs[reuse] = (zf.cpu().numpy().copy(), w.cpu().numpy().copy())
    rav, rz, rzf, rw = O.svrg_init(op, x0)
    st = ciao.IndexStream(3)
    for ep in range(3):
        O.svrg_iterate(op, og, dtype(gamma), st.rand_indices(N, 2 * N), False, rav, rz, rzf, rw)
    for reuse in (True, False):
        close(outs[reuse][0], rzf, dtype, scale={64: 710, 32: 1200}, what=f"svrg z_full reuse={reuse}", scale64=840)
        close(outs[reuse][1], rw, dtype, scale={64: 710, 32: 1200}, what=f"svrg w reuse={reuse}", scale64=840)
    # (b) z_full edited IN PLACE between two iterates (same pointer): without the flag nothing cached is read
    av, z, zf, w = (torch.empty(d, dtype=tdt, device="cuda") for _ in range(4))
    ctx.svrg_init(dp, dev(x0), av, z, zf, w)
    rav, rz, rzf, rw = O.svrg_init(op, x0)
    idx0 = ciao.IndexStream(4).rand_indices(N, N)
    ctx.svrg_iterate(dp, dg, gamma, idx0, False, av, z, zf, w, reuse_rowdots=True)
    O.svrg_iterate(op, og, dtype(gamma), idx0, False, rav, rz, rzf, rw)
    zf.mul_(0.5)                                   # warm restart / projection behind the library's back
    w.copy_(zf)
    O.scale_inplace(rzf, 0.5)                      # (the same edit on the oracle's state -- and on its Float64 twin)
    O.assign(rw, rzf)
    ctx.full_gradient(dp, zf, av)                  # the caller recomputes av at the new point ...
    O.assign(rav, O.full_pass(op, rzf))
    idx = ciao.IndexStream(5).rand_indices(N, N)
    ctx.svrg_iterate(dp, dg, gamma, idx, False, av, z, zf, w)              # ... and does not vouch for the old row dots
    O.svrg_iterate(op, og, dtype(gamma), idx, False, rav, rz, rzf, rw)
    close(zf, rzf, dtype, scale={64: 480, 32: 370}, what="svrg after an in-place z_full edit (reuse_rowdots=0)", scale64=330)
    # (c) another entry point in between: the library drops the cache even if the caller (wrongly) vouches
    av, z, zf, w = (torch.empty(d, dtype=tdt, device="cuda") for _ in range(4))
    ctx.svrg_init(dp, dev(x0), av, z, zf, w)
    rav, rz, rzf, rw = O.svrg_init(op, x0)
    x1 = (x0 * 0.5).astype(dtype)
    ctx.prox(make_g("zero", dtype, d)[1], dev(x1), 1.0, zf)     # z_full <- x1 through the library
    ctx.full_gradient(dp, zf, av)
    O.assign(rzf, x1)
    O.assign(rav, O.full_pass(op, x1))
    ctx.svrg_iterate(dp, dg, gamma, idx, False, av, z, zf, w, reuse_rowdots=True)
    O.svrg_iterate(op, og, dtype(gamma), idx, False, rav, rz, rzf, rw)
    close(zf, rzf, dtype, scale={64: 310, 32: 320}, what="svrg after external z_full change", scale64=200)
    ctx.synchronize()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_svrg_state_edit_between_epochs_through_the_iterable(ctx, ciao, dtype):
    """`solution(state)` IS state.z_full, a mutable tensor.  An in-place torch edit between two iterations
    moves its version counter, so the iterable stops vouching for the cached row dots and the next epoch recomputes --
    checked against the oracle run on the same edited state."""
    from oracle import twin as O
    from ciaoalgorithms_jl_amd import solvers as S
    N, d = 200, 1024
    A, b, x0 = P.synthetic("ls", N, d, dtype, seed=21)
    op, dp = make("ls", A, b, float(N), dtype)
    og, dg = make_g("l1", dtype, d, lam=0.01)
    gamma = 1.0 / (7 * N * float(np.max(np.sum(A.astype(np.float64) ** 2, axis=1))))
    it = S.iterator(S.SVRG(dtype, γ=gamma), dev(x0), F=dp, g=dg, N=N, ctx=ctx, stream=ciao.IndexStream(9))
    states = iter(it)
    st = next(states)
    st = next(states)                                   # one epoch: the library now holds a_i'z_full for this z_full
    rav, rz, rzf, rw = O.svrg_init(op, x0)
    ref_stream = ciao.IndexStream(9)
    O.svrg_iterate(op, og, dtype(gamma), ref_stream.rand_indices(N, N), False, rav, rz, rzf, rw)
    close(st.z_full, rzf, dtype, scale=270, what="epoch 1", scale64=380)
    st.z_full.mul_(0.25)                                # user edits the solution tensor in place
    st.w.copy_(st.z_full)
    ctx.full_gradient(dp, st.z_full, st.av)
    O.scale_inplace(rzf, 0.25)
    O.assign(rw, rzf)
    O.assign(rav, O.full_pass(op, rzf))
    st = next(states)
    O.svrg_iterate(op, og, dtype(gamma), ref_stream.rand_indices(N, N), False, rav, rz, rzf, rw)
    close(st.z_full, rzf, dtype, scale={64: 460, 32: 470}, what="epoch after an in-place edit of state.z_full", scale64=640)
    st = next(states)                                   # untouched state again: reuse is back on and still right
    O.svrg_iterate(op, og, dtype(gamma), ref_stream.rand_indices(N, N), False, rav, rz, rzf, rw)
    close(st.z_full, rzf, dtype, scale={64: 630, 32: 590}, what="epoch after that", scale64=810)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d", [1024, 1000, 4096])
def test_chain_over_a_shard_table_is_bitwise_the_unsharded_chain(ctx, ciao, dtype, d):
    """ciao_ctx_set_shards: the rows of the problem live in several allocations (here three slices of one matrix, uneven, one
    of them empty; on a node: the other GPUs' HBM, peer-mapped) and the one chain addresses each step's row through the
    shard table.  Same kernel, same arithmetic, same order -> SVRG inner cycle and SAGA steps bitwise equal to the unsharded
    run, including the table rows written through the shard pointers."""
    import torch
    import ciaoalgorithms_jl_amd._lib as L
    N = 600
    A, b, x0 = P.synthetic("logistic", N, d, dtype, seed=41)
    op, dp = make("logistic", A, b, 1.0, dtype)
    og, dg = make_g("l1", dtype, d, lam=0.01)
    tdt = dev(x0).dtype
    cuts = [0, 217, 217, 480, N]                        # shard 1 is empty
    idx = ciao.IndexStream(6).rand_indices(N, 1500)
    idx[10:13] = idx[10]                                # table-row hazards inside the prefetch window, across the staging too

    def shard_table(table=None):
        t = L.ShardTable()
        t.nshards, t.owner = len(cuts) - 1, 1
        for k in range(len(cuts) - 1):
            t.row0[k] = cuts[k]
            t.A[k] = dp.A[cuts[k]:].data_ptr() if cuts[k] < N else None
            t.b[k] = dp.b[cuts[k]:].data_ptr() if cuts[k] < N else None
            t.table[k] = table[cuts[k]:].data_ptr() if (table is not None and cuts[k] < N) else None
        t.row0[len(cuts) - 1] = N
        return t

    outs = []
    for sharded in (False, True):
        av, z, zf, w = (torch.empty(d, dtype=tdt, device="cuda") for _ in range(4))
        ctx.svrg_init(dp, dev(x0), av, z, zf, w)
        table = torch.empty((N, d), dtype=tdt, device="cuda")
        sav, sz = torch.empty(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda")
        ctx.saga_init(dp, dg, 0.3, dev(x0), table, sav, sz)
        if sharded:
            ctx.set_shards(shard_table(table))
        try:
            ctx.svrg_inner(dp, dg, 0.4, idx, av, z, zf, w)
            k1 = ctx.last_kernel()
            ctx.saga_steps(dp, dg, 0.3, False, idx, table, sav, sz)
            k2 = ctx.last_kernel()
            ctx.synchronize()
        finally:
            ctx.set_shards(None)
        assert "chain_dma_kernel" in k1 and ("chain_ws_kernel" in k2 or "chain_dma_kernel" in k2)
        outs.append([t.cpu().numpy() for t in (w, z, sz, sav, table)])
    for u, v in zip(*outs):
        assert np.array_equal(u, v)
    rav, rz, rzf, rw = O_svrg_state(op, x0)
    from oracle import twin as O
    O.svrg_inner(op, og, dtype(0.4), idx, rav, rz, rzf, rw)
    close(outs[1][0], rw, dtype, scale=8, what="sharded svrg_inner w vs oracle", scale64=8)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
@pytest.mark.parametrize("d", [256, 1000, 2048, 4096])
def test_adaptive_finito_over_a_shard_table_is_bitwise_the_unsharded_chain(ctx, ciao, dtype, loss, d):
    """Finito_adaptive.jl:118-150 with the rows, the rows of the s-table and the per-sample scalars in several allocations (three
    uneven shards, one of them empty): the owner's chain finds each step's three addresses through the shard table.  Same arithmetic,
    same order: iterates, table rows, scalars and the backtracking counts bitwise those of the unsharded chain (itself held against
    the oracle in test_adaptive_finito_steps), hazards inside the look-ahead window and across a staging boundary included."""
    import torch
    import ciaoalgorithms_jl_amd._lib as L
    N = 300
    A, b, x0 = P.synthetic(loss, N, d, dtype, seed=43)
    op, dp = make(loss, A, b, float(N) if loss == "ls" else 1.0, dtype)
    og, dg = make_g("l1", dtype, d, lam=0.02)
    tdt = dev(x0).dtype
    cuts = [0, 117, 117, 230, N]
    idx = ciao.IndexStream(8).rand_indices(N, 1300)
    idx[5:8] = idx[5]
    idx[10] = idx[8]
    idx[510:514] = idx[509]                             # a hazard across the staging boundary (512 steps)
    outs = []
    for sharded in (False, True):
        table = torch.empty((N, d), dtype=tdt, device="cuda")
        meta = torch.empty((N, 4, 4), dtype=tdt, device="cuda")
        hg = torch.empty(1, dtype=tdt, device="cuda")
        av, z = torch.empty(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda")
        ctx.afinito_init(dp, dg, 0.999, dev(x0), table, meta, av, z, hg)
        ctx.synchronize()
        if sharded:   # the shards as allocations of their own: nothing may be reached through the problem's base pointers
            parts = [(dp.A[c0:c1].clone(), dp.b[c0:c1].clone(), table[c0:c1].clone(), meta[c0:c1].clone()) for c0, c1 in zip(cuts, cuts[1:])]
            table.fill_(float("nan")), meta.fill_(float("nan"))
            t = L.ShardTable()
            t.nshards, t.owner = len(cuts) - 1, 1
            for k, (pa, pb, pt, pm) in enumerate(parts):
                t.row0[k] = cuts[k]
                if pa.shape[0]:
                    t.A[k], t.b[k], t.table[k], t.meta[k] = pa.data_ptr(), pb.data_ptr(), pt.data_ptr(), pm.data_ptr()
            t.row0[len(cuts) - 1] = N
            ctx.set_shards(t)
        ctx.set_option("chain_four_waves", 1)   # the sharded chain runs on four waves whatever the row length: the same for its twin
        try:
            done, trials = ctx.afinito_steps(dp, dg, 0.999, 1e-9, idx, table, meta, av, z, hg)
            kern = ctx.last_kernel()
            ctx.synchronize()
        finally:
            ctx.set_shards(None)
            ctx.set_option("chain_four_waves", 0)
        assert "afinito_dma_kernel" in kern and ("sharded" in kern) == sharded and "block=256" in kern, kern
        if sharded:
            assert torch.isnan(table).all() and torch.isnan(meta).all(), "the chain wrote through the unsharded pointers"
            table = torch.cat([p_[2] for p_ in parts])
            meta = torch.cat([p_[3] for p_ in parts])
        outs.append([done, trials] + [t_.cpu().numpy() for t_ in (z, av, hg, table, meta)])
    assert outs[0][0] == outs[1][0] == len(idx) and outs[0][1] == outs[1][1]
    for u, v in zip(outs[0][2:], outs[1][2:]):
        assert np.array_equal(u, v)


def test_adaptive_finito_shard_table_refusals(ctx, ciao):
    """Rows that are not whole 16-byte chunks cannot take the LDS-DMA kernel: refused over a shard table, never silently unsharded;
    a shard with rows but no meta pointer on the owner is named."""
    import torch
    import ciaoalgorithms_jl_amd._lib as L
    for d, msg in ((1001, "whole 16-byte chunks"), (1024, "no meta pointer")):
        A, b, x0 = P.synthetic("ls", 40, d, np.float64)
        _, dp = make("ls", A, b, 40.0, np.float64)
        _, dg = make_g("zero", np.float64, d)
        table = torch.empty((40, d), dtype=torch.float64, device="cuda")
        meta = torch.empty((40, 4, 4), dtype=torch.float64, device="cuda")
        hg = torch.empty(1, dtype=torch.float64, device="cuda")
        av, z = torch.empty(d, dtype=torch.float64, device="cuda"), torch.empty(d, dtype=torch.float64, device="cuda")
        ctx.afinito_init(dp, dg, 0.999, dev(x0), table, meta, av, z, hg)
        t = L.ShardTable()
        t.nshards, t.owner = 1, 1
        t.row0[0], t.row0[1] = 0, 40
        t.A[0], t.b[0], t.table[0] = dp.A.data_ptr(), dp.b.data_ptr(), table.data_ptr()
        if d == 1001:
            t.meta[0] = meta.data_ptr()
        ctx.set_shards(t)
        try:
            with pytest.raises(ciao._lib.CiaoError, match=msg):
                ctx.afinito_steps(dp, dg, 0.999, 1e-9, np.zeros(3, np.int64), table, meta, av, z, hg)
        finally:
            ctx.set_shards(None)
    ctx.synchronize()


def O_svrg_state(op, x0):
    from oracle import twin as O
    return O.svrg_init(op, x0)


def test_shard_table_is_validated(ctx, ciao):
    import torch
    import ciaoalgorithms_jl_amd._lib as L
    A, b, x0 = P.synthetic("ls", 40, 1024, np.float64)
    _, dp = make("ls", A, b, 40.0, np.float64)
    _, dg = make_g("zero", np.float64, 1024)
    t = L.ShardTable()
    t.nshards, t.owner = 2, 1
    t.row0[0], t.row0[1], t.row0[2] = 0, 10, 39        # covers 39 rows, the problem has 40
    t.A[0], t.b[0], t.A[1], t.b[1] = dp.A.data_ptr(), dp.b.data_ptr(), dp.A[10:].data_ptr(), dp.b[10:].data_ptr()
    v = [torch.zeros(1024, dtype=torch.float64, device="cuda") for _ in range(4)]
    ctx.set_shards(t)
    try:
        with pytest.raises(ciao._lib.CiaoError, match="shard table covers"):
            ctx.svrg_inner(dp, dg, 0.1, np.zeros(3, np.int64), *v)
    finally:
        ctx.set_shards(None)
    bad = L.ShardTable()
    bad.nshards = 9
    with pytest.raises(ciao._lib.CiaoError):
        ctx.set_shards(bad)
    ctx.set_shards(None)
    # rows that are not whole 16-byte chunks cannot take the LDS-DMA kernel: refused, never silently unsharded
    A2, b2, _ = P.synthetic("ls", 40, 1001, np.float64)
    _, dp2 = make("ls", A2, b2, 40.0, np.float64)
    _, dg2 = make_g("zero", np.float64, 1001)
    t2 = L.ShardTable()
    t2.nshards, t2.owner = 1, 1
    t2.row0[0], t2.row0[1] = 0, 40
    t2.A[0], t2.b[0] = dp2.A.data_ptr(), dp2.b.data_ptr()
    v2 = [torch.zeros(1001, dtype=torch.float64, device="cuda") for _ in range(4)]
    ctx.set_shards(t2)
    try:
        with pytest.raises(ciao._lib.CiaoError, match="shard table needs rows"):
            ctx.svrg_inner(dp2, dg2, 0.1, np.zeros(3, np.int64), *v2)
    finally:
        ctx.set_shards(None)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d", [52, 128, 200, 256, 512])
def test_short_rows_run_the_chains_on_one_wave(ctx, ciao, dtype, d):
    """Rows of up to 2 KiB take the single-wave chain (block=64: no cross-wave exchange); option chain_four_waves keeps them on
    the four-wave kernel.  (Until round 5 fp64 rows of 2-4 KiB ran on one wave too, four chunks per lane: since then the four-wave
    step is the faster one, and fp64 SAGA rows of 2-4 KiB take the wave-specialised chain, 0.41 against 0.48 us per update.)
    Both against the oracle, SVRG and SAGA."""
    import torch
    from oracle import twin as O
    N = 40
    rowb = d * np.dtype(dtype).itemsize
    if rowb % 16:
        pytest.skip("not whole 16-byte chunks: register-ring kernel")
    A, b, x0 = P.synthetic("logistic", N, d, dtype, seed=d)
    op, dp = make("logistic", A, b, 1.0, dtype)
    og, dg = make_g("l1", dtype, d, lam=0.01)
    gamma = 1.0 / (7 * 0.25 * np.max(np.sum(A.astype(np.float64) ** 2, axis=1)))
    tdt = dev(x0).dtype
    idx = ciao.IndexStream(3).rand_indices(N, 3 * N)
    rav, rz, rzf, rw = O.svrg_init(op, x0)
    O.svrg_iterate(op, og, dtype(gamma), idx, False, rav, rz, rzf, rw)
    rt, rsav, rsz = O.saga_init(op, og, dtype(gamma), x0)
    O.saga_steps(op, og, dtype(gamma), False, idx, rt, rsav, rsz)
    for four in (0, 1):
        ctx.set_option("chain_four_waves", four)
        try:
            av, z, zf, w = (torch.empty(d, dtype=tdt, device="cuda") for _ in range(4))
            ctx.svrg_init(dp, dev(x0), av, z, zf, w)
            ctx.svrg_iterate(dp, dg, gamma, idx, False, av, z, zf, w)
            name = ctx.last_kernel() if "chain" in ctx.last_kernel() else ""
            table = torch.empty((N, d), dtype=tdt, device="cuda")
            sav, sz = torch.empty(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda")
            ctx.saga_init(dp, dg, gamma, dev(x0), table, sav, sz)
            ctx.saga_steps(dp, dg, gamma, False, idx, table, sav, sz)
            assert ("block=64" in ctx.last_kernel()) == (rowb <= 2048 and not four), ctx.last_kernel()
            if rowb > 2048 and rowb <= 4096:
                assert "chain_ws_kernel" in ctx.last_kernel(), ctx.last_kernel()
        finally:
            ctx.set_option("chain_four_waves", 0)
        close(zf, rzf, dtype, scale={64: 230, 32: 170}, what=f"short rows svrg z_full (four_waves={four})", scale64=250)
        close(sz, rsz, dtype, scale={64: 52, 32: 70}, what=f"short rows saga z (four_waves={four}; {ctx.last_kernel()})", scale64=410)
        close(table, rt, dtype, scale={64: 17, 32: 16}, what=f"short rows saga table (four_waves={four})", scale64=21)
    ctx.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# SAGA / SAG
# ----------------------------------------------------------------------------------------------------------------------
# rows of 2-4 KiB take chain_ws_kernel, the wave-specialised chain (consumer / stager / issuer waves, barrier-free exchange); rows
# of up to 2 KiB of an unsharded problem run on ONE wave instead and reach it with option chain_four_waves=1 (or over a shard
# table); option chain_no_ws=1 keeps everything on chain_dma_kernel, where rows beyond 4 KiB always run (round 4: the 8 KiB
# variants were slower -- fp64 3.5x, it spilled -- and are not built).  Same arithmetic, operation for operation.
WS_CASES = [(np.float64, 512), (np.float64, 400), (np.float64, 260), (np.float64, 1024), (np.float32, 1024), (np.float32, 2048),
            (np.float32, 1000), (np.float32, 516), (np.float32, 700)]


@pytest.mark.parametrize("dtype,d", WS_CASES)
@pytest.mark.parametrize("sag", [False, True])
@pytest.mark.parametrize("loss,gk", [("logistic", "l1"), ("ls", "box"), ("ls", "zero"), ("logistic", "boxvec")])
def test_wave_specialised_saga_is_bitwise_the_dma_chain(ctx, ciao, dtype, d, sag, loss, gk):
    """chain_ws_kernel against chain_dma_kernel (BITWISE: state, aggregate and every table row) and against the oracle, on
    (a) N = 9: nearly every step finds its table row among the last R+K+3 samples -- the stale re-read path, the deferred
    store flushed early; (b) N = 700 with runs of repeated samples; (c) chains of 1 ... 40 steps (shorter than a ring
    revolution, than the stager's block, ending mid-revolution) continued from one another; both issuer counts."""
    import torch
    from oracle import twin as O
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    for N, m in ((9, 400), (700, 1300)):
        A, b, x0 = P.synthetic(loss, N, d, dtype, seed=d + N)
        op, dp = make(loss, A, b, 1.0 if loss == "logistic" else float(N), dtype)
        og, dg = make_g(gk, dtype, d, lam=0.01)
        L2 = np.max(np.sum(A.astype(np.float64) ** 2, axis=1)) * (0.25 if loss == "logistic" else N)
        gamma = 1.0 / ((16 if sag else 3) * L2)
        idx = ciao.IndexStream(d).rand_indices(N, m)
        idx[20:24] = idx[20]
        idx[100:103] = idx[99]
        cuts = [0, 1, 2, 5, 6, 46, 47, 80, 81, 82, 83, 200, m]      # chains of 1, 1, 3, 1, 40, 1, 33, 1, 1, 1, 117, ... steps
        rt, rav, rz = O.saga_init(op, og, dtype(gamma), x0)
        O.saga_steps(op, og, dtype(gamma), sag, idx, rt, rav, rz)
        outs = {}
        rowb = d * np.dtype(dtype).itemsize
        four = dtype == np.float64 and rowb <= 4096          # (rows of up to 2 KiB: off the one-wave kernel, for all three routes)
        takes_ws = rowb <= 4096 and (four or rowb > 2048)
        for name, opts in (("dma", {"chain_no_ws": 1}), ("ws2", {"chain_ws_issuers": 2}), ("ws1", {"chain_ws_issuers": 1})):
            for k, v in opts.items():
                ctx.set_option(k, v)
            ctx.set_option("chain_four_waves", 1 if four else 0)
            try:
                table = torch.empty((N, d), dtype=tdt, device="cuda")
                av, z = torch.empty(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda")
                ctx.saga_init(dp, dg, gamma, dev(x0), table, av, z)
                for lo, hi in zip(cuts[:-1], cuts[1:]):
                    ctx.saga_steps(dp, dg, gamma, sag, idx[lo:hi], table, av, z)
                kern = ctx.last_kernel()
                ctx.synchronize()
            finally:
                ctx.set_option("chain_no_ws", 0)
                ctx.set_option("chain_ws_issuers", 0)
                ctx.set_option("chain_four_waves", 0)
            assert ("chain_ws_kernel" in kern) == (name != "dma" and takes_ws), kern
            if name != "dma" and takes_ws:
                assert f"issuers{name[-1]}" in kern, kern
            outs[name] = [t.cpu().numpy() for t in (z, av, table)]
        for name in ("ws2", "ws1"):
            for u, v, what in zip(outs["dma"], outs[name], ("z", "av", "table")):
                assert np.array_equal(u, v), f"{name} differs from the DMA chain in {what} (N={N}, d={d})"
        close(outs["ws2"][0], rz, dtype, scale={64: 530, 32: 260}, what=f"ws saga z N={N}", scale64=750)
        if loss == "logistic":   # (an interpolating least-squares problem drives its gradients -- the table -- to rounding level)
            close(outs["ws2"][2], rt, dtype, scale={64: 75, 32: 87}, what=f"ws saga table N={N}", scale64=100)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("sag", [False, True])
@pytest.mark.parametrize("shape", CHAIN_SHAPES)
def test_saga_steps(ctx, ciao, chain_variant, dtype, sag, shape):
    """Table init + 4N steps.  Small N makes repeated indices inside the prefetch window the common case, which is
    exactly the read-after-write hazard of the table-row prefetch."""
    import torch
    from oracle import twin as O
    N, d = shape
    loss = "ls" if (N + d) % 2 else "logistic"
    A, b, x0 = P.synthetic(loss, N, d, dtype, seed=9)
    lam_f = float(N) if loss == "ls" else 1.0
    op, dp = make(loss, A, b, lam_f, dtype)
    og, dg = make_g("l1", dtype, d, lam=0.02)
    Lmax = (lam_f if loss == "ls" else 0.25) * np.max(np.sum(A.astype(np.float64) ** 2, axis=1))
    gamma = 1.0 / ((16 if sag else 3) * Lmax)
    tdt = dev(x0).dtype
    table = torch.empty((N, d), dtype=tdt, device="cuda")
    av, z = torch.empty(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda")
    ctx.saga_init(dp, dg, gamma, dev(x0), table, av, z)
    rt, rav, rz = O.saga_init(op, og, dtype(gamma), x0)
    close(table, rt, dtype, scale={64: 28, 32: 32}, what="saga_init table", scale64=9.3)
    close(av, rav, dtype, scale={64: 29, 32: 28}, what="saga_init av", scale64=13)
    close(z, rz, dtype, scale=8, what="saga_init z  (= prox((1-gamma) x0))", scale64=11)
    st = ciao.IndexStream(21)
    for chunk in (1, 2, 4 * N, 7):
        idx = st.rand_indices(N, chunk)
        if chunk == 7:
            idx[:] = idx[0]   # the same row seven times in a row
        ctx.saga_steps(dp, dg, gamma, sag, idx, table, av, z)
        O.saga_steps(op, og, dtype(gamma), sag, idx, rt, rav, rz)
        close(z, rz, dtype, scale={64: 130, 32: 100}, what=f"saga z after chunk {chunk} ({ctx.last_kernel()})", scale64=840)
        close(av, rav, dtype, scale={64: 130, 32: 140}, what=f"saga av after chunk {chunk}", scale64=110)
        close(table, rt, dtype, scale={64: 220, 32: 200}, what=f"saga table after chunk {chunk}", scale64=110)
    # invariant av == (1/N) sum_i s_i  
    close(av, table.double().mean(dim=0).cpu().numpy(), dtype, scale={64: 74, 32: 110}, what="av invariant")
    ctx.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# Finito / LFinito
# ----------------------------------------------------------------------------------------------------------------------
def _batches(stream, N, r, nit, mode):
    out = []
    for t in range(nit):
        if mode == "random":
            out.append(stream.sample_without_replacement(N, r))
        else:
            nb = -(-N // r)
            j = (t + 1) % nb
            out.append(np.arange(r * j, min(r * j + r, N), dtype=np.int64))
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape,r", [((6, 3), 1), ((8, 5), 2), ((8, 5), 3), ((50, 50), 7), ((40, 256), 1), ((64, 1024), 16),
                                     ((300, 64), 100), ((20, 1500), 4), ((10, 4096), 3), ((33, 2048), 1), ((1500, 1024), 700),
                                     ((60, 1001), 7), ((400, 259), 300)])
@pytest.mark.parametrize("path", ["chain", "block_per_row", "wave_per_row"])
def test_finito_steps(ctx, ciao, chain_variant, dtype, shape, r, path):
    """The three routes of a batch: the sequential chain kernel; batch-parallel with one workgroup per row (whole-4-KiB rows
    only, otherwise it falls through to the next); batch-parallel with one wave per row."""
    import torch
    from oracle import twin as O
    N, d = shape
    loss = "logistic" if (N + d) % 2 else "ls"
    A, b, x0 = P.synthetic(loss, N, d, dtype, seed=4)
    lam_f = float(N) if loss == "ls" else 1.0
    op, dp = make(loss, A, b, lam_f, dtype)
    og, dg = make_g("l1", dtype, d, lam=0.02)
    Li = (lam_f if loss == "ls" else 0.25) * np.sum(A.astype(np.float64) ** 2, axis=1)
    gam = (0.999 * N / Li).astype(dtype)
    tdt = dev(x0).dtype
    table = torch.empty((N, d), dtype=tdt, device="cuda")
    av, z = torch.empty(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda")
    dgam = dev(gam)
    hg = ctx.hat_gamma(dgam)
    rt, rav, rz, rhg = O.finito_init(op, og, gam, x0)
    assert abs(hg - float(rhg)) <= (1e-12 if dtype == np.float64 else 1e-5) * abs(float(rhg))
    ctx.finito_init(dp, dg, dgam, hg, dev(x0), table, av, z)
    close(table, rt, dtype, scale={64: 9.4, 32: 11}, what="finito_init table", scale64=12)
    close(av, rav, dtype, scale={64: 67, 32: 41}, what="finito_init av", scale64=12)
    close(z, rz, dtype, scale={64: 67, 32: 45}, what="finito_init z", scale64=13)
    ctx.set_option("chain_max_batch", 64 if path == "chain" else 0)
    ctx.set_option("split_max_rows", 0 if path == "wave_per_row" else -1)
    try:
        st = ciao.IndexStream(33)
        for mode, nit in (("random", 5), ("cyclic", 2 * (-(-N // r)) + 1)):
            batches = _batches(st, N, r, nit, mode)
            bptr = np.zeros(nit + 1, np.int64)
            np.cumsum([len(x) for x in batches], out=bptr[1:])
            ctx.finito_steps(dp, dg, dgam, hg, bptr, np.concatenate(batches), table, av, z)
            O.finito_steps(op, og, gam, rhg, batches, rt, rav, rz)
            close(z, rz, dtype, scale={64: 1300, 32: 14000}, what=f"finito z {mode} ({ctx.last_kernel()})", scale64=270)
            close(av, rav, dtype, scale={64: 1300, 32: 14000}, what=f"finito av {mode}", scale64=240)
            close(table, rt, dtype, scale={64: 1100, 32: 12000}, what=f"finito table {mode}", scale64=200)
    finally:
        ctx.set_option("chain_max_batch", -1)
        ctx.set_option("split_max_rows", -1)
    # invariant av == hat_gamma * sum_i s_i / gamma_i   (row F3)
    inv = (table.double() / dgam.double()[:, None]).sum(dim=0).cpu().numpy() * hg
    close(av, inv, dtype, scale={64: 60, 32: 57}, what="finito av invariant")
    ctx.synchronize()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d", [3, 5, 50, 100, 255])
@pytest.mark.parametrize("pad", [0, 3])
def test_small_rows_in_all_five_modes(ctx, ciao, dtype, d, pad):
    """Rows of tabular size (d = 3 ... 255, the shape of the reference's own problems: test/test_lasso.jl:15,
    test/test_logistic_l1.jl:12-26) in all five modes of the batch-parallel kernels, dense and padded row stride, N = 6000 (dozens
    of row groups per wave, several workgroups): the full gradient, SAGA init and Finito init on rows_small_kernel (dense rows of
    17 ... : rows_smallm_kernel), Finito batches over index lists on rows_wrow_kernel (round 5: one wave per row -- the reference's
    default sweeping = 1 draws lists) and over row blocks on rows_smallm_kernel where its tiles fit, else rows_wrow_kernel too, LFinito's
    batch sweep (index lists AND row blocks) on rows_smallb_kernel / rows_smallm_kernel -- each against the oracle, the two batch forms
    of the same batches bitwise equal where they run the same kernel; the lists again on rows_smallb_kernel (option small_wrow=0)."""
    import torch
    from oracle import twin as O
    N, r = 6000, 700
    loss = "logistic" if d % 2 else "ls"
    A, b, x0 = P.synthetic(loss, N, d, dtype, seed=d)
    lam_f = float(N) if loss == "ls" else 1.0
    op, dp = make(loss, A, b, lam_f, dtype, pad=pad)
    og, dg = make_g("l1", dtype, d, lam=0.02)
    Li = (lam_f if loss == "ls" else 0.25) * np.sum(A.astype(np.float64) ** 2, axis=1)
    gam = (0.999 * N / np.maximum(Li, 1e-3 * Li.max())).astype(dtype)
    tdt = dev(x0).dtype
    dgam = dev(gam)
    hg = ctx.hat_gamma(dgam)
    ctx.set_option("chain_max_batch", 0)
    es = np.dtype(dtype).itemsize
    mfma = d >= 17 and pad == 0 and 2 * 16 * d * es * 4 + 12000 <= 150 * 1024        # two tile buffers per wave fit LDS: the matrix-core kernel
    mfma_tab = d >= 17 and pad == 0 and 3 * 16 * d * es * 4 + 12000 <= 150 * 1024    # ... three (Finito batches: the table tile comes in too)
    try:
        # ---- modes 0, 2, 3: full gradient, SAGA init, Finito init
        av = torch.empty(d, dtype=tdt, device="cuda")
        ctx.full_gradient(dp, dev(x0), av)
        # (dense rows of 17 .. 256 elements -- fp64: .. 144: the sweep runs on the matrix cores, tests/test_gpu_small_mfma.py)
        assert ("rows_smallm_kernel" if mfma else "rows_small_kernel") in ctx.last_kernel(), ctx.last_kernel()
        close(av, O.full_pass(op, x0), dtype, scale={64: 180, 32: 200}, what=f"small rows full gradient d={d}", scale64=8)
        table = torch.empty((N, d), dtype=tdt, device="cuda")
        sav, sz = torch.empty(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda")
        ctx.saga_init(dp, dg, 0.1 / max(Li.max(), 1.0), dev(x0), table, sav, sz)
        assert ("rows_smallm_kernel" if mfma else "rows_small_kernel") in ctx.last_kernel() or "prox" in ctx.last_kernel(), ctx.last_kernel()
        rt, rav, rz = O.saga_init(op, og, dtype(0.1 / max(Li.max(), 1.0)), x0)
        close(table, rt, dtype, scale={64: 16, 32: 19}, what="small rows saga_init table", scale64=9.4)
        close(sav, rav, dtype, scale={64: 22, 32: 23}, what="small rows saga_init av", scale64=8)
        z = torch.empty(d, dtype=tdt, device="cuda")
        rt, rav, rz, rhg = O.finito_init(op, og, gam, x0)
        ctx.finito_init(dp, dg, dgam, hg, dev(x0), table, av, z)
        assert ("rows_smallm_kernel" if mfma else "rows_small_kernel") in ctx.last_kernel(), ctx.last_kernel()
        close(table, rt, dtype, scale={64: 13, 32: 16}, what="small rows finito_init table", scale64=11)
        close(av, rav, dtype, scale={64: 41, 32: 25}, what="small rows finito_init av", scale64=8.5)
        # ---- mode 4: Finito batches -- random index lists, then static blocks given BOTH as index lists and as row blocks
        st = ciao.IndexStream(d)
        rnd = [st.sample_without_replacement(N, r) for _ in range(4)]
        bptr = np.arange(len(rnd) + 1, dtype=np.int64) * r
        # (the last two lists: the rows of the one before in another order -- every row met again one batch later -- and a short list)
        rnd.append(rnd[-1][np.argsort(-rnd[-1] % 97, kind="stable")])
        rnd.append(st.sample_without_replacement(N, 37))
        bptr = np.zeros(len(rnd) + 1, np.int64)
        np.cumsum([len(x) for x in rnd], out=bptr[1:])
        t3, av3, z3 = table.clone(), av.clone(), z.clone()
        ctx.finito_steps(dp, dg, dgam, hg, bptr, np.concatenate(rnd), table, av, z)
        assert "rows_wrow_kernel" in ctx.last_kernel() and "mode4" in ctx.last_kernel(), ctx.last_kernel()
        assert ("chunks" in ctx.last_kernel()) == (pad == 0 and (d * es) % 16 == 0), ctx.last_kernel()   # 16 bytes per lane where rows allow
        O.finito_steps(op, og, gam, rhg, rnd, rt, rav, rz)
        close(z, rz, dtype, scale={64: 200, 32: 1300}, what=f"small rows finito z, index lists ({ctx.last_kernel()})", scale64=21)
        close(table, rt, dtype, scale={64: 130, 32: 800}, what="small rows finito table, index lists", scale64=14)
        ctx.set_option("small_wrow", 0)   # ... and the same lists on the several-rows-per-wave kernel: another order of summation
        try:
            ctx.finito_steps(dp, dg, dgam, hg, bptr, np.concatenate(rnd), t3, av3, z3)
            assert "rows_smallb_kernel" in ctx.last_kernel() and "mode4" in ctx.last_kernel(), ctx.last_kernel()
        finally:
            ctx.set_option("small_wrow", -1)
        close(z3, rz, dtype, scale={64: 200, 32: 1300}, what="small rows finito z, index lists on rows_smallb_kernel", scale64=21)
        close(t3, rt, dtype, scale={64: 130, 32: 800}, what="small rows finito table, index lists on rows_smallb_kernel", scale64=14)
        nb = -(-N // r)
        order = [(t + 1) % nb for t in range(nb + 2)]                     # cyclic: the first step uses batch 2 (Finito_basic.jl:99)
        static = [np.arange(r * j, min(r * j + r, N), dtype=np.int64) for j in order]   # the last block is short (6000 = 8 * 700 + 400)
        t2, av2, z2 = table.clone(), av.clone(), z.clone()
        bp = np.zeros(len(static) + 1, np.int64)
        np.cumsum([len(x) for x in static], out=bp[1:])
        ctx.finito_steps(dp, dg, dgam, hg, bp, np.concatenate(static), table, av, z)
        on_tiles = mfma_tab and (r * d * np.dtype(dtype).itemsize) % 16 == 0
        if on_tiles:   # (blocks of up to 8192 rows take the one-wave-per-row kernel by default since round 5: the tiles by option)
            ctx.set_option("small_wrow", 0)
        try:
            ctx.finito_steps_blocks(dp, dg, dgam, hg, np.array([x[0] for x in static]), np.array([len(x) for x in static]), t2, av2, z2)
        finally:
            ctx.set_option("small_wrow", -1)
        O.finito_steps(op, og, gam, rhg, static, rt, rav, rz)
        if on_tiles:
            # dense row blocks of such rows: the batch on the matrix-core kernel (row tile and table tile by LDS-DMA) -- another order
            # of summation than the index-list form: each against the oracle
            assert "rows_smallm_kernel" in ctx.last_kernel() and "mode4" in ctx.last_kernel(), ctx.last_kernel()
            close(z2, rz, dtype, scale={64: 680, 32: 3900}, what=f"small rows finito z, row blocks on the matrix-core kernel ({ctx.last_kernel()})", scale64=45)
            close(t2, rt, dtype, scale={64: 420, 32: 2200}, what="small rows finito table, row blocks on the matrix-core kernel", scale64=29)
        else:
            # the list IS a block and both forms run the one-wave-per-row kernel (row q on the same wave either way): BITWISE
            assert "rows_wrow_kernel" in ctx.last_kernel(), ctx.last_kernel()
            assert torch.equal(z, z2) and torch.equal(av, av2) and torch.equal(table, t2), "row blocks and the same batches as index lists differ"
        close(z, rz, dtype, scale={64: 1100, 32: 6900}, what="small rows finito z, row blocks", scale64=180)
        close(table, rt, dtype, scale={64: 520, 32: 2200}, what="small rows finito table, row blocks", scale64=34)
        inv = (table.double() / dgam.double()[:, None]).sum(dim=0).cpu().numpy() * hg
        close(av, inv, dtype, scale={64: 30, 32: 27}, what="small rows finito av invariant")
        # ---- mode 1: LFinito iterations (full pass + the batch sweep with two dot products per row), lists and blocks
        lav, lz, lzf = (torch.empty(d, dtype=tdt, device="cuda") for _ in range(3))
        rav, rz, rzf, rhg = O.lfinito_init(op, gam, x0)
        ctx.lfinito_init(dp, hg, dev(x0), lav, lz, lzf)
        blocks = [np.arange(r * j, min(r * j + r, N), dtype=np.int64) for j in range(nb)]
        bp = np.zeros(nb + 1, np.int64)
        np.cumsum([len(x) for x in blocks], out=bp[1:])
        lav2, lz2, lzf2 = lav.clone(), lz.clone(), lzf.clone()
        for it in range(2):
            ctx.lfinito_iterate(dp, dg, dgam, hg, bp, np.concatenate(blocks), lav, lz, lzf)
            assert "rows_wrow_kernel" in ctx.last_kernel() and "mode1" in ctx.last_kernel(), ctx.last_kernel()   # (round 5: one wave per row)
            lf_tiles = mfma and (r * d * np.dtype(dtype).itemsize) % 16 == 0
            if lf_tiles:   # (row blocks of up to 8192 rows take the one-wave-per-row kernel by default since round 5: the tiles by option)
                ctx.set_option("small_wrow", 0)
            try:
                ctx.lfinito_iterate_blocks(dp, dg, dgam, hg, np.array([x[0] for x in blocks]), np.array([len(x) for x in blocks]), lav2, lz2, lzf2)
            finally:
                ctx.set_option("small_wrow", -1)
            O.lfinito_iterate(op, og, gam, rhg, blocks, rav, rz, rzf)
            if lf_tiles:
                # dense row blocks of such rows run the batch sweep on the matrix cores (both dots from one MFMA pass): another order of
                # summation than the index-list form, so equal to rounding; each is held against the oracle below
                assert "rows_smallm_kernel" in ctx.last_kernel() and "mode1" in ctx.last_kernel(), ctx.last_kernel()
                close(lz2, rz, dtype, scale={64: 930, 32: 2100}, what=f"small rows lfinito z it {it}, row blocks ({ctx.last_kernel()})", scale64=79)
                close(lav2, rav, dtype, scale={64: 940, 32: 1800}, what=f"small rows lfinito av it {it}, row blocks", scale64=89)
                lz2.copy_(lz), lav2.copy_(lav), lzf2.copy_(lzf)       # (so that the two forms start the next iteration from the same state)
            else:
                assert torch.equal(lz, lz2) and torch.equal(lav, lav2) and torch.equal(lzf, lzf2)
            close(lz, rz, dtype, scale={64: 2400, 32: 2100}, what=f"small rows lfinito z it {it} ({ctx.last_kernel()})", scale64=79)
            close(lav, rav, dtype, scale={64: 2100, 32: 1800}, what=f"small rows lfinito av it {it}", scale64=89)
    finally:
        ctx.set_option("chain_max_batch", -1)
    ctx.synchronize()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape,r", [((6, 3), 1), ((8, 5), 2), ((8, 5), 3), ((50, 50), 7), ((64, 1024), 16), ((300, 64), 100),
                                     ((20, 1500), 1), ((17, 2048), 2), ((1300, 1024), 600), ((50, 1001), 6)])
@pytest.mark.parametrize("path", ["chain", "block_per_row", "wave_per_row"])
def test_lfinito_iterations(ctx, ciao, chain_variant, dtype, shape, r, path):
    import torch
    from oracle import twin as O
    N, d = shape
    loss = "logistic" if (N + d) % 2 else "ls"
    A, b, x0 = P.synthetic(loss, N, d, dtype, seed=6)
    lam_f = float(N) if loss == "ls" else 1.0
    op, dp = make(loss, A, b, lam_f, dtype)
    og, dg = make_g("l1", dtype, d, lam=0.02)
    Li = (lam_f if loss == "ls" else 0.25) * np.sum(A.astype(np.float64) ** 2, axis=1)
    gam = (0.999 * N / Li).astype(dtype)
    tdt = dev(x0).dtype
    av, z, zf = (torch.empty(d, dtype=tdt, device="cuda") for _ in range(3))
    dgam = dev(gam)
    hg = ctx.hat_gamma(dgam)
    rav, rz, rzf, rhg = O.lfinito_init(op, gam, x0)
    ctx.lfinito_init(dp, hg, dev(x0), av, z, zf)
    close(av, rav, dtype, scale=130, what="lfinito_init av", scale64=8)
    assert torch.equal(z, av) and torch.equal(zf, av)
    nb = -(-N // r)
    static = [np.arange(r * j, min(r * j + r, N), dtype=np.int64) for j in range(nb)]
    ctx.set_option("chain_max_batch", 64 if path == "chain" else 0)
    ctx.set_option("split_max_rows", 0 if path == "wave_per_row" else -1)
    try:
        st = ciao.IndexStream(8)
        for it in range(3):
            order = np.arange(nb) if it == 0 else st.randperm(nb)
            batches = [static[j] for j in order]
            bptr = np.zeros(nb + 1, np.int64)
            np.cumsum([len(x) for x in batches], out=bptr[1:])
            ctx.lfinito_iterate(dp, dg, dgam, hg, bptr, np.concatenate(batches), av, z, zf)
            O.lfinito_iterate(op, og, gam, rhg, batches, rav, rz, rzf)
            close(zf, rzf, dtype, scale={64: 560, 32: 4700}, what=f"lfinito z_full it {it}", scale64=160)
            close(z, rz, dtype, scale={64: 560, 32: 5700}, what=f"lfinito z it {it} ({ctx.last_kernel()})", scale64=180)
            close(av, rav, dtype, scale={64: 640, 32: 7200}, what=f"lfinito av it {it}", scale64=170)
    finally:
        ctx.set_option("chain_max_batch", -1)
        ctx.set_option("split_max_rows", -1)
    ctx.synchronize()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("r", [3, 100, 1500])
def test_row_block_batches_equal_index_list_batches(ctx, ciao, dtype, r):
    """The *_blocks entry points (static batches of sweeping 2/3 as contiguous row blocks, no index array) run the same
    kernels on the same rows as the index-list entry points fed arange(first, first+len): bitwise the same state, for the
    chain route (r = 3), the workgroup-per-row route (r = 100) and the wave-per-row route (r = 1500); Finito, LFinito, ProShI."""
    import torch
    N, d = 4000, 1024
    A, b, x0 = P.synthetic("ls", N, d, dtype, seed=31)
    _, dp = make("ls", A, b, float(N), dtype)
    _, dg = make_g("l1", dtype, d, lam=0.01)
    tdt = dev(x0).dtype
    gam = torch.full((N,), 0.9 * N / (1.4 * N), dtype=tdt, device="cuda")
    hg = ctx.hat_gamma(gam)
    nbat = (N + r - 1) // r
    order = np.random.default_rng(2).permutation(nbat)[:min(nbat, 40)]        # shuffled static batches incl. the short last one
    first = (order * r).astype(np.int64)
    length = np.minimum(first + r, N) - first
    bptr = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    bidx = np.concatenate([np.arange(f, f + l) for f, l in zip(first, length)]).astype(np.int64)
    outs = []
    for blocks in (False, True):
        table = torch.empty((N, d), dtype=tdt, device="cuda")
        av, z, zf = (torch.empty(d, dtype=tdt, device="cuda") for _ in range(3))
        ctx.finito_init(dp, dg, gam, hg, dev(x0), table, av, z)
        if blocks:
            ctx.finito_steps_blocks(dp, dg, gam, hg, first, length, table, av, z)
        else:
            ctx.finito_steps(dp, dg, gam, hg, bptr, bidx, table, av, z)
        res = [table.cpu().numpy(), av.cpu().numpy(), z.cpu().numpy()]
        ctx.lfinito_init(dp, hg, dev(x0), av, z, zf)
        if blocks:
            ctx.lfinito_iterate_blocks(dp, dg, gam, hg, first, length, av, z, zf)
        else:
            ctx.lfinito_iterate(dp, dg, gam, hg, bptr, bidx, av, z, zf)
        res += [av.cpu().numpy(), z.cpu().numpy(), zf.cpu().numpy()]
        outs.append(res)
    for u, v in zip(*outs):
        assert np.array_equal(u, v)
    # ProShI
    from ciaoalgorithms_jl_amd.device import PackedSepQuad, ProxG
    import ciaoalgorithms_jl_amd._lib as L
    rng = np.random.default_rng(4)
    Q = torch.from_numpy(np.abs(rng.standard_normal((N, d))).astype(dtype)).cuda()
    q = torch.from_numpy(rng.standard_normal((N, d)).astype(dtype)).cuda()
    f = PackedSepQuad(Q, q, eta=3.0, lo=-2.0, hi=2.0)
    gbox = ProxG(L.PROX_BOX, lo=-float("inf"), hi=1.0)
    pg = torch.full((N,), 0.5, dtype=tdt, device="cuda")
    outs = []
    for blocks in (False, True):
        table = torch.empty((N, d), dtype=tdt, device="cuda")
        av, z = (torch.empty(d, dtype=tdt, device="cuda") for _ in range(2))
        hgd = torch.empty(1, dtype=tdt, device="cuda")
        ctx.proshi_init(f, gbox, pg, dev(x0), table, av, z, hgd)
        if blocks:
            ctx.proshi_steps_blocks(f, gbox, pg, float(hgd.item()), first, length, table, av, z)
        else:
            ctx.proshi_steps(f, gbox, pg, float(hgd.item()), bptr, bidx, table, av, z)
        outs.append([table.cpu().numpy(), av.cpu().numpy(), z.cpu().numpy()])
    for u, v in zip(*outs):
        assert np.array_equal(u, v)
    ctx.synchronize()


def test_row_blocks_are_validated_on_the_host(ctx, ciao):
    import torch
    A, b, x0 = P.synthetic("ls", 50, 64, np.float64)
    _, dp = make("ls", A, b, 50.0, np.float64)
    _, dg = make_g("zero", np.float64, 64)
    gam = torch.full((50,), 0.5, dtype=torch.float64, device="cuda")
    table = torch.zeros((50, 64), dtype=torch.float64, device="cuda")
    av, z = torch.zeros(64, dtype=torch.float64, device="cuda"), torch.zeros(64, dtype=torch.float64, device="cuda")
    for first, length in (([45], [6]), ([-1], [2]), ([0], [0])):
        with pytest.raises(ciao._lib.CiaoError):
            ctx.finito_steps_blocks(dp, dg, gam, 0.01, first, length, table, av, z)


@pytest.mark.parametrize("dtype,d", [(np.float64, 16384), (np.float64, 10001), (np.float32, 40000), (np.float32, 20001)])
def test_rows_longer_than_lds(ctx, ciao, dtype, d):
    """Rows beyond what one iterate plus one accumulator fit in LDS (72 KiB: d > 9216 fp64, > 18432 fp32) used to be outside
    every rows kernel.  rows_generic_kernel<..., global_acc> keeps the iterate in global memory and one partial per WAVE in
    the workspace: sweep, SAGA / Finito init, a Finito batch and an LFinito iteration against the oracle."""
    import torch
    from oracle import twin as O
    N = 24
    A, b, x0 = P.synthetic("ls", N, d, dtype, seed=d)
    op, dp = make("ls", A, b, float(N), dtype)
    og, dg = make_g("l1", dtype, d, lam=0.01)
    tdt = dev(x0).dtype
    av, z, zf = (torch.empty(d, dtype=tdt, device="cuda") for _ in range(3))
    ctx.full_gradient(dp, dev(x0), av)
    assert "global_acc" in ctx.last_kernel() or "rows_split" in ctx.last_kernel() or "rows_long" in ctx.last_kernel()
    close(av, O.full_pass(op, x0), dtype, scale={64: 110, 32: 160}, what=f"sweep d={d} ({ctx.last_kernel()})", scale64=23)
    table = torch.empty((N, d), dtype=tdt, device="cuda")
    ctx.saga_init(dp, dg, 0.1, dev(x0), table, av, z)
    rt, rav, rz = O.saga_init(op, og, dtype(0.1), x0)
    close(table, rt, dtype, scale={64: 130, 32: 170}, what="saga_init table (long rows)", scale64=17)
    close(av, rav, dtype, scale={64: 110, 32: 160}, what="saga_init av (long rows)", scale64=25)
    gam = torch.full((N,), 0.4, dtype=tdt, device="cuda")
    hg = ctx.hat_gamma(gam)
    ctx.finito_init(dp, dg, gam, hg, dev(x0), table, av, z)
    rt, rav, rz, rhg = O.finito_init(op, og, gam.cpu().numpy(), x0)
    close(av, rav, dtype, scale={64: 18, 32: 19}, what="finito_init av (long rows)", scale64=13)
    batch = np.arange(3, 20, dtype=np.int64)
    ctx.set_option("chain_max_batch", 0)
    try:
        ctx.finito_steps(dp, dg, gam, hg, np.array([0, batch.size], np.int64), batch, table, av, z)
        O.finito_steps(op, og, gam.cpu().numpy(), rhg, [batch], rt, rav, rz)
        close(z, rz, dtype, scale={64: 30, 32: 36}, what=f"finito batch z (long rows, {ctx.last_kernel()})", scale64=24)
        close(table, rt, dtype, scale={64: 18, 32: 19}, what="finito batch table (long rows)", scale64=16)
        ctx.lfinito_init(dp, hg, dev(x0), av, z, zf)
        ctx.lfinito_iterate(dp, dg, gam, hg, np.array([0, 12, N], np.int64), np.arange(N, dtype=np.int64), av, z, zf)
        rav, rz, rzf, rhg = O.lfinito_init(op, gam.cpu().numpy(), x0)
        O.lfinito_iterate(op, og, gam.cpu().numpy(), rhg, [np.arange(12), np.arange(12, N)], rav, rz, rzf)
        close(av, rav, dtype, scale={64: 90, 32: 99}, what="lfinito av (long rows)", scale64=30)
        close(z, rz, dtype, scale={64: 76, 32: 54}, what="lfinito z (long rows)", scale64=16)
    finally:
        ctx.set_option("chain_max_batch", -1)
    ctx.synchronize()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d,forced", [(300, True), (1024, True), (9000, False), (16384, False), (8193, False)])
def test_chains_on_rows_of_any_length(ctx, ciao, dtype, d, forced):
    """Beyond 8192 elements the per-thread register state of the chain kernels no longer fits: chain_big_kernel keeps the
    iterate state in the caller's vectors (VERDICT r1 "missing" item 5: these shapes used to return CIAO_ERR_UNSUPPORTED).
    SVRG inner cycle, SAGA / SAG steps, Finito batches of 2 and the LFinito sweep against the oracle; at small d the kernel is
    forced (option chain_big) and must agree with the register kernels' answers to the same tolerance."""
    import torch
    from oracle import twin as O
    N = 40
    A, b, x0 = P.synthetic("logistic" if d % 2 else "ls", N, d, dtype, seed=d)
    loss = "logistic" if d % 2 else "ls"
    op, dp = make(loss, A, b, 1.0 if loss == "logistic" else float(N), dtype)
    og, dg = make_g("l1", dtype, d, lam=0.01)
    tdt = dev(x0).dtype
    gamma = 0.3 if loss == "logistic" else 1.0 / (7 * N * float(np.max(np.sum(A.astype(np.float64) ** 2, axis=1))))
    idx = ciao.IndexStream(d).rand_indices(N, 150)
    idx[4:7] = idx[4]
    ctx.set_option("chain_big", 1 if forced else 0)
    try:
        av, z, zf, w = (torch.empty(d, dtype=tdt, device="cuda") for _ in range(4))
        ctx.svrg_init(dp, dev(x0), av, z, zf, w)
        ctx.svrg_inner(dp, dg, gamma, idx, av, z, zf, w)
        # (SVRG and SAGA beyond 8192 elements: several workgroups share the chain, tests/test_gpu_wide_chain.py; forced: the one-workgroup kernel)
        assert ("chain_big_kernel" if forced else "chain_wide_kernel") in ctx.last_kernel(), ctx.last_kernel()
        rav, rz, rzf, rw = O.svrg_init(op, x0)
        O.svrg_inner(op, og, dtype(gamma), idx, rav, rz, rzf, rw)
        close(w, rw, dtype, scale={64: 28, 32: 23}, what="svrg_inner w (any-d chain)", scale64=460)
        close(z, rz, dtype, scale={64: 20, 32: 23}, what="svrg_inner z (any-d chain)", scale64=270)
        for sag in (False, True):
            table = torch.empty((N, d), dtype=tdt, device="cuda")
            sav, sz = torch.empty(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda")
            ctx.saga_init(dp, dg, gamma, dev(x0), table, sav, sz)
            ctx.saga_steps(dp, dg, gamma, sag, idx, table, sav, sz)
            assert ("chain_big_kernel" if forced else "chain_wide_kernel") in ctx.last_kernel(), ctx.last_kernel()
            rt, rsav, rsz = O.saga_init(op, og, dtype(gamma), x0)
            O.saga_steps(op, og, dtype(gamma), sag, idx, rt, rsav, rsz)
            close(sz, rsz, dtype, scale={64: 26, 32: 24}, what=f"saga z sag={sag} (any-d chain)", scale64=500)
            close(table, rt, dtype, scale={64: 180, 32: 120}, what="saga table (any-d chain)", scale64=210)
        gam = torch.full((N,), 0.4, dtype=tdt, device="cuda")
        hg = ctx.hat_gamma(gam)
        table = torch.empty((N, d), dtype=tdt, device="cuda")
        ctx.finito_init(dp, dg, gam, hg, dev(x0), table, av, z)
        batches = [np.array([2 * k, 2 * k + 1], dtype=np.int64) for k in range(N // 2)]
        ctx.finito_steps(dp, dg, gam, hg, np.arange(0, N + 1, 2, dtype=np.int64), np.concatenate(batches), table, av, z)
        assert ("chain_big_kernel" if forced else "chain_wide_kernel") in ctx.last_kernel(), ctx.last_kernel()
        rt, rav, rz, rhg = O.finito_init(op, og, gam.cpu().numpy(), x0)
        O.finito_steps(op, og, gam.cpu().numpy(), rhg, batches, rt, rav, rz)
        close(z, rz, dtype, scale={64: 90, 32: 100}, what="finito z (any-d chain)", scale64=73)
        close(table, rt, dtype, scale={64: 86, 32: 100}, what="finito table (any-d chain)", scale64=73)
        ctx.lfinito_init(dp, hg, dev(x0), av, z, zf)
        ctx.lfinito_iterate(dp, dg, gam, hg, np.arange(0, N + 1, 2, dtype=np.int64), np.concatenate(batches), av, z, zf)
        rav, rz, rzf, rhg = O.lfinito_init(op, gam.cpu().numpy(), x0)
        O.lfinito_iterate(op, og, gam.cpu().numpy(), rhg, batches, rav, rz, rzf)
        close(z, rz, dtype, scale={64: 120, 32: 160}, what="lfinito z (any-d chain)", scale64=130)
        close(av, rav, dtype, scale={64: 120, 32: 160}, what="lfinito av (any-d chain)", scale64=130)
        ctx.synchronize()
    finally:
        ctx.set_option("chain_big", 0)


# ----------------------------------------------------------------------------------------------------------------------
# adaptive Finito
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(6, 3), (8, 5), (50, 50), (40, 256), (30, 300), (24, 1024), (10, 4096), (700, 512), (200, 2048)])
def test_adaptive_finito_steps(ctx, ciao, dtype, shape):
    """Init (Lipschitz probe, hat_gamma, av, z) and 3N backtracking steps against the oracle, same sample sequence --
    including immediate repeats of a sample (the register hand-over path) and repeats two steps apart."""
    import torch
    from oracle import twin as O
    N, d = shape
    A, b, x0 = P.synthetic("ls", N, d, dtype, seed=21)
    lam_f = float(N)
    op, dp = make("ls", A, b, lam_f, dtype)
    og, dg = make_g("l1", dtype, d, lam=0.02)
    alpha, tol_b = 0.999, 1e-9
    tdt = dev(x0).dtype
    table = torch.empty((N, d), dtype=tdt, device="cuda")
    meta4 = torch.empty((N, 4, 4), dtype=tdt, device="cuda")
    meta = meta4[:, 0, :]
    hg = torch.empty(1, dtype=tdt, device="cuda")
    av, z = torch.empty(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda")
    ctx.afinito_init(dp, dg, alpha, dev(x0), table, meta4, av, z, hg)
    ctx.synchronize()
    rt, rg, rgam, rfi, rav, rz, rhg = O.afinito_init(op, og, dtype(alpha), x0)
    # form (i) of close(): the oracle in Float64 on the same Float32 data.  (Not for gamma_i: the stepsize is alpha N over a FINITE-
    # DIFFERENCE Lipschitz estimate |c(x0 + 1) - c(x0)| ||a_i||, Finito_adaptive.jl:65-88, whose cancellation is the algorithm's own in
    # Float32 -- the reference's Float32 run is as far from the Float64 value as the device's.)
    S = 50 if dtype == np.float64 else 10
    close(meta[:, 2], rgam, dtype, scale={64: 5400, 32: 16000}, what="adaptive init gamma_i", ref64=False)   # eps32: the comment above
    close(meta[:, 1], rfi, dtype, scale={64: 130, 32: 450}, what="adaptive init f_i(x0)", scale64=41)
    close(hg, [rhg], dtype, scale=35, what="adaptive init hat_gamma")
    close(av, rav, dtype, scale={64: 81, 32: 71}, what="adaptive init av", scale64=16)
    close(z, rz, dtype, scale={64: 81, 32: 71}, what="adaptive init z", scale64=17)
    assert torch.equal(table, dev(x0).expand(N, d))
    st = ciao.IndexStream(4)
    idx = st.rand_indices(N, 3 * N)
    idx[5:8] = idx[5]          # the same sample three times in a row
    idx[10] = idx[8]           # ... and again two steps later
    if len(idx) > 41:
        # a run of "every other step" repeats (the previous-step hand-over).  Kept short: hammering two samples drives
        # z towards their common fixed point, where the backtracking test f_i(z) <= model + tol degenerates into an
        # equality up to rounding and two correct implementations may legitimately decide differently even in fp64
        idx[20:30:2] = idx[20]
        idx[21:31:2] = idx[21]
    done, trials = ctx.afinito_steps(dp, dg, alpha, tol_b, idx, table, meta4, av, z, hg)
    rdone, rhg, rtrials = O.afinito_steps(op, og, dtype(alpha), dtype(tol_b), idx, rt, rg, rgam, rfi, rhg, rav, rz)
    assert done == rdone == len(idx)
    if (d * np.dtype(dtype).itemsize) % 16 == 0 and d * np.dtype(dtype).itemsize <= 32768:
        assert "afinito_dma_kernel" in ctx.last_kernel(), "rows of whole 16-byte chunks take the LDS-DMA path"
        assert ("masked" in ctx.last_kernel()) == ((d * np.dtype(dtype).itemsize) % 4096 != 0)
    if dtype == np.float64:
        assert trials == rtrials, "same backtracking decisions in fp64"
    S = 2000 if dtype == np.float64 else 200
    # fp32: device and oracle now keep the reference's Float64 promotions in the backtracking test and in `γ *= 0.8`
    # (Finito_adaptive.jl:128-136), so they take the same decisions unless a test f_i(z) <= model + tol sits on the boundary
    # to within the rounding of the two dot products (different summation orders).  That may flip a decision (a stepsize then
    # differs by the factor 0.8, the trajectories part and later decisions differ too), but it must stay the rare exception:
    # the trial counts may differ by at most 2 %, and every case is logged (gpurun_out/parity_observed.json, "trial flips":
    # observed 0 for eight of the nine shapes, 8 of 1229 = 0.65 % at (200, 2048)).
    P.PARITY_LOG.append({"test": "test_adaptive_finito_steps", "line": 0, "what": f"trial flips {shape}", "dtype": np.dtype(dtype).name,
                         "ratio": float(abs(trials - rtrials)), "scale": float(max(1, rtrials // 50))})
    assert abs(trials - rtrials) <= max(1, rtrials // 50), (trials, rtrials)
    if trials == rtrials:
        # (no Float64-oracle form here: oracle/twin.py runs afinito_steps untwinned, and says why)
        close(z, rz, dtype, scale={64: 910, 32: 300}, what=f"adaptive z ({ctx.last_kernel()})")
        close(av, rav, dtype, scale={64: 910, 32: 300}, what="adaptive av")
        close(hg, [rhg], dtype, scale={64: 58, 32: 48}, what="adaptive hat_gamma")
        close(meta[:, 2], rgam, dtype, scale={64: 3000, 32: 3800}, what="adaptive gamma_i")   # eps32: see the init's gamma_i
        close(table, rt, dtype, scale={64: 870, 32: 290}, what="adaptive table")
        # grad f_i = c_i a_i: the oracle's full gradient table against the device's N scalars
        gdev = meta[:, 0:1].double().cpu().numpy() * A.astype(np.float64)
        close(gdev, rg, dtype, scale={64: 250, 32: 190}, what="adaptive gradient table (c_i a_i)")
    # invariant of the algorithm (Finito_adaptive.jl:93 and every update after it):
    #   av == hat_gamma * (sum_i x_i/gamma_i - (1/N) sum_i grad f_i),   hat_gamma == 1 / sum_i 1/gamma_i
    md = meta.double()
    hgd = float(hg.item())
    assert abs(hgd - 1.0 / float((1.0 / md[:, 2]).sum())) <= (1e-10 if dtype == np.float64 else 2e-4) * hgd
    inv = hgd * ((table.double() / md[:, 2:3]).sum(dim=0) - (md[:, 0:1] * dev(A).double()).sum(dim=0) / N)
    close(av, inv.cpu().numpy(), dtype, scale={64: 310, 32: 320}, what="adaptive invariant av")
    # the stored scalars are consistent with the stored points: a_i'x_i, c_i = coef(a_i'x_i), f_i(x_i)
    dots = (dev(A).double() * table.double()).sum(dim=1)
    close(md[:, 3], dots.cpu().numpy(), dtype, scale={64: 14, 32: 10}, what="adaptive a_i'x_i")
    close(md[:, 0], (lam_f * (dots - dev(b).double())).cpu().numpy(), dtype, scale={64: 14, 32: 12}, what="adaptive c_i")
    ctx.synchronize()


@pytest.mark.parametrize("kind,gkind", [("logistic", "l1"), ("ls", "box"), ("logistic", "zero")])
@pytest.mark.parametrize("no_dma", [0, 1])
def test_adaptive_finito_variants(ctx, ciao, kind, gkind, no_dma):
    """The other loss / g combinations on a shape that takes the LDS-DMA path (d = 1024 fp64: J = 2), with samples that
    recur inside the look-ahead window (N = 5 < ring depth: nearly every row is re-read at use), and the same through the
    compiler-scheduled fallback kernel."""
    import torch
    from oracle import twin as O
    N, d, dtype = 5, 1024, np.float64
    A, b, x0 = P.synthetic(kind, N, d, dtype, seed=33)
    lam_f = 1.0 if kind == "logistic" else float(N)
    op, dp = make(kind, A, b, lam_f, dtype)
    og, dg = make_g(gkind, dtype, d, lam=0.01)
    alpha, tol_b = 0.999, 1e-9
    table = torch.empty((N, d), dtype=torch.float64, device="cuda")
    meta4 = torch.empty((N, 4, 4), dtype=torch.float64, device="cuda")
    hg = torch.empty(1, dtype=torch.float64, device="cuda")
    av, z = torch.empty(d, dtype=torch.float64, device="cuda"), torch.empty(d, dtype=torch.float64, device="cuda")
    ctx.set_option("chain_no_dma", no_dma)
    try:
        ctx.afinito_init(dp, dg, alpha, dev(x0), table, meta4, av, z, hg)
        rt, rg, rgam, rfi, rav, rz, rhg = O.afinito_init(op, og, dtype(alpha), x0)
        idx = ciao.IndexStream(9).rand_indices(N, 1300)   # three chunks of the staged index stream
        done, trials = ctx.afinito_steps(dp, dg, alpha, tol_b, idx, table, meta4, av, z, hg)
        assert ("afinito_dma_kernel" in ctx.last_kernel()) == (no_dma == 0)
    finally:
        ctx.set_option("chain_no_dma", 0)
    rdone, rhg, rtrials = O.afinito_steps(op, og, dtype(alpha), dtype(tol_b), idx, rt, rg, rgam, rfi, rhg, rav, rz)
    assert done == rdone == len(idx) and trials == rtrials
    close(z, rz, dtype, scale={64: 70000}, what=f"adaptive z ({ctx.last_kernel()})")
    close(av, rav, dtype, scale={64: 70000}, what="adaptive av")
    close(hg, [rhg], dtype, scale={64: 70}, what="adaptive hat_gamma")
    close(table, rt, dtype, scale={64: 70000}, what="adaptive table")
    assert torch.equal(meta4[:, 0], meta4[:, 1]) and torch.equal(meta4[:, 0], meta4[:, 2]) and torch.equal(meta4[:, 0], meta4[:, 3])
    ctx.synchronize()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind,N,d,forced", [("ls", 20, 5000, False), ("logistic", 12, 9000, False), ("ls", 6, 20001, False),
                                             ("logistic", 30, 300, True), ("ls", 16, 1024, True)])
@pytest.mark.parametrize("route", ["big", "default"])
def test_adaptive_finito_on_rows_of_any_length(ctx, ciao, dtype, kind, N, d, forced, route):
    """Rows beyond the register-resident shapes: afinito_big_kernel (one workgroup, the state in the caller's vectors; option chain_big
    forces it at any d, where it must agree with the fast kernels) and, by default from 32 KiB on, afinito_wide_kernel (the chain shared
    by several workgroups: one mailbox exchange per backtracking trial, workgroup 0 the keeper of the per-sample scalars); fp32 rows of
    16-32 KiB keep to the LDS-DMA kernel.  All against the oracle, a sample three times in a row at the end (the look-ahead's fix-ups)."""
    if route == "default" and forced:
        pytest.skip("the forced route is the big kernel's")
    import torch
    from oracle import twin as O
    A, b, x0 = P.synthetic(kind, N, d, dtype, seed=d)
    lam_f = 1.0 if kind == "logistic" else float(N)
    op, dp = make(kind, A, b, lam_f, dtype)
    og, dg = make_g("l1", dtype, d, lam=0.01)
    alpha, tol_b = 0.999, 1e-9
    tdt = dev(x0).dtype
    table = torch.empty((N, d), dtype=tdt, device="cuda")
    meta4 = torch.empty((N, 4, 4), dtype=tdt, device="cuda")
    hg = torch.empty(1, dtype=tdt, device="cuda")
    av, z = torch.empty(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda")
    ctx.afinito_init(dp, dg, alpha, dev(x0), table, meta4, av, z, hg)
    rt, rg, rgam, rfi, rav, rz, rhg = O.afinito_init(op, og, dtype(alpha), x0)
    close(meta4[:, 0, 2], rgam, dtype, scale={64: 5000, 32: 2300}, what="adaptive init gamma_i, long rows", scale64=840)   # c(x0 .+ 1) - c(x0) cancels
    close(av, rav, dtype, scale={64: 70, 32: 220}, what="adaptive init av, long rows", scale64=16)
    idx = np.concatenate([ciao.IndexStream(4).rand_indices(N, 3 * N), np.full(3, 2, np.int64), np.array([1, 2, 1, 0, 1], np.int64)])
    ctx.set_option("chain_big", int(forced))
    if route == "big":
        ctx.set_option("chain_no_wide", 1)
        ctx.set_option("chain_no_dma", 1)
    try:
        done, trials = ctx.afinito_steps(dp, dg, alpha, tol_b, idx, table, meta4, av, z, hg)
        rowb = d * np.dtype(dtype).itemsize
        want = "afinito_big_kernel" if route == "big" else ("afinito_wide_kernel" if rowb > 32768 else "afinito_dma_kernel")
        assert want in ctx.last_kernel(), ctx.last_kernel()
    finally:
        ctx.set_option("chain_big", 0)
        ctx.set_option("chain_no_wide", 0)
        ctx.set_option("chain_no_dma", 0)
    rdone, rhg, rtrials = O.afinito_steps(op, og, dtype(alpha), dtype(tol_b), idx, rt, rg, rgam, rfi, rhg, rav, rz)
    assert done == rdone == len(idx)
    assert abs(trials - rtrials) <= max(2, 0.02 * rtrials), (trials, rtrials)
    if trials == rtrials:
        close(z, rz, dtype, scale={64: 300, 32: 290}, what=f"adaptive z ({ctx.last_kernel()})")
        close(av, rav, dtype, scale={64: 300, 32: 290}, what="adaptive av, long rows")
        close(hg, [rhg], dtype, scale={64: 580, 32: 360}, what="adaptive hat_gamma, long rows")
        close(table, rt, dtype, scale={64: 310, 32: 280}, what="adaptive table, long rows")
        close(meta4[:, 0, 2], rgam, dtype, scale={64: 350, 32: 440}, what="adaptive gamma_i, long rows")
    assert torch.equal(meta4[:, 0], meta4[:, 1]) and torch.equal(meta4[:, 0], meta4[:, 2]) and torch.equal(meta4[:, 0], meta4[:, 3])
    ctx.synchronize()


@pytest.mark.parametrize("d", [64, 1024])
def test_adaptive_finito_stops_when_the_stepsize_collapses(ctx, ciao, d):
    """tol_b so large that the very first step finds gamma_i < tol_b/N: the chain ends (reference :121-124)."""
    import torch
    N = 12
    A, b, x0 = P.synthetic("ls", N, d, np.float64, seed=2)
    _, dp = make("ls", A, b, float(N), np.float64)
    _, dg = make_g("l1", np.float64, d)
    table = torch.empty((N, d), dtype=torch.float64, device="cuda")
    meta4 = torch.empty((N, 4, 4), dtype=torch.float64, device="cuda")
    meta = meta4[:, 0, :]
    hg = torch.empty(1, dtype=torch.float64, device="cuda")
    av, z = torch.empty(d, dtype=torch.float64, device="cuda"), torch.empty(d, dtype=torch.float64, device="cuda")
    ctx.afinito_init(dp, dg, 0.999, dev(x0), table, meta4, av, z, hg)
    done, trials = ctx.afinito_steps(dp, dg, 0.999, 1e12, np.arange(5, dtype=np.int64), table, meta4, av, z, hg)
    assert done == 0 and trials == 0
    ctx.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# ProShI
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape,r", [((3, 2), 1), ((3, 2), 2), ((40, 7), 5), ((64, 256), 8), ((30, 1000), 30), ((9, 4096), 4),
                                     ((700, 1100), 600), ((12, 8192), 5)])
@pytest.mark.parametrize("generic", [0, 1])
def test_proshi_steps(ctx, ciao, dtype, shape, r, generic):
    """generic=0: proshi_vec_kernel wherever rows are whole 16-byte chunks (masked tail at d = 1000, 1100; several rows per
    workgroup at N = 700); generic=1: the scalar kernel for every shape."""
    import torch
    if generic and shape[1] * np.dtype(dtype).itemsize * 2 > 144 * 1024:
        pytest.skip("beyond the generic kernel's LDS budget")
    from oracle import twin as O
    from ciaoalgorithms_jl_amd.device import PackedSepQuad
    N, d = shape
    rng = np.random.default_rng(N + d)
    Q = rng.uniform(-1.0, 3.0, (N, d)).astype(dtype)
    q = rng.standard_normal((N, d)).astype(dtype)
    eta, lo, hi = 3.0 * N, -2.0, 2.0
    x0 = (0.5 * rng.standard_normal(d)).astype(dtype)
    gam = (0.999 * N / (np.abs(Q).max(axis=1) + eta)).astype(dtype)
    g_hi = np.linspace(0.5, 1.5, d).astype(dtype)
    of, og = O.SepQuad(Q, q, eta, lo, hi), O.Prox("box", lo=-np.inf, hi=g_hi, dtype=dtype)
    from ciaoalgorithms_jl_amd.device import ProxG
    import ciaoalgorithms_jl_amd._lib as L
    df = PackedSepQuad(dev(Q), dev(q), eta, lo, hi)
    dg = ProxG(L.PROX_BOX, lo=-float("inf"), hi_vec=dev(g_hi))
    tdt = dev(x0).dtype
    table = torch.empty((N, d), dtype=tdt, device="cuda")
    av, z = torch.empty(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda")
    hg = torch.empty(1, dtype=tdt, device="cuda")
    ctx.set_option("force_generic", generic)
    try:
        ctx.proshi_init(df, dg, dev(gam), dev(x0), table, av, z, hg)
        rowb = d * np.dtype(dtype).itemsize
        vec_ok = rowb % 16 == 0 and rowb <= 32768 and not generic
        assert ("proshi_vec_kernel" in ctx.last_kernel()) == vec_ok, ctx.last_kernel()
    finally:
        ctx.set_option("force_generic", 0)
    rt, rav, rz, rhg = O.proshi_init(of, og, gam, x0)
    close(table, rt, dtype, scale={64: 9.9, 32: 8}, what="proshi init table", scale64=8)
    close(hg, [rhg], dtype, scale={64: 16, 32: 520}, what="proshi hat_gamma")
    close(av, rav, dtype, scale={64: 74, 32: 60}, what="proshi init av", scale64=10)
    close(z, rz, dtype, scale={64: 67, 32: 480}, what="proshi init z", size=np.abs(rav).max() / abs(float(rhg)), scale64=13)
    st = ciao.IndexStream(2)
    batches = [st.sample_without_replacement(N, r) for _ in range(12)]
    bptr = np.arange(len(batches) + 1, dtype=np.int64) * r
    ctx.set_option("force_generic", generic)
    try:
        ctx.proshi_steps(df, dg, dev(gam), float(hg.item()), bptr, np.concatenate(batches), table, av, z)
    finally:
        ctx.set_option("force_generic", 0)
    O.proshi_steps(of, og, gam, rhg, batches, rt, rav, rz)
    close(table, rt, dtype, scale={64: 170, 32: 530}, what=f"proshi table ({ctx.last_kernel()})", scale64=41)
    close(av, rav, dtype, scale={64: 140, 32: 190}, what="proshi av", scale64=36)
    # z = (prox(av) - av) / hat_gamma (ProShI_basic.jl:119-121): a difference of quantities |av| large, divided by hat_gamma -- its
    # rounding unit is theirs (at (700, 1100) |z| is a thousandth of |av| / hat_gamma, and the reference's own Float32 z is 100-1500
    # eps32 of |z| from its Float64 value)
    close(z, rz, dtype, scale={64: 11, 32: 30}, what="proshi z", size=np.abs(rav).max() / abs(float(rhg)), scale64=29)
    close(av, table.double().sum(dim=0).cpu().numpy(), dtype, scale={64: 45, 32: 83}, what="invariant av == sum_i s_i")
    ctx.proshi_solution(df, dev(gam), z, table)
    close(table, O.proshi_solution(of, gam, rz, rt), dtype, scale={64: 170, 32: 530}, what="proshi solution", scale64=39)
    ctx.synchronize()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape,r", [((3, 2), 1), ((5, 7), 2), ((40, 65), 5), ((12, 256), 12), ((600, 33), 300), ((6, 1000), 3),
                                     ((3, 2048), 2)])
def test_proshi_dense_quadratic(ctx, ciao, dtype, shape, r):
    """f_i = Sum(Quadratic(Q_i, q_i), SqrDistL2(box, eta)) with a full d x d matrix per agent (ciao_sepquad.dense = 1;
    ProShI_basic.jl:113 calls the operator's own gradient!, i.e. Q_i x + q_i): proshi_dense_kernel against the oracle."""
    import torch
    from oracle import twin as O
    from ciaoalgorithms_jl_amd.device import PackedSepQuad, ProxG
    import ciaoalgorithms_jl_amd._lib as L
    N, d = shape
    rng = np.random.default_rng(N + d)
    B = rng.standard_normal((N, d, d)) / np.sqrt(d)
    Q = (B.transpose(0, 2, 1) @ B + 0.1 * np.eye(d)).astype(dtype)                # SPD, genuinely dense
    q = rng.standard_normal((N, d)).astype(dtype)
    eta, lo, hi = 3.0 * N, -2.0, 2.0
    x0 = (0.5 * rng.standard_normal(d)).astype(dtype)
    Lc = np.array([np.linalg.norm(Q[i].astype(np.float64)) for i in range(N)]) + eta   # Frobenius >= spectral norm
    gam = (0.999 * N / Lc).astype(dtype)
    g_hi = np.linspace(0.5, 1.5, d).astype(dtype)
    of, og = O.SepQuad(Q, q, eta, lo, hi), O.Prox("box", lo=-np.inf, hi=g_hi, dtype=dtype)
    df = PackedSepQuad(dev(Q), dev(q), eta, lo, hi)
    assert df.dense and of.dense
    dg = ProxG(L.PROX_BOX, lo=-float("inf"), hi_vec=dev(g_hi))
    tdt = dev(x0).dtype
    table = torch.empty((N, d), dtype=tdt, device="cuda")
    av, z = torch.empty(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda")
    hg = torch.empty(1, dtype=tdt, device="cuda")
    ctx.proshi_init(df, dg, dev(gam), dev(x0), table, av, z, hg)
    assert "proshi_dense_kernel" in ctx.last_kernel(), ctx.last_kernel()
    rt, rav, rz, rhg = O.proshi_init(of, og, gam, x0)
    # independent statement of the init table in numpy: s_i = x0 - gam_i/N (Q_i x0 + q_i + eta (x0 - clamp(x0)))
    want = x0.astype(np.float64) - (gam.astype(np.float64) / N)[:, None] * (
        Q.astype(np.float64) @ x0.astype(np.float64) + q + eta * (x0 - np.clip(x0, lo, hi)).astype(np.float64))
    close(table, want, dtype, scale=8, what="dense proshi init table vs numpy")
    close(table, rt, dtype, scale=8, what="dense proshi init table", scale64=8)
    close(av, rav, dtype, scale={64: 29, 32: 35}, what="dense proshi init av", scale64=8)
    close(z, rz, dtype, scale={64: 22, 32: 63}, what="dense proshi init z", size=np.abs(rav).max() / abs(float(rhg)), scale64=12)
    st = ciao.IndexStream(2)
    batches = [st.sample_without_replacement(N, r) if 2 * r <= N else np.sort(st.randperm(N)[:r]) for _ in range(10)]
    bptr = np.arange(len(batches) + 1, dtype=np.int64) * r
    ctx.proshi_steps(df, dg, dev(gam), float(hg.item()), bptr, np.concatenate(batches), table, av, z)
    O.proshi_steps(of, og, gam, rhg, batches, rt, rav, rz)
    close(table, rt, dtype, scale={64: 130, 32: 140}, what=f"dense proshi table ({ctx.last_kernel()})", scale64=20)
    close(av, rav, dtype, scale={64: 270, 32: 95}, what="dense proshi av", scale64=25)
    close(z, rz, dtype, scale={64: 8, 32: 10}, what="dense proshi z", size=np.abs(rav).max() / abs(float(rhg)), scale64=8)
    close(av, table.double().sum(dim=0).cpu().numpy(), dtype, scale={64: 20, 32: 25}, what="dense invariant av == sum_i s_i")
    # contiguous blocks of agents (sweeping 2 / 3) are the same batches
    t2, av2, z2 = table.clone(), av.clone(), z.clone()
    first = np.array([0, N // 2], np.int64)
    ln = np.array([N // 2, N - N // 2], np.int64)
    ctx.proshi_steps_blocks(df, dg, dev(gam), float(hg.item()), first, ln, t2, av2, z2)
    ctx.proshi_steps(df, dg, dev(gam), float(hg.item()), np.array([0, N // 2, N], np.int64), np.arange(N, dtype=np.int64), table, av, z)
    assert torch.equal(t2, table) and torch.equal(av2, av) and torch.equal(z2, z)
    ctx.synchronize()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape,r", [((3, 2), 1), ((3, 2), 3), ((5, 7), 2), ((40, 300), 1), ((64, 1024), 8), ((200, 1500), 18), ((9, 4099), 4)])
def test_proshi_small_batches_run_as_one_coordinate_parallel_chain(ctx, ciao, dtype, shape, r):
    """Batches of up to 18 separable agents: a run of iterations is ONE launch (proshi_chain_kernel: thread k carries av_k, z_k
    through every visited agent, the reference's operation order, no reduction).  Against the oracle, against the batch-parallel
    path (option proshi_chain_max_batch = 0), index lists and row blocks, with agents revisited inside the look-ahead window
    (N = 3) and a per-coordinate IndBox as g."""
    import torch
    from oracle import twin as O
    from ciaoalgorithms_jl_amd.device import PackedSepQuad, ProxG
    import ciaoalgorithms_jl_amd._lib as L
    N, d = shape
    rng = np.random.default_rng(N * 13 + d)
    Q = rng.uniform(-1.0, 3.0, (N, d)).astype(dtype)
    q = rng.standard_normal((N, d)).astype(dtype)
    eta, lo, hi = 3.0 * N, -2.0, 2.0
    x0 = (0.5 * rng.standard_normal(d)).astype(dtype)
    gam = (0.999 * N / (np.abs(Q).max(axis=1) + eta)).astype(dtype)
    g_hi = np.linspace(0.5, 1.5, d).astype(dtype)
    of, og = O.SepQuad(Q, q, eta, lo, hi), O.Prox("box", lo=-np.inf, hi=g_hi, dtype=dtype)
    df = PackedSepQuad(dev(Q), dev(q), eta, lo, hi)
    dg = ProxG(L.PROX_BOX, lo=-float("inf"), hi_vec=dev(g_hi))
    tdt = dev(x0).dtype
    st = ciao.IndexStream(4)
    nit = 40
    batches = [st.sample_without_replacement(N, r) for _ in range(nit)]
    bptr = np.arange(nit + 1, dtype=np.int64) * r
    rt, rav, rz, rhg = O.proshi_init(of, og, gam, x0)
    O.proshi_steps(of, og, gam, rhg, batches, rt, rav, rz)
    res = {}
    for lim in (-1, 0):
        table = torch.empty((N, d), dtype=tdt, device="cuda")
        av, z = torch.empty(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda")
        hg = torch.empty(1, dtype=tdt, device="cuda")
        ctx.proshi_init(df, dg, dev(gam), dev(x0), table, av, z, hg)
        ctx.set_option("proshi_chain_max_batch", lim)
        try:
            ctx.proshi_steps(df, dg, dev(gam), float(hg.item()), bptr, np.concatenate(batches), table, av, z)
            assert ("proshi_chain_kernel" in ctx.last_kernel()) == (lim == -1), ctx.last_kernel()
        finally:
            ctx.set_option("proshi_chain_max_batch", -1)
        close(table, rt, dtype, scale={64: 190, 32: 160}, what=f"proshi small batches table ({ctx.last_kernel()})", scale64=140)
        close(av, rav, dtype, scale={64: 94, 32: 89}, what="proshi small batches av", scale64=79)
        close(z, rz, dtype, scale={64: 20, 32: 16}, what="proshi small batches z", size=np.abs(rav).max() / abs(float(rhg)), scale64=9.5)
        res[lim] = (table, av, z)
    # static contiguous blocks (sweeping 2 / 3) through the chain == the same batches as index lists
    if r <= N:
        nb = N // r
        first = (np.arange(3 * nb) % nb * r).astype(np.int64)
        ln = np.full(3 * nb, r, np.int64)
        t1, a1, z1 = (x.clone() for x in res[-1])
        t2, a2, z2 = (x.clone() for x in res[-1])
        ctx.proshi_steps_blocks(df, dg, dev(gam), float(rhg), first, ln, t1, a1, z1)
        assert "proshi_chain_kernel" in ctx.last_kernel()
        idx = (first[:, None] + np.arange(r)[None, :]).reshape(-1)
        ctx.proshi_steps(df, dg, dev(gam), float(rhg), np.arange(3 * nb + 1, dtype=np.int64) * r, idx, t2, a2, z2)
        assert torch.equal(t1, t2) and torch.equal(a1, a2) and torch.equal(z1, z2)
    ctx.synchronize()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d", [2, 50, 300, 1500, 449])
def test_proshi_chain_with_wholly_dead_waves_over_thousands_of_visits(ctx, ciao, dtype, d):
    """d mod 256 in 1..192 leaves whole waves of the last block without a coordinate.  They used to shadow coordinate d-1 --
    loads AND stores -- unsynchronised with the wave that owns it: once the waves drifted apart by the look-ahead depth (the
    loop has no barrier), a prefetch could read, and a late store overwrite, the owner's table entry.  Now
    they take no part in the visits.  Here: agents revisited just outside the look-ahead window (N = depth + 2, cyclic order)
    and inside it (runs of repeats), 6000 visits in one launch -- far more than the drift needs -- against the oracle, and
    bitwise reproducible from run to run."""
    import torch
    from oracle import twin as O
    from ciaoalgorithms_jl_amd.device import PackedSepQuad, ProxG
    import ciaoalgorithms_jl_amd._lib as L
    depth = 9 if dtype == np.float64 else 16
    N = depth + 2
    rng = np.random.default_rng(d)
    Q = rng.uniform(0.5, 3.0, (N, d)).astype(dtype)
    q = rng.standard_normal((N, d)).astype(dtype)
    eta, lo, hi = 3.0 * N, -2.0, 2.0
    x0 = (0.5 * rng.standard_normal(d)).astype(dtype)
    gam = (0.999 * N / (np.abs(Q).max(axis=1) + eta)).astype(dtype)
    g_hi = np.linspace(0.5, 1.5, d).astype(dtype)
    of, og = O.SepQuad(Q, q, eta, lo, hi), O.Prox("box", lo=-np.inf, hi=g_hi, dtype=dtype)
    df = PackedSepQuad(dev(Q), dev(q), eta, lo, hi)
    dg = ProxG(L.PROX_BOX, lo=-float("inf"), hi_vec=dev(g_hi))
    tdt = dev(x0).dtype
    nit = 6000
    order = np.arange(nit, dtype=np.int64) % N
    order[1000:1004] = order[1000]                      # revisits inside the window as well
    order[3000:3600] = rng.integers(0, N, 600)
    batches = [order[i:i + 1] for i in range(nit)]
    bptr = np.arange(nit + 1, dtype=np.int64)
    rt, rav, rz, rhg = O.proshi_init(of, og, gam, x0)
    O.proshi_steps(of, og, gam, rhg, batches, rt, rav, rz)
    runs = []
    for _ in range(2):
        table = torch.empty((N, d), dtype=tdt, device="cuda")
        av, z = torch.empty(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda")
        hg = torch.empty(1, dtype=tdt, device="cuda")
        ctx.proshi_init(df, dg, dev(gam), dev(x0), table, av, z, hg)
        ctx.proshi_steps(df, dg, dev(gam), float(hg.item()), bptr, order, table, av, z)
        assert "proshi_chain_kernel" in ctx.last_kernel(), ctx.last_kernel()
        ctx.synchronize()
        runs.append((table.clone(), av.clone(), z.clone()))
    for u, v in zip(*runs):
        assert torch.equal(u, v)
    close(runs[0][0], rt, dtype, scale={64: 100, 32: 78}, what="proshi long chain table", scale64=81)
    close(runs[0][0][:, d - 1], rt[:, d - 1], dtype, scale={64: 8, 32: 19}, what="proshi long chain table, coordinate d-1")
    close(runs[0][1], rav, dtype, scale={64: 100, 32: 280}, what="proshi long chain av", scale64=840)


def test_proshi_dense_is_validated(ctx, ciao):
    import torch
    from ciaoalgorithms_jl_amd.device import PackedSepQuad, ProxG
    import ciaoalgorithms_jl_amd._lib as L
    d = 64 * 1024 // 4 + 4                                  # one element past 64 KiB of fp32
    Q = torch.zeros((1, d, d), dtype=torch.float32, device="cuda")
    q = torch.zeros((1, d), dtype=torch.float32, device="cuda")
    df = PackedSepQuad(Q, q, 0.0, 0.0, 0.0)
    v = lambda: torch.zeros(d, dtype=torch.float32, device="cuda")
    with pytest.raises(ciao._lib.CiaoError, match="64 KiB"):
        ctx.proshi_init(df, ProxG(L.PROX_ZERO), torch.ones(1, dtype=torch.float32, device="cuda"), v(), torch.zeros((1, d), dtype=torch.float32, device="cuda"),
                        v(), v(), torch.zeros(1, dtype=torch.float32, device="cuda"))
    df._c.dense = 7
    with pytest.raises(ciao._lib.CiaoError, match="dense must be 0 or 1"):
        ctx.proshi_init(df, ProxG(L.PROX_ZERO), torch.ones(1, dtype=torch.float32, device="cuda"), v(), torch.zeros((1, d), dtype=torch.float32, device="cuda"),
                        v(), v(), torch.zeros(1, dtype=torch.float32, device="cuda"))


# ----------------------------------------------------------------------------------------------------------------------
# error behaviour at the boundary
# ----------------------------------------------------------------------------------------------------------------------
def test_out_of_range_index_is_reported_not_faulted(ctx, ciao):
    import torch
    from ciaoalgorithms_jl_amd._lib import CiaoError
    A, b, x0 = P.synthetic("ls", 10, 8, np.float64)
    _, dp = make("ls", A, b, 10.0, np.float64)
    _, dg = make_g("zero", np.float64, 8)
    av, z, zf, w = (torch.zeros(8, dtype=torch.float64, device="cuda") for _ in range(4))
    ctx.svrg_init(dp, dev(x0), av, z, zf, w)
    ctx.svrg_inner(dp, dg, 0.1, np.array([1, 2, 10, 3], np.int64), av, z, zf, w)   # 10 is out of range
    with pytest.raises(CiaoError):
        ctx.synchronize()
    ctx.synchronize()   # the sticky flag is cleared once reported


def test_argument_validation(ctx):
    import torch
    from ciaoalgorithms_jl_amd._lib import CiaoError
    A, b, x0 = P.synthetic("ls", 10, 8, np.float64)
    _, dp = make("ls", A, b, 10.0, np.float64)
    _, dg = make_g("zero", np.float64, 8)
    av = torch.zeros(8, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        ctx.full_gradient(dp, torch.zeros(7, dtype=torch.float64, device="cuda"), av)      # wrong length
    with pytest.raises(ValueError):
        ctx.full_gradient(dp, torch.zeros(8, dtype=torch.float32, device="cuda"), av)      # silent promotion refused
    with pytest.raises(CiaoError):
        ctx.proxgrad_step(dp, dg, -1.0, dev(x0), av, av)                                   # gamma <= 0
    with pytest.raises(CiaoError):
        ctx.gradient(dp, 10, dev(x0), av)                                                  # sample index out of range
    with pytest.raises(CiaoError):
        ctx.set_option("no_such_option", 1)


# ----------------------------------------------------------------------------------------------------------------------
# kernel-selection boundaries: row lengths on either side of every dispatch threshold
# ----------------------------------------------------------------------------------------------------------------------
BOUNDARY_D = [63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1023, 1025, 2047, 2049, 4095, 4097, 8191, 8192, 8193, 16383, 16384, 16385]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d", BOUNDARY_D)
def test_row_length_boundaries(ctx, ciao, dtype, d):
    """Sweep, SAGA / Finito table init and a Finito batch on row lengths around every threshold of the dispatch (wave-per-row
    shapes, 16-byte chunks, element-wise chunks, 4096-element and 64 KiB limits, generic kernel): whichever kernel is chosen,
    the result is the oracle's."""
    import torch
    from oracle import twin as O
    from ciaoalgorithms_jl_amd._lib import CiaoError
    N = 23
    A, b, x0 = P.synthetic("ls", N, d, dtype, seed=d)
    op, dp = make("ls", A, b, float(N), dtype)
    og, dg = make_g("l1", dtype, d, lam=0.02)
    tdt = dev(x0).dtype
    av, z = torch.empty(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda")
    ctx.full_gradient(dp, dev(x0), av)   # every row length has a kernel (beyond LDS: the generic kernel with global accumulators)
    k_sweep = ctx.last_kernel()
    close(av, O.full_pass(op, x0), dtype, scale={64: 130, 32: 81}, what=f"sweep d={d} ({k_sweep})", scale64=16)
    table = torch.empty((N, d), dtype=tdt, device="cuda")
    gamma = 0.5 / N
    ctx.saga_init(dp, dg, gamma, dev(x0), table, av, z)
    rt, rav, rz = O.saga_init(op, og, dtype(gamma), x0)
    close(table, rt, dtype, scale={64: 220, 32: 120}, what=f"saga_init table d={d} ({ctx.last_kernel()})", scale64=16)
    close(av, rav, dtype, scale={64: 130, 32: 82}, what="saga_init av", scale64=16)
    Li = float(N) * np.sum(A.astype(np.float64) ** 2, axis=1)
    gam = (0.999 * N / Li).astype(dtype)
    dgam = dev(gam)
    hg = ctx.hat_gamma(dgam)
    rt, rav, rz, rhg = O.finito_init(op, og, gam, x0)
    ctx.finito_init(dp, dg, dgam, hg, dev(x0), table, av, z)
    close(table, rt, dtype, scale={64: 9.600000000000001, 32: 9.8}, what=f"finito_init table d={d}", scale64=8)
    ctx.set_option("chain_max_batch", 0)
    try:
        batch = np.array([3, 19, 0, 7, 11, 22, 5], dtype=np.int64)
        ctx.finito_steps(dp, dg, dgam, hg, np.array([0, 7], np.int64), batch, table, av, z)
    finally:
        ctx.set_option("chain_max_batch", -1)
    O.finito_steps(op, og, gam, rhg, [batch], rt, rav, rz)
    close(table, rt, dtype, scale=27, what=f"finito batch table d={d} ({ctx.last_kernel()})", scale64=14)
    close(z, rz, dtype, scale={64: 37, 32: 35}, what="finito batch z", scale64=18)
    ctx.synchronize()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d", [1, 2, 4, 63, 64, 65, 66, 127, 128, 129, 130, 255, 256, 257, 260, 511, 512, 513, 516, 1023, 1025, 2047, 2049, 3071, 4095,
                               4096, 4097, 6000, 8192, 8193])
def test_chain_row_length_boundaries(ctx, ciao, dtype, d):
    """SVRG inner cycle and SAGA steps on row lengths around the chain kernels' thresholds (single-wave / four-wave, LDS-DMA
    exact / masked, register ring E = 1 / 4 / 8 / 16 / 32, and beyond 8192 elements the any-length kernel chain_big_kernel)."""
    import torch
    from oracle import twin as O
    from ciaoalgorithms_jl_amd._lib import CiaoError
    N = 12
    A, b, x0 = P.synthetic("ls", N, d, dtype, seed=d)
    op, dp = make("ls", A, b, float(N), dtype)
    og, dg = make_g("l1", dtype, d, lam=0.01)
    tdt = dev(x0).dtype
    av, z, zf, w = (torch.empty(d, dtype=tdt, device="cuda") for _ in range(4))
    ctx.svrg_init(dp, dev(x0), av, z, zf, w)
    rav, rz, rzf, rw = O.svrg_init(op, x0)
    idx = ciao.IndexStream(d).rand_indices(N, 60)
    gamma = 0.05 / N
    ctx.svrg_inner(dp, dg, gamma, idx, av, z, zf, w)
    # (beyond one workgroup's registers -- 8192 elements, fp64: 4096 -- several workgroups share the chain)
    assert ("chain_wide_kernel" in ctx.last_kernel()) == (d > (4096 if dtype == np.float64 else 8192)), ctx.last_kernel()
    O.svrg_inner(op, og, dtype(gamma), idx, rav, rz, rzf, rw)
    close(w, rw, dtype, scale={64: 340, 32: 240}, what=f"svrg_inner w d={d} ({ctx.last_kernel()})", scale64=460)
    table = torch.empty((N, d), dtype=tdt, device="cuda")
    ctx.saga_init(dp, dg, gamma, dev(x0), table, av, z)
    rt, rav, rz = O.saga_init(op, og, dtype(gamma), x0)
    ctx.saga_steps(dp, dg, gamma, False, idx, table, av, z)
    O.saga_steps(op, og, dtype(gamma), False, idx, rt, rav, rz)
    close(z, rz, dtype, scale={64: 20, 32: 200}, what=f"saga z d={d} ({ctx.last_kernel()})", scale64=480)   # 20.4 eps observed at d = 2 (a two-element vector)
    close(table, rt, dtype, scale={64: 91, 32: 120}, what="saga table", scale64=100)
    ctx.synchronize()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("small_i", [8, 16])
@pytest.mark.parametrize("shape", [(333, 50), (97, 200), (1000, 7), (41, 255)])
def test_small_row_kernel_group_sizes(ctx, ciao, dtype, small_i, shape):
    """rows_small_kernel with 8 and 16 elements per lane (both exist for both types; the automatic choice uses one of each):
    sweep, SAGA init and Finito init against the oracle, row counts that are not multiples of the rows per group."""
    import torch
    from oracle import twin as O
    N, d = shape
    A, b, x0 = P.synthetic("logistic" if d == 200 else "ls", N, d, dtype, seed=N)
    loss = "logistic" if d == 200 else "ls"
    lam_f = 1.0 if loss == "logistic" else float(N)
    op, dp = make(loss, A, b, lam_f, dtype)
    og, dg = make_g("l1", dtype, d, lam=0.02)
    tdt = dev(x0).dtype
    av, z = torch.empty(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda")
    table = torch.empty((N, d), dtype=tdt, device="cuda")
    ctx.set_option("small_i", small_i)
    ctx.set_option("small_mfma", 0)   # (the sweep of dense rows of 17 .. 256 elements otherwise runs on the matrix cores)
    try:
        ctx.full_gradient(dp, dev(x0), av)
        rowb = d * np.dtype(dtype).itemsize
        if rowb % 16 == 0 and rowb >= 1024:   # whole 16-byte chunks of at least 1 KiB: a workgroup per row instead
            assert "rows_split_kernel" in ctx.last_kernel(), ctx.last_kernel()
        else:
            assert "rows_small_kernel" in ctx.last_kernel() and f"I{small_i}" in ctx.last_kernel(), ctx.last_kernel()
        close(av, O.full_pass(op, x0), dtype, scale={64: 37, 32: 54}, what=f"sweep ({ctx.last_kernel()})", scale64=14)
        gamma = 0.5 / N
        ctx.saga_init(dp, dg, gamma, dev(x0), table, av, z)
        rt, rav, rz = O.saga_init(op, og, dtype(gamma), x0)
        close(table, rt, dtype, scale={64: 18, 32: 20}, what="saga_init table", scale64=8.200000000000001)
        close(av, rav, dtype, scale={64: 27, 32: 47}, what="saga_init av", scale64=14)
        Li = (lam_f if loss == "ls" else 0.25) * np.sum(A.astype(np.float64) ** 2, axis=1)
        gam = (0.999 * N / Li).astype(dtype)
        dgam = dev(gam)
        hg = ctx.hat_gamma(dgam)
        rt, rav, rz, rhg = O.finito_init(op, og, gam, x0)
        ctx.finito_init(dp, dg, dgam, hg, dev(x0), table, av, z)
        close(table, rt, dtype, scale={64: 9.4, 32: 16}, what="finito_init table", scale64=14)
        close(av, rav, dtype, scale={64: 38, 32: 46}, what="finito_init av", scale64=9.700000000000001)
        close(z, rz, dtype, scale={64: 38, 32: 46}, what="finito_init z", scale64=11)
    finally:
        ctx.set_option("small_i", 0)
        ctx.set_option("small_mfma", -1)
    ctx.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# seeded random shapes: row counts, row lengths and row strides nobody picked by hand
# ----------------------------------------------------------------------------------------------------------------------
def _random_cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        N = int(rng.choice([1, 2, 3, 5, 17, 63, 64, 65, 130, 257, 600, 1500]))
        d = int(rng.choice([rng.integers(1, 40), rng.integers(40, 300), rng.integers(300, 1100), rng.integers(1100, 2600)]))
        pad = int(rng.choice([0, 0, 0, 1, 2, 4, 7]))
        dtype = [np.float64, np.float32][int(rng.integers(0, 2))]
        loss = ["ls", "logistic"][int(rng.integers(0, 2))]
        out.append((N, d, pad, dtype, loss))
    return out


@pytest.mark.parametrize("case", _random_cases(int(os.environ.get("CIAO_FUZZ_SHAPES", "300")), int(os.environ.get("CIAO_FUZZ_SEED", "2024"))), ids=lambda c: f"N{c[0]}-d{c[1]}-pad{c[2]}-{'f64' if c[3] == np.float64 else 'f32'}-{c[4]}")
def test_random_shapes(ctx, ciao, case):
    """Sweep, both table inits, a Finito batch (batch-parallel) and a short SAGA chain on seeded random (N, d, row stride,
    type, loss): every combination lands on some kernel, and that kernel agrees with the oracle."""
    import torch
    from oracle import twin as O
    N, d, pad, dtype, loss = case
    A, b, x0 = P.synthetic(loss, N, d, dtype, seed=N * 7919 + d)
    lam_f = float(N) if loss == "ls" else 1.0
    op, dp = make(loss, A, b, lam_f, dtype, pad=pad)
    og, dg = make_g("l1", dtype, d, lam=0.02)
    tdt = dev(x0).dtype
    av, z = torch.empty(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda")
    table = torch.empty((N, d), dtype=tdt, device="cuda")
    # Iterates and Finito table rows are x - gamma (...): on rows of one or two elements the result can be orders of magnitude smaller than
    # its operands, and its rounding is theirs -- one rounding unit is taken at the size of the operands (`size=`, as close() says)
    osz = lambda ref: max(float(np.abs(np.asarray(ref)).max(initial=0.0)), float(np.abs(x0).max(initial=0.0)))
    ctx.full_gradient(dp, dev(x0), av)
    close(av, O.full_pass(op, x0), dtype, scale={64: 140, 32: 400}, what=f"sweep ({ctx.last_kernel()})", scale64=120)
    gamma = 0.5 / max(lam_f, 1.0)
    ctx.saga_init(dp, dg, gamma, dev(x0), table, av, z)
    rt, rav, rz = O.saga_init(op, og, dtype(gamma), x0)
    close(table, rt, dtype, scale={64: 190, 32: 400}, what=f"saga_init table ({ctx.last_kernel()})", scale64=120)
    idx = ciao.IndexStream(N + d).rand_indices(N, 25)
    ctx.saga_steps(dp, dg, gamma, False, idx, table, av, z)
    O.saga_steps(op, og, dtype(gamma), False, idx, rt, rav, rz)
    close(z, rz, dtype, scale={64: 94, 32: 82}, what=f"saga z ({ctx.last_kernel()})", scale64=130, size=osz(rz))
    Li = (lam_f if loss == "ls" else 0.25) * np.sum(A.astype(np.float64) ** 2, axis=1) + 1e-12
    gam = (0.999 * N / Li).astype(dtype)
    dgam = dev(gam)
    hg = ctx.hat_gamma(dgam)
    rt, rav, rz, rhg = O.finito_init(op, og, gam, x0)
    ctx.finito_init(dp, dg, dgam, hg, dev(x0), table, av, z)
    close(table, rt, dtype, scale={64: 24, 32: 23}, what=f"finito_init table ({ctx.last_kernel()})", scale64=16, size=osz(rt))
    r = min(N, 9)
    batch = ciao.IndexStream(d).sample_without_replacement(N, r)
    ctx.set_option("chain_max_batch", 0)
    try:
        ctx.finito_steps(dp, dg, dgam, hg, np.array([0, r], np.int64), batch, table, av, z)
    finally:
        ctx.set_option("chain_max_batch", -1)
    O.finito_steps(op, og, gam, rhg, [batch], rt, rav, rz)
    close(table, rt, dtype, scale={64: 110, 32: 100}, what=f"finito batch table ({ctx.last_kernel()})", scale64=20, size=osz(rt))
    close(z, rz, dtype, scale={64: 150, 32: 130}, what="finito batch z", scale64=31, size=osz(rz))
    ctx.synchronize()

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d", [1024, 50])
def test_adaptive_finito_random_reprobe(ctx, ciao, dtype, d):
    """Finito_adaptive.jl:78-85: when grad f_i(x0 .+ 1) == grad f_i(x0) (here: rows whose entries sum to exactly zero, probed at
    x0 = 0) the reference probes random points x0 .+ rand(t*[-1,1]), t = 1, 2, 4, ...  The draws are an input on this path
    (IndexStream.rand_signs): the device init flags those samples, the host mirror re-probes them in increasing i
    (ciao_afinito_probe) and repeats the init pass with the resolved stepsizes.  Oracle: the same branch with the same draws
    (roughly every second draw leaves a'signs = 0 again, so t doubles: the quirk of using t AFTER its doubling is covered)."""
    import torch
    from oracle import twin as O
    from ciaoalgorithms_jl_amd import solvers as S
    N = 30
    A, b, _ = P.synthetic("ls", N, d, dtype, seed=77)
    for i in (3, 7, 8, 29):                    # rows with entries +v, -v and zeros: the sum is exactly 0 in any order
        A[i] = 0
        A[i, 5], A[i, 6] = dtype(0.7), dtype(-0.7)
    x0 = np.zeros(d, dtype)
    op, dp = make("ls", A, b, float(N), dtype)
    og, dg = make_g("l1", dtype, d, lam=0.02)
    seed = 123
    draws = ciao.IndexStream(seed)
    signs = np.stack([draws.rand_signs(d).astype(dtype) for _ in range(64)])
    with pytest.raises(RuntimeError):          # the oracle without draws refuses, as the device does without a host
        O.afinito_init(op, og, dtype(0.999), x0)
    rt, rg, rgam, rfi, rav, rz, rhg = O.afinito_init(op, og, dtype(0.999), x0, retry_signs=signs)
    it = S.iterator(S.Finito(dtype, adaptive=True), dev(x0), F=dp, g=dg, N=N, ctx=ctx, stream=ciao.IndexStream(seed))
    st = next(iter(it))
    close(st.γ, rgam, dtype, scale={64: 200, 32: 140}, what="gamma_i after the random re-probe", scale64=100)
    close(st.av, rav, dtype, scale={64: 27, 32: 9.4}, what="av after the random re-probe", scale64=10)
    close(st.z, rz, dtype, scale={64: 28, 32: 9.5}, what="z after the random re-probe", scale64=13)
    assert abs(st.hat_γ - float(rhg)) <= 200 * float(np.finfo(dtype).eps) * float(rhg)
    assert float(st.γ.min()) > 0
    # the low-level contract: without a host the flagged samples carry gamma_i = -1 and the status is CIAO_ERR_UNSUPPORTED
    table = torch.empty((N, d), dtype=dev(x0).dtype, device="cuda")
    meta4 = torch.empty((N, 4, 4), dtype=dev(x0).dtype, device="cuda")
    hg = torch.empty(1, dtype=dev(x0).dtype, device="cuda")
    av, z = torch.empty(d, dtype=dev(x0).dtype, device="cuda"), torch.empty(d, dtype=dev(x0).dtype, device="cuda")
    ctx.afinito_init(dp, dg, 0.999, dev(x0), table, meta4, av, z, hg)
    with pytest.raises(ciao._lib.CiaoError) as e:
        ctx.synchronize()
    assert e.value.status == ciao._lib.ERR_UNSUPPORTED
    assert sorted(torch.nonzero(meta4[:, 0, 2] < 0).flatten().tolist()) == [3, 7, 8, 29]
    # and the steps run on from the resolved state exactly as the oracle's
    idx = ciao.IndexStream(5).rand_indices(N, 60)
    done, trials = ctx.afinito_steps(dp, dg, 0.999, 1e-9, idx, st.s, st.meta, st.av, st.z, st.hat_γ_dev)
    rdone, rhg2, rtrials = O.afinito_steps(op, og, dtype(0.999), dtype(1e-9), idx, rt, rg, rgam, rfi, rhg, rav, rz)
    assert done == rdone == 60
    if trials == rtrials:
        close(st.z, rz, dtype, scale={64: 210, 32: 120}, what="z after 60 steps from the re-probed init")


def _random_chain_cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    dmax = int(os.environ.get("CIAO_FUZZ_DMAX", "0"))   # a one-off hunt on long rows too (the several-workgroup chains): e.g. 20000
    for _ in range(n):
        N = int(rng.choice([2, 3, 7, 33, 100]))
        d = int(rng.choice([rng.integers(1, 70), rng.integers(70, 600), 2 * int(rng.integers(35, 300)), 4 * int(rng.integers(16, 700)),
                            rng.integers(600, 3000)]))
        if dmax > 4100 and rng.integers(0, 2):
            d = int(rng.integers(4097, dmax))
        dtype = [np.float64, np.float32][int(rng.integers(0, 2))]
        loss = ["ls", "logistic"][int(rng.integers(0, 2))]
        gk = ["zero", "l1", "box", "boxvec"][int(rng.integers(0, 4))]
        alg = ["svrg", "svrg_cached", "saga", "sag", "finito", "lfinito"][int(rng.integers(0, 6))]
        r = int(rng.choice([1, 1, 2, 5]))
        out.append((alg, N, d, dtype, loss, gk, min(r, N)))
    return out


# CIAO_FUZZ_CASES / CIAO_FUZZ_SEED: a longer one-off hunt with other seeds (the default 1000 cases with seed 77 are the suite's: the stated scales are 10 x the largest error over all of them)
@pytest.mark.parametrize("case", _random_chain_cases(int(os.environ.get("CIAO_FUZZ_CASES", "1000")), int(os.environ.get("CIAO_FUZZ_SEED", "77"))),
                         ids=lambda c: f"{c[0]}-N{c[1]}-d{c[2]}-{'f64' if c[3] == np.float64 else 'f32'}-{c[4]}-{c[5]}-r{c[6]}")
def test_random_chain_configurations(ctx, ciao, case):
    """Seeded random (algorithm, N, d, type, loss, g, batch) through the chain kernels -- every prox family (the IndBox clamp is its
    own version of each step group), single-wave and four-wave shapes, masked and exact rows, chunks and single elements --
    against the oracle on the same index stream."""
    import torch
    from oracle import twin as O
    alg, N, d, dtype, loss, gk, r = case
    A, b, x0 = P.synthetic(loss, N, d, dtype, seed=N * 31 + d)
    lam_f = float(N) if loss == "ls" else 1.0
    op, dp = make(loss, A, b, lam_f, dtype)
    og, dg = make_g(gk, dtype, d, lam=0.02)
    Li = (lam_f if loss == "ls" else 0.25) * np.sum(A.astype(np.float64) ** 2, axis=1) + 1e-12
    tdt = dev(x0).dtype
    st = ciao.IndexStream(N * 1000 + d)
    new = lambda: torch.empty(d, dtype=tdt, device="cuda")
    S = 5000
    # (iterates and Finito table rows: one rounding unit at the size of the operands -- test_random_shapes says why)
    osz = lambda ref: max(float(np.abs(np.asarray(ref)).max(initial=0.0)), float(np.abs(x0).max(initial=0.0)))
    if alg in ("svrg", "svrg_cached"):
        gamma = 1.0 / (7 * Li.max())
        av, z, zf, w = new(), new(), new(), new()
        ctx.svrg_init(dp, dev(x0), av, z, zf, w)
        rav, rz, rzf, rw = O.svrg_init(op, x0)
        for ep in range(2):
            idx = st.rand_indices(N, 3 * N + 5)
            ctx.svrg_iterate(dp, dg, gamma, idx, False, av, z, zf, w, reuse_rowdots=(alg == "svrg_cached"))
            O.svrg_iterate(op, og, dtype(gamma), idx, False, rav, rz, rzf, rw)
        close(zf, rzf, dtype, scale={64: 1100, 32: 1000}, what=f"random chain {alg} z_full ({ctx.last_kernel()})", scale64=840, size=osz(rzf))
        close(av, rav, dtype, scale={64: 1200, 32: 430}, what=f"random chain {alg} av", scale64=840)
    elif alg in ("saga", "sag"):
        gamma = 1.0 / ((16 if alg == "sag" else 3) * Li.max())
        table = torch.empty((N, d), dtype=tdt, device="cuda")
        av, z = new(), new()
        ctx.saga_init(dp, dg, gamma, dev(x0), table, av, z)
        rt, rav, rz = O.saga_init(op, og, dtype(gamma), x0)
        idx = st.rand_indices(N, 6 * N + 3)
        ctx.saga_steps(dp, dg, gamma, alg == "sag", idx, table, av, z)
        O.saga_steps(op, og, dtype(gamma), alg == "sag", idx, rt, rav, rz)
        close(z, rz, dtype, scale={64: 120, 32: 110}, what=f"random chain {alg} z ({ctx.last_kernel()})", scale64=840, size=osz(rz))
        close(table, rt, dtype, scale={64: 1100, 32: 1900}, what=f"random chain {alg} table", scale64=840)
    else:
        gam = (0.999 * N / Li).astype(dtype)
        dgam = dev(gam)
        hg = ctx.hat_gamma(dgam)
        nb = -(-N // r)
        static = [np.arange(r * j, min(r * j + r, N), dtype=np.int64) for j in range(nb)]
        ctx.set_option("chain_max_batch", 64)
        try:
            if alg == "finito":
                table = torch.empty((N, d), dtype=tdt, device="cuda")
                av, z = new(), new()
                rt, rav, rz, rhg = O.finito_init(op, og, gam, x0)
                ctx.finito_init(dp, dg, dgam, hg, dev(x0), table, av, z)
                batches = [st.sample_without_replacement(N, r) for _ in range(2 * nb + 3)]
                bptr = np.zeros(len(batches) + 1, np.int64)
                np.cumsum([len(x) for x in batches], out=bptr[1:])
                ctx.finito_steps(dp, dg, dgam, hg, bptr, np.concatenate(batches), table, av, z)
                O.finito_steps(op, og, gam, rhg, batches, rt, rav, rz)
                close(z, rz, dtype, scale={64: 230, 32: 220}, what=f"random chain finito z ({ctx.last_kernel()})", scale64=210, size=osz(rz))
                close(table, rt, dtype, scale={64: 220, 32: 210}, what="random chain finito table", scale64=200, size=osz(rt))
            else:
                av, z, zf = new(), new(), new()
                rav, rz, rzf, rhg = O.lfinito_init(op, gam, x0)
                ctx.lfinito_init(dp, hg, dev(x0), av, z, zf)
                for it in range(2):
                    order = np.arange(nb) if it == 0 else st.randperm(nb)
                    batches = [static[j] for j in order]
                    bptr = np.zeros(nb + 1, np.int64)
                    np.cumsum([len(x) for x in batches], out=bptr[1:])
                    ctx.lfinito_iterate(dp, dg, dgam, hg, bptr, np.concatenate(batches), av, z, zf)
                    O.lfinito_iterate(op, og, gam, rhg, batches, rav, rz, rzf)
                close(zf, rzf, dtype, scale={64: 310, 32: 250}, what=f"random chain lfinito z_full ({ctx.last_kernel()})", scale64=270, size=osz(rzf))
                close(av, rav, dtype, scale={64: 450, 32: 490}, what="random chain lfinito av", scale64=350)
        finally:
            ctx.set_option("chain_max_batch", -1)
    ctx.synchronize()

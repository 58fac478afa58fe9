"""Which kernel a chain call gets: the whole `last_kernel` string at the smallest shape that reaches each decision of the chain
dispatch (chain_launch.inc plan_chain: the LDS-DMA ring on one / four / eight waves, exact or masked; the wave-specialised SAGA
chain and its issuer count; the register ring E = 1 ... 32 on one wave or four; the several-workgroup and the any-length kernels;
the complex chains; the options that force a route), the names a chain batch records, and the UNSUPPORTED answers, which are
host-side statuses returned before any launch.

Six rows, five steps; the problems are built as tests/test_gpu_every_kernel.py builds them.  The results are held against the
oracle there: here only names, and bitwise equality between two routes to the same kernel.

The chain of svrg_iterate(..., reuse_rowdots=True) (cached row dots, algorithm 4) has no observable name: the full pass that closes
the iteration overwrites `last_kernel`.  Its cases pin that name and what the results allow: on rows that fall back to the register
ring the run is bitwise the one without the cache (the algorithm-0 kernel recomputes the dots)."""
import numpy as np
import pytest

import problems as P
from test_gpu_parity import dev, make, make_g
from test_gpu_every_kernel import _shard_table, _with

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
N, STEPS = 6, 5
IDX = np.array([3, 0, 3, 5, 1], dtype=np.int64)       # the same row met again two steps later
TY = {F64: "f64", F32: "f32"}


def run(ctx, alg, d, dtype=F64, opts=None, form="lists", sharded=False, cached=False):
    """Init + five steps of `alg` ("svrg", "saga", "finito", "lfinito") on a 6 x d least-squares problem
    -> (last_kernel, [state tensors after the call])."""
    import torch
    import ciaoalgorithms_jl_amd._lib as L
    A, b, x0 = P.synthetic("ls", N, d, dtype, seed=N * 31 + d)
    _, dp = make("ls", A, b, float(N), dtype)
    _, dg = make_g("l1", dtype, d, lam=0.02)
    Li = float(N) * np.sum(A.astype(np.float64) ** 2, axis=1) + 1e-12
    tdt = dev(x0).dtype
    new = lambda: torch.empty(d, dtype=tdt, device="cuda")
    cuts = [0, N // 3, N // 3, N]                     # three shards, the middle one empty
    for k, v in (opts or {}).items():
        ctx.set_option(k, v)
    try:
        if alg == "svrg":
            gamma = 1.0 / (7 * Li.max())
            av, z, zf, w = new(), new(), new(), new()
            ctx.svrg_init(dp, dev(x0), av, z, zf, w)
            state = [z, w]
            if sharded:
                ctx.set_shards(_shard_table(L, dp, N, cuts))
            try:
                if cached:
                    ctx.svrg_iterate(dp, dg, gamma, IDX, False, av, z, zf, w, reuse_rowdots=True)
                    state = [av, z, zf, w]
                else:
                    ctx.svrg_inner(dp, dg, gamma, IDX, av, z, zf, w)
            finally:
                if sharded:
                    ctx.set_shards(None)
        elif alg == "saga":
            gamma = 1.0 / (3 * Li.max())
            table = torch.empty((N, d), dtype=tdt, device="cuda")
            av, z = new(), new()
            ctx.saga_init(dp, dg, gamma, dev(x0), table, av, z)
            ctx.saga_steps(dp, dg, gamma, False, IDX, table, av, z)
            state = [table, av, z]
        else:
            dgam = dev((0.999 * N / Li).astype(dtype))
            hg = ctx.hat_gamma(dgam)
            ones = np.ones(STEPS, dtype=np.int64)     # batches of one sample
            if alg == "finito":
                table = torch.empty((N, d), dtype=tdt, device="cuda")
                av, z = new(), new()
                ctx.finito_init(dp, dg, dgam, hg, dev(x0), table, av, z)
                if form == "lists":
                    ctx.finito_steps(dp, dg, dgam, hg, np.arange(STEPS + 1), IDX, table, av, z)
                else:
                    ctx.finito_steps_blocks(dp, dg, dgam, hg, IDX, ones, table, av, z)
                state = [table, av, z]
            else:
                av, z, zf = new(), new(), new()
                ctx.lfinito_init(dp, hg, dev(x0), av, z, zf)
                if form == "lists":
                    ctx.lfinito_iterate(dp, dg, dgam, hg, np.arange(STEPS + 1), IDX, av, z, zf)
                else:
                    ctx.lfinito_iterate_blocks(dp, dg, dgam, hg, IDX, ones, av, z, zf)
                state = [av, z, zf]
        name = ctx.last_kernel()
        ctx.synchronize()
    finally:
        for k in (opts or {}):
            ctx.set_option(k, 0)
    return name, [t.clone() for t in state]


TAIL = " grid=1 block=%d steps=5"

# fp64 SVRG, default options: (d, options, the string)
RING = [
    (8, {}, "chain_dma_kernel<f64,J1,alg0,masked>" + TAIL % 64),
    (128, {}, "chain_dma_kernel<f64,J1,alg0>" + TAIL % 64),                # 1 KiB: one wave, one chunk per lane, exact
    (130, {}, "chain_dma_kernel<f64,J1,alg0,masked>" + TAIL % 64),         # two chunks per lane, reported by the row's 4 KiB class
    (256, {}, "chain_dma_kernel<f64,J1,alg0>" + TAIL % 64),                # 2 KiB: exact for the one-wave kernel
    (258, {}, "chain_dma_kernel<f64,J1,alg0,masked>" + TAIL % 256),
    (512, {}, "chain_dma_kernel<f64,J1,alg0>" + TAIL % 256),
    (514, {}, "chain_dma_kernel<f64,J2,alg0,masked>" + TAIL % 256),
    (1024, {}, "chain_dma_kernel<f64,J2,alg0>" + TAIL % 256),
    (1026, {}, "chain_dma_kernel<f64,J4,alg0,masked>" + TAIL % 256),
    (2048, {}, "chain_dma_kernel<f64,J4,alg0>" + TAIL % 256),
    (2050, {}, "chain_dma_kernel<f64,J8,alg0,masked>" + TAIL % 512),       # eight waves of four chunks per thread
    (4096, {}, "chain_dma_kernel<f64,J8,alg0>" + TAIL % 512),
    (4098, {}, "chain_wide_kernel<f64,E8,alg0> grid=3 block=256 steps=5"),
    (4098, {"chain_no_wide": 1}, "chain_big_kernel<f64,alg0>" + TAIL % 1024),
    (8, {"chain_four_waves": 1}, "chain_dma_kernel<f64,J1,alg0,masked>" + TAIL % 256),
]


@pytest.mark.parametrize("d,opts,want", RING, ids=[f"d{r[0]}" + "".join(f"-{k}" for k in r[1]) for r in RING])
def test_svrg_ring_wide_and_big_names(ctx, d, opts, want):
    assert run(ctx, "svrg", d, F64, opts)[0] == want


# rows with no 16-byte structure (or the ring switched off): (dtype, d, options, the string)
REG = [
    (F64, 7, {}, "chain_kernel<f64,E1,alg0,masked>" + TAIL % 64),
    (F64, 64, {"chain_no_dma": 1}, "chain_kernel<f64,E1,alg0,full>" + TAIL % 64),
    (F64, 65, {}, "chain_kernel<f64,E1,alg0,masked>" + TAIL % 256),
    (F64, 257, {}, "chain_kernel<f64,E4,alg0,masked>" + TAIL % 256),
    (F64, 1025, {}, "chain_kernel<f64,E8,alg0,masked>" + TAIL % 256),
    (F64, 2049, {}, "chain_kernel<f64,E16,alg0,masked>" + TAIL % 256),
    (F32, 4097, {}, "chain_kernel<f32,E32,alg0,masked>" + TAIL % 256),
    (F64, 7, {"chain_four_waves": 1}, "chain_kernel<f64,E1,alg0,masked>" + TAIL % 256),
]


@pytest.mark.parametrize("dtype,d,opts,want", REG, ids=[f"{TY[r[0]]}-d{r[1]}" + "".join(f"-{k}" for k in r[2]) for r in REG])
def test_svrg_register_ring_names(ctx, dtype, d, opts, want):
    assert run(ctx, "svrg", d, dtype, opts)[0] == want


SAGA = [
    (256, {}, "chain_dma_kernel<f64,J1,alg1>" + TAIL % 64),
    (258, {}, "chain_ws_kernel<f64,J1,alg1,masked,issuers2>" + TAIL % 448),
    (258, {"chain_ws_issuers": 1}, "chain_ws_kernel<f64,J1,alg1,masked,issuers1>" + TAIL % 384),
    (258, {"chain_no_ws": 1}, "chain_dma_kernel<f64,J1,alg1,masked>" + TAIL % 256),
]


@pytest.mark.parametrize("d,opts,want", SAGA, ids=[f"d{r[0]}" + "".join(f"-{k}" for k in r[1]) for r in SAGA])
def test_saga_names(ctx, d, opts, want):
    assert run(ctx, "saga", d, F64, opts)[0] == want


@pytest.mark.parametrize("alg,no", [("finito", 2), ("lfinito", 3)])
@pytest.mark.parametrize("d,kernel,block", [(8, "chain_dma_kernel<f64,J1,alg%d,masked>", 64), (7, "chain_kernel<f64,E1,alg%d,masked>", 64)],
                         ids=["ring", "register-ring"])
def test_finito_chains_by_lists_and_by_blocks(ctx, alg, no, d, kernel, block):
    """Batches of one sample as index lists and as row blocks: the same chain launch, bitwise the same results."""
    import torch
    want = kernel % no + TAIL % block
    k_lists, by_lists = run(ctx, alg, d, form="lists")
    k_blocks, by_blocks = run(ctx, alg, d, form="blocks")
    assert k_lists == want and k_blocks == want
    for a, b in zip(by_lists, by_blocks):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_cached_row_dots_svrg(ctx):
    """(see the module docstring: the chain's own name is not observable)"""
    import torch
    full_pass = "rows_small_kernel<f64,mode0,I8> grid=1 block=256"
    name, ring = run(ctx, "svrg", 8, cached=True)
    assert name == full_pass
    assert all(torch.isfinite(t).all() for t in ring)
    name7, reg = run(ctx, "svrg", 7, cached=True)
    assert name7 == full_pass
    # d = 7: the register ring holds no cached-dots instantiation; its algorithm-0 kernel recomputes a_i'z_full
    A, b, x0 = P.synthetic("ls", N, 7, F64, seed=N * 31 + 7)
    _, dp = make("ls", A, b, float(N), F64)
    _, dg = make_g("l1", F64, 7, lam=0.02)
    gamma = 1.0 / (7 * (float(N) * np.sum(A ** 2, axis=1) + 1e-12).max())
    av, z, zf, w = (torch.empty(7, dtype=torch.float64, device="cuda") for _ in range(4))
    ctx.svrg_init(dp, dev(x0), av, z, zf, w)
    ctx.svrg_iterate(dp, dg, gamma, IDX, False, av, z, zf, w, reuse_rowdots=False)
    ctx.synchronize()
    for a, b_ in zip(reg, (av, z, zf, w)):
        assert torch.equal(a, b_)


def run_zero(ctx, d, zero):
    """Five SVRG steps from a fixed random state on F = fill(Zero(), N), or on its twin: least squares on an all-zero A, b with
    lam = 0 -> (last_kernel, [z, w], the w it started from)."""
    import torch
    import ciaoalgorithms_jl_amd._lib as L
    from ciaoalgorithms_jl_amd.device import PackedF, ProxG
    rng = np.random.default_rng(d)
    av, z, zf, w = (dev(0.3 * rng.standard_normal(d)) for _ in range(4))
    w0 = w.clone()
    if zero:
        F = PackedF.zero(N, d, torch.float64)
    else:
        F = PackedF.least_squares(torch.zeros((N, d), dtype=torch.float64, device="cuda"), torch.zeros(N, dtype=torch.float64, device="cuda"), 0.0)
    ctx.svrg_inner(F, ProxG(L.PROX_L1, lam=0.02), 0.1, IDX, av, z, zf, w)
    name = ctx.last_kernel()
    ctx.synchronize()
    return name, [z, w], w0


@pytest.mark.parametrize("d,want", [(8, "chain_dma_kernel<f64,J1,alg0,masked>" + TAIL % 64), (7, "chain_kernel<f64,E1,alg0,masked>" + TAIL % 64)],
                         ids=["ring", "register-ring"])
def test_zero_loss_runs_the_least_squares_kernel_on_aliased_rows(ctx, d, want):
    """F = fill(Zero(), N): the names of least squares, the results of an all-zero A, b with lam = 0."""
    import torch
    k_zero, zero, w0 = run_zero(ctx, d, True)
    k_ls, ls, _ = run_zero(ctx, d, False)
    assert k_zero == want and k_ls == want
    for a, b in zip(zero, ls):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert not torch.equal(zero[1], w0)   # (the steps did something)


CPLX = [
    (np.complex128, 512, {}, "chain_cdma_kernel<f64,J2,alg0>" + TAIL % 256),           # 8 KiB rows
    (np.complex128, 128, {}, "chain_cdma_kernel<f64,J1,alg0,masked>" + TAIL % 256),    # 2 KiB
    (np.complex64, 3, {}, "chain_cplx_reg_kernel<f32,alg0,EP1>" + TAIL % 256),         # 24-byte rows: no 16-byte structure
    (np.complex64, 3, {"chain_big": 1}, "chain_cplx_kernel<f32,alg0>" + TAIL % 1024),
]


def run_complex(ctx, ctype, n, opts=None):
    """Five SVRG steps on a 6 x n complex least-squares problem -> (last_kernel, [z, w])."""
    import torch
    from oracle import twin as O
    from test_gpu_complex import cmake, cg
    A, b, x0 = P.synthetic_complex(N, n, ctype, seed=n)
    _, dp = cmake(A, b, float(N))
    _, dg = cg(0.01)
    gamma = 1.0 / (7 * float(N) * np.max(np.sum(np.abs(A.astype(np.complex128)) ** 2, axis=1)))
    xp = O.as_pairs(x0)
    av, z, zf, w = (torch.empty(2 * n, dtype=dev(xp).dtype, device="cuda") for _ in range(4))
    ctx.svrg_init(dp, dev(xp), av, z, zf, w)
    name = _with(ctx, opts or {}, lambda: (ctx.svrg_inner(dp, dg, gamma, IDX, av, z, zf, w), ctx.last_kernel())[1])
    ctx.synchronize()
    return name, [z, w]


@pytest.mark.parametrize("ctype,n,opts,want", CPLX, ids=[f"{np.dtype(r[0]).name}-n{r[1]}" + "".join(f"-{k}" for k in r[2]) for r in CPLX])
def test_complex_chain_names(ctx, ctype, n, opts, want):
    import torch
    name, (z, w) = run_complex(ctx, ctype, n, opts)
    assert name == want and torch.isfinite(w).all()


def _two_svrg_chains(ctx, d):
    import torch
    A, b, x0 = P.synthetic("ls", N, d, F64, seed=N * 31 + d)
    _, dp = make("ls", A, b, float(N), F64)
    _, dg = make_g("l1", F64, d, lam=0.02)
    gamma = 1.0 / (7 * (float(N) * np.sum(A ** 2, axis=1) + 1e-12).max())
    chains = []
    for k in range(2):
        av, z, zf, w = (torch.empty(d, dtype=torch.float64, device="cuda") for _ in range(4))
        ctx.svrg_init(dp, dev(x0), av, z, zf, w)
        chains.append((dp, dg, gamma * (k + 1), IDX, av, z, zf, w))
    ctx.synchronize()
    return chains


def test_a_chain_batch_reports_the_first_recorded_name(ctx):
    import torch
    chains = _two_svrg_chains(ctx, 8)
    with ctx.chain_batch():
        for c in chains:
            ctx.svrg_inner(*c)
    ctx.synchronize()
    assert ctx.last_kernel() == "chain batch: 2 chains in 1 launch(es); first: chain_dma_kernel<f64,J1,alg0,masked>" + TAIL % 64 + " grid=2"
    alone = _two_svrg_chains(ctx, 8)
    for c in alone:
        ctx.svrg_inner(*c)
    ctx.synchronize()
    for c, s in zip(chains, alone):
        assert torch.equal(c[5], s[5]) and torch.equal(c[7], s[7])


def test_a_chain_batch_refuses_rows_that_are_not_the_ring(ctx):
    import ciaoalgorithms_jl_amd._lib as L
    c = _two_svrg_chains(ctx, 7)[0]
    with pytest.raises(L.CiaoError) as ei:
        with ctx.chain_batch():
            ctx.svrg_inner(*c)
    assert ei.value.status == L.ERR_UNSUPPORTED and "a chain batch takes" in str(ei.value)
    ctx.synchronize()


def test_shard_table_names_and_refusal(ctx):
    import ciaoalgorithms_jl_amd._lib as L
    assert run(ctx, "svrg", 8, sharded=True)[0] == "chain_dma_kernel<f64,J1,alg0,masked,sharded>" + TAIL % 256
    with pytest.raises(L.CiaoError) as ei:
        run(ctx, "svrg", 7, sharded=True)
    assert ei.value.status == L.ERR_UNSUPPORTED and "whole 16-byte chunks" in str(ei.value)
    ctx.synchronize()

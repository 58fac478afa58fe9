"""Which kernel a ProShI call gets, on what grid: the whole `last_kernel` string at the smallest shape that reaches each plan
decision of the ProShI dispatch (rows_launch.inc: dense / vectorised J = 1, 2, 4, 8 / generic on four waves or one; the
coordinate-parallel chain), the UNSUPPORTED answer beyond the generic kernel's LDS, and which of the paths record timing events.

The problems are built as tests/test_gpu_parity.py::test_proshi_steps builds them.  No grid here reaches a cap that depends on
the number of CUs (N = 3 agents)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Case:
    """PackedSepQuad + ProxG + stepsizes + state tensors for N agents of d coordinates (Q of N x d x d when dense)."""

    def __init__(self, N, d, dtype, dense=False):
        import torch
        from ciaoalgorithms_jl_amd.device import PackedSepQuad, ProxG
        import ciaoalgorithms_jl_amd._lib as L
        rng = np.random.default_rng(N + d)
        Q = rng.uniform(-1.0, 3.0, (N, d, d) if dense else (N, d)).astype(dtype)
        q = rng.standard_normal((N, d)).astype(dtype)
        eta, lo, hi = 3.0 * N, -2.0, 2.0
        self.x0 = dev((0.5 * rng.standard_normal(d)).astype(dtype))
        self.gam = dev((0.999 * N / (np.abs(Q.reshape(N, -1)).max(axis=1) * (d if dense else 1) + eta)).astype(dtype))
        self.f = PackedSepQuad(dev(Q), dev(q), eta, lo, hi)
        self.g = ProxG(L.PROX_BOX, lo=-float("inf"), hi_vec=dev(np.linspace(0.5, 1.5, d).astype(dtype)))
        tdt = self.x0.dtype
        self.table = torch.empty((N, d), dtype=tdt, device="cuda")
        self.av, self.z = torch.empty(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda")
        self.hg = torch.empty(1, dtype=tdt, device="cuda")

    def init(self, ctx):
        ctx.proshi_init(self.f, self.g, self.gam, self.x0, self.table, self.av, self.z, self.hg)

    def steps(self, ctx, batches):
        r = len(batches[0])
        bptr = np.arange(len(batches) + 1, dtype=np.int64) * r
        ctx.proshi_steps(self.f, self.g, self.gam, float(self.hg.item()), bptr, np.concatenate(batches).astype(np.int64), self.table,
                         self.av, self.z)

    def state(self):
        return [t.clone() for t in (self.table, self.av, self.z)]


def init_then_one_parallel_step(ctx, c):
    """(last_kernel after proshi_init, last_kernel after one batch of all three agents with the chain switched off)"""
    c.init(ctx)
    k_init = ctx.last_kernel()
    ctx.set_option("proshi_chain_max_batch", 0)
    try:
        c.steps(ctx, [np.array([2, 0, 1])])
    finally:
        ctx.set_option("proshi_chain_max_batch", -1)
    k_step = ctx.last_kernel()
    ctx.synchronize()
    return k_init, k_step


# (dtype, d, dense, the proshi_init string with %s for the type)
PLANS = [
    (np.float64, 2, False, "proshi_vec_kernel<%s,init,J1> grid=3 block=256"),
    (np.float32, 4, False, "proshi_vec_kernel<%s,init,J1> grid=3 block=256"),
    (np.float64, 514, False, "proshi_vec_kernel<%s,init,J2> grid=3 block=256"),      # 257 chunks
    (np.float64, 1026, False, "proshi_vec_kernel<%s,init,J4> grid=3 block=256"),
    (np.float64, 2050, False, "proshi_vec_kernel<%s,init,J8> grid=3 block=256"),
    (np.float64, 4096, False, "proshi_vec_kernel<%s,init,J8> grid=3 block=256"),     # the last vectorised shape
    (np.float64, 3, False, "proshi_rows_kernel<%s,init,NW4> grid=1 block=256"),
    (np.float32, 3, False, "proshi_rows_kernel<%s,init,NW4> grid=1 block=256"),
    (np.float64, 4098, False, "proshi_rows_kernel<%s,init,NW1> grid=3 block=64"),    # 5 rows exceed 144 KiB
    (np.float64, 2, True, "proshi_dense_kernel<%s,init> grid=3 block=256"),
]


@pytest.mark.parametrize("dtype,d,dense,want", PLANS, ids=[f"{np.dtype(p[0]).name}-d{p[1]}{'-dense' if p[2] else ''}" for p in PLANS])
def test_proshi_plan_names(ctx, ciao, dtype, d, dense, want):
    want = want % ("f64" if dtype == np.float64 else "f32")
    k_init, k_step = init_then_one_parallel_step(ctx, Case(3, d, dtype, dense))
    assert k_init == want
    assert k_step == want.replace("init", "step")


def test_proshi_force_generic_takes_the_four_wave_kernel(ctx, ciao):
    ctx.set_option("force_generic", 1)
    try:
        k_init, k_step = init_then_one_parallel_step(ctx, Case(3, 2, np.float64))
    finally:
        ctx.set_option("force_generic", 0)
    assert k_init == "proshi_rows_kernel<f64,init,NW4> grid=1 block=256"
    assert k_step == "proshi_rows_kernel<f64,step,NW4> grid=1 block=256"


def test_proshi_chain_name_lists_and_blocks(ctx, ciao):
    """Six batches of two agents: one chain launch, by index lists and by row blocks, with bitwise equal results."""
    import torch
    want = "proshi_chain_kernel<f64> grid=1 block=256 visits=12 batch=2"
    c = Case(5, 7, np.float64)
    c.init(ctx)
    start = c.state()
    c.steps(ctx, [np.array([0, 1]), np.array([2, 3])] * 3)
    assert ctx.last_kernel() == want
    ctx.synchronize()
    by_lists = c.state()
    for t, s in zip((c.table, c.av, c.z), start):
        t.copy_(s)
    ctx.proshi_steps_blocks(c.f, c.g, c.gam, float(c.hg.item()), [0, 2, 0, 2, 0, 2], [2] * 6, c.table, c.av, c.z)
    assert ctx.last_kernel() == want
    ctx.synchronize()
    for name, a, b in zip(("table", "av", "z"), by_lists, c.state()):
        assert torch.equal(a, b), name
    assert not torch.equal(by_lists[0], start[0])   # (the steps did something)


def test_proshi_beyond_the_generic_lds_is_unsupported(ctx, ciao):
    """2 * d * 8 bytes > 144 KiB on the generic kernel (force_generic: the vectorised kernel does not take d = 9217 either way)."""
    import ciaoalgorithms_jl_amd._lib as L
    c = Case(2, 9217, np.float64)
    ctx.set_option("force_generic", 1)
    try:
        with pytest.raises(L.CiaoError) as ei:
            c.init(ctx)
    finally:
        ctx.set_option("force_generic", 0)
    assert ei.value.status == L.ERR_UNSUPPORTED
    assert "144 KiB of LDS" in str(ei.value) and "d=9217" in str(ei.value)
    ctx.synchronize()


def test_proshi_timing_events_per_path(ctx, ciao):
    """The vectorised (and dense) launches record a timing event pair; the generic kernel and the chain record none."""
    vec, gen, chain = Case(3, 2, np.float64), Case(3, 3, np.float64), Case(5, 7, np.float64)
    chain.init(ctx)
    ctx.timing_enable(1)
    try:
        ctx.timing_read()
        vec.init(ctx)
        assert "proshi_vec_kernel" in ctx.last_kernel()
        assert ctx.timing_read()[1] == 1
        gen.init(ctx)
        assert "proshi_rows_kernel" in ctx.last_kernel()
        assert ctx.timing_read()[1] == 0
        chain.steps(ctx, [np.array([0, 1]), np.array([2, 3])] * 3)
        assert "proshi_chain_kernel" in ctx.last_kernel()
        assert ctx.timing_read()[1] == 0
    finally:
        ctx.timing_enable(0)
    ctx.synchronize()

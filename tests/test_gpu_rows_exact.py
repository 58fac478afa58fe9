"""The rows kernels and finalize_kernel held to EXACT sums (tests/rows_exact.py: lattice data on which every order of addition gives the
same bits; tests/test_rows_exact_host.py for the method itself), at every trip count of their persistent loops and every partial count
finalize_kernel's structure turns on.  No tolerance in this file: every comparison is on integer views.

  a. every family (rows_exact.CASES), the five modes (GRAD with the objective's extra scalar and -- through ciao_row_dots, the same sweep
     with rowdot_out set -- the row dots it stores per row, SAGA_INIT, FINITO_INIT, FINITO_BATCH and --
     through ciao_lfinito_iterate -- GRAD2; the batches as index lists and as row blocks off row 0), with `sweep_grid` 1, 2, 3 and the
     plan's own grid: the classifier (rows_exact.classify, from the launcher's report) must see an idle worker, 1, 2, 3 and >= 5 trips,
     two trip counts in one launch and a short last group / tile / R-row iteration -- asserted, so a changed plan fails instead of passing
     on fewer trips; at ld = d and, where the family takes it, at a poisoned ld = d + 2 VEC; the logistic loss at x = 0;
  b. finalize_kernel alone: 1 .. 1025 partials (rows_exact.PARTIAL_COUNTS) of a d that is whole 128-byte lines and of d = 257;
  c. before every test one sweep with b all NaN on a larger d with 1500 partials leaves NaN all over the context's workspace (partials,
     extra scalars, the raw sum): the exact calls after it must not see any of it;
  d. rows_long_kernel: the occupancy cache by element type (a context that ran the other type first plans what a fresh one plans), and
     Finito / LFinito batches that wrap the mailbox ring (8 rows a cluster).

Every output sits in a guarded buffer (tests/layouts.py); after every call the guards, the inputs and the outputs' NaN-freeness are
checked, and every entry point is called twice from the same state: the second call must give the same bits."""
import re

import numpy as np
import pytest

import rows_exact as X
from layouts import Guarded, bits, has_poison, poison_bits

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
BOTH = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]


@pytest.fixture(scope="module")
def num_cu(ctx):
    import torch
    return int(torch.cuda.get_device_properties(ctx.device).multi_processor_count)


@pytest.fixture(scope="module")
def pollute(ctx):
    """part c: -> pollute(dtype): one GRAD sweep whose targets are all NaN (ordinary input: its result is NaN, and so is every partial
    d-vector, extra scalar and raw sum it leaves in the context's workspace), 1500 rows of 1200 VEC elements, a workgroup and a partial per row"""
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    kept = {}

    def run(dtype):
        if dtype not in kept:
            d = 1200 * X.vec_of(dtype)
            tdt = torch.float64 if dtype == F64 else torch.float32
            A = torch.ones((1500, d), dtype=tdt, device="cuda")
            b = torch.full((1500,), float("nan"), dtype=tdt, device="cuda")
            kept[dtype] = (PackedF.least_squares(A, b, 1.0), torch.ones(d, dtype=tdt, device="cuda"), torch.empty(d, dtype=tdt, device="cuda"),
                           torch.zeros(3, dtype=torch.float64, device="cuda"))
        F, x, av, obj = kept[dtype]
        ctx.set_monitor(None, obj)
        try:
            with Options(ctx, split_blocks_per_cu=8):            # min(1500 rows, 8 workgroups a CU): beyond finalize's 1025 partials of part b
                ctx.full_gradient(F, x, av)
        finally:
            ctx.set_monitor(None, None)
        c = X.classify(ctx.last_kernel(), 1500, F.d)
        assert c["parts"] >= max(X.PARTIAL_COUNTS) and bool(torch.isnan(av).all()) and bool(torch.isnan(obj[1])), ctx.last_kernel()

    return run


class Options:
    """library options for a block, put back whatever happens"""

    def __init__(self, ctx, **opts):
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.ctx.set_option(k, X.OPTION_DEFAULTS[k])


def same_bits(t, want):
    import torch
    return torch.equal(bits(t.contiguous()), bits(torch.from_numpy(np.ascontiguousarray(want)).to(t.device)))


def repoison(g):
    bits(g.flat).fill_(poison_bits(g.flat.dtype))


class Runner:
    """One problem on the device.  call(): an entry point twice from the same state, with every check of the module's docstring; the
    launch report goes to `seen` with the rows it covered."""

    def __init__(self, ctx, case, P, dtype, padded):
        import ciaoalgorithms_jl_amd._lib as L
        from ciaoalgorithms_jl_amd.device import PackedF, ProxG
        self.ctx, self.case, self.P, self.dtype, self.padded, self.seen = ctx, case, P, dtype, padded, []
        self.PackedF = PackedF
        ld = P.d + 2 * X.vec_of(dtype) if padded else P.d
        self.kind = L.LOSS_LS if P.loss == "ls" else L.LOSS_LOGISTIC
        c = lambda a: X.lossless(a, dtype)
        G = lambda a, name, **kw: Guarded(c(a), device="cuda", name=name, **kw)
        self.A, self.b, self.b2 = G(P.A, "A", ld=ld), G(P.b, "b"), G(P.b2, "b (LFinito)")
        self.gam, self.x0 = G(P.gam, "gam"), G(P.x0, "x0")
        self.g_finito, self.g_saga = ProxG(L.PROX_L1, lam=P.lam_g), ProxG(L.PROX_L1, lam=P.saga_lam_g)
        self.inputs = [self.A, self.b, self.b2, self.gam, self.x0]

    def F(self, n=None, lfinito=False):
        b = self.b2 if lfinito else self.b
        n = self.P.Np if n is None else n
        return self.PackedF(self.kind, self.A.view[:n], b.view[:n], self.P.lam, N_total=self.P.Nt)

    def out(self, name, shape):
        return Guarded(shape=shape, dtype=self.dtype, device="cuda", name=name)

    def state(self, a, name):
        return Guarded(X.lossless(a, self.dtype), device="cuda", name=name)

    def call(self, mode, n, grid, fn, outs, inputs=(), reset=None, scalar=None):
        """outs: {name: (guarded buffer, expected float64 array)}; reset(): put the call's in/out state back; scalar: () -> (got, want)"""
        what = f"{self.case.name} {self.dtype.__name__} {self.P.loss} {mode} n={n} sweep_grid={grid}{' padded' if self.padded else ''}"
        family = self.case.family(mode, self.dtype, self.padded)
        for rep in range(2):
            if rep:
                reset()
            fn()
            report = self.ctx.last_kernel()
            assert re.search(family, report), f"{what}: the plan gives {family!r}, the launcher reports {report!r}"
            for g, _ in outs.values():
                g.check_outside(what)
            for g in list(inputs) + self.inputs:
                g.check_outside(what)
                g.check_unchanged(what)
            for name, (g, want) in outs.items():
                assert not has_poison(g.view), f"{what}, call {rep}: NaN in {name} ({report})"
                assert same_bits(g.view, X.lossless(want, self.dtype)), f"{what}, call {rep}: {name} differs from the exact result ({report})"
            if scalar is not None:
                got, want = scalar()
                assert got == want, f"{what}, call {rep}: the extra scalar gives {got!r}, exactly {want!r} ({report})"
        c = X.classify(report, n, self.P.d)
        if grid:
            assert c["grid"] == grid, f"{what}: asked for {grid} workgroups ({report})"
        if self.case.kind not in ("split", "long"):
            assert c["workers"] == c["grid"] * self.case.wpb(self.dtype) and c["unit"] == self.case.unit(self.dtype), (what, report)
        self.seen.append(c)

    def run(self, mode, n, grid, want):
        import torch
        P, ctx, d = self.P, self.ctx, self.P.d
        if mode == "grad":
            av, obj = self.out("av", (d,)), torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
            F = self.F(n)

            def fn():
                if P.loss == "ls":
                    ctx.set_monitor(None, obj)
                try:
                    ctx.full_gradient(F, self.x0.view, av.view)
                finally:
                    ctx.set_monitor(None, None)

            def reset():
                repoison(av)
                obj.fill_(float("nan"))

            self.call(mode, n, grid, fn, {"av": (av, want["av"])}, reset=reset,
                      scalar=(lambda: (float(obj[1]), float(want["obj"]))) if P.loss == "ls" else None)
            # the row dots the same sweep stores per row (rowdot_out: what it caches for the SVRG chain, and ciao_row_dots' output)
            dots = self.out("row dots", (n,))
            self.call(mode, n, grid, lambda: ctx.row_dots(F, self.x0.view, out=dots.view), {"row dots": (dots, want["dots"])},
                      reset=lambda: repoison(dots))
        elif mode in ("saga_init", "finito_init"):
            table, av, z = self.out("table", (n, d)), self.out("av", (d,)), self.out("z", (d,))
            F, gam = self.F(n), self.state(P.gam[:n], "gam (the sweep's rows)")
            if mode == "saga_init":
                fn = lambda: ctx.saga_init(F, self.g_saga, P.saga_gamma, self.x0.view, table.view, av.view, z.view)
            else:
                fn = lambda: ctx.finito_init(F, self.g_finito, gam.view, P.hg, self.x0.view, table.view, av.view, z.view)
            self.call(mode, n, grid, fn, {k: (g, want[k]) for k, g in (("table", table), ("av", av), ("z", z))}, inputs=[gam],
                      reset=lambda: [repoison(g) for g in (table, av, z)])
        else:
            lists = mode.endswith("lists")
            rows = X.batch_rows(P, n, lists)
            idx = Guarded(rows, device="cuda", name="index list")
            bptr, first, length = np.array([0, n], np.int64), np.array([X.ROW0], np.int64), np.array([n], np.int64)
            av = self.state(P.av, "av")
            if mode.startswith("finito"):
                F, table, z = self.F(), self.state(P.start_table(), "table"), self.state(P.z, "z")
                if lists:
                    fn = lambda: ctx.finito_steps(F, self.g_finito, self.gam.view, P.hg, bptr, idx.view, table.view, av.view, z.view)
                else:
                    fn = lambda: ctx.finito_steps_blocks(F, self.g_finito, self.gam.view, P.hg, first, length, table.view, av.view, z.view)
                start = [(g, g.view.clone()) for g in (table, av, z)]
                self.call(mode, n, grid, fn, {k: (g, want[k]) for k, g in (("table", table), ("av", av), ("z", z))}, inputs=[idx],
                          reset=lambda: [g.view.copy_(t) for g, t in start])
            else:
                F, z, zf = self.F(lfinito=True), self.out("z", (d,)), self.out("z_full", (d,))
                if lists:
                    fn = lambda: ctx.lfinito_iterate(F, self.g_finito, self.gam.view, P.hg, bptr, idx.view, av.view, z.view, zf.view)
                else:
                    fn = lambda: ctx.lfinito_iterate_blocks(F, self.g_finito, self.gam.view, P.hg, first, length, av.view, z.view, zf.view)
                start = av.view.clone()
                self.call(mode, n, grid, fn, {"av": (av, want["av"]), "z": (z, want["z"]), "z_full": (zf, want["zf"])}, inputs=[idx],
                          reset=lambda: (av.view.copy_(start), repoison(z), repoison(zf)))


# ---- a. every family, five modes, every trip class -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.name)
def test_every_family_at_every_trip_class_exactly(ctx, ciao, num_cu, pollute, case, dtype):
    pollute(dtype)
    launches = case.launches(dtype, num_cu)
    deep = max((n for n, g in launches if g == 1), default=launches[-1][0])      # the >= 5-trip launch: also padded, and the logistic leg's
    B, seen, refs = X.Bounds(), [], {}
    P = case.problem(dtype, num_cu)
    assert X.vec_of(dtype) * np.dtype(dtype).itemsize == 16 and P.Np <= 4100
    with Options(ctx, chain_max_batch=0, **case.opts):
        for padded in (False, True) if case.pad else (False,):
            R = Runner(ctx, case, P, dtype, padded)
            for n, grid in (launches if not padded else [(deep, 1 if case.kind != "long" else 0)]):
                with Options(ctx, sweep_grid=grid):
                    for mode in case.modes:
                        if (mode, n) not in refs:
                            refs[mode, n] = X.reference(P, mode, n, B)
                        R.run(mode, n, grid, refs[mode, n])
            seen += R.seen
        if case.logistic:
            Pl = case.problem(dtype, num_cu, "logistic")
            R = Runner(ctx, case, Pl, dtype, False)
            with Options(ctx, sweep_grid=1 if case.kind != "long" else 0):
                for mode in case.modes:
                    if not mode.startswith("lfinito"):
                        R.run(mode, deep, 1 if case.kind != "long" else 0, X.reference(Pl, mode, deep, B))
            seen += R.seen
    ctx.synchronize()
    assert B.worst() < X.LIMIT_BITS, sorted(B.bits.items(), key=lambda kv: -kv[1])[:3]
    reached = set().union(*(X.classes(c) for c in seen))
    need = set().union(*(X.required(c) for c in seen))
    assert need <= reached, f"{case.name} on {num_cu} compute units: its launches never reach {sorted(need - reached)}"
    assert {c["family"] for c in seen} == {case.kind}, {c["family"] for c in seen}


# ---- b. finalize_kernel alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("name,dof,family,opts", X.FINALIZE_SHAPES, ids=[s[0] for s in X.FINALIZE_SHAPES])
def test_finalize_at_every_partial_count_exactly(ctx, ciao, pollute, name, dof, family, opts, dtype):
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    pollute(dtype)
    d, n = dof(X.vec_of(dtype)), X.FINALIZE_ROWS
    P = X.finalize_problem(d)
    B = X.Bounds()
    want = X.grad(P, n, B)
    assert B.worst() < X.LIMIT_BITS
    GA, Gb, Gx = (Guarded(X.lossless(a, dtype), device="cuda", name=nm) for a, nm in ((P.A, "A"), (P.b, "b"), (P.x0, "x0")))
    F = PackedF.least_squares(GA.view, Gb.view, P.lam, N_total=P.Nt)
    av, obj = Guarded(shape=(d,), dtype=dtype, device="cuda", name="av"), torch.empty(3, dtype=torch.float64, device="cuda")
    dots = Guarded(shape=(n,), dtype=dtype, device="cuda", name="row dots")
    counts = []
    with Options(ctx, **opts):
        for parts in X.PARTIAL_COUNTS:
            with Options(ctx, sweep_grid=parts):
                for rep in range(2):
                    repoison(av)
                    obj.fill_(float("nan"))
                    ctx.set_monitor(None, obj)
                    try:
                        ctx.full_gradient(F, Gx.view, av.view)
                    finally:
                        ctx.set_monitor(None, None)
                    report = ctx.last_kernel()
                    what = f"{name} {dtype.__name__}, {parts} partials, call {rep} ({report})"
                    c = X.classify(report, n, d)
                    assert re.search(family, report) and c["grid"] == parts and c["parts"] == parts, what
                    av.check_outside(what)
                    for g in (GA, Gb, Gx):
                        g.check_unchanged(what)
                    assert not has_poison(av.view), what
                    assert same_bits(av.view, X.lossless(want["av"], dtype)), f"{what}: av differs from the exact result"
                    assert float(obj[1]) == float(want["obj"]), f"{what}: the extra scalar gives {float(obj[1])!r}, exactly {float(want['obj'])!r}"
                repoison(dots)                                                # the per-row stores of the same sweep, on this grid
                ctx.row_dots(F, Gx.view, out=dots.view)
                assert re.search(family, ctx.last_kernel()) and X.classify(ctx.last_kernel(), n, d)["grid"] == parts, ctx.last_kernel()
                dots.check_outside(what)
                assert same_bits(dots.view, X.lossless(want["dots"], dtype)), f"{what}: the row dots differ from the exact result"
            counts.append(c["parts"])
    assert tuple(counts) == X.PARTIAL_COUNTS
    ctx.synchronize()


# ---- d. rows_long_kernel: the occupancy cache, the mailbox ring -----------------------------------------------------------------------------------
def test_long_rows_plan_does_not_depend_on_the_type_a_context_ran_first(ciao, num_cu):
    """long_j = 4, the sweep and the two inits (modes 0, 2, 3; the cache is per mode): a context that ran one type first reports for the
    other exactly the segments, clusters and grid a fresh context reports, and every result is exact.  The test covers the cache only
    while the two types' kernels differ in resident workgroups in at least one of these modes (three fp32 against two fp64 a CU when
    this was written): that is asserted, so that it cannot start passing on nothing."""
    from ciaoalgorithms_jl_amd.device import Context
    case, n, plans = X.CASE_BY_NAME["long_j4"], 200, {}
    want = {(dt, m): X.reference(case.problem(dt, num_cu), m, n, X.Bounds()) for dt in (F64, F32) for m in X.SWEEPS}

    def sweeps(c, dtype):
        R, out = Runner(c, case, case.problem(dtype, num_cu), dtype, False), []
        for mode in X.SWEEPS:
            R.run(mode, n, 0, want[dtype, mode])
            out.append(re.search(r"segments=\d+ clusters=\d+ grid=\d+", c.last_kernel()).group(0))
        return out

    for order in ((F64,), (F32,), (F32, F64), (F64, F32)):
        c = Context(0)
        try:
            c.set_option("long_j", 4)
            got = [sweeps(c, dt) for dt in order]
            c.synchronize()
        finally:
            c.close()
        if len(order) == 1:
            plans[order[0]] = got[0]
        else:
            assert got == [plans[dt] for dt in order], f"{[dt.__name__ for dt in order]}: {got}, fresh contexts plan {plans}"
    assert plans[F64] != plans[F32], f"both types plan {plans[F64]}: their occupancies agree in every mode, and this test holds nothing"


@pytest.mark.parametrize("dtype", BOTH)
def test_long_rows_batches_that_wrap_the_mailbox_ring(ctx, ciao, num_cu, pollute, dtype):
    """Finito and LFinito batches of 400 long rows on a table of 512, one workgroup a CU: every cluster takes five rows and more, so the
    four mailbox buffers are reused and, on the 16 KiB segments (J = 4: the total collected one row late), the tail collect follows the
    loop's last one."""
    pollute(dtype)
    case = X.CASE_BY_NAME["long_j4"]
    P = X.Problem(512, case.d(dtype), seed=5)
    B = X.Bounds()
    with Options(ctx, chain_max_batch=0, split_blocks_per_cu=1, long_j=4):
        R = Runner(ctx, case, P, dtype, False)
        for mode in X.BATCHES:
            R.run(mode, 400, 0, X.reference(P, mode, 400, B))
    ctx.synchronize()
    assert B.worst() < X.LIMIT_BITS
    assert all(c["family"] == "long" and min(c["trips"]) >= 5 for c in R.seen), R.seen

"""Every kernel family on rows beyond 2^31 and 2^32 elements (tests/far_rows.py has the method).

The matrix is a view of one zeroed 17.4 GB buffer per type (fp32: 2^32 + 2^26 elements, fp64: 2^31 + 2^25) with K <= 16 marked rows of
small integers around every boundary the view crosses: byte 2^31, byte 2^32, element 2^31 and -- fp32 -- element 2^32; at d = 2 the row
index itself passes 2^31.  Dense views (ld = d) and strided ones (5, 65, 200 rows at a stride of up to 3.5 GB) reach the address
expressions of each family; the family is asserted from ctx.last_kernel() in every case.  The reference is the oracle, or an int64 /
float64 restatement, on the gathered rows with N_total = N: sweeps, inits and chains through test_gpu_parity.close under the scales of
far_rows.SCALES (taken from existing call sites, never larger), the statistics passes in bits.  Row-wise outputs too large to copy are
checked on the device: the marked rows against the reference, everything else by count.  tests/test_far_rows_host.py shows that every
reference here moves by more than the tolerance when a marked row is dropped or read through a wrapped offset.

Memory: the matrix and ONE second buffer of its size (the table, the scaled matrix, b and the row dots or the row norms at d = 2), 17.4 GB
each and allocated once per type, plus vectors of N elements (b, labels, the stepsizes, row dots: under 1.1 GB together, d = 50): every case
asserts that its tensors stay within 36 GB at once (torch.cuda.max_memory_allocated); the library's own workspaces (partial sums, the Gram
tiles: 0.23 GB) come on top.  The one case that needs room for something else -- the N row dots the library keeps
behind an svrg_init at d = 2, 8.7 GB -- runs before the second buffer exists (far_rows.Buffers.drop_second otherwise): 34.9 GB.  A case is
skipped only where the device has less free memory than what it is about to allocate plus 4 GB; the skip states both figures."""
import numpy as np
import pytest

import far_rows as FR
from test_gpu_parity import BASELINE_EPS, close

pytestmark = pytest.mark.gpu

CASES = [pytest.param(v, op, id=f"{v.id}-{op}") for dt in (FR.F32, FR.F64) for v in FR.views(dt).values() for op in FR.ops_of(v)]
KERNELS = []                                           # (case, call, ctx.last_kernel()) of every launch report a case asserted


@pytest.fixture(scope="module")
def far():
    import torch
    b = FR.Buffers()
    torch.cuda.reset_peak_memory_stats()
    yield b
    b.release()
    torch.cuda.empty_cache()
    print(f"far rows: at most {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB of tensors at once (the library's workspaces come on top)")


def tdtype(view):
    import torch
    return torch.float64 if view.dtype == FR.F64 else torch.float32


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def kernel(ctx, view, call, *families):
    """the launch report, held to the families the call is there to reach"""
    k = ctx.last_kernel()
    KERNELS.append((view.id, call, k))
    assert any(f in k for f in families), f"{view.id} {call}: {k} is none of {families}"
    return k


def targets(view, data, loss):
    """the device vector of targets (zero off the marked rows) or labels (+1 off them); complex: the (re, im) pairs of N targets"""
    import torch
    if view.complex:
        t = torch.zeros(2 * view.N, dtype=tdtype(view), device="cuda")
        for r, v in zip(data.rows, data.b):
            t[2 * int(r):2 * int(r) + 2] = dev(v)
        return t
    return FR.sparse_vector(view.N, data, data.targets(loss), 1.0 if loss == "logistic" else 0.0, tdtype(view))


def problem(view, A, data, loss, lam=1.0, b=None):
    import ciaoalgorithms_jl_amd._lib as L
    from ciaoalgorithms_jl_amd.device import PackedF
    kind = L.LOSS_LS_COMPLEX if view.complex else {"ls": L.LOSS_LS, "logistic": L.LOSS_LOGISTIC}[loss]
    F = PackedF(kind, A, targets(view, data, loss) if b is None else b, lam)
    assert F.N == view.N and F.ld == view.ld and F.d == view.d
    return F


def prox(kind):
    import ciaoalgorithms_jl_amd._lib as L
    from ciaoalgorithms_jl_amd.device import ProxG
    return ProxG(L.PROX_ZERO) if kind == "zero" else ProxG(L.PROX_L1, lam=2.0 ** -6)


def wide(view, ref64, name):
    """close()'s Float64 form: the reference again in Float64 on the same data, for a Float32 run"""
    return ref64[name] if view.dtype == FR.F32 else None


def bits_equal(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)


def sweep_families(view):
    """the kernel a full gradient over the view takes (rows_launch.inc: plan_rows)"""
    if view.complex:
        return ("rows_csplit_kernel",)
    if view.d == 1024:
        return ("rows_fast_kernel", "rows_multi_kernel")
    if view.d == 1000:
        return ("rows_split_kernel",)
    if view.d == FR.LONG_D[view.dtype]:
        return ("rows_long_kernel",)
    if view.d == 8193:
        return ("rows_generic_kernel",)
    if view.ld == view.d and view.d == 50:
        return ("rows_smallm_kernel",)
    if view.ld < 2 ** 24:
        return ("rows_small_kernel",)                  # d = 2; the padded rows below the bound
    return ("rows_generic_kernel",)                    # padded short rows at a stride of 2^24 elements and more


# ---- sweeps -----------------------------------------------------------------------------------------------------------------------------
def run_sweep(ctx, far, view):
    import torch
    data = FR.fill(view)
    d64 = data.astype(np.float64)
    T = view.dtype.type
    x = dev(FR.x_vector(view.d, T))
    long_rows = view.d == FR.LONG_D[view.dtype]
    options = [("", None)]
    if view.name == "d50":
        options.append(("small_mfma", 0))              # the same rows on rows_small_kernel
    if view.name == "d1024" and view.dtype == FR.F32:
        options.append(("sweep_multi", 0))             # one row per wave: rows_fast_kernel
    with FR.Placed(far, view, data) as A:
        for loss in (("ls",) if view.complex else ("ls", "logistic")):
            F = problem(view, A, data, loss)
            ref, ref64 = FR.ref_sweep(data, loss), FR.ref_sweep(d64, loss)
            scale, scale64 = FR.scale_of("sweep", "av")
            for opt, val in options:
                av = torch.full((view.d,), float("nan"), dtype=tdtype(view), device="cuda")
                if opt:
                    ctx.set_option(opt, val)
                try:
                    ctx.full_gradient(F, x, av)
                finally:
                    if opt:
                        ctx.set_option(opt, 1 if opt == "sweep_multi" else -1)
                fam = {"small_mfma": ("rows_small_kernel",), "sweep_multi": ("rows_fast_kernel",)}.get(opt, sweep_families(view))
                k = kernel(ctx, view, f"full_gradient {loss} {opt}", *fam)
                close(av, ref["av"], T, scale=scale, what=f"far rows full_gradient {view.id} {loss} ({k})", ref64=wide(view, ref64, "av"), scale64=scale64)
            if view.name == "guard-at":
                assert "rows_small_kernel" not in ctx.last_kernel()
            if view.complex or long_rows:
                continue
            if loss == "ls":
                obj = ctx.objective(F, prox("zero"), x)
                want = float(ref64["objective"][0])
                print(f"{view.id} objective {obj!r} want {want!r}")
                assert abs(obj - want) <= (1e-9 if view.dtype == FR.F64 else 2e-4) * abs(want), (view.id, obj, want)
            dots = ctx.row_dots(F, x)
            kernel(ctx, view, f"row_dots {loss}", "rows_")
            assert bits_equal(FR.gather_rows(dots, data.rows), ref["dots"]), f"{view.id}: the row dots of the marked rows"
            assert FR.count_nonzero(dots) == np.count_nonzero(ref["dots"]), f"{view.id}: a row dot landed off the marked rows"
            del dots, F
    ctx.synchronize()


def run_rowindex(ctx, far, view):
    """d = 2, N > 2^31 rows: the row index itself, b[row], rowdot_out[row], out[row]"""
    import torch
    data = FR.fill(view)
    d64 = data.astype(np.float64)
    T = view.dtype.type
    x = dev(FR.x_vector(view.d, T))
    ref, ref64 = FR.ref_sweep(data, "ls"), FR.ref_sweep(d64, "ls")
    st = FR.ref_stats(data, Ks=(), Kg=())
    scale, scale64 = FR.scale_of("sweep", "av")
    from ciaoalgorithms_jl_amd.device import Context

    def marked_b(b):
        b.zero_()
        for r, v in zip(data.rows, data.b):
            b[int(r)] = float(v)
        return b

    # 1. the full gradient that also keeps every row dot (svrg_init), on a context of its own: the N row dots the library keeps (8.7 GB)
    # go with it.  Matrix, b and those: 34.9 GB, so this runs while there is no second buffer.  (What the cache holds is not read back
    # here: rows of 8 bytes take the register chain, which recomputes a_i'z_full (chain_launch.inc: CK_REG); the store is ciao_row_dots'
    # own, checked below, and the cached values are read at far rows in run_svrg's epoch.)
    far.drop_second()
    with FR.Placed(far, view, data) as A:
        FR.need(2 * view.N * view.es, f"{view.id}: b and the row dots the library keeps")
        F = problem(view, A, data, "ls", b=marked_b(torch.empty(view.N, dtype=tdtype(view), device="cuda")))
        av, z, zf, w = (torch.full((view.d,), float("nan"), dtype=tdtype(view), device="cuda") for _ in range(4))
        own = Context(ctx.device)
        try:
            own.svrg_init(F, x, av, z, zf, w)
            k = kernel(own, view, "svrg_init", "rows_small_kernel")
            own.synchronize()
        finally:
            own.close()
        close(av, ref["av"], T, scale=scale, what=f"far rows full gradient with cached row dots {view.id} ({k})", ref64=wide(view, ref64, "av"), scale64=scale64)
        assert torch.equal(zf, x) and torch.equal(w, x) and not z.any().item()
        del F
    torch.cuda.empty_cache()
    # 2. b and the row dots in the two halves of the second buffer; at the end the N row norms (float64) take all of it
    both = far.second(view.dtype, (2, view.N))
    with FR.Placed(far, view, data) as A:
        F = problem(view, A, data, "ls", b=marked_b(both[0]))
        av = torch.full((view.d,), float("nan"), dtype=tdtype(view), device="cuda")
        ctx.full_gradient(F, x, av)
        k = kernel(ctx, view, "full_gradient", "rows_small_kernel")
        close(av, ref["av"], T, scale=scale, what=f"far rows full gradient {view.id} ({k})", ref64=wide(view, ref64, "av"), scale64=scale64)
        dots = ctx.row_dots(F, x, out=both[1])
        kernel(ctx, view, "row_dots", "rows_small_kernel")
        assert bits_equal(FR.gather_rows(dots, data.rows), ref["dots"]), "the row dots of the marked rows"
        assert FR.count_nonzero(dots) == data.K, "a row dot landed off the marked rows"
        ms = ctx.margin_stats(F, dots)
        kernel(ctx, view, "margin_stats", "mstat_")
        assert bits_equal(np.array(ms, np.float64), st["margin_stats ls"]), (ms, st["margin_stats ls"])
        del dots
        rs = ctx.row_sqnorm_stats(F)
        kernel(ctx, view, "row_sqnorm_stats", "rowsq_")
        assert bits_equal(np.array(rs, np.float64), st["row_sqnorm_stats"]), (rs, st["row_sqnorm_stats"])
        assert rs.argmax == FR.peak_row(view) >= 2 ** 31
        cs = ctx.col_sqnorms(F)
        kernel(ctx, view, "col_sqnorms", "colsq_")
        assert bits_equal(cs.cpu().numpy(), st["col_sqnorms"])
        # out[row] of the row norms: N float64 are exactly the second buffer.  b lies in it and is written over: the pass reads A only
        out = far.second(view.dtype).view(torch.float64)
        assert out.numel() == view.N
        ctx.row_sqnorms(F, out=out)
        kernel(ctx, view, "row_sqnorms", "rowsq_")
        assert bits_equal(FR.gather_rows(out, data.rows), st["row_sqnorms"]), "the row norms of the marked rows"
        assert FR.count_nonzero(out) == data.K, "a row norm landed off the marked rows"
        del F, out
    ctx.synchronize()


# ---- chains over marked rows only ------------------------------------------------------------------------------------------------------
def chain_families(view, alg):
    """chain_launch.inc: plan_chain"""
    rowb = view.d * view.es
    if view.d == 8193:
        return ("chain_wide_kernel",)
    if rowb % 16:
        return ("chain_kernel<",)                      # the register ring (d = 50 fp32: one wave)
    if alg == "saga" and 2048 < rowb <= 4096:
        return ("chain_ws_kernel",)
    return ("chain_dma_kernel",)


def run_svrg(ctx, far, view):
    import torch
    data = FR.fill(view)
    d64 = data.astype(np.float64)
    T = view.dtype.type
    idx = FR.chain_steps(data)
    assert idx.max() * view.ld >= FR.boundaries(view)[-1][1]
    with FR.Placed(far, view, data) as A:
        for loss in ("ls", "logistic"):
            F = problem(view, A, data, loss)
            ref, ref64 = FR.ref_svrg(data, loss), FR.ref_svrg(d64, loss)
            zf, w, av = (dev(v) for v in FR.chain_state(view.d, T))
            z = torch.zeros(view.d, dtype=tdtype(view), device="cuda")
            ctx.svrg_inner(F, prox("l1"), FR.chain_gamma(loss), idx, av, z, zf, w)
            k = kernel(ctx, view, f"svrg_inner {loss}", *chain_families(view, "svrg"))
            assert view.d != 1000 or "masked" in k, k
            s, s64 = FR.scale_of("svrg", "w")
            close(w, ref["w"], T, scale=s, what=f"far rows svrg_inner w {view.id} {loss} ({k})", ref64=wide(view, ref64, "w"), scale64=s64)
            s, s64 = FR.scale_of("svrg", "z")
            close(z, ref["z"], T, scale=s, what=f"far rows svrg_inner z {view.id} {loss}", ref64=wide(view, ref64, "z"), scale64=s64)
            if view.name == "d1024":
                # one epoch with the cached row dots: svrg_init's pass leaves a_i'z_full for all N rows, the inner cycle (the LDS-DMA chain's
                # cached-dots form) reads them at the far rows it visits; a dot read from another row is that row's zero, an O(1) error in w
                ref, ref64 = FR.ref_svrg_epoch(data, loss), FR.ref_svrg_epoch(d64, loss)
                av, z, zf, w = (torch.full((view.d,), float("nan"), dtype=tdtype(view), device="cuda") for _ in range(4))
                ctx.svrg_init(F, dev(FR.x_vector(view.d, T)), av, z, zf, w)
                ctx.svrg_iterate(F, prox("l1"), FR.chain_gamma(loss), idx, False, av, z, zf, w, reuse_rowdots=True)
                kernel(ctx, view, f"svrg_iterate {loss} (its tail's full pass)", "rows_fast_kernel", "rows_multi_kernel")
                s, s64 = FR.scale_of("svrg", "z_full")
                close(zf, ref["epoch z_full"], T, scale=s, what=f"far rows svrg epoch z_full {view.id} {loss}", ref64=wide(view, ref64, "epoch z_full"), scale64=s64)
                close(w, ref["epoch w"], T, scale=s, what=f"far rows svrg epoch w {view.id} {loss}", ref64=wide(view, ref64, "epoch w"), scale64=s64)
                s, s64 = FR.scale_of("svrg", "av")
                close(av, ref["epoch av"], T, scale=s, what=f"far rows svrg epoch av {view.id} {loss}", ref64=wide(view, ref64, "epoch av"), scale64=s64)
                assert not z.any().item()
            del F
    ctx.synchronize()


def table_rows_check(table, data, want, what):
    """the gathered rows of the device table for close(); everything else by count: nonzero exactly where the reference's rows are"""
    got = FR.gather_rows(table, data.rows)
    assert FR.count_nonzero(table) == np.count_nonzero(want), f"{what}: the table holds a nonzero off the rows the reference has them on"
    return got


def run_saga(ctx, far, view):
    import torch
    data = FR.fill(view)
    d64 = data.astype(np.float64)
    T = view.dtype.type
    x0 = dev(FR.x_vector(view.d, T))
    idx = FR.chain_steps(data)
    g = prox("l1")
    table = far.second(view.dtype, (view.N, view.d))
    with FR.Placed(far, view, data) as A:
        for loss in ("ls", "logistic"):
            F = problem(view, A, data, loss)
            ref, ref64 = FR.ref_saga(data, loss), FR.ref_saga(d64, loss)
            av, z = (torch.full((view.d,), float("nan"), dtype=tdtype(view), device="cuda") for _ in range(2))
            for sag in (False, True):
                ctx.saga_init(F, g, FR.chain_gamma(loss), x0, table, av, z)
                kernel(ctx, view, f"saga_init {loss}", "rows_", "prox")
                if not sag:
                    s, s64 = FR.scale_of("saga", "init table")
                    got = table_rows_check(table, data, ref["init table"], f"{view.id} saga_init")
                    close(got, ref["init table"], T, scale=s, what=f"far rows saga_init table {view.id} {loss}", ref64=wide(view, ref64, "init table"), scale64=s64)
                    s, s64 = FR.scale_of("saga", "init av")
                    close(av, ref["init av"], T, scale=s, what=f"far rows saga_init av {view.id} {loss}", ref64=wide(view, ref64, "init av"), scale64=s64)
                    s, s64 = FR.scale_of("saga", "init z")
                    close(z, ref["init z"], T, scale=s, what=f"far rows saga_init z {view.id} {loss}", ref64=wide(view, ref64, "init z"), scale64=s64)
                ctx.saga_steps(F, g, FR.chain_gamma(loss), sag, idx, table, av, z)
                k = kernel(ctx, view, f"saga_steps {loss} sag={int(sag)}", *chain_families(view, "saga"))
                tag = f"sag{int(sag)}"
                got = table_rows_check(table, data, ref[f"{tag} table"], f"{view.id} saga_steps {tag}")
                s, s64 = FR.scale_of("saga", "table")
                close(got, ref[f"{tag} table"], T, scale=s, what=f"far rows saga table {view.id} {loss} {tag} ({k})", ref64=wide(view, ref64, f"{tag} table"), scale64=s64)
                s, s64 = FR.scale_of("saga", "z")
                close(z, ref[f"{tag} z"], T, scale=s, what=f"far rows saga z {view.id} {loss} {tag}", ref64=wide(view, ref64, f"{tag} z"), scale64=s64)
                s, s64 = FR.scale_of("saga", "av")
                close(av, ref[f"{tag} av"], T, scale=s, what=f"far rows saga av {view.id} {loss} {tag}", ref64=wide(view, ref64, f"{tag} av"), scale64=s64)
            del F
    ctx.synchronize()


# ---- Finito and LFinito ---------------------------------------------------------------------------------------------------------------------
def finito_compare(view, loss, tag, k, table, av, z, data, ref, ref64, T):
    got = table_rows_check(table, data, ref[f"{tag} table"], f"{view.id} finito {tag}")
    s, s64 = FR.scale_of("finito", "table")
    close(got, ref[f"{tag} table"], T, scale=s, what=f"far rows finito table {view.id} {loss} {tag} ({k})", ref64=wide(view, ref64, f"{tag} table"), scale64=s64)
    s, s64 = FR.scale_of("finito", "z")
    close(z, ref[f"{tag} z"], T, scale=s, what=f"far rows finito z {view.id} {loss} {tag}", ref64=wide(view, ref64, f"{tag} z"), scale64=s64)
    s, s64 = FR.scale_of("finito", "av")
    close(av, ref[f"{tag} av"], T, scale=s, what=f"far rows finito av {view.id} {loss} {tag}", ref64=wide(view, ref64, f"{tag} av"), scale64=s64)


def run_finito(ctx, far, view):
    import torch
    data = FR.data_of(view, "finito")
    d64 = data.astype(np.float64)
    T = view.dtype.type
    x0 = FR.x_vector(view.d, T)
    gamv, hg = (T(v) for v in FR.finito_gam(view))
    g = prox(FR.FINITO_PROX)
    first, length = FR.block_rows(view)
    assert len(first) >= 2 and first[-1] * view.ld * view.es >= 2 ** 32
    small = view.d == 50
    table = far.second(view.dtype, (view.N, view.d))
    gam = torch.full((view.N,), float(gamv), dtype=tdtype(view), device="cuda")

    def state():
        """the table zero but for the state's rows, av, z"""
        st, a, zz = FR.finito_state(data, T)
        for r, row in zip(data.rows, st):
            table[int(r)] = dev(row)
        return dev(a), dev(zz)

    def clear():
        for r in data.rows:
            table[int(r)].zero_()

    with FR.Placed(far, view, data) as A:
        for loss in ("ls", "logistic"):
            F = problem(view, A, data, loss)
            ref, ref64 = FR.ref_finito(data, loss), FR.ref_finito(d64, loss)
            av, z = (torch.full((view.d,), float("nan"), dtype=tdtype(view), device="cuda") for _ in range(2))
            ctx.finito_init(F, g, gam, float(hg), dev(x0), table, av, z)
            k = kernel(ctx, view, f"finito_init {loss}", "rows_")
            got = FR.gather_rows(table, data.rows)
            assert FR.count_rows_not(table, dev(x0)) == np.count_nonzero((ref["init table"] != x0).any(axis=1)), "a table row off the marked rows is not x0"
            s, s64 = FR.scale_of("finito", "init table")
            close(got, ref["init table"], T, scale=s, what=f"far rows finito_init table {view.id} {loss}", ref64=wide(view, ref64, "init table"), scale64=s64)
            # av = hat_gamma sum_i s_i / gamma_i runs over ALL N rows (N - K equal terms x0 / gamma): not a sum of K terms, and the scale
            # of the call sites (a few hundred rows) does not cover it.  The bound is the length of the longest chain of additions
            # the launch can make (far_rows.sum_scale), with the grid the launch report names, and never beyond BASELINE's 1e-10 / 1e-4;
            # the table above is what tells rows apart
            s = min(FR.sum_scale(view.N, k), BASELINE_EPS[view.dtype])
            close(av, ref["init av"], T, scale=s, what=f"far rows finito_init av {view.id} {loss}", ref64=wide(view, ref64, "init av"), scale64=s)
            close(z, ref["init z"], T, scale=s, what=f"far rows finito_init z {view.id} {loss}", ref64=wide(view, ref64, "init z"), scale64=s)
            table.zero_()
            # index lists of marked rows: as a chain (batches of 1 and 3), and batch-parallel (one wave per row; several rows per wave)
            routes = [("chain", {}, ("chain_",))]
            if small:
                routes += [("wrow", {"chain_max_batch": 0}, ("rows_wrow_kernel",)), ("smallb", {"chain_max_batch": 0, "small_wrow": 0}, ("rows_smallb_kernel",))]
            else:
                routes += [("rows", {"chain_max_batch": 0}, ("rows_split_kernel", "rows_fast_kernel", "rows_multi_kernel"))]
            for r in (1, 3):
                batches = FR.finito_batches(data, r)
                bptr = np.zeros(len(batches) + 1, np.int64)
                np.cumsum([len(b) for b in batches], out=bptr[1:])
                for route, opts, fam in routes:
                    av, z = state()
                    for o, v in opts.items():
                        ctx.set_option(o, v)
                    try:
                        ctx.finito_steps(F, g, gam, float(hg), bptr, np.concatenate(batches), table, av, z)
                    finally:
                        for o in opts:
                            ctx.set_option(o, -1)
                    k = kernel(ctx, view, f"finito_steps {loss} r={r} {route}", *fam)
                    finito_compare(view, loss, f"lists r={r}", k, table, av, z, data, ref, ref64, T)
                    clear()
            # row blocks that start at far rows
            for route, opts, fam in ([("blocks", {}, ("rows_wrow_kernel", "chain_")), ("tiles", {"chain_max_batch": 0, "small_wrow": 0}, ("rows_smallm_kernel", "rows_smallb_kernel"))]
                                     if small else [("blocks", {"chain_max_batch": 0}, ("rows_split_kernel", "rows_fast_kernel", "rows_multi_kernel"))]):
                av, z = state()
                for o, v in opts.items():
                    ctx.set_option(o, v)
                try:
                    ctx.finito_steps_blocks(F, g, gam, float(hg), first, length, table, av, z)
                finally:
                    for o in opts:
                        ctx.set_option(o, -1)
                k = kernel(ctx, view, f"finito_steps_blocks {loss} {route}", *fam)
                finito_compare(view, loss, "blocks", k, table, av, z, data, ref, ref64, T)
                clear()
            del F
    ctx.synchronize()


def run_lfinito(ctx, far, view):
    import torch
    data = FR.data_of(view, "lfinito")
    d64 = data.astype(np.float64)
    T = view.dtype.type
    x0 = dev(FR.x_vector(view.d, T))
    gamv, hg = (T(v) for v in FR.lfinito_params(view))
    g = prox(FR.FINITO_PROX)
    first, length = FR.block_rows(view)
    bptr = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    bidx = np.concatenate([np.arange(f, f + n) for f, n in zip(first, length)]).astype(np.int64)
    gam = torch.full((view.N,), float(gamv), dtype=tdtype(view), device="cuda")
    with FR.Placed(far, view, data) as A:
        for loss in ("ls", "logistic"):
            F = problem(view, A, data, loss)
            ref, ref64 = FR.ref_lfinito(data, loss), FR.ref_lfinito(d64, loss)
            for form in ("blocks", "lists"):
                av, z, zf = (torch.full((view.d,), float("nan"), dtype=tdtype(view), device="cuda") for _ in range(3))
                ctx.lfinito_init(F, float(hg), x0, av, z, zf)
                kernel(ctx, view, f"lfinito_init {loss}", "rows_", "prox")
                s, s64 = FR.scale_of("lfinito", "init av")
                close(av, ref["init av"], T, scale=s, what=f"far rows lfinito_init av {view.id} {loss}", ref64=wide(view, ref64, "init av"), scale64=s64)
                assert torch.equal(z, av) and torch.equal(zf, av)
                ctx.set_option("chain_max_batch", 0)   # the batch sweep on the batch-parallel kernels, not as a chain
                try:
                    if form == "blocks":
                        ctx.lfinito_iterate_blocks(F, g, gam, float(hg), first, length, av, z, zf)
                    else:
                        ctx.lfinito_iterate(F, g, gam, float(hg), bptr, bidx, av, z, zf)
                finally:
                    ctx.set_option("chain_max_batch", -1)
                k = kernel(ctx, view, f"lfinito_iterate {loss} {form}", "rows_")
                for name, t in (("z_full", zf), ("z", z), ("av", av)):
                    s, s64 = FR.scale_of("lfinito", name)
                    close(t, ref[name], T, scale=s, what=f"far rows lfinito {name} {view.id} {loss} {form} ({k})", ref64=wide(view, ref64, name), scale64=s64)
            del F
    del gam
    ctx.synchronize()


def run_afinito(ctx, far, view):
    """adaptive Finito steps over marked rows from a consistent state written by hand: afinito_init probes every sample's Lipschitz modulus,
    and a zero row has none (the reference draws random probes for it)"""
    import torch
    data = FR.fill(view)
    T = view.dtype.type
    alpha, tol_b, _, hg0 = FR.afinito_params(view)
    idx = FR.chain_steps(data)
    ref = FR.ref_afinito(data)
    st, c, f, gam, dots, av0, z0 = FR.afinito_state(data, T)
    table = far.second(view.dtype, (view.N, view.d)).zero_()
    meta4 = torch.zeros((view.N, 4, 4), dtype=tdtype(view), device="cuda")
    with FR.Placed(far, view, data) as A:
        F = problem(view, A, data, "ls")
        for k, r in enumerate(data.rows):
            table[int(r)] = dev(st[k])
            meta4[int(r)] = dev(np.array([c[k], f[k], gam[k], dots[k]], T)).expand(4, 4)
        av, z, hg = dev(av0), dev(z0), dev(np.array([hg0], T))
        done, trials = ctx.afinito_steps(F, prox(FR.FINITO_PROX), alpha, tol_b, idx, table, meta4, av, z, hg)
        k = kernel(ctx, view, "afinito_steps", "afinito_dma_kernel" if view.d == 1024 else "afinito_")
        assert [done, trials] == ref["counts"].tolist() == [len(idx), len(idx)], (done, trials, ref["counts"])
        rows4 = FR.gather_rows(meta4, data.rows)                               # (K, 4, 4)
        assert all(np.array_equal(rows4[:, 0], rows4[:, j]) for j in range(1, 4)), "the four copies of a sample's scalars differ"
        assert FR.count_nonzero(meta4) == 4 * np.count_nonzero(rows4[:, 0]), "a sample's scalars landed off the marked rows"
        got = table_rows_check(table, data, ref["table"], f"{view.id} afinito_steps")
        s, _ = FR.scale_of("afinito", "table")
        close(got, ref["table"], T, scale=s, what=f"far rows adaptive table {view.id} ({k})", ref64=False)   # (afinito_steps runs untwinned: oracle/twin.py)
        s, _ = FR.scale_of("afinito", "z")
        close(z, ref["z"], T, scale=s, what=f"far rows adaptive z {view.id}", ref64=False)
        s, _ = FR.scale_of("afinito", "av")
        close(av, ref["av"], T, scale=s, what=f"far rows adaptive av {view.id}", ref64=False)
        s, _ = FR.scale_of("afinito", "hat_gamma")
        close(hg, ref["hat_gamma"], T, scale=s, what=f"far rows adaptive hat_gamma {view.id}", ref64=False)
        s, _ = FR.scale_of("afinito", "gam")
        close(rows4[:, 0, 2], ref["gam"], T, scale=s, what=f"far rows adaptive gamma_i {view.id}", ref64=False)
        s, _ = FR.scale_of("afinito", "f")
        close(rows4[:, 0, 1], ref["f"], T, scale=s, what=f"far rows adaptive f_i(x_i) {view.id}", ref64=False)
        s, _ = FR.scale_of("afinito", "gradient table")
        close(rows4[:, 0, 0:1].astype(np.float64) * data.A.astype(np.float64), ref["gradient table"], T, scale=s,
              what=f"far rows adaptive gradient table (c_i a_i) {view.id}", ref64=False)
        del F
    ctx.synchronize()


def run_proshi(ctx, far, view):
    """agents at far rows of Q and q (one buffer serves both: Q = q), of the table and of the stepsizes"""
    import torch
    import ciaoalgorithms_jl_amd._lib as L
    from ciaoalgorithms_jl_amd.device import PackedSepQuad, ProxG
    data = FR.fill(view)
    d64 = data.astype(np.float64)
    T = view.dtype.type
    gamv, hg, eta, lo, hi, ghi = FR.proshi_params(view)
    ref, ref64 = FR.ref_proshi(data), FR.ref_proshi(d64)
    batches = FR.proshi_batches(data)
    bptr = np.concatenate([[0], np.cumsum([len(b) for b in batches])]).astype(np.int64)
    st, av0, _ = FR.finito_state(data, T)
    z0 = (FR.x_vector(view.d, T, 2) / T(gamv)).astype(T)
    table = far.second(view.dtype, (view.N, view.d)).zero_()
    gam = torch.full((view.N,), float(T(gamv)), dtype=tdtype(view), device="cuda")
    g = ProxG(L.PROX_BOX, lo=-float("inf"), hi=ghi)
    with FR.Placed(far, view, data) as A:
        assert A.is_contiguous()
        F = PackedSepQuad(A, A, eta, lo, hi)
        for route, opt, fam in (("chain", -1, "proshi_chain_kernel"), ("batches", 0, "proshi_")):
            for r, row in zip(data.rows, st):
                table[int(r)] = dev(row)
            av, z = dev(av0), dev(z0)
            ctx.set_option("proshi_chain_max_batch", opt)
            try:
                ctx.proshi_steps(F, g, gam, float(T(hg)), bptr, np.concatenate(batches), table, av, z)
            finally:
                ctx.set_option("proshi_chain_max_batch", -1)
            k = kernel(ctx, view, f"proshi_steps {route}", fam)
            assert route == "chain" or "proshi_chain_kernel" not in k, k
            got = table_rows_check(table, data, ref["table"], f"{view.id} proshi_steps {route}")
            s, s64 = FR.scale_of("proshi", "table")
            close(got, ref["table"], T, scale=s, what=f"far rows proshi table {view.id} {route} ({k})", ref64=wide(view, ref64, "table"), scale64=s64)
            s, s64 = FR.scale_of("proshi", "av")
            close(av, ref["av"], T, scale=s, what=f"far rows proshi av {view.id} {route}", ref64=wide(view, ref64, "av"), scale64=s64)
            s, s64 = FR.scale_of("proshi", "z")          # z = (prox(av) - av) / hat_gamma: its rounding unit is theirs (test_proshi_steps)
            close(z, ref["z"], T, scale=s, what=f"far rows proshi z {view.id} {route}", size=np.abs(ref["av"]).max() / float(T(hg)),
                  ref64=wide(view, ref64, "z"), scale64=s64)
            for r in data.rows:
                table[int(r)].zero_()
        del F
    ctx.synchronize()


# ---- statistics passes on integer rows: bits -------------------------------------------------------------------------------------------------
def run_stats(ctx, far, view):
    import math
    import torch
    data = FR.fill(view)
    T = view.dtype.type
    ref = FR.ref_stats(data)
    x = dev(FR.x_vector(view.d, T))
    with FR.Placed(far, view, data) as A:
        F = problem(view, A, data, "ls")
        out = ctx.row_sqnorms(F, out=far.second(view.dtype).view(torch.float64)[:view.N])      # (the second buffer is free until the scaled matrix)
        kernel(ctx, view, "row_sqnorms", "rowsq_")
        assert bits_equal(FR.gather_rows(out, data.rows), ref["row_sqnorms"]) and FR.count_nonzero(out) == data.K
        del out
        rs = ctx.row_sqnorm_stats(F)
        assert bits_equal(np.array(rs, np.float64), ref["row_sqnorm_stats"]), (rs, ref["row_sqnorm_stats"])
        assert rs.argmax == FR.peak_row(view) and rs.argmax * view.ld >= FR.boundaries(view)[-1][1]
        cs = ctx.col_sqnorms(F)
        kernel(ctx, view, "col_sqnorms", "colsq_")
        assert bits_equal(cs.cpu().numpy(), ref["col_sqnorms"])
        s1, s2 = ctx.col_moments(F)
        kernel(ctx, view, "col_moments", "colmom_")
        assert bits_equal(s1.cpu().numpy(), ref["col_moments s1"]) and bits_equal(s2.cpu().numpy(), ref["col_moments s2"])
        scaled = ctx.scale_columns(F, center=None, scale=dev(FR.x_vector(view.d, np.float64, 5)), out=far.second(view.dtype, (view.N, view.d)))
        kernel(ctx, view, "scale_columns", "colscale_")
        assert bits_equal(FR.gather_rows(scaled, data.rows), ref["scaled"]), "the scaled marked rows"
        assert FR.count_nonzero(scaled) == np.count_nonzero(ref["scaled"]), "a zero did not stay zero"
        del scaled
        if view.d <= 1024:
            G, u, colsum, bsum = ctx.gram(F)
            kernel(ctx, view, "gram", "gram_")
            for name, t in (("G", G), ("u", u), ("colsum", colsum), ("bsum", bsum)):
                assert bits_equal(t.cpu().numpy(), ref[f"gram {name}"]), f"gram {name}"
            del G
        dots = ctx.row_dots(F, x)
        ms = ctx.margin_stats(F, dots)
        kernel(ctx, view, "margin_stats", "mstat_")
        assert bits_equal(np.array(ms, np.float64), ref["margin_stats ls"]), (ms, ref["margin_stats ls"])
        for K in (3, 17):
            xs = [dev(m) for m in FR.models(view.d, T, K)]
            got = np.array([tuple(s) for s in ctx.margin_stats_multi(F, xs)], np.float64)
            kernel(ctx, view, f"margin_stats_multi K={K}", "mscore_")
            assert bits_equal(got, ref[f"margin_stats_multi K={K}"]), f"margin_stats_multi K={K}"
        for K in (2, 17):
            xs = [dev(m) for m in FR.models(view.d, T, K)]
            avs = torch.full((K, view.d), float("nan"), dtype=tdtype(view), device="cuda")
            ctx.full_gradient_multi(F, xs, [avs[k] for k in range(K)])
            k = kernel(ctx, view, f"full_gradient_multi K={K}", "mrhs_kernel", "rows_")
            S = ref[f"full_gradient_multi K={K}"]
            want = FR.multi_expected(S, 1.0, view.N, T)
            if "mrhs_kernel" in k and float(T(view.N)) == view.N:     # the exact recipe of test_gpu_multi_rhs_paths: N exact in the type
                assert bits_equal(avs.cpu().numpy(), want), f"full_gradient_multi K={K}: not the exact result"
            else:                                      # K single sweeps: that file's scale against its own single sweeps
                want64 = S.astype(np.float64) / view.N
                for j in range(K):
                    close(avs[j], want64[j].astype(T), T, scale={64: 44, 32: 48}, what=f"far rows full_gradient_multi {view.id} K={K} ({k})", ref64=False)
        del F
        # logistic rows: a zero row has margin 0 -- an error, log 2 of loss; the count and the minimum are exact
        F = problem(view, A, data, "logistic")
        ms = ctx.margin_stats(F, dots)
        kernel(ctx, view, "margin_stats logistic", "mstat_")
        want = ref["margin_stats logistic"]
        print(f"{view.id} logistic loss_sum {ms.loss_sum!r} want {want[0]!r}")
        assert abs(ms.loss_sum - want[0]) <= (view.N + 8) * FR.EPS[FR.F64] * want[0]      # test_gpu_margins.check_logistic's bound
        assert ms.errors == want[1] and ms.min_margin == want[2], (ms, want)
        assert math.isfinite(ms.entropy)
        del F, dots
    ctx.synchronize()


RUN = {"sweep": run_sweep, "rowindex": run_rowindex, "svrg": run_svrg, "saga": run_saga, "finito": run_finito, "lfinito": run_lfinito,
       "afinito": run_afinito, "proshi": run_proshi, "stats": run_stats}


# the families a case is there to reach (the table of DESIGN.md section 5.1), each held to be in a launch report the case itself asserted
REACH = {("d1024", "sweep"): ("rows_fast_kernel",), ("d1000", "sweep"): ("rows_split_kernel", "masked"), ("d50", "sweep"): ("rows_smallm_kernel", "rows_small_kernel"),
         ("d2", "rowindex"): ("rows_small_kernel", "mstat_", "rowsq_", "colsq_"), ("c1024", "sweep"): ("rows_csplit_kernel",),
         ("d16388", "sweep"): ("rows_long_kernel",), ("d8194", "sweep"): ("rows_long_kernel",), ("d8193", "sweep"): ("rows_generic_kernel",),
         ("s65x1000odd", "sweep"): ("rows_split_kernel", "scalar"), ("guard-below", "sweep"): ("rows_small_kernel",), ("guard-at", "sweep"): ("rows_generic_kernel",),
         ("d1024", "svrg"): ("chain_dma_kernel",), ("d1000", "svrg"): ("chain_dma_kernel", "masked"), ("d50", "svrg"): ("block=64",), ("d8193", "svrg"): ("chain_wide_kernel",),
         ("d50", "saga"): ("block=64",), ("d50", "finito"): ("rows_wrow_kernel", "rows_smallb_kernel", "rows_smallm_kernel", "block=64"),
         ("d1024", "afinito"): ("afinito_dma_kernel",), ("d1024", "proshi"): ("proshi_chain_kernel", "proshi_vec_kernel"),
         ("d1024", "stats"): ("mrhs_kernel", "mscore_", "gram_", "rowsq_", "colsq_", "colmom_", "colscale_", "mstat_"), ("d50", "stats"): ("mscore_", "gram_"),
         ("d1000", "stats"): ("mscore_", "gram_")}
FAULT = []                                             # the case after which the device reported an error: nothing more is launched


@pytest.mark.parametrize("view,op", CASES)
def test_far_rows(ctx, far, view, op):
    assert not FAULT, f"not run: the device reported an error in {FAULT[0]}"
    import torch
    n0 = len(KERNELS)
    torch.cuda.reset_peak_memory_stats()
    try:
        RUN[op](ctx, far, view)
        peak = torch.cuda.max_memory_allocated()
        print(f"{view.id}-{op}: at most {peak / 1e9:.2f} GB of tensors at once")
        assert peak <= 36e9, f"{view.id}-{op}: {peak / 1e9:.2f} GB of tensors at once: more than the matrix, one buffer of its size and 1.1 GB"
        seen = " ".join(k for _, _, k in KERNELS[n0:])
        need = REACH.get((view.name, op), ()) + (("chain_ws_kernel",) if (view.id, op) in (("f32-d1024", "saga"), ("f32-d1000", "saga")) else ())
        assert all(f in seen for f in need), f"{view.id}-{op}: of {need}, the launch reports hold only {[f for f in need if f in seen]}"
    except AssertionError:
        raise
    except Exception as e:                             # (a skip is a BaseException: not caught here)
        if getattr(e, "status", 0) == -2 or "hiperror" in str(e).lower() or "illegal memory" in str(e).lower():   # (-2: CIAO_ERR_HIP)
            FAULT.append(f"{view.id}-{op}: {e}")
        raise


def test_the_samplers_index_rows_beyond_2_31_and_refuse_2_32(ctx, ciao):
    """The real limit of this path: the uniform draws are 32-bit fractions of N (sampling.py), so N < 2^32 -- refused on the device
    and on the host with a message, never drawn wrongly; below it the draws pass 2^31 and are the host's."""
    assert not FAULT, f"not run: the device reported an error in {FAULT[0]}"
    N = FR.views(FR.F32)["d2"].N                       # 2 181 038 080 rows
    host = ciao.IndexStream(7).rand_indices(N, 4096)
    got = ctx.sample_uniform(7, 0, N, 4096).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, host) and host.max() >= 2 ** 31 and 0 <= host.min() and host.max() < N
    top = ctx.sample_uniform(7, 0, 2 ** 32 - 1, 4096).cpu().numpy()
    assert np.array_equal(top, ciao.IndexStream(7).rand_indices(2 ** 32 - 1, 4096)) and top.max() < 2 ** 32 - 1
    with pytest.raises(ciao._lib.CiaoError, match=r"N < 2\^32"):
        ctx.sample_uniform(7, 0, 2 ** 32, 4)
    with pytest.raises(AssertionError):
        ciao.IndexStream(7).rand_indices_device(ctx, 2 ** 32, 4)
    ctx.synchronize()

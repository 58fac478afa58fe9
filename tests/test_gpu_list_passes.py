"""A matrix-vector product and its adjoint over a list of rows on the device (ciao_list_dots, ciao_list_combine, Context.list_dots /
list_combine; csrc/list_kernels.h).

The specification is an equality of bits: the call over idx is the call without a list on the gathered copy A[idx] (c unchanged), and a
row's dot product has one bit pattern wherever the row stands.

  1. exact on integers: |a| <= 64, |x| <= 8, c = (5 m mod 9) - 4: every partial sum is an integer far below 2^53, so both results equal
     numpy's int64 result bit for bit: fp32 and fp64 rows, d over every group width and chunks-per-lane mode of the row decomposition and
     one and several panels of the column decomposition, M over every threshold of the two plans (restated here from (M, d) alone), four
     lists, the four layouts of A, idx / x / c / out inside guarded buffers that end at their last element at both 16-byte alignments,
     the launch's report against the restated plan; the identity list against no list;
  2. bits on Gaussian data: against the NULL-list call on A[idx].contiguous(), the identity list against NULL, one row at several
     positions of several lists, a second call, and the host twins within 2 (d + 2) 2^-53 sum|a x| and 2 (M + 3) 2^-53 sum|c a| (each
     side at most half of that from the exact value: one rounding per product, one per addition);
  3. entries outside [0, N) through the raw ABI, A between poisoned guard rows; refused by Context.list_dots / list_combine;
  4. far rows: rows beyond 2^31 (fp32: 2^32) elements;
  5. refusals, each with nothing launched."""
import ctypes as C

import numpy as np
import pytest

import far_rows as FR
from layouts import Guarded, bits, has_poison
from test_gpu_gram import input_layouts, int_matrix, kind_of, problem, tname
from test_gpu_gram_rows import master_lists

pytestmark = pytest.mark.gpu

D_INT = [1, 3, 17, 128, 129, 257, 1025, 4096]


# ---- the two plans, restated from (M, d) ----------------------------------------------------------------------------------------------------
def dot_plan(M, d, vec):
    """rowsq_plan(M, d) of csrc/rowsq_kernels.h for d <= 4096 -> (G, mode, rows of a wave per trip, rows per workgroup, grid)"""
    chunks = -(-d // vec)
    g = 0
    while g < 6 and (1 << g) < chunks:
        g += 1
    trips = -(-chunks // (1 << g))
    mode = 0 if trips <= 1 else 1 if trips <= 2 else 2 if trips <= 4 else 3
    wave = (8 >> mode) * (64 >> g)
    step = 4 * wave
    per = max(step, -(-(-(-M // 2048)) // step) * step)
    return 1 << g, mode, wave, per, max(1, -(-M // per))


def comb_plan(M, d, vec):
    """col_plan(M, d, vec, 1) of csrc/col_walk.h -> (tc, panels, step, slab, nslab)"""
    chunks = -(-d // vec)
    tc = 1
    while tc < 256 and tc < chunks:
        tc *= 2
    panels = -(-chunks // tc)
    step = (256 // tc) * 8
    want = max(1, min(2048 // panels, (32 << 20) // (8 * d)))
    slab = max(4 * step, -(-(-(-M // want)) // step) * step)
    return tc, panels, step, slab, max(1, -(-M // slab))


def m_sizes(d):
    """1; one wave's rows +-1 and one workgroup's rows +-1 of the dots; 4 step +-1 and two slabs + 1 of the combine -- of both types"""
    ms = {1}
    for vec in (4, 2):
        _, _, wave, per, _ = dot_plan(1, d, vec)
        _, _, step, slab, _ = comb_plan(1, d, vec)
        assert slab == 4 * step
        ms |= {wave - 1, wave, wave + 1, per - 1, per, per + 1, 4 * step - 1, 4 * step, 4 * step + 1, 8 * step + 1}
        assert dot_plan(per + 1, d, vec)[4] == 2 and [comb_plan(m, d, vec)[4] for m in (4 * step, 4 * step + 1, 8 * step + 1)] == [1, 2, 3]
    return sorted(m for m in ms if m >= 1)


def dots_report(M, d, dtype, kind, listed):
    G, mode, _, per, grid = dot_plan(M, d, 2 if dtype == np.float64 else 4)
    return f"listdot_kernel<{tname(dtype)},{kind}{',rows' if listed else ''}> grid={grid} block=256 G={G} mode={mode} rows_per_wg={per}"


def comb_report(M, d, dtype, kind, listed):
    tc, panels, _, slab, nslab = comb_plan(M, d, 2 if dtype == np.float64 else 4)
    return f"listcomb_partial_kernel<{tname(dtype)},{kind}> grid={panels}x{nslab} block=256 tc={tc} slab={slab}{',rows' if listed else ''}"


def int_x(d):
    return (3 * np.arange(d, dtype=np.int64)) % 17 - 8


def int_c(M):
    return (5 * np.arange(M, dtype=np.int64)) % 9 - 4


def exact(v):
    assert v.dtype == np.int64 and int(np.abs(v).max(initial=0)) < 2 ** 53
    return v.astype(np.float64)


# ---- 1. exact on integers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", D_INT)
def test_integer_rows_over_lists_exactly(ctx, d):
    import torch
    sizes = m_sizes(d)
    Mmax = sizes[-1]
    ints, bi = int_matrix(3 * Mmax, d)
    xi = int_x(d)
    lists = master_lists(Mmax)
    layouts = {dt: input_layouts(torch.from_numpy(ints.astype(dt)), torch.from_numpy(bi.astype(dt)), dt) for dt in (np.float32, np.float64)}
    modes, kinds, offs = set(), set(), set()
    for ni, M in enumerate(sizes):
        ci = int_c(M)
        rev = np.arange(M - 1, -1, -1, dtype=np.int64)
        cases = [(name, idx[:M]) for name, idx in lists.items()] + [("reversed", rev)]
        for ki, (name, idx) in enumerate(cases):
            want_d = torch.from_numpy(exact(ints[idx] @ xi)).cuda()
            want_c = torch.from_numpy(exact(ints[idx].T @ ci)).cuda()
            for off in (0, 1):
                Gi = Guarded(torch.from_numpy(idx.copy()), off=off, device="cuda", name=f"idx {name} M={M} off={off}")
                Gc = Guarded(torch.from_numpy(ci.astype(np.float64)), off=1 - off if ki % 2 else off, device="cuda", name=f"c M={M}")
                out_d = Guarded(shape=(M,), dtype=np.float64, off=(off + ki) % 2, device="cuda", name="dots")
                out_c = Guarded(shape=(d,), dtype=np.float64, off=(off + ni) % 2, device="cuda", name="combination")
                assert Gi.view.data_ptr() % 16 == 8 * off
                for dt in (np.float32, np.float64):
                    Gx = Guarded(torch.from_numpy(xi.astype(dt)), off=(off + ki + ni) % 2, device="cuda", name="x")
                    for li, (lname, GA, Gb) in enumerate(layouts[dt]):
                        if (li + ni + ki) % 2 != off:      # every layout, every M and every list meet both offsets
                            continue
                        F = problem(GA.view, Gb.view)
                        runs = [(F, Gi.view)]
                        if name == "identity":             # ... and no list at all: the first M rows as a problem of their own
                            runs.append((problem(GA.view[:M], Gb.view[:M]), None))
                        for F_, rows in runs:
                            for g in (out_d, out_c):
                                bits(g.view).fill_(bits(g.flat[:1]).item())
                            got = ctx.list_dots(F_, Gx.view, rows=rows, out=out_d.view)
                            assert ctx.last_kernel() == dots_report(M, d, dt, kind_of(F_), rows is not None), ctx.last_kernel()
                            out_d.check_outside(ctx.last_kernel())
                            assert got is out_d.view and torch.equal(bits(got), bits(want_d)), ("dots", name, lname, M, d, tname(dt), off, ctx.last_kernel())
                            got = ctx.list_combine(F_, Gc.view, rows=rows, out=out_c.view)
                            assert ctx.last_kernel() == comb_report(M, d, dt, kind_of(F_), rows is not None), ctx.last_kernel()
                            out_c.check_outside(ctx.last_kernel())
                            assert got is out_c.view and torch.equal(bits(got), bits(want_c)), ("combine", name, lname, M, d, tname(dt), off, ctx.last_kernel())
                            kinds.add((tname(dt), kind_of(F_), rows is not None))
                        offs.add((M, off))
                    Gx.check_unchanged("x")
                Gi.check_unchanged(name)
                Gc.check_unchanged("c")
        modes.add(dot_plan(M, d, 2)[1])
    for dt in layouts:
        for lname, GA, Gb in layouts[dt]:
            GA.check_unchanged(lname)
            Gb.check_unchanged(lname)
    assert len(kinds) == 8 and len(offs) == 2 * len(sizes)


def test_the_sizes_cover_every_mode_of_both_plans():
    seen = {(dot_plan(1, d, vec)[0], dot_plan(1, d, vec)[1]) for d in D_INT for vec in (2, 4)}
    assert {m for _, m in seen} == {0, 1, 2, 3} and {g for g, _ in seen} >= {1, 2, 8, 16, 32, 64}
    assert {comb_plan(1, d, 2)[1] for d in D_INT} >= {1, 3, 8} and {comb_plan(1, d, 2)[0] for d in D_INT} >= {1, 2, 16, 64, 256}


# ---- 2. bits ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
@pytest.mark.parametrize("d", [150, 1030])
def test_the_bits_of_the_gathered_copy(ctx, dtype, d):
    """N = 1400 Gaussian rows, M = 700 drawn with repeats: several workgroups and slabs, a partial last chunk; d = 150 on a group of
    lanes, d = 1030 a wave per row and several panels."""
    import torch
    from ciaoalgorithms_jl_amd.host_route import host_list_combine, host_list_dots
    rng = np.random.default_rng(12)
    N, M = 1400, 700
    A = torch.from_numpy(rng.standard_normal((N, d)).astype(dtype))
    b = torch.from_numpy(rng.standard_normal(N).astype(dtype))
    x = torch.from_numpy(rng.standard_normal(d).astype(dtype))
    idx = torch.from_numpy(rng.integers(0, N, M))
    assert len(torch.unique(idx)) < M
    cv = torch.from_numpy(rng.standard_normal(M))
    Ad, bd, xd, cd, gath = A.cuda(), b.cuda(), x.cuda(), cv.cuda(), idx.cuda()
    copy = problem(Ad[gath].contiguous(), bd[gath].contiguous())
    want_d = ctx.list_dots(copy, xd).clone()
    assert ctx.last_kernel() == dots_report(M, d, dtype, kind_of(copy), False)
    want_c = ctx.list_combine(copy, cd).clone()
    assert ctx.last_kernel() == comb_report(M, d, dtype, kind_of(copy), False)
    for li, (name, GA, Gb) in enumerate(input_layouts(A, b, dtype)):
        Gi = Guarded(idx, off=li % 2, device="cuda", name=f"idx {name}")
        Gc = Guarded(cv, off=(li // 2) % 2, device="cuda", name=f"c {name}")
        Gx = Guarded(x, off=(li + 1) % 2, device="cuda", name=f"x {name}")
        for kind in ("ls", "logistic"):
            F = problem(GA.view, Gb.view, kind)
            for rep in range(2):
                got_d = ctx.list_dots(F, Gx.view, rows=Gi.view)
                assert ",rows> " in ctx.last_kernel()
                got_c = ctx.list_combine(F, Gc.view, rows=Gi.view)
                assert ctx.last_kernel().endswith(",rows")
                assert not has_poison(got_d) and not has_poison(got_c), name
                assert torch.equal(bits(got_d), bits(want_d)) and torch.equal(bits(got_c), bits(want_c)), (name, kind, rep)
        for g in (GA, Gb, Gi, Gc, Gx):
            g.check_unchanged(name)
    # the identity list: the bits of no list on A itself
    F = problem(Ad, bd)
    ident = torch.arange(N, device="cuda")
    cN = torch.from_numpy(rng.standard_normal(N)).cuda()
    whole_d, whole_c = ctx.list_dots(F, xd).clone(), ctx.list_combine(F, cN).clone()
    assert torch.equal(bits(ctx.list_dots(F, xd, rows=ident)), bits(whole_d)) and torch.equal(bits(ctx.list_combine(F, cN, rows=ident)), bits(whole_c))
    # one row at several positions of several lists of different M: one bit pattern in the dots
    row = 777
    for Mk, places in ((1, [0]), (5, [0, 4]), (65, [0, 31, 64]), (700, [3, 256, 257, 699]), (2051, [0, 1024, 2050])):
        lst = rng.integers(0, N, Mk)
        lst[places] = row
        got = ctx.list_dots(F, xd, rows=torch.from_numpy(lst).cuda())
        assert bool((bits(got[torch.tensor(places, device="cuda")]) == bits(whole_d[row:row + 1])).all()), (Mk, places)
    # the host twins
    a64, x64 = A.numpy().astype(np.float64), x.numpy().astype(np.float64)
    hd, hc = host_list_dots(A.numpy(), x.numpy(), idx.numpy()), host_list_combine(A.numpy(), cv.numpy(), idx.numpy())
    bound_d = 2 * (d + 2) * 2.0 ** -53 * (np.abs(a64[idx.numpy()]) @ np.abs(x64))
    bound_c = 2 * (M + 3) * 2.0 ** -53 * (np.abs(a64[idx.numpy()]).T @ np.abs(cv.numpy()))
    assert (np.abs(want_d.cpu().numpy() - hd) <= bound_d).all() and (np.abs(want_c.cpu().numpy() - hc) <= bound_c).all()


# ---- 3. entries outside [0, N) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
def test_entries_that_name_no_row(ctx, ciao, dtype):
    """Through the raw ABI a list with -1 and N inserted: the dots are 0 at those positions and the others' bits do not change; the
    combination equals that of the list with those positions removed (integer data: exact).  c is NaN at those positions: no term
    means no term.  A lies between poisoned guard rows: a load that the predicate should have stopped shows as NaN."""
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    rng = np.random.default_rng(13)
    N, d, M = 300, 150, 200
    ints, bi = int_matrix(N, d)
    A, b = torch.from_numpy(ints.astype(dtype)), torch.from_numpy(bi.astype(dtype))
    GA = Guarded(A, guard=2 * d, device="cuda", name="A")            # two poisoned rows on either side
    Gb = Guarded(b, device="cuda", name="b")
    idx = rng.integers(0, N, M)
    bad = np.array([0, 3, 16, 17, 63, 64, 130, 199])
    idx[bad[::2]], idx[bad[1::2]] = -1, N
    keep = np.setdiff1d(np.arange(M), bad)
    xi, ci = int_x(d), int_c(M)
    cn = ci.astype(np.float64)
    cn[bad] = np.nan
    want_d = np.zeros(M)
    want_d[keep] = exact(ints[idx[keep]] @ xi)
    want_c = exact(ints[idx[keep]].T @ ci[keep])
    F = problem(GA.view, Gb.view)
    Gi = Guarded(torch.from_numpy(idx), off=1, device="cuda", name="idx")
    x, c = torch.from_numpy(xi.astype(dtype)).cuda(), torch.from_numpy(cn).cuda()
    out_d = Guarded(shape=(M,), dtype=np.float64, device="cuda", name="dots")
    out_c = Guarded(shape=(d,), dtype=np.float64, device="cuda", name="combination")
    lib, h = ctx.lib, ctx._h
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert lib.ciao_list_dots(h, F.ref, ptr(Gi.view), M, ptr(x), ptr(out_d.view)) == L.OK, lib.ciao_last_error()
    assert ",rows> " in ctx.last_kernel()
    assert lib.ciao_list_combine(h, F.ref, ptr(Gi.view), M, ptr(c), ptr(out_c.view)) == L.OK, lib.ciao_last_error()
    assert ctx.last_kernel().endswith(",rows")
    for g, e, what in ((out_d, want_d, "dots"), (out_c, want_c, "combination")):
        g.check_outside(what)
        assert not has_poison(g.view), what
        assert torch.equal(bits(g.view), bits(torch.from_numpy(e).cuda())), what
    GA.check_unchanged("A")
    ctx.full_gradient(F, torch.zeros(d, dtype=A.dtype, device="cuda"), torch.empty(d, dtype=A.dtype, device="cuda"))
    before = ctx.last_kernel()
    assert not before.startswith("list")
    with pytest.raises(ValueError):
        ctx.list_dots(F, x, rows=Gi.view)
    with pytest.raises(ValueError):
        ctx.list_combine(F, c, rows=Gi.view)
    assert ctx.last_kernel() == before


# ---- 4. far rows -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
def test_rows_beyond_two_to_the_31_elements(ctx, dtype):
    """d = 1024, a zero matrix of far_rows.ELEMS elements with three marked rows: row 0, the first row wholly beyond 2^31 elements (fp32:
    2^32) and the last; the list is those three, a repeat of the last and two zero rows: the bits of no list on the copy."""
    import torch
    d = 1024
    dt = np.dtype(dtype)
    elems = FR.ELEMS[dt]
    FR.need(elems * dt.itemsize, f"the {tname(dtype)} matrix")
    N = elems // d
    far = -(-(2 ** 32 if dtype == np.float32 else 2 ** 31) // d)
    assert 0 < far < N - 1 and far * d >= (2 ** 32 if dtype == np.float32 else 2 ** 31)
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    A = torch.zeros((N, d), dtype=tdt, device="cuda")
    b = torch.zeros(N, dtype=tdt, device="cuda")
    rng = np.random.default_rng(14)
    rows = [0, far, N - 1]
    for r in rows:
        A[r] = torch.from_numpy(rng.standard_normal(d).astype(dtype)).cuda()
    idx = torch.tensor([far - 1, 0, far, N - 1, 1, N - 1], dtype=torch.int64, device="cuda")
    x = torch.from_numpy(rng.standard_normal(d).astype(dtype)).cuda()
    c = torch.from_numpy(rng.standard_normal(6)).cuda()
    try:
        F = problem(A, b)
        got_d, got_c = ctx.list_dots(F, x, rows=idx).clone(), ctx.list_combine(F, c, rows=idx).clone()
        copy = problem(A[idx].contiguous(), b[idx].contiguous())
        want_d, want_c = ctx.list_dots(copy, x), ctx.list_combine(copy, c)
        assert torch.equal(bits(got_d), bits(want_d)) and torch.equal(bits(got_c), bits(want_c))
        assert torch.equal(bits(got_d[3:4]), bits(got_d[5:6])) and got_d[[1, 2, 3]].abs().min() > 0 and not bool(got_d[[0, 4]].any())
        assert len({float(v) for v in got_d[[1, 2, 3]]}) == 3 and bool(got_c.any())
    finally:
        del A, b
        torch.cuda.empty_cache()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, ciao):
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd.device import PackedF
    f64 = dict(dtype=torch.float64, device="cuda")
    i64 = dict(dtype=torch.int64, device="cuda")
    F = PackedF.least_squares(torch.randn((9, 8), **f64), torch.randn(9, **f64), 1.0)
    Fc = PackedF.least_squares_complex(torch.randn((4, 8), **f64), torch.randn(8, **f64), 4.0)
    Fz = PackedF.zero(4, 8, torch.float64)
    Fwide = PackedF.least_squares(torch.zeros((1, 4097), **f64), torch.zeros(1, **f64), 1.0)
    x = torch.zeros(8, **f64)
    xw = torch.zeros(4097, **f64)
    out = Guarded(shape=(16,), dtype=np.float64, device="cuda", name="out")
    wide = torch.zeros(4097, **f64)                    # (never written: every call that names it is refused first)
    rows = torch.tensor([1, 1, 4, 0, 8], **i64)
    c = torch.ones(9, **f64)
    odd = torch.zeros(24, dtype=torch.int32, device="cuda")[1:21].view(torch.uint8)     # a base 4 bytes off 8-byte alignment
    ctx.full_gradient(F, x, torch.empty_like(x))
    before = ctx.last_kernel()
    assert not before.startswith("list") and odd.data_ptr() % 8 == 4
    lib, h = ctx.lib, ctx._h
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def raw(status):
        if status != L.OK:
            raise L.CiaoError(status, lib.ciao_last_error().decode())

    for fn, v in ((lib.ciao_list_dots, x), (lib.ciao_list_combine, c)):
        call = lambda F_, idx, M, v_, o: raw(fn(h, F_.ref if F_ is not None else None, idx, M, v_, o))
        cases = [("NULL x / c", lambda: call(F, ptr(rows), 5, None, ptr(out.view))),
                 ("NULL out", lambda: call(F, ptr(rows), 5, ptr(v), None)),
                 ("M < 0", lambda: call(F, ptr(rows), -1, ptr(v), ptr(out.view))),
                 ("no list, M != N", lambda: call(F, None, 5, ptr(v), ptr(out.view))),
                 ("misaligned idx", lambda: call(F, ptr(odd), 2, ptr(v), ptr(out.view))),
                 ("misaligned out", lambda: call(F, ptr(rows), 2, ptr(v), ptr(odd))),
                 ("complex", lambda: call(Fc, ptr(rows), 2, ptr(v), ptr(out.view))),
                 ("Zero", lambda: call(Fz, ptr(rows), 2, ptr(v), ptr(out.view))),
                 ("NULL ctx", lambda: raw(fn(None, F.ref, ptr(rows), 5, ptr(v), ptr(out.view)))),
                 ("NULL problem", lambda: call(None, ptr(rows), 5, ptr(v), ptr(out.view))),
                 ("d > 4096", lambda: call(Fwide, ptr(rows), 1, ptr(xw), ptr(wide)))]
        if fn is lib.ciao_list_combine:
            cases.append(("misaligned c", lambda: call(F, ptr(rows), 2, ptr(odd), ptr(out.view))))
        for what, case in cases:
            with pytest.raises(L.CiaoError) as e:
                case()
            assert e.value.status == L.ERR_ARG, what
            assert len(str(e.value)) - len("libciao_hip status -1: ") > 30, (what, str(e.value))
            assert ctx.last_kernel() == before, what
    for what, bad in (("dtype", rows.int()), ("device", rows.cpu()), ("shape", rows[:, None]), ("stride", torch.zeros(10, **i64)[::2]),
                      ("type", np.zeros(5, np.int64)), ("float", rows.double()), ("below", torch.tensor([0, -1], **i64)),
                      ("beyond", torch.tensor([9, 0], **i64))):
        with pytest.raises(ValueError):
            ctx.list_dots(F, x, rows=bad)
        with pytest.raises(ValueError):
            ctx.list_combine(F, torch.ones(len(bad), **f64), rows=bad)
        assert ctx.last_kernel() == before, what
    for what, bad in (("length", torch.ones(9, **f64)), ("dtype", torch.ones(5, dtype=torch.float32, device="cuda")), ("device", torch.ones(5, dtype=torch.float64)),
                      ("stride", torch.ones(10, **f64)[::2])):
        with pytest.raises(ValueError):
            ctx.list_combine(F, bad, rows=rows)
        assert ctx.last_kernel() == before, what
    for what, bad in (("length", torch.zeros(7, **f64)), ("dtype", torch.zeros(8, dtype=torch.float32, device="cuda"))):
        with pytest.raises(ValueError):
            ctx.list_dots(F, bad, rows=rows)
    for bad in (torch.zeros(4, **f64), torch.zeros(5, dtype=torch.float32, device="cuda")):
        with pytest.raises(ValueError):
            ctx.list_dots(F, x, rows=rows, out=bad)
    with pytest.raises(L.CiaoError):
        ctx.list_dots(Fwide, xw, rows=torch.zeros(1, **i64))
    with pytest.raises(L.CiaoError):
        ctx.list_combine(Fwide, torch.ones(1, **f64), rows=torch.zeros(1, **i64))
    assert ctx.last_kernel() == before
    out.check_outside("refused calls")
    assert bool((bits(out.view) == bits(out.flat[:1])).all()) and not bool(wide.any())      # no refused call wrote
    # M = 0: nothing launched; the combination is d zeros
    none = torch.empty(0, **i64)
    assert ctx.list_dots(F, x, rows=none).shape == (0,)
    got = ctx.list_combine(F, torch.empty(0, **f64), rows=none, out=torch.ones(8, **f64))
    assert got.shape == (8,) and not bool(got.any()) and ctx.last_kernel() == before

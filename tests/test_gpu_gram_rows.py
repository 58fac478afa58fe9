"""Gram statistics over a list of rows on the device, and the cross-validation driver on them (ciao_gram_rows, Context.gram(rows=),
gram.gram_stats(rows=), cv.py; csrc/gram_kernels.h: gram_partial_kernel<Indexed<...>>).

The specification is an equality of bits: gram(rows=idx) is gram -- with weights, the weighted gram -- on the gathered copy A[idx], b[idx].

  1. exact on integers: |a| <= 64, integer weights (5 m) mod 9 by list position: every partial sum is an integer far below 2^53, so all
     outputs must equal numpy's int64 result on A[idx] bit for bit: fp32 and fp64 rows, M over every row threshold of gram_plan, four
     lists (identity, reversed, stride 3 from 1, a seeded draw with repeats from the first 2 M rows), four layouts of the matrix, idx and
     w inside guarded buffers that end at their last element at both 16-byte alignments, every output guarded, the launch's report
     against a restatement of the plan from M;
  2. bits: against gram on A[idx].contiguous(), plain and weighted, ls and logistic views, symmetry, a second call, every NULL output,
     the identity list against gram(F), five fold_lists folds adding up to the whole;
  3. entries outside [0, N) through the raw ABI, A between poisoned guard rows; refused by Context.gram;
  4. far rows: rows beyond 2^31 (fp32: 2^32) elements;
  5. refusals;
  6. the driver: lasso_cv on the device against lasso_cv_from_stats on host_gram(rows=) statistics, bit for bit.

The references of item 1.  A list for M is the first M entries of a master list (stride: 1 + 3 k; draw: entry k uniform in [0, 2 (k + 1)),
so the first M entries lie in the first 2 M rows), and the weight belongs to the position, so the expected sums grow by slabs of
positions as M grows; the reversed list names the rows of the identity list, so unweighted it has the identity's sums, and weighted its
own, formed directly."""
import ctypes as C

import numpy as np
import pytest

import far_rows as FR
from layouts import Guarded, bits, has_poison
from test_gpu_gram import input_layouts, int_matrix, kind_of, n_sizes, plan, problem, tname

pytestmark = pytest.mark.gpu

WS = 256 << 20
D_INT = [1, 3, 17, 128, 129, 257, 1025]
NAMES = ("G", "u", "colsum", "bsum")


def check_report(ctx, M, d, dtype, kind, weighted):
    ntiles, per, P, xcd, ws = plan(M, d)
    want = (f"gram_partial_kernel<{tname(dtype)},{kind}{',w' if weighted else ''},rows> grid={ntiles * P} block=256 tile=128x128 chunk=16 "
            f"tiles={ntiles} partitions={P} rows={per} map={'xcd' if xcd else 'plain'} workspace={ws}")
    assert ctx.last_kernel() == want, (ctx.last_kernel(), want)
    assert ws <= WS


class Outputs:
    """G (row stride d + 3), u, colsum, bsum (nb elements), each inside a poisoned buffer of its own"""

    def __init__(self, d, nb):
        self.G = Guarded(shape=(d, d), dtype=np.float64, ld=d + 3, device="cuda", name="G")
        self.u, self.cs, self.bs = (Guarded(shape=(n,), dtype=np.float64, device="cuda", name=nm) for n, nm in ((d, "u"), (d, "colsum"), (nb, "bsum")))

    def run(self, ctx, F, rows, w=None, u=True, colsum=True, bsum=True, **kw):
        got = ctx.gram(F, G=self.G.view, u=self.u.view if u else None, colsum=self.cs.view if colsum else None, bsum=self.bs.view if bsum else None,
                       weights=w, rows=rows, **kw)
        for g in (self.G, self.u, self.cs, self.bs):
            g.check_outside(ctx.last_kernel())
        return got


def int_weights(M):
    return (5 * np.arange(M, dtype=np.int64)) % 9


def master_lists(Mmax):
    k = np.arange(Mmax, dtype=np.int64)
    draw = (np.random.default_rng(415).random(Mmax) * (2 * (k + 1))).astype(np.int64)
    assert (draw < 2 * (k + 1)).all() and len(np.unique(draw[:129])) < 129          # repeats, already among the small lists
    return {"identity": k, "stride3": 1 + 3 * k, "draw": draw}


def int_sums(a, bb, w):
    """[G, u, colsum, bsum (3)] of the rows a, targets bb under integer weights w, in int64 by slabs of 32 rows"""
    d = a.shape[1]
    G = np.zeros((d, d), np.int64)
    wa = w[:, None] * a
    for k in range(0, a.shape[0], 32):
        G += np.ascontiguousarray(a[k:k + 32].T) @ wa[k:k + 32]
    return [G, a.T @ (w * bb), a.T @ w, np.array([(w * bb).sum(), (w * bb * bb).sum(), w.sum()])]


def as_expected(acc, weighted):
    assert all(v.dtype == np.int64 for v in acc) and max(int(np.abs(v).max()) for v in acc) < 2 ** 53
    out = [v.astype(np.float64) for v in acc]
    if not weighted:
        out[3] = out[3][:2]
    return out


# ---- 1. exact on integers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", D_INT)
def test_integer_rows_over_lists_exactly(ctx, d):
    import torch
    sizes = n_sizes(d)
    Mmax = sizes[-1]
    ints, bi = int_matrix(3 * Mmax, d)
    lists = master_lists(Mmax)
    wi = int_weights(Mmax)
    layouts = {dt: input_layouts(torch.from_numpy(ints.astype(dt)), torch.from_numpy(bi.astype(dt)), dt) for dt in (np.float32, np.float64)}
    outs = {False: Outputs(d, 2), True: Outputs(d, 3)}
    ones = np.ones(Mmax, np.int64)
    zero = lambda: [np.zeros((d, d), np.int64), np.zeros(d, np.int64), np.zeros(d, np.int64), np.zeros(3, np.int64)]
    acc = {(name, wt): zero() for name in lists for wt in (False, True)}
    kinds, offs, prev = set(), set(), 0
    for ni, M in enumerate(sizes):
        want = {}
        for name, idx in lists.items():               # the slab of positions [prev, M) onto the running sums
            rows = idx[prev:M]
            for wt in (False, True):
                part = int_sums(ints[rows], bi[rows], wi[prev:M] if wt else ones[prev:M])
                acc[(name, wt)] = [s + p for s, p in zip(acc[(name, wt)], part)]
                want[(name, wt)] = as_expected(acc[(name, wt)], wt)
        rev = np.arange(M - 1, -1, -1, dtype=np.int64)
        want[("reversed", False)] = want[("identity", False)]                      # the same rows
        want[("reversed", True)] = as_expected(int_sums(ints[rev], bi[rev], wi[:M]), True)
        prev = M
        want = {k: [torch.from_numpy(v).cuda() for v in vs] for k, vs in want.items()}
        cases = [(name, idx[:M]) for name, idx in lists.items()] + [("reversed", rev)]
        for ki, (name, idx) in enumerate(cases):
            for off in (0, 1):
                # the list and the weights of this M in buffers of their own that end at their last element, at both alignments
                Gi = Guarded(torch.from_numpy(idx.copy()), off=off, device="cuda", name=f"idx {name} M={M} off={off}")
                Gw = Guarded(torch.from_numpy(wi[:M].astype(np.float64)), off=1 - off if ki % 2 else off, device="cuda", name=f"w M={M}")
                assert Gi.view.data_ptr() % 16 == 8 * off and Gi.view.data_ptr() % 8 == 0
                for dt in (np.float32, np.float64):
                    for li, (lname, GA, Gb) in enumerate(layouts[dt]):
                        if (li + ni + ki) % 2 != off:      # every layout, every M and every list meet both offsets
                            continue
                        F = problem(GA.view, Gb.view)
                        for wt in (False, True):
                            got = outs[wt].run(ctx, F, Gi.view, Gw.view if wt else None)
                            check_report(ctx, M, d, dt, kind_of(F), wt)
                            for g, e, what in zip(got, want[(name, wt)], NAMES):
                                assert torch.equal(bits(g.contiguous()), bits(e)), (what, name, lname, M, d, tname(dt), wt, off, ctx.last_kernel())
                        kinds.add((lname, kind_of(F)))
                        offs.add((M, off))
                Gi.check_unchanged(name)
                Gw.check_unchanged("weights")
    for dt in layouts:
        for lname, GA, Gb in layouts[dt]:
            GA.check_unchanged(lname)
            Gb.check_unchanged(lname)
    assert ("padding", "vec16") in kinds and ("base+1", "elem") in kinds and len(offs) == 2 * len(sizes)


# ---- 2. bits ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
def test_the_bits_of_the_gathered_copy(ctx, dtype):
    """N = 1400 Gaussian rows, d = 150, M = 700: three tiles, several partitions, a partial last chunk."""
    import torch
    rng = np.random.default_rng(12)
    N, d, M = 1400, 150, 700
    A = torch.from_numpy(rng.standard_normal((N, d)).astype(dtype))
    b = torch.from_numpy(rng.standard_normal(N).astype(dtype))
    idx = torch.from_numpy(rng.integers(0, N, M))
    assert len(torch.unique(idx)) < M
    wv = torch.from_numpy(rng.standard_normal(M))
    assert bool((wv < 0).any()) and bool((wv > 0).any())
    Ad, bd, w = A.cuda(), b.cuda(), wv.cuda()
    gath = idx.cuda()
    for weighted in (False, True):
        out = Outputs(d, 3 if weighted else 2)
        copy = problem(Ad[gath].contiguous(), bd[gath].contiguous())
        want = [g.contiguous().clone() for g in ctx.gram(copy, weights=w if weighted else None)]
        assert ctx.last_kernel().startswith(f"gram_partial_kernel<{tname(dtype)},{kind_of(copy)}{',w' if weighted else ''}> ")
        for li, (name, GA, Gb) in enumerate(input_layouts(A, b, dtype)):
            Gi = Guarded(idx, off=li % 2, device="cuda", name=f"idx {name}")
            Gw = Guarded(wv, off=(li // 2) % 2, device="cuda", name=f"w {name}")
            for kind in ("ls", "logistic"):
                for rep in range(2):
                    got = [g.contiguous().clone() for g in out.run(ctx, problem(GA.view, Gb.view, kind), Gi.view, Gw.view if weighted else None)]
                    assert ctx.last_kernel().startswith(f"gram_partial_kernel<{tname(dtype)},") and ",rows> " in ctx.last_kernel()
                    assert not any(has_poison(g) for g in got), name
                    assert torch.equal(bits(got[0]), bits(got[0].T.contiguous())), "G is not symmetric to the bit"
                    assert all(torch.equal(bits(a), bits(e)) for a, e in zip(got, want)), (name, kind, rep, weighted)
            for g in (GA, Gb, Gi, Gw):
                g.check_unchanged(name)
        F = problem(Ad, bd)
        for mask in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
            fresh = Outputs(d, 3 if weighted else 2)
            got = fresh.run(ctx, F, gath, w if weighted else None, *map(bool, mask))
            assert torch.equal(bits(got[0].contiguous()), bits(want[0]))
            for k, (on, g, held) in enumerate(zip(mask, got[1:], (fresh.u, fresh.cs, fresh.bs))):
                if on:
                    assert torch.equal(bits(g), bits(want[1 + k]))
                else:
                    assert g is None and not held.outside_touched() and bool((bits(held.view) == bits(held.flat[:1])).all())   # still the poison
    # the identity list: ciao_gram's bits on A itself
    F = problem(Ad, bd)
    whole = [g.contiguous().clone() for g in ctx.gram(F)]
    ident = ctx.gram(F, rows=torch.arange(N, device="cuda"))
    assert all(torch.equal(bits(a.contiguous()), bits(e)) for a, e in zip(ident, whole))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
def test_folds_add_up_to_the_whole(ctx, dtype):
    """five fold_lists folds of integer rows: each the statistics of its gathered rows, together exactly the unweighted whole"""
    import torch
    from ciaoalgorithms_jl_amd.cv import fold_lists
    N, d = 1000, 129
    ints, bi = int_matrix(N, d)
    A, b = torch.from_numpy(ints.astype(dtype)).cuda(), torch.from_numpy(bi.astype(dtype)).cuda()
    F = problem(A, b)
    whole = [g.clone() for g in ctx.gram(F)]
    total = None
    for rows in fold_lists(N, 5, seed=3, device="cuda"):
        part = [g.clone() for g in ctx.gram(F, rows=rows)]
        sub = ctx.gram(problem(A[rows].contiguous(), b[rows].contiguous()))
        assert all(torch.equal(bits(p.contiguous()), bits(s.contiguous())) for p, s in zip(part, sub))
        total = part if total is None else [t + p for t, p in zip(total, part)]
    assert all(torch.equal(bits(t.contiguous()), bits(e.contiguous())) for t, e in zip(total, whole))


# ---- 3. entries outside [0, N) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
def test_entries_that_name_no_row(ctx, ciao, dtype):
    """Through the raw ABI a list with -1 and N inserted gives the bits of the gathered copy with those rows zeroed, b included (the same
    plan M; with weights: their weights zeroed too -- such a row counts in no sum, sum w included).  A lies between poisoned guard rows:
    a load that the predicate should have stopped shows as NaN.  Context.gram refuses the list before any launch."""
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    rng = np.random.default_rng(13)
    N, d, M = 300, 150, 200
    A = torch.from_numpy(rng.standard_normal((N, d)).astype(dtype))
    b = torch.from_numpy(rng.standard_normal(N).astype(dtype))
    GA = Guarded(A, guard=2 * d, device="cuda", name="A")            # two poisoned rows on either side
    Gb = Guarded(b, device="cuda", name="b")
    idx = rng.integers(0, N, M)
    bad = np.array([0, 3, 16, 17, 63, 64, 130, 199])                 # in the first chunk, across chunk and partition borders, the last position
    idx[bad[::2]], idx[bad[1::2]] = -1, N
    safe = idx.copy()
    safe[bad] = 0
    Az, bz = A[torch.from_numpy(safe)].clone(), b[torch.from_numpy(safe)].clone()
    Az[torch.from_numpy(bad)] = 0
    bz[torch.from_numpy(bad)] = 0
    wv = rng.standard_normal(M)
    wz = wv.copy()
    wz[bad] = 0
    F = problem(GA.view, Gb.view)
    Gi = Guarded(torch.from_numpy(idx), off=1, device="cuda", name="idx")
    lib, h = ctx.lib, ctx._h
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for weighted in (False, True):
        want = ctx.gram(problem(Az.cuda(), bz.cuda()), weights=torch.from_numpy(wz).cuda() if weighted else None)
        out = Outputs(d, 3 if weighted else 2)
        w = torch.from_numpy(wv).cuda()
        st = lib.ciao_gram_rows(h, F.ref, ptr(Gi.view), M, ptr(w) if weighted else None, ptr(out.G.view), d + 3, ptr(out.u.view), ptr(out.cs.view),
                                ptr(out.bs.view))
        assert st == L.OK, lib.ciao_last_error()
        assert ",rows> " in ctx.last_kernel()
        for g, e, what in zip((out.G, out.u, out.cs, out.bs), want, NAMES):
            g.check_outside(what)
            assert not has_poison(g.view), what
            assert torch.equal(bits(g.view.contiguous()), bits(e.contiguous())), (what, weighted)
    GA.check_unchanged("A")
    before = ctx.last_kernel()
    ctx.full_gradient(F, torch.zeros(d, dtype=A.dtype, device="cuda"), torch.empty(d, dtype=A.dtype, device="cuda"))
    before = ctx.last_kernel()
    assert not before.startswith("gram")
    with pytest.raises(ValueError):
        ctx.gram(F, rows=Gi.view)
    assert ctx.last_kernel() == before


# ---- 4. far rows -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
def test_rows_beyond_two_to_the_31_elements(ctx, dtype):
    """d = 1024, a zero matrix of far_rows.ELEMS elements with three marked rows: row 0, the first row wholly beyond 2^31 elements (fp32:
    2^32) and the last; the list is those three plus a repeat of the last: one launch over four rows, the bits of gram on the copy."""
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
        b[r] = float(rng.standard_normal())
    idx = torch.tensor(rows + [N - 1], dtype=torch.int64, device="cuda")
    try:
        got = [g.clone() for g in ctx.gram(problem(A, b), rows=idx)]
        assert ctx.last_kernel().startswith(f"gram_partial_kernel<{tname(dtype)},vec16,rows> grid=36 ")
        want = ctx.gram(problem(A[idx].contiguous(), b[idx].contiguous()))
        assert all(torch.equal(bits(a.contiguous()), bits(e.contiguous())) for a, e in zip(got, want))
        assert bool(got[0].any()) and float(got[3][1]) > 0
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
    out = Guarded(shape=(8, 8), dtype=np.float64, ld=8, device="cuda", name="G")
    wide = torch.zeros(8, **f64)                       # (never written: every call that names it is refused first)
    rows = torch.tensor([1, 1, 4, 0, 8], **i64)
    w = torch.ones(5, **f64)
    odd = torch.zeros(24, dtype=torch.int32, device="cuda")[1:21].view(torch.uint8)     # a base 4 bytes off 8-byte alignment
    ctx.full_gradient(F, x, torch.empty_like(x))
    before = ctx.last_kernel()
    assert not before.startswith("gram")
    lib, h = ctx.lib, ctx._h
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert odd.data_ptr() % 8 == 4

    def raw(status):
        if status != L.OK:
            raise L.CiaoError(status, lib.ciao_last_error().decode())

    call = lambda F_, idx, M, w_, G, ldg: raw(lib.ciao_gram_rows(h, F_.ref if F_ is not None else None, idx, M, w_, G, ldg, None, None, None))
    cases = [("NULL idx", lambda: call(F, None, 5, None, ptr(out.view), 8)),
             ("misaligned idx", lambda: call(F, ptr(odd), 2, None, ptr(out.view), 8)),
             ("M < 0", lambda: call(F, ptr(rows), -1, None, ptr(out.view), 8)),
             ("misaligned w", lambda: call(F, ptr(rows), 2, ptr(odd), ptr(out.view), 8)),
             ("complex", lambda: call(Fc, ptr(rows), 2, None, ptr(out.view), 8)),
             ("Zero", lambda: call(Fz, ptr(rows), 2, None, ptr(out.view), 8)),
             ("NULL ctx", lambda: raw(lib.ciao_gram_rows(None, F.ref, ptr(rows), 5, None, ptr(out.view), 8, None, None, None))),
             ("NULL problem", lambda: call(None, ptr(rows), 5, None, ptr(out.view), 8)),
             ("NULL G", lambda: call(F, ptr(rows), 5, None, None, 8)),
             ("ldg < d", lambda: call(F, ptr(rows), 5, None, ptr(out.view), 7)),
             ("d > 4096", lambda: call(Fwide, ptr(rows), 1, None, ptr(wide), 4097))]
    for what, c in cases:
        with pytest.raises(L.CiaoError) as e:
            c()
        assert e.value.status == L.ERR_ARG, what
        assert len(str(e.value)) - len("libciao_hip status -1: ") > 30, (what, str(e.value))
        assert ctx.last_kernel() == before, what
    for what, bad in (("dtype", rows.int()), ("device", rows.cpu()), ("shape", rows[:, None]), ("stride", torch.zeros(10, **i64)[::2]),
                      ("type", np.zeros(5, np.int64)), ("float", rows.double())):
        with pytest.raises(ValueError):
            ctx.gram(F, rows=bad)
        assert ctx.last_kernel() == before, what
    for what, bad in (("length N", torch.ones(9, **f64)), ("dtype", torch.ones(5, dtype=torch.float32, device="cuda")), ("device", torch.ones(5, dtype=torch.float64)),
                      ("stride", torch.ones(10, **f64)[::2])):
        with pytest.raises(ValueError):
            ctx.gram(F, rows=rows, weights=bad)
        assert ctx.last_kernel() == before, what
    for what, bad in (("below", torch.tensor([0, -1], **i64)), ("beyond", torch.tensor([9, 0], **i64))):
        with pytest.raises(ValueError):
            ctx.gram(F, rows=bad)
        assert ctx.last_kernel() == before, what
    with pytest.raises(ValueError):
        ctx.gram(F, rows=rows, weights=w, bsum=torch.zeros(2, **f64))       # three sums with weights
    with pytest.raises(L.CiaoError):
        ctx.gram(Fwide, rows=torch.zeros(1, **i64))
    assert ctx.last_kernel() == before
    out.check_outside("refused calls")
    assert bool((bits(out.view.contiguous()) == bits(out.flat[:1])).all()) and not bool(wide.any())      # no refused call wrote
    # M = 0: zeros (two sums, three with weights), nothing launched
    for wts, nb in ((None, 2), (torch.empty(0, **f64), 3)):
        got = ctx.gram(F, rows=torch.empty(0, **i64), weights=wts)
        assert all(not bool(g.any()) for g in got) and got[0].shape == (8, 8) and got[3].shape == (nb,) and ctx.last_kernel() == before


# ---- 6. the driver on device statistics --------------------------------------------------------------------------------------------------------
def test_cross_validation_on_device_statistics(ctx):
    """Integer rows (|a| <= 8, integer b), N = 600, d = 40, 5 folds, 4 values of mu: the folds' statistics are exact, so the device and
    host_gram(rows=) give the same bits, lasso_cd on the device equals its numpy twin (section 8.14) and the table is formed on the host
    either way: the two CVResults are equal bit for bit.  Each fold's training statistics equal gram_stats under the 0/1 weights of
    the fold's complement."""
    import torch
    from ciaoalgorithms_jl_amd import cv as CV
    from ciaoalgorithms_jl_amd import gram as GR
    from ciaoalgorithms_jl_amd.device import PackedF
    rng = np.random.default_rng(16)
    N, d, folds = 600, 40, 5
    A = rng.integers(-8, 9, (N, d)).astype(np.float64)
    x_true = np.zeros(d)
    x_true[:6] = rng.integers(-3, 4, 6)
    b = A @ x_true + rng.integers(-4, 5, N)
    F = PackedF.least_squares(torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda(), 1.0)
    whole = GR.gram_stats(ctx, F)
    mus = [f * GR.mu_max(whole) for f in (0.5, 0.2, 0.05, 0.01)]
    dev = CV.lasso_cv(ctx, F, mus, folds=folds, seed=5)
    assert ctx.last_kernel().startswith("gramcd_kernel<")
    lists = CV.fold_lists(N, folds, seed=5)
    host_stats = CV.fold_stats(None, (A, b, 1.0), lists)
    host = CV.lasso_cv_from_stats(host_stats, mus)
    assert dev.mus == host.mus and (dev.best, dev.one_se) == (host.best, host.one_se) and dev.floor == host.floor
    for name in ("mse", "mean", "stderr"):
        assert torch.equal(bits(getattr(dev, name).contiguous()), bits(getattr(host, name).contiguous())), name
    assert dev.mse.shape == (folds, len(mus)) and not has_poison(dev.mse)
    assert dev.path.converged == host.path.converged and dev.path.iterations == host.path.iterations and all(dev.path.converged)
    assert all(x.is_cuda and torch.equal(bits(x.cpu()), bits(y)) for x, y in zip(dev.path.x, host.path.x))
    # the training statistics of every fold: the sum of the other folds' against the 0/1 weights of the complement
    dev_stats = CV.fold_stats(ctx, F, [r.cuda() for r in lists])
    assert ",rows> " in ctx.last_kernel()
    for f in range(folds):
        train = GR.add_stats([s for g, s in enumerate(dev_stats) if g != f])
        keep = torch.ones(N, dtype=torch.float64, device="cuda")
        keep[lists[f].cuda()] = 0
        ref = GR.gram_stats(ctx, F, weights=keep)
        assert train.N == N - len(lists[f]) == int(ref.sum_w)
        for a, e in ((train.G, ref.G), (train.u, ref.u), (train.colsum, ref.colsum)):
            assert torch.equal(bits(a.contiguous()), bits(e.contiguous())), f
        assert (train.sum_b, train.sum_bb) == (ref.sum_b, ref.sum_bb)
        h = host_stats[f]
        assert torch.equal(bits(dev_stats[f].G.cpu().contiguous()), bits(h.G.contiguous())) and dev_stats[f].N == h.N

"""K models with offsets scored over a row LIST in one pass (ciao_margin_stats_multi_rows; csrc/mscore_kernels.h, the MscoreRows
instantiations).  The method is tests/test_gpu_score_many.py's, whose helpers are imported.

(a) exact integer cases (|a| <= 8, |x| <= 4, integer offsets |off| <= 4: every dot and every sum of the LeastSquares statistics is exact in
    any order): LeastSquares BITWISE against the numpy twin, against the call without a list on the gathered copy, and (without offsets)
    against margin_stats_multi on the materialised A[idx]; logistic: errors and minimum exact, the two sums within 2 M 2^-53 |value|
    (M same-signed terms in another order).  M in {1, 15, 16, 17, 33, 2050} over N = 97 rows (repeats, unsorted), d in {3, 64, 65, 257,
    513, 1024}, K in {1, 16, 17}, and M = 32768 + 17 at d = 3 (partitions of two tiles); four layouts, poisoned padding, guard bands;
(b) bits: the list call is the call without a list on the gathered copy (general data, both types, every SL tier, every layout);
    idx = NULL and off = NULL give ciao_margin_stats_multi's bits; one row gives the same contribution at every list position; a
    model's bits do not depend on K, its place or a NaN neighbour;
(c) entries outside [0, N) with check_rows=False are skipped (the error count shows they are not counted as zero rows);
(d) general data against the float64 twin within test_gpu_score_many.general_bounds' (d + 1) u sum |a x| law;
(e) the per-model route (d = 1025, an unaligned iterate) agrees with score(rows=, intercept=) bitwise; the C refusals;
(f) far rows: a zero matrix of far_rows.ELEMS elements at d = 1024 with three marked rows, one wholly beyond 2^31 (fp32: 2^32) elements,
    named by a list: the bits of the call without a list on the gathered copy, both types, both losses."""
import ctypes as C
import math

import numpy as np
import pytest

import far_rows as FR
import layouts as LY
import problems as P
from test_gpu_score_many import LAYOUTS, Case, bits, general_bounds, integer_problem, part_rows, tname

pytestmark = pytest.mark.gpu

N_ROWS = 97
MS = (1, 15, 16, 17, 33, 2050)
DS = (3, 64, 65, 257, 513, 1024)
KS = (1, 16, 17)
# every (M, d) pair, K in turn; then two tiles a partition
EXACT = [(M, d, KS[(i + j) % 3]) for i, M in enumerate(MS) for j, d in enumerate(DS)] + [(32768 + 17, 3, 17)]


def row_list(rng, M, N):
    """M row numbers in [0, N): unsorted, with repeats wherever M >= 2"""
    idx = rng.integers(0, N, size=M).astype(np.int64)
    if M >= 2:
        idx[M // 2] = idx[0]
    return idx


def on_device(idx, lead=0):
    """the list as a device int64 vector, `lead` entries into a longer one (8-byte aligned, not 16)"""
    import torch
    big = torch.zeros(lead + len(idx), dtype=torch.int64, device="cuda")
    big[lead:].copy_(torch.from_numpy(idx))
    return big[lead:]


def rows_kernel(dtype, d, loss, vec16, listed, offset):
    sl = 4 if d <= 64 else 16 if d <= 256 else 32 if d <= 512 else 64
    return (f"mscore_partial_kernel<rows,{tname(dtype)},SL{sl},{'logistic' if loss == 'logistic' else 'ls'},{'vec16' if vec16 else 'elem'},"
            f"{'list' if listed else 'all'},{'offset' if offset else 'plain'}>")


def gathered_case(loss, A, b, xs, idx):
    return Case(loss, np.ascontiguousarray(A[idx]), np.ascontiguousarray(b[idx]), xs, LAYOUTS[0])


# ---- (a) exact cases --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
@pytest.mark.parametrize("shape", list(enumerate(EXACT)), ids=[f"M{m}-d{d}-K{k}" for m, d, k in EXACT])
def test_exact_cases(ctx, shape, loss, dtype):
    from ciaoalgorithms_jl_amd import host_route as HR
    i, (M, d, K) = shape
    layout = LAYOUTS[(i + (loss == "ls") + 2 * (dtype == np.float64)) % 4]
    rng = np.random.default_rng(1000 + i)
    A, b, xs = integer_problem(loss, N_ROWS, d, K, dtype, seed=100 * i + 3)
    idx = row_list(rng, M, N_ROWS)
    off = [float(v) for v in rng.integers(-4, 5, size=K)]
    s = [(1.0, 0.5, 0.0)[k % 3] for k in range(K)]
    c = Case(loss, A, b, xs, layout)
    rows = on_device(idx, lead=i % 2)
    got = ctx.margin_stats_multi(c.F, c.xs, s, rows=rows, offsets=off)
    vec16 = c.gA.view.data_ptr() % 16 == 0 and (c.F.ld * A.itemsize) % 16 == 0
    name = ctx.last_kernel()
    parts = -(-M // part_rows(M))
    assert name.startswith(rows_kernel(dtype, d, loss, vec16, True, True)) and f"K={K} partitions={parts}" in name, (name, layout)
    c.check_untouched(f"margin_stats_multi(rows=) {layout[0]}")
    plain = ctx.margin_stats_multi(c.F, c.xs, s, rows=rows)                                 # no offsets: off = NULL
    g = gathered_case(loss, A, b, xs, idx)
    copy = ctx.margin_stats_multi(g.F, g.xs, s, offsets=off)                                # idx = NULL on the gathered copy
    assert ctx.last_kernel().startswith(rows_kernel(dtype, d, loss, (d * A.itemsize) % 16 == 0, False, True)), ctx.last_kernel()
    old = ctx.margin_stats_multi(g.F, g.xs, s)                                              # the kernel of section 8.11 on the copy
    assert "<rows," not in ctx.last_kernel()
    twin = HR.host_margin_stats_multi(loss, A, xs, b, s, rows=idx, offsets=off)
    assert bits(got) == bits(copy), layout
    assert bits(plain) == bits(old), layout
    if loss == "ls":
        assert bits(got) == bits(twin), layout
        assert bits(plain) == bits(HR.host_margin_stats_multi(loss, A, xs, b, s, rows=idx)), layout
        return
    for k in range(K):
        assert got[k].errors == twin[k][2] and got[k].min_margin == twin[k][3], (k, got[k], twin[k])
        for j, name in ((0, "loss_sum"), (1, "entropy")):
            tol = 2 * M * 2.0 ** -53 * abs(twin[k][j])
            assert abs(got[k][j] - twin[k][j]) <= tol, (k, name, got[k][j], twin[k][j], tol)


def test_the_exact_cases_cover_every_size():
    assert {m for m, _, _ in EXACT} >= set(MS) and {d for _, d, _ in EXACT} == set(DS) and {k for _, _, k in EXACT} == set(KS)
    seen = {(loss, dt, LAYOUTS[(i + (loss == "ls") + 2 * dt) % 4][0]) for i in range(len(EXACT)) for loss in ("ls", "logistic") for dt in (0, 1)}
    assert len(seen) == 16


# ---- (b) bits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
@pytest.mark.parametrize("d", [50, 200, 400, 1000])
def test_the_list_call_is_the_plain_call_on_the_gathered_copy(ctx, d, loss, dtype):
    N, M, K = 211, 333, 5
    A, b, x0 = P.synthetic(loss, N, d, dtype, seed=d + 1)
    rng = np.random.default_rng(d)
    xs = [x0] + [((0.2 + 0.2 * k) * rng.standard_normal(d)).astype(dtype) for k in range(1, K)]
    idx = row_list(rng, M, N)
    off = [0.0, 0.75, -1.5, 1e-3, 3.0]
    s = [1.0, 0.5, 0.0, 0.25, 1.0]
    g = gathered_case(loss, A, b, xs, idx)
    want = ctx.margin_stats_multi(g.F, g.xs, s, offsets=off)
    want_plain = ctx.margin_stats_multi(g.F, g.xs, s)
    for layout in LAYOUTS:
        c = Case(loss, A, b, xs, layout)
        for lead in (0, 1):
            rows = on_device(idx, lead)
            assert bits(ctx.margin_stats_multi(c.F, c.xs, s, rows=rows, offsets=off)) == bits(want), (layout, lead)
            assert "<rows," in ctx.last_kernel() and ",list,offset>" in ctx.last_kernel()
            assert bits(ctx.margin_stats_multi(c.F, c.xs, s, rows=rows)) == bits(want_plain), (layout, lead)
        c.check_untouched(f"list call {layout[0]}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
def test_no_list_and_no_offset_give_the_plain_entry_points_bits(ctx, loss, dtype):
    N, d, K = 1201, 300, 3
    A, b, x0 = P.synthetic(loss, N, d, dtype, seed=9)
    xs = [x0, (0.5 * x0).astype(dtype), (-x0).astype(dtype)]
    c = Case(loss, A, b, xs, LAYOUTS[3])
    s = [1.0, 0.5, 0.0]
    want = ctx.margin_stats_multi(c.F, c.xs, s)
    tab = (C.c_void_p * K)(*[x.data_ptr() for x in c.xs])
    sv = (C.c_double * K)(*s)
    out = (C.c_double * (4 * K))()
    assert ctx.lib.ciao_margin_stats_multi_rows(ctx._h, c.F.ref, None, N, K, tab, None, sv, out) == 0
    assert ctx.last_kernel().startswith(rows_kernel(dtype, d, loss, False, False, False))
    assert np.array(list(out), dtype=np.float64).view(np.uint64).tolist() == [v for row in bits(want) for v in row]


def test_a_row_has_one_contribution_at_every_position(ctx):
    import torch
    N, d = 64, 130
    for loss in ("ls", "logistic"):
        A, b, x0 = P.synthetic(loss, N, d, np.float64, seed=4)
        c = Case(loss, A, b, [x0, (0.3 * x0)], LAYOUTS[1])
        long = torch.arange(40, dtype=torch.int64, device="cuda")
        r = 23
        alone = ctx.margin_stats_multi(c.F, c.xs, rows=on_device(np.array([r], dtype=np.int64)), offsets=[0.25, -0.5])
        for sl in (long[r:r + 1], on_device(np.array([5, r, 7, 9, 11], dtype=np.int64))[1:2]):
            assert sl.numel() == 1 and int(sl[0]) == r
            assert bits(ctx.margin_stats_multi(c.F, c.xs, rows=sl, offsets=[0.25, -0.5])) == bits(alone)
        # ... and inside a longer list: the LeastSquares maximum and the logistic minimum over the list are those of its rows alone
        every = [ctx.margin_stats_multi(c.F, c.xs, rows=long[m:m + 1], offsets=[0.25, -0.5]) for m in range(40)]
        whole = ctx.margin_stats_multi(c.F, c.xs, rows=long, offsets=[0.25, -0.5])
        for k in range(2):
            pick = max if loss == "ls" else min
            assert whole[k][3] == pick(e[k][3] for e in every)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
def test_a_model_depends_on_nothing_but_itself(ctx, loss, dtype):
    import torch
    N, d, K, M = 53, 300, 17, 71
    A, b, x0 = P.synthetic(loss, N, d, dtype, seed=5)
    rng = np.random.default_rng(6)
    xs = [x0] + [(0.3 * rng.standard_normal(d)).astype(dtype) for _ in range(K - 1)]
    c = Case(loss, A, b, xs, LAYOUTS[1])
    rows = on_device(row_list(rng, M, N))
    s = [(1.0, 0.5, 0.0)[k % 3] for k in range(K)]
    off = [0.125 * (k - 8) for k in range(K)]
    all17 = ctx.margin_stats_multi(c.F, c.xs, s, rows=rows, offsets=off)
    assert bits(ctx.margin_stats_multi(c.F, c.xs, s, rows=rows, offsets=off)) == bits(all17)
    for k in (0, 7, 16):
        assert bits(ctx.margin_stats_multi(c.F, [c.xs[k]], [s[k]], rows=rows, offsets=[off[k]])) == bits([all17[k]]), k
    rev = ctx.margin_stats_multi(c.F, c.xs[::-1], s[::-1], rows=rows, offsets=off[::-1])
    assert bits(rev[::-1]) == bits(all17)
    poisoned = list(c.xs)
    poisoned[3] = torch.full_like(c.xs[3], float("nan"))
    got = ctx.margin_stats_multi(c.F, poisoned, s, rows=rows, offsets=off)
    assert bits(got[:3] + got[4:]) == bits(all17[:3] + all17[4:])
    assert math.isnan(got[3][0])
    c.check_untouched("independence")


# ---- (c) entries outside [0, N) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
@pytest.mark.parametrize("M,d", [(16, 3), (45, 65), (2050, 1024), (45, 1025)])     # (d = 1025: the per-model route skips them too)
def test_entries_outside_the_rows_are_skipped(ctx, M, d, loss, dtype):
    from ciaoalgorithms_jl_amd import host_route as HR
    K = 3
    rng = np.random.default_rng(M + d)
    A, b, xs = integer_problem(loss, N_ROWS, d, K, dtype, seed=M)
    idx = row_list(rng, M, N_ROWS)
    bad = rng.choice(M, size=max(1, M // 5), replace=False)
    idx[bad] = rng.choice([-1, N_ROWS, N_ROWS + 5, -2 ** 40, 2 ** 40, 2 ** 62], size=len(bad))
    if M >= 33:
        idx[16:32] = -1                                      # a whole tile of nothing
    keep = idx[(idx >= 0) & (idx < N_ROWS)]
    assert 0 < len(keep) < M
    off = [1.0, -2.0, 0.0]
    c = Case(loss, A, b, xs, LAYOUTS[(M + d) % 4])
    with pytest.raises(ValueError):
        ctx.margin_stats_multi(c.F, c.xs, rows=on_device(idx), offsets=off)
    got = ctx.margin_stats_multi(c.F, c.xs, rows=on_device(idx), offsets=off, check_rows=False)
    assert ("<rows," in ctx.last_kernel()) == (d <= 1024), ctx.last_kernel()
    c.check_untouched("entries outside [0, N)")
    none = ctx.margin_stats_multi(c.F, c.xs, rows=on_device(np.array([-1, N_ROWS, 2 ** 40], dtype=np.int64)), offsets=off, check_rows=False)
    assert all(tuple(v) == (0.0, 0.0, 0.0, math.inf if loss == "logistic" else 0.0) for v in none)        # the statistics of no sample
    twin = HR.host_margin_stats_multi(loss, A, xs, b, rows=keep, offsets=off)
    if loss == "ls":
        assert bits(got) == bits(twin)
        return
    zero_rows_would_count = M - len(keep)
    for k in range(K):
        assert got[k].errors == twin[k][2] and got[k].errors <= len(keep) < len(keep) + zero_rows_would_count
        assert got[k].min_margin == twin[k][3]
        for j in (0, 1):
            assert abs(got[k][j] - twin[k][j]) <= 2 * M * 2.0 ** -53 * abs(twin[k][j])
    # a list that is nothing but one existing row among entries that name none: the statistics of that row alone (a row of zeros
    # would be an error of its own: t = 0 counts as misclassified)
    lone = np.full(17, -1, dtype=np.int64)
    lone[9] = 5
    one = ctx.margin_stats_multi(c.F, c.xs, rows=on_device(lone), offsets=off, check_rows=False)
    assert bits(one) == bits(ctx.margin_stats_multi(c.F, c.xs, rows=on_device(np.array([5], dtype=np.int64)), offsets=off))
    assert all(o.errors in (0.0, 1.0) for o in one)


# ---- (d) general data against the float64 twin ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
@pytest.mark.parametrize("M,d", [(37, 50), (3001, 256), (37, 1000), (3001, 50), (37, 256), (3001, 1000)])
def test_general_data_against_the_float64_twin(ctx, M, d, loss, dtype):
    """general_bounds' law on the gathered rows.  The offset enters after the dot, in double: it moves a margin by nothing more than the
    rounding of one double addition, 2^-53 (|dot| + |off|), which is added to delta_i."""
    from ciaoalgorithms_jl_amd import host_route as HR
    N, K = 501, 5
    A, b, x0 = P.synthetic(loss, N, d, dtype, seed=M + d)
    rng = np.random.default_rng(M * d)
    xs = [x0] + [((0.2 + 0.2 * k) * rng.standard_normal(d)).astype(dtype) for k in range(1, K)]
    idx = row_list(rng, M, N)
    off = [0.0, 0.5, -0.25, 1.0, -2.0]
    c = Case(loss, A, b, xs, LAYOUTS[(M + d) % 4])
    got = ctx.margin_stats_multi(c.F, c.xs, rows=on_device(idx), offsets=off)
    assert "<rows," in ctx.last_kernel() and f"K={K}" in ctx.last_kernel()
    A64, b64 = A.astype(np.float64)[idx], b.astype(np.float64)[idx]
    twin = HR.host_margin_stats_multi(loss, A.astype(np.float64), xs, b.astype(np.float64), rows=idx, offsets=off)
    for k in range(K):
        x64 = xs[k].astype(np.float64)
        g, w = got[k], twin[k]
        delta, _ = general_bounds(loss, dtype, A64, b64, x64, M, d)
        dots = A64 @ x64
        delta = delta + 2.0 ** -53 * (np.abs(dots) + abs(off[k]))
        if loss == "ls":
            r = dots + off[k] - b64
            bound = {"sum_r2": float(np.sum(2 * np.abs(r) * delta + delta ** 2) + 2 * M * 2.0 ** -53 * np.sum(r * r)),
                     "sum_b": 2 * M * 2.0 ** -53 * float(np.sum(np.abs(b64))), "sum_b2": 2 * M * 2.0 ** -53 * float(np.sum(b64 * b64)),
                     "max_abs_r": float(delta.max())}
            for i, name in enumerate(("sum_r2", "sum_b", "sum_b2", "max_abs_r")):
                err = abs(g[i] - w[i])
                print(f"M={M} d={d} {tname(dtype)} ls model {k}: {name} err {err:.3e} <= {bound[name]:.3e}")
                assert err <= bound[name], (k, name, g[i], w[i], err, bound[name])
            continue
        t = (dots + off[k]) * b64
        sd = float(np.sum(delta))
        bl = sd + 2 * M * 2.0 ** -52 * w[0]
        be = 0.23 * sd + 2 * M * 2.0 ** -52 * abs(w[1])
        print(f"M={M} d={d} {tname(dtype)} logistic model {k}: loss err {abs(g[0] - w[0]):.3e} <= {bl:.3e}  E err {abs(g[1] - w[1]):.3e} <= {be:.3e}")
        assert abs(g.loss_sum - w[0]) <= bl and abs(g.entropy - w[1]) <= be, (k, g, w, bl, be)
        assert np.count_nonzero(t < -delta) <= g.errors <= np.count_nonzero(t <= delta), (k, g.errors)
        assert abs(g.min_margin - w[3]) <= float(delta.max()), (k, g.min_margin, w[3])
    c.check_untouched("general data")


# ---- (e) the per-model route and the refusals ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
@pytest.mark.parametrize("how", ["d=1025", "unaligned"])
def test_the_per_model_route_is_score_bitwise(ctx, how, loss, dtype):
    import torch
    from ciaoalgorithms_jl_amd.scoring import score, score_many
    N, d, M = 131, (1025 if how == "d=1025" else 256), 77
    A, b, x0 = P.synthetic(loss, N, d, dtype, seed=11)
    xs = [x0, (2 * x0).astype(dtype), (-x0).astype(dtype)]
    c = Case(loss, A, b, xs, LAYOUTS[0])
    vecs = list(c.xs)
    if how == "unaligned":
        big = torch.zeros(d + 1, dtype=vecs[1].dtype, device="cuda")
        big[1:].copy_(vecs[1])
        vecs[1] = big[1:]
        assert vecs[1].data_ptr() % 16 != 0
    rows = on_device(row_list(np.random.default_rng(2), M, N))
    cs = [0.5, 0.0, -1.25]
    for r, ic in ((rows, cs), (rows, None), (None, [0.5, 0.25, -1.25])):
        many = score_many(ctx, c.F, vecs, rows=r, intercepts=ic)
        assert "mscore" not in ctx.last_kernel(), ctx.last_kernel()
        one = [score(ctx, c.F, x, rows=r, intercept=0.0 if ic is None else ic[k]) for k, x in enumerate(vecs)]
        assert many == one
    if how == "unaligned":                     # aligned again: the same shape takes the kernel, and agrees to rounding
        many = score_many(ctx, c.F, c.xs, rows=rows, intercepts=cs)
        assert "<rows," in ctx.last_kernel()
        one = [score(ctx, c.F, x, rows=rows, intercept=cs[k]) for k, x in enumerate(c.xs)]
        # general_bounds' law for the pair of device evaluations (fp32: doubled, as test_gpu_score_many does), the offset's one addition added
        idx = rows.cpu().numpy()
        A64, b64 = A.astype(np.float64)[idx], b.astype(np.float64)[idx]
        pair = 1 if dtype == np.float64 else 2
        for k in range(3):
            x64 = xs[k].astype(np.float64)
            delta, _ = general_bounds(loss, dtype, A64, b64, x64, M, d)
            delta = pair * (delta + 2.0 ** -53 * (np.abs(A64 @ x64) + abs(cs[k])))
            if loss == "ls":
                r = A64 @ x64 + cs[k] - b64
                bound = float(np.sum(2 * np.abs(r) * delta + delta ** 2) + 2 * M * 2.0 ** -53 * np.sum(r * r)) / M
                assert abs(many[k].mse - one[k].mse) <= bound, (k, many[k].mse, one[k].mse, bound)
            else:
                bound = float(np.sum(delta)) / M + 2 * M * 2.0 ** -52 * one[k].log_loss
                assert abs(many[k].log_loss - one[k].log_loss) <= bound, (k, many[k].log_loss, one[k].log_loss, bound)


def test_refusals(ctx):
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd.device import PackedF
    f64 = dict(dtype=torch.float64, device="cuda")
    N, d = 9, 8
    F = PackedF.logistic(torch.randn((N, d), **f64), torch.ones(N, **f64))
    Fw = PackedF.logistic(torch.randn((2, 1025), **f64), torch.ones(2, **f64))
    x = torch.zeros(d, **f64)
    xw = torch.zeros(1025, **f64)
    xu = torch.zeros(d + 1, **f64)[1:]
    idx = torch.arange(5, dtype=torch.int64, device="cuda")
    odd = torch.zeros(12, dtype=torch.int32, device="cuda")
    ctx.full_gradient(F, x, torch.empty_like(x))
    before = ctx.last_kernel()
    lib, h = ctx.lib, ctx._h
    tab = (C.c_void_p * 2)(x.data_ptr(), x.data_ptr())
    tabu = (C.c_void_p * 2)(x.data_ptr(), xu.data_ptr())
    tabw = (C.c_void_p * 2)(xw.data_ptr(), xw.data_ptr())
    hole = (C.c_void_p * 2)(x.data_ptr(), None)
    out = (C.c_double * 8)()
    dv = lambda *v: (C.c_double * len(v))(*v)
    ip = C.c_void_p(idx.data_ptr())
    call = lib.ciao_margin_stats_multi_rows
    raw = [("NULL ctx", lambda: call(None, F.ref, ip, 5, 2, tab, None, None, out)),
           ("NULL problem", lambda: call(h, None, ip, 5, 2, tab, None, None, out)),
           ("NULL x", lambda: call(h, F.ref, ip, 5, 2, None, None, None, out)),
           ("NULL out", lambda: call(h, F.ref, ip, 5, 2, tab, None, None, None)),
           ("NULL x[1]", lambda: call(h, F.ref, ip, 5, 2, hole, None, None, out)),
           ("M = 0", lambda: call(h, F.ref, ip, 0, 2, tab, None, None, out)),
           ("M < 0", lambda: call(h, F.ref, ip, -3, 2, tab, None, None, out)),
           ("idx off 8 bytes", lambda: call(h, F.ref, C.c_void_p(odd.data_ptr() + 4), 5, 2, tab, None, None, out)),
           ("offset inf", lambda: call(h, F.ref, ip, 5, 2, tab, dv(0.0, math.inf), None, out)),
           ("offset nan", lambda: call(h, F.ref, ip, 5, 2, tab, dv(math.nan, 0.0), None, out)),
           ("idx NULL, M != N", lambda: call(h, F.ref, None, 5, 2, tab, None, None, out)),
           ("d > 1024", lambda: call(h, Fw.ref, None, 2, 2, tabw, None, None, out)),
           ("unaligned iterate", lambda: call(h, F.ref, ip, 5, 2, tabu, None, None, out)),
           ("K = 0", lambda: call(h, F.ref, ip, 5, 0, tab, None, None, out)),
           ("K = 257", lambda: call(h, F.ref, ip, 5, 257, tab, None, None, out)),
           ("s > 1", lambda: call(h, F.ref, ip, 5, 2, tab, None, dv(1.0, 1.5), out))]
    for what, f in raw:
        assert f() == L.ERR_ARG, what
        assert len(lib.ciao_last_error()) > 20 and ctx.last_kernel() == before, what
    assert call(h, F.ref, ip, 5, 2, tab, dv(0.5, -0.5), dv(1.0, 0.5), out) == 0 and "<rows," in ctx.last_kernel()
    for what, f in [("an empty list", lambda: ctx.margin_stats_multi(F, [x], rows=idx[:0])),
                    ("offsets of another length", lambda: ctx.margin_stats_multi(F, [x, x], offsets=[1.0])),
                    ("an offset that is not finite", lambda: ctx.margin_stats_multi(F, [x], rows=idx, offsets=[math.inf]))]:
        with pytest.raises(L.CiaoError) as e:
            f()
        assert e.value.status == L.ERR_ARG, what
    with pytest.raises(ValueError):
        ctx.margin_stats_multi(F, [x], rows=idx.cpu())
    ctx.synchronize()


# ---- (f) far rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
def test_rows_beyond_two_to_the_31_elements(ctx, dtype):
    """tests/test_gpu_list_passes.py's far-rows matrix: d = 1024, zeros but for row 0, the first row wholly beyond 2^31 elements (fp32:
    2^32) and the last, with labels / targets there.  The list is those three, a repeat of the last and two zero rows; three models with
    offsets, both losses: the bits of the call without a list on the gathered copy, and (without offsets) of section 8.11's kernel on
    it.  The row offset idx * ld and the label's address come from lane reads of the entries' 32-bit halves: a half dropped on the way
    names a row before it -- a zero row -- and the statistics of the list that is the far row alone would be a zero row's."""
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    d, K = 1024, 3
    dt = np.dtype(dtype)
    elems = FR.ELEMS[dt]
    FR.need(elems * dt.itemsize, f"the {tname(dtype)} matrix")
    N = elems // d
    limit = 2 ** 32 if dtype == np.float32 else 2 ** 31
    far = -(-limit // d)
    assert 0 < far < N - 1 and far * d >= limit
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    A = torch.zeros((N, d), dtype=tdt, device="cuda")
    b = torch.zeros(N, dtype=tdt, device="cuda")
    rng = np.random.default_rng(14)
    for r, label in zip((0, far, N - 1), (1.0, -1.0, 1.0)):
        A[r] = torch.from_numpy(rng.standard_normal(d).astype(dtype)).cuda()
        b[r] = label
    idx = torch.tensor([far - 1, 0, far, N - 1, 1, N - 1], dtype=torch.int64, device="cuda")
    xs = [torch.from_numpy(rng.standard_normal(d).astype(dtype)).cuda() for _ in range(K)]
    off, s = [0.5, -0.25, 0.0], [1.0, 0.5, 0.0]
    try:
        Ac, bc = A[idx].contiguous(), b[idx].contiguous()
        for make in (lambda a_, b_: PackedF.least_squares(a_, b_, 1.0), PackedF.logistic):
            F, copy = make(A, b), make(Ac, bc)
            got = ctx.margin_stats_multi(F, xs, s, rows=idx, offsets=off)
            assert "<rows," in ctx.last_kernel() and ",list,offset>" in ctx.last_kernel()
            assert bits(got) == bits(ctx.margin_stats_multi(copy, xs, s, offsets=off))
            plain = ctx.margin_stats_multi(F, xs, s, rows=idx)
            assert bits(plain) == bits(ctx.margin_stats_multi(copy, xs, s))
            assert "<rows," not in ctx.last_kernel()
            # the far row alone is not a zero row, and is the far row
            alone = ctx.margin_stats_multi(F, xs, s, rows=idx[2:3], offsets=off)
            zero = ctx.margin_stats_multi(F, xs, s, rows=idx[0:1], offsets=off)
            assert bits(alone) == bits(ctx.margin_stats_multi(make(Ac[2:3].contiguous(), bc[2:3].contiguous()), xs, s, offsets=off))
            assert all(bits([a]) != bits([z]) for a, z in zip(alone, zero))
    finally:
        del A, b
        torch.cuda.empty_cache()

"""tests/far_rows.py without a GPU: (1) the boundaries and marked rows of every view of tests/test_gpu_far_rows.py; (2) the reduction of
a pass over a zero matrix with marked rows to the gathered rows -- on small dense problems the oracle on the full matrix equals the
oracle (or the restatement far_rows uses where the oracle's own routine runs over all N rows) on the gathered rows with N_total, in bits
for integer LeastSquares data and to 4 eps otherwise, and the int64 restatements of the statistics passes equal numpy on the full matrix;
(3) the proof that the GPU test can fail: for every view and every operation, dropping any one marked row, or replacing a far marked row by
what its offset reaches modulo 2^32 bytes, 2^31 or 2^32 elements, moves some compared output by more than twice the tolerance the GPU test
allows (in bits where it compares bits)."""
import numpy as np
import pytest

import far_rows as FR

BOTH = [pytest.param(np.float64, id="f64"), pytest.param(np.float32, id="f32")]


# ---- 1. boundaries ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", FR.ALL_VIEWS, ids=lambda v: v.id)
def test_boundaries_and_marked_rows(view):
    rows = FR.marked_rows(view)
    assert len(rows) <= FR.MAX_MARKED and {0, 1, view.N - 1} <= set(rows.tolist())
    assert all(0 <= r < view.N and r * view.ld + view.d <= FR.ELEMS[view.dtype] for r in rows.tolist()), "a marked row leaves the buffer"
    reached = FR.boundaries(view)
    assert reached, "the view crosses no boundary"
    for name, B in reached:
        below, straddle, after = FR.rows_at(view, B)
        assert {below, after} <= set(rows.tolist()) and (straddle is None or straddle in rows), name
        assert below * view.ld + view.d <= B and after * view.ld >= B and after - below in (1, 2)
        assert (below + 1) * view.ld + view.d > B, "not the LAST row ending at or below the boundary"
        assert (after - 1) * view.ld < B, "not the FIRST row starting at or after the boundary"
    # byte offsets: every view passes 2^32 bytes; the dense fp32 views pass 2^32 elements, d = 2 passes 2^31 ROWS
    assert any(n == "byte 2^32" for n, _ in reached)
    if view.ld == view.d and view.dtype == FR.F32:
        assert [n for n, _ in reached][-1] == "element 2^32"
    if view.name == "d2":
        assert view.N > 2 ** 31 and 2 ** 31 in rows
    assert FR.peak_row(view) in rows and FR.peak_row(view) * view.ld >= reached[-1][1]
    data = FR.fill(view)
    assert np.array_equal(data.rows, rows) and np.abs(data.A).max() == 4 and np.all(data.A[:, [0, view.d - 1]] != 0)
    assert np.all(data.A == np.rint(data.A)) and len({a.tobytes() for a in data.A}) == data.K
    sq = (data.A.astype(np.float64) ** 2).sum(axis=1)
    assert data.rows[np.argmax(sq)] == FR.peak_row(view) and np.count_nonzero(sq == sq.max()) == 1, "the argmax of the row norms is not one far row"
    ex = FR.block_extra(view)
    assert all(0 <= r < view.N for r in ex)


def test_the_views_cover_the_table():
    for dt in (FR.F32, FR.F64):
        vs = FR.views(dt)
        assert {"d1024", "d1000", "d50", "d8193", "c1024", f"d{FR.LONG_D[dt]}", "guard-below", "guard-at", "s65x1000odd"} <= set(vs)
        assert {f"s{N}x{d}" for N in (5, 65) for d in (50, 1000, 1024)} <= set(vs)
        assert vs["guard-below"].ld == 2 ** 24 - 4 and vs["guard-at"].ld == 2 ** 24 and vs["s65x1000odd"].ld % 2 == 1
        for v in vs.values():
            if v.name.startswith("s") and not v.name.endswith("odd"):
                assert (v.ld * v.es) % 16 == 0 and FR.ELEMS[dt] // v.N - v.ld < 16 // v.es
    assert "d2" in FR.views(FR.F32) and "d2" not in FR.views(FR.F64)


# ---- 2. the reduction to gathered rows ------------------------------------------------------------------------------------------------
MARKED = (0, 1, 7, 63, 64, 100, 198, 199)
BLOCKS = (np.array([0, 63, 100], np.int64), np.array([3, 3, 3], np.int64))


def small(dtype, d, extra=()):
    """(view, Data, full A, full b, full y): N = 200 dense, the zero and marked pattern of the far views"""
    view = FR.View("small", dtype, 200, d, d)
    data = FR.fill(view, extra=extra, marked=MARKED)
    A, b, y = np.zeros((200, d), dtype), np.zeros(200, dtype), np.ones(200, dtype)
    A[data.rows], b[data.rows], y[data.rows] = data.A, data.b, data.y
    return view, data, A, b, y


def same(got, want, loss, what, units=4.0):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if loss == "ls":
        assert np.array_equal(got, want), f"{what}: integer LeastSquares data must match in bits"
    else:
        tol = units * FR.EPS[got.dtype] * max(float(np.abs(want).max()), 1e-30)
        assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= tol, what


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("loss", ["ls", "logistic"])
@pytest.mark.parametrize("d", [3, 50])
def test_the_oracle_on_the_full_matrix_is_the_oracle_on_the_gathered_rows(dtype, loss, d):
    from oracle import oracle as O
    T = dtype
    view, data, A, b, y = small(dtype, d, extra=[int(f) + j for f, n in zip(*BLOCKS) for j in range(n)])
    full = O.Problem(loss, A, y if loss == "logistic" else b, 1.0)
    x = FR.x_vector(d, T)
    # full_pass, the objective
    ref = FR.ref_sweep(data, loss)
    same(ref["av"], O.full_pass(full, x), loss, "full_pass")
    assert np.array_equal(ref["dots"], (A.astype(np.float64) @ x.astype(np.float64)).astype(T)[data.rows])
    if loss == "ls":
        assert abs(ref["objective"][0] - O.objective(full, O.Prox("zero"), x)) <= 4 * FR.EPS[np.dtype(T)] * ref["objective"][0]
    # svrg_inner
    zf, w, av = FR.chain_state(d, T)
    z = np.zeros(d, T)
    g = O.Prox("l1", lam=2.0 ** -6)
    O.svrg_inner(full, g, T(FR.chain_gamma(loss)), FR.chain_steps(data), av, z, zf, w)
    ref = FR.ref_svrg(data, loss)
    same(ref["w"], w, "ls", "svrg_inner w")            # (the same arithmetic on the same rows: bits for both losses)
    same(ref["z"], z, "ls", "svrg_inner z")
    # svrg_init + one svrg_iterate (the epoch the device runs with the cached row dots)
    eav, ez, ezf, ew = O.svrg_init(full, x)
    O.svrg_iterate(full, g, T(FR.chain_gamma(loss)), FR.chain_steps(data), False, eav, ez, ezf, ew)
    ref = FR.ref_svrg_epoch(data, loss)
    same(ref["epoch z_full"], ezf, "ls", "svrg epoch z_full")
    same(ref["epoch w"], ew, "ls", "svrg epoch w")
    same(ref["epoch av"], eav, loss, "svrg epoch av")
    # saga_init, saga_steps
    gamma = T(FR.chain_gamma(loss))
    ref = FR.ref_saga(data, loss)
    table, av, z = O.saga_init(full, g, gamma, x)
    same(ref["init table"], table[data.rows], "ls", "saga_init table")
    assert not table[np.setdiff1d(np.arange(200), data.rows)].any(), "a zero row's table row is not zero"
    same(ref["init av"], av, loss, "saga_init av")
    same(ref["init z"], z, "ls", "saga_init z")
    for sag in (False, True):
        t, a, zz = table.copy(), ref["init av"].copy(), z.copy()   # (from the restated av: the steps, not the init, are compared here)
        O.saga_steps(full, g, gamma, sag, FR.chain_steps(data), t, a, zz)
        for name, v in (("table", t[data.rows]), ("av", a), ("z", zz)):
            same(ref[f"sag{int(sag)} {name}"], v, "ls", f"saga_steps sag={sag} {name}")
    # finito_init (the oracle's own hat_gamma), finito_steps
    g0 = O.Prox("zero")
    gam = T(200 * 2.0 ** -7)
    table, av, z, hg = O.finito_init(full, g0, np.full(200, gam, T), x)
    _, rt, rav, rz = FR.finito_init_restated(data, loss, 1.0, g0, x, params=(gam, hg))
    same(rt, table[data.rows], "ls", "finito_init table")
    assert np.array_equal(table[np.setdiff1d(np.arange(200), data.rows)], np.broadcast_to(x, (200 - data.K, d))), "a zero row's table row is not x0"
    # av = hat_gamma sum_i s_i / gamma_i: the restatement adds in float64, the oracle pairwise in T over all 200 rows with a hat_gamma of its
    # own summing (14 eps32 between them in Float32): the formula is held to the Float64 oracle on the same data, to 4 eps64
    A64 = O.Problem(loss, A.astype(np.float64), (y if loss == "logistic" else b).astype(np.float64), 1.0)
    _, av64, z64, hg64 = O.finito_init(A64, g0, np.full(200, np.float64(gam)), x.astype(np.float64))
    _, _, rav, rz = FR.finito_init_restated(data.astype(np.float64), loss, 1.0, g0, x.astype(np.float64), params=(np.float64(gam), hg64))
    # (the oracle's pairwise sum of 200 rounded quotients, times hat_gamma: ceil(log2 200) + 3 = 11 roundings of eps / 2 each at the most;
    # all terms x0 / gamma up to K of them, so that is relative to the result)
    same(rav, av64, "logistic", "finito_init av", units=5.5)
    same(rz, z64, "logistic", "finito_init z", units=5.5)
    ref = FR.ref_finito(data, loss)
    gamf, hgf = (T(v) for v in FR.finito_gam(view))
    runs = [(f"lists r={r}", FR.finito_batches(data, r)) for r in (1, 3)]
    for name, batches in runs:
        st, a, zz = FR.finito_state(data, T)
        t = np.zeros((200, d), T)
        t[data.rows] = st
        O.finito_steps(full, g0, np.full(200, gamf, T), hgf, batches, t, a, zz)
        for out, v in (("table", t[data.rows]), ("av", a), ("z", zz)):
            same(ref[f"{name} {out}"], v, "ls", f"finito_steps {name} {out}")
    # the lfinito iteration (restated in far_rows: the oracle's own full pass runs over all N rows)
    gv = np.full(200, T(0.4), T)
    av, z, zf, hg = O.lfinito_init(full, gv, x)
    ref = FR.ref_lfinito(data, loss, params=(T(0.4), hg), blocks=BLOCKS)
    same(ref["init av"], av, "ls", "lfinito_init av")
    O.lfinito_iterate(full, g0, gv, hg, [np.arange(f, f + n) for f, n in zip(*BLOCKS)], av, z, zf)
    for name, v in (("av", av), ("z", z), ("z_full", zf)):
        same(ref[name], v, "ls", f"lfinito_iterate {name}")


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("d", [3, 50])
def test_adaptive_finito_and_proshi_steps_on_the_gathered_rows(dtype, d):
    """the same arithmetic on the same rows: bits"""
    from oracle import oracle as O
    T = dtype
    view, data, A, b, y = small(dtype, d)
    rest = np.setdiff1d(np.arange(200), data.rows)
    # afinito_steps from the consistent state of far_rows.afinito_state, the other samples at x_i = 0 (c_i = f_i = 0)
    alpha, tol_b, _, hg = FR.afinito_params(view)
    st, c, f, gam, dots, av, z = FR.afinito_state(data, T)
    table, gtable, gfull, ffull = np.zeros((200, d), T), np.zeros((200, d), T), np.full(200, gam[0], T), np.zeros(200, T)
    table[data.rows], gtable[data.rows], ffull[data.rows] = st, (c[:, None] * data.A).astype(T), f
    done, hg1, trials = O.afinito_steps(O.Problem("ls", A, b, 1.0), O.Prox(FR.FINITO_PROX), T(alpha), T(tol_b), FR.chain_steps(data), table, gtable,
                                        gfull, ffull, T(hg), av, z)
    ref = FR.ref_afinito(data)
    assert ref["counts"].tolist() == [done, trials] == [40, 40], "a step backtracked"
    for name, v in (("table", table[data.rows]), ("gradient table", gtable[data.rows]), ("gam", gfull[data.rows]), ("f", ffull[data.rows]), ("av", av),
                    ("z", z), ("hat_gamma", np.array([hg1], T))):
        same(ref[name], v, "ls", f"afinito_steps {name}")
    assert not table[rest].any() and not gtable[rest].any()
    # proshi_steps with Q = q = the matrix
    gam, hg, eta, lo, hi, ghi = FR.proshi_params(view)
    st, av, _ = FR.finito_state(data, T)
    table = np.zeros((200, d), T)
    table[data.rows] = st
    z = (FR.x_vector(d, T, 2) / T(gam)).astype(T)
    O.proshi_steps(O.SepQuad(A, A.copy(), eta, lo, hi), O.Prox("box", lo=-np.inf, hi=ghi, dtype=T), np.full(200, T(gam), T), T(hg),
                   FR.proshi_batches(data), table, av, z)
    ref = FR.ref_proshi(data)
    for name, v in (("table", table[data.rows]), ("av", av), ("z", z)):
        same(ref[name], v, "ls", f"proshi_steps {name}")
    assert not table[rest].any()


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("d", [3, 50])
def test_the_statistics_restatements_are_numpy_on_the_full_matrix(dtype, d):
    view, data, A, b, y = small(dtype, d)
    ref = FR.ref_stats(data)
    A, b, y = A.astype(np.float64), b.astype(np.float64), y.astype(np.float64)
    sq = (A * A).sum(axis=1)
    assert np.array_equal(ref["row_sqnorms"], sq[data.rows]) and np.count_nonzero(sq) == data.K
    assert np.array_equal(ref["row_sqnorm_stats"], [sq.max(), np.argmax(sq), sq.min(), sq.sum()])
    assert np.array_equal(ref["col_sqnorms"], (A * A).sum(axis=0))
    assert np.array_equal(ref["col_moments s1"], (A - A[0]).sum(axis=0)) and np.array_equal(ref["col_moments s2"], ((A - A[0]) ** 2).sum(axis=0))
    assert np.array_equal(ref["scaled"], (A * FR.x_vector(d, np.float64, 5))[data.rows].astype(dtype))
    assert np.array_equal(ref["gram G"], A.T @ A) and np.array_equal(ref["gram u"], A.T @ b) and np.array_equal(ref["gram colsum"], A.sum(axis=0))
    assert np.array_equal(ref["gram bsum"], [b.sum(), (b * b).sum()])
    x = FR.x_vector(d, np.float64)
    r = A @ x - b
    assert np.array_equal(ref["margin_stats ls"], [(r * r).sum(), b.sum(), (b * b).sum(), np.abs(r).max()])
    t = y * (A @ x)
    got = ref["margin_stats logistic"]
    assert abs(got[0] - np.sum(np.maximum(-t, 0) + np.log1p(np.exp(-np.abs(t))))) <= 200 * FR.EPS[FR.F64] * got[0]
    assert got[1] == np.count_nonzero(t <= 0) and got[2] == t.min()
    for K in (3, 17):
        X = np.stack(FR.models(d, np.float64, K))
        R = A @ X.T - b[:, None]
        assert np.array_equal(ref[f"margin_stats_multi K={K}"], np.stack([(R * R).sum(axis=0), np.full(K, b.sum()), np.full(K, (b * b).sum()), np.abs(R).max(axis=0)], axis=1))
    for K in (2, 17):
        X = np.stack(FR.models(d, np.float64, K))
        assert np.array_equal(ref[f"full_gradient_multi K={K}"], (A.T @ (A @ X.T - b[:, None])).T)


# ---- 3. the GPU test would notice ----------------------------------------------------------------------------------------------------------
def moved(op, ref, mut, dtype):
    """an output of `mut` that the GPU test would refuse where the device gave it: beyond twice the tolerance, or other bits"""
    for name, (want, scale) in ref.items():
        got = mut[name][0]
        if scale is None:
            if not np.array_equal(np.asarray(want), np.asarray(got)):
                return name
        elif np.abs(np.asarray(want, np.float64) - np.asarray(got, np.float64)).max() > 2 * FR.tolerance(scale, want, dtype):
            return name
    return None


@pytest.mark.parametrize("view", FR.ALL_VIEWS, ids=lambda v: v.id)
def test_a_dropped_or_aliased_row_changes_every_reference(view):
    far = 0
    for op in FR.ops_of(view):
        data = FR.data_of(view, op)
        ref = FR.reference(op, data)
        ms = FR.mutants(view, data)
        assert sum(w.endswith("dropped") for w, _ in ms) == len(FR.marked_rows(view))
        far += sum("modulo" in w for w, _ in ms)
        for what, m in ms:
            assert moved(op, ref, FR.reference(op, m), view.dtype) is not None, f"{view.id} {op}: {what} goes unnoticed"
    assert far > 0, "no marked row lies beyond a wrap"


def test_the_host_sampler_refuses_what_32_bit_fractions_cannot_index():
    """sampling.py draws a row as a 32-bit fraction of N: N < 2^32 is its real limit, refused, never drawn wrongly; the d = 2 view's row
    count lies under it and its draws pass 2^31"""
    import ciao_loader
    ciao = ciao_loader.load()
    N = FR.views(FR.F32)["d2"].N
    assert 2 ** 31 < N < 2 ** 32
    idx = ciao.IndexStream(7).rand_indices(N, 4096)
    assert idx.dtype == np.int64 and 0 <= idx.min() and 2 ** 31 <= idx.max() < N
    with pytest.raises(AssertionError):
        ciao.IndexStream(7).rand_indices(2 ** 32, 4)


def test_the_scales_stay_inside_the_baseline():
    """as tests/test_tolerances.py for the files it reads: 1e-10 (Float64), and 1e-4 (Float32) for the form against the Float64 oracle; a Float32
    scale beyond 1e-4 against the Float32 oracle only beside that form"""
    f64_max, f32_max = 1e-10 / FR.EPS[FR.F64], 1e-4 / FR.EPS[FR.F32]
    for key, (scale, scale64) in FR.SCALES.items():
        a, b = (scale[64], scale[32]) if isinstance(scale, dict) else (scale, scale)
        assert a <= f64_max and (scale64 is None or scale64 <= f32_max + 1.2), key
        assert b <= f32_max + 1.2 or scale64 is not None, key

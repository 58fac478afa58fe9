"""tests/rows_exact.py on the CPU: (1) its restatement of the five rows modes equals the oracle (oracle/twin.py, Float64) in bits on
power-of-two N; (2) the bound that makes every order of addition exact holds for every case tests/test_gpu_rows_exact.py runs; (3) the
launches whose grid the host knows reach every required trip class on 256 and on 304 compute units; (4) planted defects: bit
comparison notices a dropped row, a doubled row, a dropped last chunk, a dropped partial, a stale partial and an extra scalar short
by one term -- and does NOT notice the order of addition."""
import numpy as np
import pytest

import rows_exact as X

F64, F32 = np.float64, np.float32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int64 if a.dtype == F64 else np.int32),
                                                                        b.view(np.int64 if b.dtype == F64 else np.int32))


# ---- 1. the restatement against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", [(64, 50), (256, 257)])
def test_restatement_equals_the_oracle_in_bits(N, d):
    from oracle import twin as O
    P = X.Problem(N, d, seed=N + d)
    assert P.Nt == N and P.b.dtype == F64
    B = X.Bounds()
    op = O.Problem("ls", P.A, P.b, P.lam)
    g = X.grad(P, N, B)
    assert same_bits(np.asarray(O.full_pass(op, P.x0)), g["av"])
    assert O.objective(op, O.Prox("zero"), P.x0) == g["obj"]
    assert same_bits(P.A @ P.x0, g["dots"])                            # (the cached row dots: plain a_i'x)
    rt, rav, rz = O.saga_init(op, O.Prox("l1", lam=P.saga_lam_g), P.saga_gamma, P.x0)
    s = X.saga_init(P, N, B)
    assert same_bits(rt, s["table"]) and same_bits(rav, s["av"]) and same_bits(rz, s["z"])
    # Finito's init forms hat_gamma = 1 / sum_i 1 / gam_i itself: a power of two for uniform gam only (both lattice values in turn)
    for gam in (N / 2.0, N / 4.0):
        Q = X.Problem(N, d, seed=N + d)
        Q.gam[:] = gam
        Q.hg = gam / N
        Q.lam_g = Q.gl / Q.hg
        rt, rav, rz, rhg = O.finito_init(op, O.Prox("l1", lam=Q.lam_g), Q.gam, Q.x0)
        f = X.finito_init(Q, N, B)
        assert rhg == Q.hg and same_bits(rt, f["table"]) and same_bits(rav, f["av"]) and same_bits(rz, f["z"])
    # the batches take hat_gamma as a number: mixed gam, the module's hat_gamma, index lists and row blocks
    og = O.Prox("l1", lam=P.lam_g)
    op2 = O.Problem("ls", P.A, P.b2, P.lam)
    for lists in (True, False):
        rows = X.batch_rows(P, N // 2, lists)
        table, av, z = P.start_table().copy(), P.av.copy(), P.z.copy()
        O.finito_steps(op, og, P.gam, P.hg, [rows], table, av, z)
        f = X.finito_batch(P, rows, B)
        assert same_bits(table, f["table"]) and same_bits(av, f["av"]) and same_bits(z, f["z"])
        av, z, zf = P.av.copy(), np.zeros(d), np.zeros(d)
        O.lfinito_iterate(op2, og, P.gam, P.hg, [rows], av, z, zf)
        f = X.lfinito_batch(P, rows, B)
        assert same_bits(av, f["av"]) and same_bits(z, f["z"]) and same_bits(zf, f["zf"])
    assert B.worst() < 53


# ---- 2. the bound, for every case of the GPU file ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", X.CASES, ids=lambda c: c.name)
def test_every_sum_of_every_case_is_exact_in_any_order(case, dtype):
    for loss in ("ls",) + (("logistic",) if case.logistic else ()):
        P = case.problem(dtype, 256, loss)
        B = X.Bounds()
        for n, _ in case.launches(dtype, 256):
            for mode in case.modes:
                if loss == "logistic" and mode.startswith("lfinito"):
                    continue
                for v in X.reference(P, mode, n, B).values():
                    X.lossless(v, dtype)
        assert B.worst() < X.LIMIT_BITS, (case.name, loss, sorted(B.bits.items(), key=lambda kv: -kv[1])[:3])


@pytest.mark.parametrize("name,d,_f,_o", X.FINALIZE_SHAPES, ids=[s[0] for s in X.FINALIZE_SHAPES])
def test_the_finalize_problems_are_exact_in_any_order(name, d, _f, _o):
    for dtype in (F64, F32):
        B = X.Bounds()
        g = X.grad(X.finalize_problem(d(X.vec_of(dtype))), X.FINALIZE_ROWS, B)
        X.lossless(g["av"], dtype), X.lossless(g["extra"], dtype)
        assert B.worst() < X.LIMIT_BITS, sorted(B.bits.items(), key=lambda kv: -kv[1])[:3]


# ---- 3. the trip classes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_cu", [256, 304])
def test_the_forced_grids_reach_every_trip_class(num_cu):
    for case in X.CASES:
        for dtype in (F64, F32):
            got = [c for _, c in case.forced(dtype, num_cu)]
            reached = set().union(*(X.classes(c) for c in got))
            need = set().union(*(X.required(c) for c in got))
            assert need <= reached, (case.name, dtype.__name__, num_cu, sorted(need - reached))
            assert max(n for n, _ in case.launches(dtype, num_cu)) <= 4096


def test_classifier_reads_the_launch_reports():
    c = X.classify("rows_multi_kernel<f64,K2,mode0> grid=2 block=256", 4 * 9 - 3, 256)
    assert (c["workers"], c["unit"], c["trips"], c["short"], c["parts"]) == (8, 4, [1] * 7 + [2], 1, 2)
    c = X.classify("rows_long_kernel<f32,J4,mode4> segments=5 clusters=51 grid=255 block=256", 103, 16416)
    assert (c["workers"], c["parts"], c["trips"][0], c["trips"][-1]) == (51, 51, 2, 3)
    c = X.classify("rows_generic_kernel<f64,NW4,mode0,global_acc> grid=3 block=256", 5, 9217)
    assert (c["workers"], c["parts"], c["trips"]) == (12, 12, [0] * 7 + [1] * 5)
    c = X.classify("rows_small_kernel<f32,mode3,I8> grid=1 block=256", 21, 50)
    assert (c["unit"], c["trips"], c["short"]) == (10, [0, 1, 1, 1], 1)
    assert X.classes(c) == {"an idle worker", "1 trip", "a short last unit"} and "an idle worker" in X.required(c)


# ---- 4. planted defects -----------------------------------------------------------------------------------------------------------------------
def device_like(P, n, dtype, workers=7, drop=None, twice=None, short_chunk=None, drop_partial=None, stale=None, extra_short=None, seed=0):
    """A GRAD sweep as a device would form it, IN the type: the rows dealt to `workers` in turn, every worker's rows added in a shuffled
    order, the partials added in a shuffled order -- with one defect planted.  -> (av, extra) in the type"""
    rng = np.random.default_rng(seed)
    A, x, b = P.A[:n].astype(dtype), P.x0.astype(dtype), P.b[:n].astype(dtype)
    lam, v = dtype(P.lam), X.vec_of(dtype)
    parts, extras = np.zeros((workers, P.d), dtype), np.zeros(workers, dtype)
    for w in range(workers):
        rows = list(range(w, n, workers))
        rng.shuffle(rows)
        for i in rows:
            if i == drop:
                continue
            cols = P.d - v if i == short_chunk else P.d
            dot = dtype(0)
            for k in rng.permutation(cols):
                dot += A[i, k] * x[k]
            r = dot - b[i]
            for _ in range(2 if i == twice else 1):
                parts[w] += (r * lam) * A[i]
            if i != extra_short:
                extras[w] += (lam / dtype(2)) * r * r
    order = [w for w in rng.permutation(workers) if w != drop_partial]
    tot, ex = np.zeros(P.d, dtype), dtype(0)
    for w in order:
        tot += parts[w]
    for w in rng.permutation(workers):
        ex += extras[w]
    if stale is not None:
        tot += stale
    return (dtype(1) / dtype(P.Nt)) * tot, ex


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_bit_comparison_notices_each_planted_defect(dtype):
    n, d = 90, 50
    P = X.Problem(n, d, seed=11)
    ref = X.grad(P, n, X.Bounds())
    want, want_extra = X.lossless(ref["av"], dtype), X.lossless(ref["extra"], dtype)
    for seed, workers in ((0, 7), (1, 4), (2, 90), (3, 1)):            # any deal, any order: the same bits
        av, ex = device_like(P, n, dtype, workers=workers, seed=seed)
        assert same_bits(av, want) and same_bits(np.array(ex), np.array(want_extra))
    res = ref["dots"] - P.b[:n]
    v = X.vec_of(dtype)
    live = int(np.flatnonzero(res != 0)[3])                            # a row that contributes (a zero residual contributes nothing to drop)
    chunk = int(np.flatnonzero((res != 0) & ((P.A[:n, d - v:] * P.x0[d - v:]).sum(axis=1) != 0))[0])
    stale = np.zeros(d, dtype)
    stale[17] = 1
    for what, kw, hits_av in (("a row dropped", dict(drop=live), True), ("a row taken twice", dict(twice=live), True),
                              ("the last chunk of one row dropped", dict(short_chunk=chunk), True), ("one partial dropped", dict(drop_partial=2), True),
                              ("one stale partial added", dict(stale=stale), True), ("the extra scalar short by one term", dict(extra_short=live), False)):
        av, ex = device_like(P, n, dtype, **kw)
        assert same_bits(av, want) != hits_av, what
        assert not (same_bits(av, want) and same_bits(np.array(ex), np.array(want_extra))), what

"""tests/complex_exact.py on the CPU: (1) its restatement of the complex chain steps and of the complex rows modes equals the oracle
(oracle/twin.py on complex data) IN BITS, in both types, after every compared step count; (2) the bound that makes every association exact
holds for every case, and the largest figure is printed; the device file's cases are well formed; (3) every live step matters; (4)
planted defects change the bits of a compared output in every case where they apply.

Exempt from (3): under Finito (whose iterate is 0 after every prox: the dead zone) a repeat of a row rewrites the table row with the value
it has and the aggregate telescopes over the row's visits -- every visit of a designed repeat and of the seven-fold row; they are held by
the stale-row defect at the second visit.  Under LFinito in the dead zone z = z_full = 0: the step's two gradients cancel in av and NO step of its chain matters, nor does any
defect of a dot product, of b_i or of gamma_i -- what its device cases hold is that the chain leaves the full pass's av, z = 0 and
z_full = 0 in bits (complex_exact's docstring says so as well)."""
import numpy as np
import pytest

import complex_exact as E
import rows_exact as X

F64, F32 = np.float64, np.float32
_found = {}


def found(spec):
    if spec.name not in _found:
        _found[spec.name] = E.found(spec)
    return _found[spec.name]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    view = lambda v: v.view(np.int64 if v.dtype == F64 else np.int32)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(view(a), view(b))


def differs(ref, got):
    return any(not same_bits(ref[k][name], got[k][name]) for k in ref for name in ref[k])


BY_NAME = {s.name: s for s in E.HOST_SPECS}
SPEC_IDS = list(BY_NAME)
PAIRS = [pytest.param(s.name, dt, id=f"{s.name}-{'f64' if dt == F64 else 'f32'}") for s in E.HOST_SPECS for dt in (F64, F32)
         if dt == F64 or s.limit == X.LIMIT_BITS]


# ---- 1. the restatement against the oracle -----------------------------------------------------------------------------------------------------
def oracle_chain(P, k, dtype):
    from oracle import twin as O
    s = P.spec
    ctype = np.complex128 if dtype == F64 else np.complex64
    c = lambda v: X.lossless(E.pairs(v), dtype)                          # complex128 -> (re, im) pairs of the type, without rounding
    cc = lambda v: c(v).view(ctype).reshape(np.shape(v))
    op = O.Problem("ls", cc(P.A), cc(P.b), P.lam, N_total=E.N)
    g = O.Prox("l1_complex", lam=P.lam_g, dtype=dtype) if s.prox == "dead" else O.Prox("zero", dtype=dtype)
    idx = P.idx[:k]
    gam = X.lossless(P.gam, dtype)
    if s.alg == "svrg":
        av, z, zf, w = c(P.av0), c(P.z0), c(P.zf0), c(P.p0)
        O.svrg_inner(op, g, dtype(P.gamma), idx, av, z, zf, w)
        return {"z": z, "w": w}
    if s.alg in ("saga", "sag"):
        table, av, z = c(P.table0), c(P.av0), c(P.p0)
        O.saga_steps(op, g, dtype(P.gamma), s.alg == "sag", idx, table, av, z)
        return {"z": z, "av": av, "table": table}
    if s.alg == "finito":
        table, av, z = c(P.table0), c(P.av0), c(P.p0)
        O.finito_steps(op, g, gam, dtype(E.HG), P.batches(k), table, av, z)
        return {"z": z, "av": av, "table": table}
    av, z, zf = c(P.av0), c(P.p0), c(P.zf0)
    O.lfinito_iterate(op, g, gam, dtype(E.HG), P.batches(k), av, z, zf)
    return {"av": av, "z": z, "z_full": zf}


@pytest.mark.parametrize("name,dtype", PAIRS)
def test_chain_restatement_equals_the_oracle_in_bits(name, dtype):
    P, B, ref = found(BY_NAME[name])
    for k in P.spec.counts:
        got = oracle_chain(P, k, dtype)
        for what, want in ref[k].items():
            assert same_bits(got[what], X.lossless(want, dtype)), f"{name}: {what} after {k} steps differs from the oracle's"


# ---- 2. the bound; the cases -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SPEC_IDS)
def test_every_sum_of_every_chain_step_is_exact_in_any_association(name):
    P, B, ref = found(BY_NAME[name])
    s = P.spec
    assert s.limit in (X.LIMIT_BITS, 53) and (s.limit == 53) == name.endswith("_f64only")
    top = sorted(B.bits.items(), key=lambda kv: -kv[1])[:3]
    print(f"{name}: seed {P.seed}, the largest sums in log2 quanta: {top}")
    assert B.worst() < s.limit, top
    for k in ref:
        for v in ref[k].values():
            X.lossless(v, F32 if s.limit == X.LIMIT_BITS else F64)
    steps = set(np.nonzero(P.live)[0])
    assert set(E.live_steps(s.nsteps, s.depth, s.marks, s.counts)) <= steps
    assert not P.A[E.NLIVE:].any() and not P.table0[E.NLIVE:].any() and not P.b[E.NLIVE:].any()
    assert all(P.idx[k] < E.NLIVE for k in steps) and all(P.idx[k] >= E.NLIVE for k in set(range(s.nsteps)) - steps)
    assert set(np.unique(np.abs(P.A.real))) <= {0.0, 1.0} and set(np.unique(np.abs(P.A.imag))) <= {0.0, 1.0}
    E.check_placements(P)


def test_the_device_chain_cases_are_well_formed():
    kinds, seen = set(), set()
    for f, alg, r, dtype in E.chain_cases():
        s = f.spec(alg, dtype, r)
        n, pc = f.n(dtype), E.pc_of(dtype)
        rowb = 2 * n * np.dtype(dtype).itemsize
        kinds.add((f.kind, dtype))
        if (f.name, dtype) not in seen:
            seen.add((f.name, dtype))
            cols = E.marked_entries(n, pc)
            assert cols[0] == 0 and cols[-1] == n - 1 and len(set(cols)) == len(cols) <= E.MARKED
            for w in range(min(4, -(-n // (64 * pc)))):                      # every wave's share, by entries and by chunks
                assert any((c % 256) // 64 == w for c in cols) and any((c // pc % 256) // 64 == w for c in cols), (f.name, w)
            if pc == 2 and n > 2:                                            # both entries of the first and of the last chunk
                assert {0, 1} <= set(cols) and {(n - 1) // 2 * 2, n - 1} <= set(cols)
            if f.kind == "cdma":                                             # chain_launch.inc plan_chain / ring_row_class
                assert rowb % 16 == 0 and rowb <= 16384
                J = next(j for j in (1, 2, 4) if j * 4096 >= rowb)
                assert (f._J, f.masked) == (J, J * 4096 != rowb), f.name
            elif f.kind == "creg":
                assert E._of(f._EP, dtype) == next(e for e in (1, 2, 4, 8) if e * 256 >= n)
                assert rowb % 16 != 0 or f.opts(dtype).get("chain_no_dma"), f.name
            else:
                assert n > 2048 or f.opts(dtype).get("chain_big")
        dep = f.depth(alg)
        assert s.n == n and {1, 2, dep + 1, 511, 512, 513, 1025, 1100} <= set(s.counts)
        assert set(s.repeats) >= (set(range(1, dep + 2)) if alg in E.TABLE_ALGS else set())
        E.check_placements(E.Chain(s, s.seed0))
    assert kinds == {(k, t) for k in ("cdma", "creg", "cbig") for t in (F64, F32)}
    assert any(f.kind == "creg" and f.n(F32) % 2 == 1 and not f.opts(F32) for f in E.FORMS)       # an odd complex count in fp32, unforced
    for name in E.RING_VS_REG:
        assert E.FORM_BY_NAME[name].kind == "cdma" and E.FORM_BY_NAME[name].n(F32) <= 2048


def test_the_classifier_reads_the_complex_launchers_reports():
    c = E.classify_chain("chain_cdma_kernel<f64,J2,alg0,masked> grid=1 block=256 steps=5")
    assert (c["kind"], c["J"], c["alg"], c["masked"], c["threads"], c["steps"], c["dtype"]) == ("cdma", 2, 0, True, 256, 5, F64)
    c = E.classify_chain("chain_cplx_reg_kernel<f32,alg1,EP4> grid=1 block=256 steps=600")
    assert (c["kind"], c["EP"], c["alg"], c["masked"], c["dtype"]) == ("creg", 4, 1, False, F32)
    c = E.classify_chain("chain_cplx_kernel<f64,alg3> grid=1 block=1024 steps=9")
    assert (c["kind"], c["alg"], c["threads"]) == ("cbig", 3, 1024)
    with pytest.raises(AssertionError):
        E.classify_chain("chain_dma_kernel<f64,J2,alg0> grid=1 block=256 steps=5")


# ---- 3. every live step matters -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in SPEC_IDS if "lfinito" not in n])
def test_every_live_chain_step_matters(name):
    P, B, ref = found(BY_NAME[name])
    s = P.spec
    keep = {}
    assert not differs(ref, E.run(P, keep=keep))
    last = {s.nsteps: ref[s.nsteps]}
    idle = [int(k) for k in np.nonzero(P.live)[0] if not differs(last, E.run(P, counts=[s.nsteps], resume=(int(k), keep[int(k)])))]
    if s.alg == "finito":                                                    # (the module docstring: the visits of a row that comes again)
        again = {int(i) for i in np.nonzero(np.bincount(P.idx[P.live], minlength=E.N) > 1)[0]}
        idle = [k for k in idle if int(P.idx[k]) not in again]
    assert not idle, f"{name}: the chain without live step(s) {idle} ends in the same bits"


def test_no_step_of_the_dead_zone_lfinito_chain_matters():
    """what the module docstring states: z = z_full = 0, the two gradients cancel"""
    P, B, ref = found(BY_NAME["host_lfinito_n300"])
    assert not differs(ref, E.run(P, D={"skip": 1})) and not differs(ref, E.run(P, D={"b_from": (None, 0)}))
    assert not any(ref[k]["z"].any() or ref[k]["z_full"].any() for k in ref) and ref[1]["av"].any()


# ---- 4. planted defects ----------------------------------------------------------------------------------------------------------------------------------
def planted(name, D):
    P, B, ref = found(BY_NAME[name])
    return differs(ref, E.run(P, D=D))


LIVE_DOTS = ["host_svrg_n300", "host_saga_n300", "host_sag_n300", "host_svrg_n64", "host_saga_n64_f64only", "host_svrg_n1001_depth1", "host_saga_n300_depth1"]
FIRST_BATCH_DOTS = ["host_finito_n300", "host_finito_n300_r2", "host_finito_n300_r5", "host_finito_n64"]     # step 0 (r > 1: the first batch) runs on p0


@pytest.mark.parametrize("name", ["host_saga_n300", "host_sag_n300", "host_finito_n300", "host_finito_n300_r2", "host_saga_n64_f64only",
                                  "host_finito_n64", "host_saga_n300_depth1"])
def test_a_stale_table_row_inside_a_chunk_and_across_step_512(name):
    P, B, ref = found(BY_NAME[name])
    assert P.placed
    for k, places in P.placed.items():
        for a, b, m in places:
            assert planted(name, {"stale": b}), f"{name}: the table row of step {a} read stale at step {b} (distance {k}, boundary {m}) goes unnoticed"


@pytest.mark.parametrize("name", ["host_saga_n300_run7_f64only", "host_sag_n300_run5_f64only", "host_finito_n300_run7"])
def test_a_stale_table_row_in_the_run_of_one_row_across_step_512(name):
    P, B, ref = found(BY_NAME[name])
    a = E.CCHUNK - P.spec.run // 2
    late = range(a + 1, a + P.spec.run) if P.spec.alg != "finito" else (a + 1,)     # (Finito: the later visits rewrite the same value)
    for b in late:
        assert planted(name, {"stale": b}), (name, b)


@pytest.mark.parametrize("name", ["host_saga_n300", "host_sag_n300", "host_finito_n300", "host_finito_n300_r2"])
def test_the_imaginary_half_of_b_or_gamma_from_another_slot(name):
    P, B, ref = found(BY_NAME[name])
    K = E.CCHUNK
    assert planted(name, {"b_im_from": (K, 0)}), "slot 0 of the second chunk holds the first chunk's imaginary part of b_i"
    assert planted(name, {"b_from": (K, 0)})
    k = next(int(k) for k in np.nonzero(P.live)[0] if k + 1 < P.spec.nsteps and P.live[k + 1] and P.b[P.idx[k]].imag != P.b[P.idx[k + 1]].imag)
    assert planted(name, {"b_im_from": (k, k + 1)}), "the imaginary half of s_b read from the neighbouring slot"
    if P.spec.alg == "finito":
        assert planted(name, {"gam_from": (K, 0)})


@pytest.mark.parametrize("name", LIVE_DOTS + FIRST_BATCH_DOTS)
def test_complex_only_mistakes_change_bits(name):
    """on every step; and on ONE step alone for most of the first live steps (a single step can hide a mistake by coincidence: the two
    entries' cross terms cancelling, a share whose parts are equal).  Finito in the dead zone has live dots in its first batch only:
    r = 2 and r = 5 take the dot defects, every Finito case the gradient's conjugation (its residual is -b_i on every later step)"""
    P, B, ref = found(BY_NAME[name])
    n, pc = P.n, P.spec.pc
    assert planted(name, {"no_conj": None}), "the conjugation sign in the gradient"
    if name in FIRST_BATCH_DOTS and P.spec.r == 1:
        return
    assert planted(name, {"conj_dot": None}), "a.x with conjugation"
    assert planted(name, {"drop_cross": None}), "one cross term of the product dropped"
    first = [int(k) for k in np.nonzero(P.live)[0][:8]] if name in LIVE_DOTS else []
    for key in ("no_conj", "conj_dot", "drop_cross"):
        assert sum(planted(name, {key: k}) for k in first) >= len(first) // 2 + (1 if first else 0), (name, key)
    rows = P.idx[:P.spec.r] if name in FIRST_BATCH_DOTS else P.idx[P.live]
    entries = sorted({int(e) for i in rows for e in np.nonzero(P.A[i])[0]})
    for by in (lambda e: (e % 256) // 64, lambda e: (e // pc % 256) // 64):      # a wave's share, by entries (register chains) and by chunks (the ring)
        swapped = []
        for wave in sorted({by(e) for e in entries}):
            share = np.array([e for e in range(n) if by(e) == wave])
            swapped.append(planted(name, {"swap": (None, share)}))
            assert planted(name, {"dot": (None, share, 0.0)}), f"wave {wave}'s share dropped"
        # (a first batch of two rows can hold an entry whose product has equal parts: there, some wave's swap must show; elsewhere every wave's)
        assert any(swapped) if name in FIRST_BATCH_DOTS else all(swapped), f"re and im swapped in one wave's share of every dot: {swapped}"
    e0 = entries[0]
    assert planted(name, {"dot": (None, np.array([e for e in range(n) if e % 64 == e0 % 64]), 0.0)}), "one lane's share dropped"
    assert planted(name, {"dot": (None, np.array([n - 1]), 0.0)}), "the last entry dropped"
    if pc == 2:
        assert {e % 2 for e in entries} == {0, 1}
        assert planted(name, {"dot": (None, np.arange(1, n, 2), 0.0)}), "every chunk's second entry dropped"


def test_the_order_of_sagas_and_sags_av_update_swapped():
    for name in ("host_saga_n300", "host_sag_n300"):
        P, B, ref = found(BY_NAME[name])
        keep = {}
        E.run(P, keep=keep)
        assert planted(name, {"swap_sag": None})
        moved = [k for k in keep["moved"] if P.live[k]]
        assert len(moved) > 40
        moved = moved[::3]                                                   # (every third: each costs a chain)
        seen = [k for k in moved if planted(name, {"swap_sag": k})]        # (no box here: every single swapped step shows)
        assert seen == moved and {k < E.CCHUNK for k in seen} == {True, False}, (name, len(seen), len(moved))


def test_the_prox_of_a_short_last_finito_batch_skipped():
    """in the dead zone the iterate is 0 after the first batch's prox whether or not a short last batch ends in one: the defect shows
    where the short batch is the first (1 .. 4 steps of r = 5, 1 step of r = 2)"""
    for name, short in (("host_finito_n300_r5", {1, 2}), ("host_finito_n300_r2", {1})):
        P, B, ref = found(BY_NAME[name])
        got = E.run(P, D={"no_last_prox": True})
        seen = {k for k in P.spec.counts if not same_bits(ref[k]["z"], got[k]["z"])}
        assert seen == short & set(P.spec.counts), (name, seen)


# ---- the rows sweeps ---------------------------------------------------------------------------------------------------------------------------------------
ROWS_HOST = [(3, 64), (35, 1024), (128, 64), (2000, 64)]                     # (complex entries, rows): the oracle's passes take all N_total rows


def _oracle_rows(P, dtype):
    from oracle import twin as O
    ctype = np.complex128 if dtype == F64 else np.complex64
    c = lambda v: X.lossless(E.pairs(v), dtype)
    op = O.Problem("ls", c(P.A).view(ctype).reshape(P.A.shape), c(P.b).view(ctype), P.lam)
    return O, op, O.Prox("zero", dtype=dtype), c


@pytest.mark.parametrize("dtype", [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")])
@pytest.mark.parametrize("n,k", ROWS_HOST)
def test_rows_restatement_equals_the_oracle_in_bits(n, k, dtype):
    P, B = E.RowsProblem(k, n, seed=n), X.Bounds()
    assert P.Nt == k
    O, op, g, c = _oracle_rows(P, dtype)
    ref = E.rows_reference(P, "grad", k, B)
    assert same_bits(O.full_pass(op, c(P.x0)), X.lossless(ref["av"], dtype)) and O.objective(op, g, c(P.x0)) == ref["obj"]
    ref = E.rows_reference(P, "saga_init", k, B)
    table, av, z = O.saga_init(op, g, dtype(P.saga_gamma), c(P.x0))
    assert all(same_bits(u, X.lossless(ref[w], dtype)) for u, w in ((table, "table"), (av, "av"), (z, "z")))
    ref = E.rows_reference(P, "finito_init", k, B)
    table = O.finito_init(op, g, X.lossless(P.gam, dtype), c(P.x0))[0]       # (the oracle's own hat_gamma = 1 / sum(1 / gam_i) is no power of two: the table alone)
    assert same_bits(table, X.lossless(ref["table"], dtype))
    assert np.array_equal(E.cpx(ref["av"]), P.hg * (E.cpx(ref["table"]) / P.gam[:, None]).sum(axis=0))
    assert B.worst() < X.LIMIT_BITS


@pytest.mark.parametrize("case", E.ROWS_CASES, ids=lambda c: c.name)
def test_every_sum_of_every_rows_case_is_exact_and_a_dropped_partial_changes_bits(case):
    """on the chip the device cases are sized for (256 compute units); the device test asserts the bound for the chip it runs on"""
    worst = 0.0
    for dtype in (F64, F32):
        P, B = case.problem(dtype, 256), X.Bounds()
        for k in case.launches(256):
            for mode in E.ROW_SWEEPS:
                ref = E.rows_reference(P, mode, k, B)
                for v in ref.values():
                    X.lossless(v, F32)
            E.rows_reference(P, "grad", k, B, x=P.x_axis)
            for mode in E.ROW_BATCHES:
                for kind in E.BATCH_PROX[mode.split("_")[0]]:
                    for v in E.rows_batch_reference(P, mode, k, B, kind).values():
                        X.lossless(v, F32)
            parts = min(k, 4)
            for j in {0, parts - 1} if k >= 7 else ():                       # (a partial of ONE row of three entries can be all zero)
                got = E.rows_reference(P, "grad", k, X.Bounds(), D={"drop_partial": (parts, j)})
                assert not same_bits(E.rows_reference(P, "grad", k, X.Bounds())["av"], got["av"]), (case.name, k, j)
        assert B.worst() < X.LIMIT_BITS, (case.name, sorted(B.bits.items(), key=lambda kv: -kv[1])[:3])
        worst = max(worst, B.worst())
    print(f"{case.name}: the largest sum: 2^{worst:.1f} quanta")


def test_the_rows_classifier_reads_the_complex_reports():
    c = E.classify_rows("rows_cplx_kernel<f32,mode0> grid=2 block=256", 7)
    assert (c["kind"], c["mode"], c["workers"], c["parts"], c["trips"]) == ("cplx", 0, 8, 8, [0, 1, 1, 1, 1, 1, 1, 1])
    c = E.classify_rows("rows_csplit_kernel<f64,J4,mode3> (cplx) grid=256 block=256", 257)
    assert (c["kind"], c["J"], c["mode"], c["parts"], max(c["trips"]), min(c["trips"])) == ("csplit", 4, 3, 256, 2, 1)
    assert E.trip_classes(c) == {"1 trip", "2 trips"}
    for case in E.ROWS_CASES:                                                # every case's launches reach what it needs, on 256 compute units
        reached = set()
        for k in case.launches(256):
            grid = min(-(-k // 4), 256) if case.kind == "cplx" else min(k, 256)
            name = f"rows_{case.kind}_kernel<f64,{'J%d,' % case.J if case.J else ''}mode0>{' (cplx)' if case.J else ''} grid={grid} block=256"
            reached |= E.trip_classes(E.classify_rows(name, k))
        assert case.need() <= reached, (case.name, reached)


@pytest.mark.parametrize("dtype", [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")])
@pytest.mark.parametrize("n,k", [(3, 20), (35, 37), (128, 9), (2000, 20)])
def test_rows_batch_restatement_equals_the_oracle_in_bits(n, k, dtype):
    """FINITO_BATCH (g = Zero, the dead zone, live on-axis arguments) and LFinito's GRAD2 (Zero, the dead zone), over an index list and a
    row block off row 0, one batch from the lattice state"""
    from oracle import twin as O
    P, B = E.RowsProblem(64, n, seed=n), X.Bounds()
    ctype = np.complex128 if dtype == F64 else np.complex64
    c = lambda v: X.lossless(E.pairs(v), dtype)
    gam = X.lossless(P.gam, dtype)
    for mode in E.ROW_BATCHES:
        for kind in E.BATCH_PROX[mode.split("_")[0]]:
            ref = E.rows_batch_reference(P, mode, k, B, kind)
            rows = E.batch_rows(P, k, mode.endswith("lists"))
            assert (rows[0] == E.ROW0 and np.array_equal(np.diff(rows), np.ones(k - 1))) != mode.endswith("lists")
            g = O.Prox("zero", dtype=dtype) if kind == "zero" else O.Prox("l1_complex", lam=P.lam_g(kind), dtype=dtype)
            if mode.startswith("finito"):
                op = O.Problem("ls", c(P.A).view(ctype).reshape(P.A.shape), c(P.b).view(ctype), P.lam)
                table, av, z = c(P.table0), X.lossless(ref["av_in"], dtype), c(P.z)
                O.finito_steps(op, g, gam, dtype(P.hg), [rows], table, av, z)
                got = {"table": table, "av": av, "z": z}
                if kind == "axis":                                           # live arguments: some give 0 at |v| == gl, the others |v| - gl on their axis
                    zc = E.cpx(ref["z"])
                    assert (zc == 0).any() and (zc != 0).any() and ((zc.real == 0) | (zc.imag == 0)).all()
                if kind == "dead":
                    assert not ref["z"].any() and ref["av"].any()
            else:
                op = O.Problem("ls", c(P.A).view(ctype).reshape(P.A.shape), c(P.b2(kind)).view(ctype), P.lam)
                av, z, zf = X.lossless(ref["av_in"], dtype), np.zeros(2 * n, dtype), np.zeros(2 * n, dtype)
                O.lfinito_iterate(op, g, gam, dtype(P.hg), [rows], av, z, zf)
                got = {"av": av, "z": z, "z_full": zf}
                assert kind != "zero" or (ref["z"] != ref["z_full"]).any()  # (two different points: the GRAD2 difference is live)
            for name, v in got.items():
                assert same_bits(v, X.lossless(ref[name], dtype)), (mode, kind, name)
    assert B.worst() < X.LIMIT_BITS


def test_the_on_axis_objective_term_is_the_oracles():
    from oracle import twin as O
    P = E.RowsProblem(64, 35, seed=2)
    ref = E.rows_reference(P, "grad", 64, X.Bounds(), x=P.x_axis)
    assert ((P.x_axis.real == 0) | (P.x_axis.imag == 0)).all() and P.x_axis.any()
    for dtype, ctype in ((F64, np.complex128), (F32, np.complex64)):
        c = lambda v: X.lossless(E.pairs(v), dtype)
        op = O.Problem("ls", c(P.A).view(ctype).reshape(P.A.shape), c(P.b).view(ctype), P.lam)
        assert O.objective(op, O.Prox("l1_complex", lam=P.lam_axis, dtype=dtype), c(P.x_axis)) == ref["obj"] + ref["gval"]

"""tests/chains_exact.py on the CPU: (1) its restatement of the chain steps equals the oracle (oracle/twin.py) IN BITS, in both types, on
the same data, after every compared step count; (2) the bound that makes every association exact holds for every host case, and the
device file's cases are well formed (every repeat distance placed inside a chunk and across a staging boundary; the reports the classifier
reads); (3) every live step matters: the chain with live step k skipped differs in the bits of a compared output, for every live k of every
case here; (4) planted defects: a stale table row on a repeat inside the window (inside a chunk and across a boundary), the previous chunk's
b_i or gamma_i at a chunk's first step, a 16-byte chunk left out of a dot product, a masked row's last element dropped, a wave's partial
dropped or doubled, a step missing from SVRG's sum, SAG's and SAGA's order of the av update swapped, the prox of a short last Finito batch
skipped, a workgroup's share missing from a wide chain's dot: each changes the bits of a compared output."""
import numpy as np
import pytest

import chains_exact as C
import rows_exact as X

F64, F32 = np.float64, np.float32
BOTH = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
_found = {}


def found(spec):
    if spec.name not in _found:
        _found[spec.name] = C.found(spec)
    return _found[spec.name]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    view = lambda v: v.view(np.int64 if v.dtype == F64 else np.int32)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(view(a), view(b))


def differs(ref, got):
    """some compared output of some compared step count has other bits"""
    return any(not same_bits(ref[n][k], got[n][k]) for n in ref for k in ref[n])


SPEC_IDS = [s.name for s in C.HOST_SPECS]
BY_NAME = {s.name: s for s in C.HOST_SPECS}


def test_column_worst_is_the_quantum_of_rows_exact_column_by_column():
    rng = np.random.default_rng(3)
    t = rng.integers(-40, 41, (5, 30)) * 2.0 ** rng.integers(-9, 4, (5, 30))
    t[:, 7] = 0
    t[2, 9] = 0
    want = max(np.abs(t[:, j]).sum() / X.quantum(t[:, j]) for j in range(30) if t[:, j].any())
    assert C.column_worst(t) == want
    B = C.ChainBounds()
    B.update("x", t[0], t[1], t[2], t[3], t[4])
    assert B.worst() == np.log2(want)


# ---- 1. the restatement against the oracle -----------------------------------------------------------------------------------------------------
def oracle_run(P, n, dtype):
    from oracle import twin as O
    s = P.spec
    c = lambda a: X.lossless(a, dtype)
    op = O.Problem(s.loss, c(P.A), c(P.b), P.lam, N_total=C.N)
    if s.prox == "l1":
        g = O.Prox("l1", lam=P.lam_g, dtype=dtype)
    elif s.prox == "box":
        g = O.Prox("box", lo=-2.0, hi=2.0, dtype=dtype)
    else:
        g = O.Prox("box", lo=c(P.lo), hi=c(P.hi), dtype=dtype)
    idx = P.idx[:n]
    if s.alg == "svrgc":                                                     # a whole iterate from the init at x0 = P.zf0; its tail divides by n
        av, z, zf, w = O.svrg_init(op, c(P.zf0))
        O.svrg_iterate(op, g, dtype(P.gamma), idx, s.plus, av, z, zf, w)
        return {"av": av, "z": z, "z_full": zf, "w": w}
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
        O.finito_steps(op, g, c(P.gam), dtype(C.HG), P.batches(n), table, av, z)
        return {"z": z, "av": av, "table": table}
    av, z, zf = c(P.av0), c(P.p0), c(P.zf0)
    O.lfinito_iterate(op, g, c(P.gam), dtype(C.HG), P.batches(n), av, z, zf)
    return {"av": av, "z": z, "z_full": zf}


PAIRS = [pytest.param(s.name, dt, id=f"{s.name}-{'f64' if dt == F64 else 'f32'}") for s in C.HOST_SPECS for dt in (F64, F32)
         if dt == F64 or s.limit == X.LIMIT_BITS]


@pytest.mark.parametrize("name,dtype", PAIRS)
def test_restatement_equals_the_oracle_in_bits(name, dtype):
    P, B, ref = found(BY_NAME[name])
    for n in P.spec.counts:
        got = oracle_run(P, n, dtype)
        for k, want in ref[n].items():
            assert same_bits(got[k], X.lossless(want, dtype)), f"{name}: {k} after {n} steps differs from the oracle's"


# ---- 2. the bound; the device file's cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SPEC_IDS)
def test_every_sum_of_every_step_is_exact_in_any_association(name):
    P, B, ref = found(BY_NAME[name])
    assert P.spec.limit in (X.LIMIT_BITS, 53) and (P.spec.limit == 53) == name.endswith("_f64only")
    assert B.worst() < P.spec.limit, sorted(B.bits.items(), key=lambda kv: -kv[1])[:3]
    for n in ref:
        for v in ref[n].values():
            X.lossless(v, F32 if P.spec.limit == X.LIMIT_BITS else F64)
    s = P.spec
    steps = set(np.nonzero(P.live)[0])
    assert set(C.live_steps(s.nsteps, s.depth, s.marks, s.counts)) <= steps
    idle_table = P.p0 if (s.alg, s.loss) == ("finito", "ls") else 0.0        # (Finito: the start iterate -- an idle step then adds z - z = 0)
    assert not P.A[C.NLIVE:].any() and (P.table0[C.NLIVE:] == idle_table).all() and (s.loss == "logistic" or not P.b[C.NLIVE:].any())
    assert all(P.idx[k] < C.NLIVE for k in steps) and all(P.idx[k] >= C.NLIVE for k in set(range(s.nsteps)) - steps)
    C.check_placements(P)                                                    # every distance inside a chunk and across a boundary


def test_the_device_cases_are_well_formed():
    names = set()
    for f in C.FORMS:
        for dtype in f.dtypes:
            d = f.d(dtype)
            cols = C.marked_columns(d, C.vec_of(dtype))
            assert cols[0] == 0 and cols[-1] == d - 1 and len(set(cols)) == len(cols) <= C.MARKED
            assert {g for g in range(-(-d // C.WIDE_SLICE))} == set(cols // C.WIDE_SLICE)          # every workgroup's columns
            for w in range(min(4, -(-d // 64))):                                                      # every wave's share, by elements and by chunks
                assert any((c % 256) // 64 == w for c in cols) or d <= 64 * w
            for alg in f.algs:
                for r in (f.r if alg in ("finito", "lfinito") else (1,)):
                    s = f.spec(alg, dtype, r)
                    names.add((s.name, dtype))
                    want = {1, 2, s.depth, 2 * s.depth, 1024, 2048} if alg == "svrgc" else {1, 2, s.depth - 1, s.depth, s.depth + 1, 1023, 1024, 1025}
                    assert s.d == d and want <= set(s.counts) | {0}
                    C.check_placements(C.Chain(s, s.seed0))                   # (data only: no chain is run here)
    assert {f.kind for f in C.FORMS} == {"reg", "dma", "ws", "wide", "big"}
    for kind in ("reg", "dma", "ws", "wide", "big"):                         # both types on every family
        assert {dt for f in C.FORMS if f.kind == kind for dt in f.dtypes} == {F64, F32}


def test_the_classifier_reads_the_launchers_reports():
    c = C.classify("chain_dma_kernel<f64,J8,alg0,masked> grid=1 block=512 steps=5")
    assert (c["kind"], c["J"], c["alg"], c["masked"], c["threads"], c["waves"], c["workgroups"], c["steps"]) == ("dma", 8, 0, True, 512, 8, 1, 5)
    c = C.classify("chain_ws_kernel<f32,J1,alg1,masked,issuers2> grid=1 block=448 steps=600")
    assert (c["kind"], c["dtype"], c["issuers"], c["masked"], c["waves"]) == ("ws", F32, 2, True, 7)
    c = C.classify("chain_kernel<f64,E4,alg2,full> grid=1 block=256 steps=9")
    assert (c["kind"], c["E"], c["alg"], c["masked"]) == ("reg", 4, 2, False)
    c = C.classify("chain_wide_kernel<f64,E8,alg3> grid=3 block=256 steps=5")
    assert (c["kind"], c["workgroups"], c["E"]) == ("wide", 3, 8)
    c = C.classify("chain batch: 3 chains in 1 launch(es); first: chain_dma_kernel<f64,J1,alg0,masked> grid=1 block=64 steps=5 grid=3")
    assert (c["chains"], c["launches"], c["kind"], c["workgroups"], c["threads"]) == (3, 1, "dma", 3, 64)
    with pytest.raises(AssertionError):
        C.classify("chain_cdma_kernel<f64,J2,alg0> grid=1 block=256 steps=5")


# ---- 3. every live step matters -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SPEC_IDS)
def test_every_live_step_matters(name):
    P, B, ref = found(BY_NAME[name])
    keep = {}
    again = C.run(P, keep=keep)
    assert not differs(ref, again)
    last = {P.spec.nsteps: ref[P.spec.nsteps]}
    idle = [int(k) for k in np.nonzero(P.live)[0] if not differs(last, C.run(P, counts=[P.spec.nsteps], resume=(int(k), keep[int(k)])))]
    if P.spec.alg == "finito" or P.spec.loss == "logistic":
        # Finito takes z at its batch's start and its aggregate telescopes over a row's visits (the logistic leg's iterate is pinned): a
        # repeat within the window can write the row's value again.  Those steps are held by the stale-row defects below, which every
        # placement must notice; every other live step must matter here, and under SVRG, SAGA, SAG and LFinito every live step does.
        idle = [k for k in idle if not any(k in (a, b) for v in P.placed.values() for a, b, m in v)]
    assert not idle, f"{name}: the chain without live step(s) {idle} ends in the same bits"


# ---- 4. planted defects ----------------------------------------------------------------------------------------------------------------------------------
def planted(name, D):
    P, B, ref = found(BY_NAME[name])
    return differs(ref, C.run(P, D=D))


@pytest.mark.parametrize("name", ["host_saga_d300", "host_sag_d300", "host_finito_d300_r2", "host_saga_d50_f64only", "host_finito_d50",
                                  "host_saga_ws_d400", "host_saga_seven_d300", "host_saga_d300_logistic", "host_finito_d300_logistic"])
def test_a_stale_table_row_inside_a_chunk_and_across_a_boundary(name):
    P, B, ref = found(BY_NAME[name])
    for k, places in P.placed.items():
        for a, b, m in places:
            assert planted(name, {"stale": b}), f"{name}: the table row of step {a} read stale at step {b} (distance {k}, boundary {m}) goes unnoticed"
    if P.spec.seven:
        for b in range(C.CHUNK - 2, C.CHUNK + 4):
            assert planted(name, {"stale": b}), (name, b)


@pytest.mark.parametrize("name", ["host_saga_d300", "host_sag_d300", "host_finito_d300_r2", "host_lfinito_d50"])
def test_the_previous_chunks_b_or_gamma_at_a_chunks_first_step(name):
    P, B, ref = found(BY_NAME[name])
    assert P.b[P.idx[0]] != P.b[P.idx[C.CHUNK]] and P.gam[P.idx[0]] != P.gam[P.idx[C.CHUNK]]
    if P.spec.alg in C.TABLE_ALGS:                                           # (SVRG and LFinito take the difference of two gradients of the row: b_i cancels)
        assert planted(name, {"b_from": (C.CHUNK, 0)})
    if P.spec.alg in ("finito", "lfinito"):
        assert planted(name, {"gam_from": (C.CHUNK, 0)})


@pytest.mark.parametrize("name", ["host_svrg_d300", "host_saga_d300", "host_finito_d300_r2", "host_lfinito_d300_r2"])
def test_a_chunk_an_element_or_a_waves_partial_missing_from_a_dot_product(name):
    P, B, ref = found(BY_NAME[name])
    d, a0 = P.d, P.A[P.idx[0]]
    j = int(np.nonzero(a0)[0][0])
    chunk = np.arange(j // 2 * 2, j // 2 * 2 + 2)
    assert planted(name, {"dot": (0, chunk, 0.0)}), "one 16-byte chunk of step 0's row left out of its dot product"
    assert planted(name, {"dot": (None, np.array([d - 1]), 0.0)}), "a masked row's last valid element dropped"
    wave1 = np.array([c for c in range(d) if (c % 256) // 64 == 1])
    assert planted(name, {"dot": (None, wave1, 0.0)}), "one wave's partial dropped"
    assert planted(name, {"dot": (None, wave1, 2.0)}), "one wave's partial doubled"


@pytest.mark.parametrize("name", ["host_svrgc_d50", "host_svrgc_d300_plus"])
def test_cached_row_dots_give_svrgs_bits_and_a_wrong_rows_dot_does_not(name):
    P, B, ref = found(BY_NAME[name])
    assert not differs(ref, C.run(P, D={"recompute": True})), "the chain on cached a_i'z_full must give the bits of the chain that forms them"
    dots = P.A @ P.zf0
    for k in (1, 1023, 1024):
        j = next(j for j in np.nonzero(P.live)[0] if dots[P.idx[j]] != dots[P.idx[k]])
        assert planted(name, {"cache_from": (k, int(j))}), (k, j)
    assert planted(name, {"no_zsum": 1023})


def test_a_step_missing_from_svrgs_sum():
    for k in (0, 1023, 1024, 2099):
        assert planted("host_svrg_d50", {"no_zsum": k}), k


def test_the_order_of_sagas_and_sags_av_update_swapped():
    for name in ("host_saga_d300", "host_sag_d300"):
        P, B, ref = found(BY_NAME[name])
        keep = {}
        C.run(P, keep=keep)
        assert planted(name, {"swap_sag": None})
        moved = [k for k in keep["moved"] if P.live[k]]
        assert len(moved) > 40
        seen = [k for k in moved if planted(name, {"swap_sag": k})]
        # a single swapped step shows unless both forms' iterates leave the box on the same side at every coordinate of the row
        assert len(seen) >= len(moved) // 2 and {k < C.CHUNK for k in seen} == {True, False}, (name, len(seen), len(moved))


def test_the_prox_of_a_short_last_finito_batch_skipped():
    P, B, ref = found(BY_NAME["host_finito_r5_d300"])
    got = C.run(P, D={"no_last_prox": True})
    short = [n for n in P.spec.counts if n % 5]
    assert {1, 2, 7, 8, 9, 1023, 1024} <= set(short)
    seen = {n for n in short if not same_bits(ref[n]["z"], got[n]["z"])}     # (1023 and 1024: the short batch at the staging boundary)
    assert seen == set(short), sorted(set(short) - seen)


def test_a_workgroups_share_missing_from_a_wide_chains_dot():
    spec = C.Spec("host_svrg_wide_d4097", "svrg", 4097, nsteps=40, marks=())
    P, B, ref = C.found(spec)
    assert B.worst() < X.LIMIT_BITS
    for g in range(3):                                                       # the last workgroup owns the single column 4096
        cols = np.arange(g * C.WIDE_SLICE, min((g + 1) * C.WIDE_SLICE, 4097))
        assert differs(ref, C.run(P, D={"dot": (None, cols, 0.0)})), f"workgroup {g}'s share missing from every dot product goes unnoticed"

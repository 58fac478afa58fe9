"""The rows kernels and the chains under hostile memory layouts: poisoned padding, guard bands around every buffer, bases one element
off 16-byte alignment (tests/layouts.py; tests/test_layouts_host.py shows on the CPU that the harness notices what it is for).

Every class below runs once per layout:

    tight        exact-size allocations, as the other test files make them (the baseline run)
    guarded      every device buffer of the call inside a poisoned flat buffer, 64 elements of guard on each side
    pad16        as guarded, the data rows at stride d + 2 VEC (VEC = 16 / sizeof(T)), the padding columns poisoned
    pad3         as guarded, the data rows at stride d + 3
    shift:<buf>  as guarded, ONE buffer one element (sizeof(T) bytes) off 16-byte alignment: one layout per pointer the call's plan
                 looks at (plan_rows / wrow_plan: A, table, x1, x2; plan_chain: A, table, av, z, zf, w; launch_afinito: meta too;
                 plan_proshi: Q, q, table, x)

and asserts, in this order: (1) the kernel the launcher reports is the one the plan gives a caller with those pointers (the literal
tables ROWS_EXPECT, chain_expect, af_expect and proshi_expect below, written from csrc/rows_launch.inc, rowsw_launch.inc and
chain_launch.inc before the first run; `guarded` reports `tight`'s string character for character); (2) nothing outside any view was written; (3) no input
changed; (4) no NaN in any output; (5) where every kernel an output depends on has the name it had under `tight`, the output has
`tight`'s bits (bitwise reproducible); (6) where one differs, the output is held against the oracle.
No entry of the tables is a refusal: the rows and chain entry points fall back on every layout here.

The problems, options and oracle calls are those of run_modes / run_chain / run_afinito of tests/test_gpu_every_kernel.py at the
smallest shapes that reach the kernel and keep a short last group, tile or chunk; the oracle runs once per class."""
import re

import numpy as np
import pytest

import layouts as LY
import problems as P
from test_gpu_parity import close

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
TY = {F64: "f64", F32: "f32"}
DTYPES = pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])


def vec_of(dtype):
    return 16 // np.dtype(dtype).itemsize


class Plain:
    """A buffer of the `tight` layout: an allocation of its own, no guards to check"""

    def __init__(self, view):
        self.view = view

    def check_outside(self, what=""):
        pass

    def check_unchanged(self, what=""):
        pass


class Placer:
    """Places the buffers of one call as `layout` says.  role: the pointer of the plan the buffer is ("A", "table", "x1", ...), which
    `shift:<role>` moves; data: the matrix whose rows take the padded stride."""

    def __init__(self, layout, dtype):
        self.layout, self.dtype = layout, dtype
        self.bufs, self.inputs = [], []
        self.shift = layout[6:] if layout.startswith("shift:") else None

    def _ld(self, d):
        # (pad2: complex rows are (re, im) pairs and take no odd stride; one entry of padding breaks the alignment of fp32 rows only)
        return {"pad16": d + 2 * vec_of(self.dtype), "pad3": d + 3, "pad2": d + 2}.get(self.layout)

    def inp(self, name, a, role=None, data=False):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a))
        if self.layout == "tight":
            g = Plain(t.cuda())
        else:
            g = LY.Guarded(t, off=int(role is not None and role == self.shift), ld=self._ld(a.shape[1]) if data else None, device="cuda", name=name)
        self.bufs.append(g)
        self.inputs.append(g)
        return g

    def out(self, name, shape, role=None):
        import torch
        tdt = LY.as_torch_dtype(self.dtype)
        if self.layout == "tight":
            g = Plain(torch.empty(shape, dtype=tdt, device="cuda"))
        else:
            g = LY.Guarded(shape=shape if isinstance(shape, tuple) else (shape,), dtype=tdt, off=int(role is not None and role == self.shift), device="cuda", name=name)
        self.bufs.append(g)
        return g

    def check(self, what):
        for g in self.bufs:                               # (2) outside the views, outputs and inputs alike
            g.check_outside(what)
        for g in self.inputs:                             # (3) the inputs
            g.check_unchanged(what)


def snap(ref):
    """an oracle result as it is now, with its Float64 twin (oracle/twin.py): the oracle updates its states in place"""
    from oracle import twin
    t = twin.twin_of(ref)
    return np.array(ref, copy=True), (None if t is None else np.array(t, dtype=np.float64, copy=True))


def problem(pl, loss, A, b, lam_f):
    """(oracle Problem, device PackedF over the placed A and b)"""
    from oracle import twin as O
    from ciaoalgorithms_jl_amd.device import PackedF
    import ciaoalgorithms_jl_amd._lib as L
    gA, gb = pl.inp("A", A, role="A", data=True), pl.inp("b", b)
    kind = {"ls": L.LOSS_LS, "logistic": L.LOSS_LOGISTIC}[loss]
    return O.Problem(loss, A, b, lam_f), PackedF(kind, gA.view, gb.view, lam_f)


def prox(pl, gk, dtype, d, lam=0.02):
    """(oracle Prox, device ProxG): l1, or a box with bound vectors (placed as every other input)"""
    from oracle import twin as O
    from ciaoalgorithms_jl_amd.device import ProxG
    import ciaoalgorithms_jl_amd._lib as L
    if gk == "l1":
        return O.Prox("l1", lam=lam), ProxG(L.PROX_L1, lam=lam)
    lo, hi = np.linspace(-0.3, 0.0, d).astype(dtype), np.linspace(0.05, 0.4, d).astype(dtype)
    glo, ghi = pl.inp("lo", lo), pl.inp("hi", hi)
    return O.Prox("box", lo=lo, hi=hi, dtype=dtype), ProxG(L.PROX_BOX, lo_vec=glo.view, hi_vec=ghi.view)


def setup(pl, loss, N, d, dtype, seed, gk="l1"):
    """-> (oracle Problem, device PackedF, oracle Prox, device ProxG, x0 as the device takes it, the L_i).  loss "cplx": complex least
    squares as tests/test_gpu_complex.py builds it, d = 2n reals, every vector as (re, im) pairs of `dtype`"""
    if loss != "cplx":
        A, b, x0 = P.synthetic(loss, N, d, dtype, seed=seed)
        lam_f = float(N) if loss == "ls" else 1.0
        op, dp = problem(pl, loss, A, b, lam_f)
        og, dg = prox(pl, gk, dtype, d)
        return op, dp, og, dg, x0, (lam_f if loss == "ls" else 0.25) * np.sum(A.astype(np.float64) ** 2, axis=1)
    from oracle import twin as O
    from ciaoalgorithms_jl_amd.device import PackedF, ProxG
    import ciaoalgorithms_jl_amd._lib as L
    A, b, x0 = P.synthetic_complex(N, d // 2, np.complex128 if dtype == F64 else np.complex64, seed=seed)
    gA, gb = pl.inp("A", O.as_pairs(A).reshape(N, -1), role="A", data=True), pl.inp("b", O.as_pairs(b))
    op, dp = O.Problem("ls", A, b, float(N)), PackedF.least_squares_complex(gA.view, gb.view, float(N))
    return (op, dp, O.Prox("l1_complex", lam=0.02), ProxG(L.PROX_L1_COMPLEX, lam=0.02), O.as_pairs(x0),
            float(N) * np.sum(np.abs(A.astype(np.complex128)) ** 2, axis=1))


def no_poison(what, **outs):
    for k, t in outs.items():                             # (4)
        assert not LY.has_poison(t), f"{what}: NaN in {k}: padding or guard content reached a result, or an element was left unwritten"


def expect_name(expected, got, dtype, what):
    """(1): `expected` is a regular expression, or {64: ..., 32: ...} where the two types' plans differ"""
    if isinstance(expected, dict):
        expected = expected[64 if dtype == F64 else 32]
    assert re.search(expected, got), f"{what}: the plan gives {expected!r}, the launcher reports {got!r}"


def compare(run, base, deps, refs, dtype, what, sites):
    """(5) / (6) for every output of `run`: deps[key] names the kernels (keys of run['names']) the output depends on"""
    import torch
    for key, out in run["outs"].items():
        same = all(run["names"][m] == base["names"][m] for m in deps[key])
        if same and run is not base:
            assert out.shape == base["outs"][key].shape and torch.equal(out, base["outs"][key]), \
                f"{what}: {key} is not bitwise the tight layout's although the kernels are ({[run['names'][m] for m in deps[key]]})"
        if (not same or run is base) and key in refs:
            sites(key, out, refs[key], dtype, f"{what}: {key} ({run['names'][deps[key][-1]]})")


# =====================================================================================================================================
# rows
# =====================================================================================================================================
ROWS_LAYOUTS = ("tight", "guarded", "pad16", "pad3", "shift:A", "shift:table", "shift:x1", "shift:x2")
MODES = ("grad", "saga_init", "finito_init", "finito_lists", "finito_blocks", "lfinito_init", "lfinito_pass", "lfinito_lists", "lfinito_blocks", "afinito_init")
# what each output depends on (the kernels before it in its own algorithm's sequence)
_FIN = ["finito_init", "finito_lists", "finito_blocks"]
_LF = ["lfinito_init", "lfinito_pass", "lfinito_lists", "lfinito_blocks"]
ROWS_DEPS = {"grad.av": ["grad"], "saga_init.table": ["saga_init"], "saga_init.av": ["saga_init"], "saga_init.z": ["saga_init"],
             "finito_init.table": _FIN[:1], "finito_init.av": _FIN[:1], "finito_init.z": _FIN[:1],
             "finito_lists.table": _FIN[:2], "finito_lists.av": _FIN[:2], "finito_lists.z": _FIN[:2],
             "finito_blocks.table": _FIN, "finito_blocks.av": _FIN, "finito_blocks.z": _FIN,
             "lfinito_init.av": _LF[:1], "lfinito_lists.z": _LF[:3], "lfinito_lists.av": _LF[:3], "lfinito_lists.zf": _LF[:3],
             "lfinito_blocks.z": _LF, "lfinito_blocks.av": _LF, "lfinito_blocks.zf": _LF,
             "afinito_init.table": ["afinito_init"], "afinito_init.av": ["afinito_init"], "afinito_init.z": ["afinito_init"],
             "afinito_init.hg": ["afinito_init"], "afinito_init.fi": ["afinito_init"], "afinito_init.meta": ["afinito_init"]}


def run_modes(ctx, ciao, N, d, dtype, loss, r, layout, refs):
    """The six modes of the rows kernels (run_modes of tests/test_gpu_every_kernel.py) with every buffer placed as `layout` says.
    x1 is x0 (the sweeps and inits), Finito's z (its batches) and LFinito's z_full (its batches); x2 is LFinito's z.
    refs: filled by the first run (the oracle's results, shared by the layouts).  -> {names, outs}"""
    from oracle import twin as O
    pl = Placer(layout, dtype)
    op, dp, og, dg, x0, Li = setup(pl, loss, N, d, dtype, d + N)
    gam = (0.999 * N / np.maximum(Li, 1e-3 * Li.max())).astype(dtype)
    gx0, ggam = pl.inp("x0", x0, role="x1"), pl.inp("gam", gam)
    hg = ctx.hat_gamma(ggam.view)
    table = pl.out("table", (N, d), role="table")
    av, sav, sz, aav, az = (pl.out(k, d) for k in ("av", "saga av", "saga z", "adaptive av", "adaptive z"))
    fav, fz = pl.out("finito av", d), pl.out("finito z", d, role="x1")
    lav, lz, lzf = pl.out("lfinito av", d), pl.out("lfinito z", d, role="x2"), pl.out("lfinito z_full", d, role="x1")
    scratch = pl.out("scratch", d)
    meta4, hgd = pl.out("meta4", (N, 16)), pl.out("hat_gamma", 1)
    st = ciao.IndexStream(d)
    rnd = [st.sample_without_replacement(N, r) for _ in range(3)] + [st.sample_without_replacement(N, max(1, r // 3))]
    bptr = np.zeros(len(rnd) + 1, np.int64)
    np.cumsum([len(x) for x in rnd], out=bptr[1:])
    nb = -(-N // r)
    blocks = [np.arange(r * j, min(r * j + r, N), dtype=np.int64) for j in range(nb)]
    first, length = np.array([x[0] for x in blocks]), np.array([len(x) for x in blocks])
    bp = np.zeros(nb + 1, np.int64)
    np.cumsum(length, out=bp[1:])
    grnd, gblk = pl.inp("batch lists", np.concatenate(rnd)), pl.inp("block lists", np.concatenate(blocks))
    names, outs = {}, {}
    fill = not refs
    g0 = 0.1 / max(Li.max(), 1.0)
    what = f"rows N={N} d={d} {TY[dtype]} {loss} {layout}"

    def keep(mode, **kw):
        names[mode] = ctx.last_kernel()
        for k, g in kw.items():
            outs[f"{mode}.{k}"] = g.view.clone()

    def ref(**kw):
        if fill:
            refs.update({k.replace("__", "."): snap(v) for k, v in kw.items()})

    ctx.set_option("chain_max_batch", 0)              # batches of any size on the rows kernels, none as a chain
    try:
        ctx.full_gradient(dp, gx0.view, av.view)
        keep("grad", av=av)
        ctx.saga_init(dp, dg, g0, gx0.view, table.view, sav.view, sz.view)
        keep("saga_init", table=table, av=sav, z=sz)
        ctx.finito_init(dp, dg, ggam.view, hg, gx0.view, table.view, fav.view, fz.view)
        keep("finito_init", table=table, av=fav, z=fz)
        ctx.finito_steps(dp, dg, ggam.view, hg, bptr, grnd.view, table.view, fav.view, fz.view)
        keep("finito_lists", table=table, av=fav, z=fz)
        ctx.finito_steps_blocks(dp, dg, ggam.view, hg, first, length, table.view, fav.view, fz.view)
        keep("finito_blocks", table=table, av=fav, z=fz)
        ctx.lfinito_init(dp, hg, gx0.view, lav.view, lz.view, lzf.view)
        keep("lfinito_init", av=lav)
        # (an LFinito iteration opens with a full pass at z_full, whose kernel the launcher's last name does not show: the same sweep
        # over the same pointers, asked on its own)
        ctx.full_gradient(dp, lzf.view, scratch.view)
        keep("lfinito_pass")
        ctx.lfinito_iterate(dp, dg, ggam.view, hg, bp, gblk.view, lav.view, lz.view, lzf.view)
        keep("lfinito_lists", z=lz, av=lav, zf=lzf)
        ctx.lfinito_iterate_blocks(dp, dg, ggam.view, hg, first, length, lav.view, lz.view, lzf.view)
        keep("lfinito_blocks", z=lz, av=lav, zf=lzf)
        ctx.afinito_init(dp, dg, 0.999, gx0.view, table.view, meta4.view, aav.view, az.view, hgd.view)
        names["afinito_init"] = ctx.last_kernel()
        m = meta4.view.view(N, 4, 4)
        outs.update({"afinito_init.table": table.view.clone(), "afinito_init.av": aav.view.clone(), "afinito_init.z": az.view.clone(),
                     "afinito_init.hg": hgd.view.clone(), "afinito_init.fi": m[:, 0, 1].clone(), "afinito_init.meta": meta4.view.clone()})
    finally:
        ctx.set_option("chain_max_batch", -1)
    ctx.synchronize()
    if fill:
        ref(grad__av=O.full_pass(op, x0))
        rt, rav, rz = O.saga_init(op, og, dtype(g0), x0)
        ref(saga_init__table=rt, saga_init__av=rav, saga_init__z=rz)
        rt, rav, rz, rhg = O.finito_init(op, og, gam, x0)
        ref(finito_init__table=rt, finito_init__av=rav, finito_init__z=rz)
        O.finito_steps(op, og, gam, rhg, rnd, rt, rav, rz)
        ref(finito_lists__table=rt, finito_lists__av=rav, finito_lists__z=rz)
        O.finito_steps(op, og, gam, rhg, blocks, rt, rav, rz)
        ref(finito_blocks__table=rt, finito_blocks__av=rav, finito_blocks__z=rz)
        rav, rz, rzf, rhg = O.lfinito_init(op, gam, x0)
        ref(lfinito_init__av=rav)
        O.lfinito_iterate(op, og, gam, rhg, blocks, rav, rz, rzf)
        ref(lfinito_lists__z=rz, lfinito_lists__av=rav, lfinito_lists__zf=rzf)
        O.lfinito_iterate(op, og, gam, rhg, blocks, rav, rz, rzf)
        ref(lfinito_blocks__z=rz, lfinito_blocks__av=rav, lfinito_blocks__zf=rzf)
        rt, rg, rgam, rfi, rav, rz, rhg = O.afinito_init(op, og, dtype(0.999), x0)
        ref(afinito_init__av=rav, afinito_init__fi=rfi)
    pl.check(what)
    no_poison(what, **outs)
    return {"names": names, "outs": outs, "what": what}


def rows_sites(key, out, ref, dtype, what):
    """(6): one stated tolerance per output of the rows modes (tools/retune_scales.py sets them from a calibration run)"""
    r, r64 = ref
    if key == "grad.av":
        close(out, r, dtype, scale={64: 99, 32: 89}, what=what, ref64=r64, scale64=17)
    elif key == "saga_init.table":
        close(out, r, dtype, scale={64: 89, 32: 94}, what=what, ref64=r64, scale64=13)
    elif key == "saga_init.av":
        close(out, r, dtype, scale={64: 98, 32: 87}, what=what, ref64=r64, scale64=17)
    elif key == "saga_init.z":
        close(out, r, dtype, scale=8, what=what, ref64=r64, scale64=10)
    elif key == "finito_init.table":
        close(out, r, dtype, scale={64: 13, 32: 14}, what=what, ref64=r64, scale64=11)
    elif key == "finito_init.av":
        close(out, r, dtype, scale={64: 66, 32: 69}, what=what, ref64=r64, scale64=11)
    elif key == "finito_init.z":
        close(out, r, dtype, scale={64: 66, 32: 75}, what=what, ref64=r64, scale64=12)
    elif key == "finito_lists.table":
        close(out, r, dtype, scale={64: 130, 32: 150}, what=what, ref64=r64, scale64=58)
    elif key == "finito_lists.av":
        close(out, r, dtype, scale={64: 220, 32: 280}, what=what, ref64=r64, scale64=64)
    elif key == "finito_lists.z":
        close(out, r, dtype, scale={64: 220, 32: 280}, what=what, ref64=r64, scale64=63)
    elif key == "finito_blocks.table":
        close(out, r, dtype, scale=250, what=what, ref64=r64, scale64=67)
    elif key == "finito_blocks.av":
        close(out, r, dtype, scale={64: 460, 32: 470}, what=what, ref64=r64, scale64=78)
    elif key == "finito_blocks.z":
        close(out, r, dtype, scale={64: 490, 32: 470}, what=what, ref64=r64, scale64=77)
    elif key == "lfinito_init.av":
        close(out, r, dtype, scale={64: 110, 32: 180}, what=what, ref64=r64, scale64=8)
    elif key == "lfinito_lists.z":
        close(out, r, dtype, scale={64: 460, 32: 370}, what=what, ref64=r64, scale64=36)
    elif key == "lfinito_lists.av":
        close(out, r, dtype, scale={64: 490, 32: 430}, what=what, ref64=r64, scale64=37)
    elif key == "lfinito_lists.zf":
        close(out, r, dtype, scale={64: 120, 32: 180}, what=what, ref64=r64, scale64=10)
    elif key == "lfinito_blocks.z":
        close(out, r, dtype, scale={64: 540, 32: 580}, what=what, ref64=r64, scale64=62)
    elif key == "lfinito_blocks.av":
        close(out, r, dtype, scale={64: 540, 32: 480}, what=what, ref64=r64, scale64=64)
    elif key == "lfinito_blocks.zf":
        close(out, r, dtype, scale={64: 490, 32: 500}, what=what, ref64=r64, scale64=42)
    elif key == "afinito_init.av":
        close(out, r, dtype, scale={64: 75, 32: 89}, what=what, ref64=r64, scale64=16)
    elif key == "afinito_init.fi":
        close(out, r, dtype, scale={64: 100, 32: 110}, what=what, ref64=r64, scale64=14)
    else:
        raise KeyError(key)


# ---- the name table ------------------------------------------------------------------------------------------------------------------
# families (regular expressions on the launcher's report, rows_kernel_name of csrc/rows_launch.inc)
WAVE = r"^rows_(fast|multi)_kernel<"                     # RK_WAVE_ROW
FAST = r"^rows_fast_kernel<"
MULTI = r"^rows_multi_kernel<"
EXACT = r"^rows_split_kernel<\w+,J\d+,mode\d> "          # RK_SPLIT, exact J x 256 chunks
MASKED = r"^rows_split_kernel<\w+,J\d+,mode\d,masked> "
SCALAR = r"^rows_split_kernel<\w+,J\d+,mode\d,scalar> "
SMALL = r"^rows_small_kernel<"
SMALLM = r"^rows_smallm_kernel<"
DENSE = r"^rows_smallb_kernel<\w+,mode\d,I8,dense> "
GATHER = r"^rows_smallb_kernel<\w+,mode\d,I8,gather> "
WCH = r"^rows_wrow_kernel<\w+,chunks,K1,"
WEL = r"^rows_wrow_kernel<\w+,elements,K\d,"
LONG = r"^rows_long_kernel<"
GEN = r"^rows_generic_kernel<"
CHAINW = r"^chain_wide_kernel<"                          # (a batch that runs as a chain, below)


def T2(f64, f32):
    return {64: f64, 32: f32}


def modes(grad, saga_init, finito_init, finito, lfinito, afinito_init=GEN, lfinito_init=None, lfinito_pass=None, finito_blocks=None,
          lfinito_blocks=None):
    """one layout's row of the table: mode -> family.  lfinito_init and the pass that opens an LFinito iteration are GRAD sweeps (their
    x1: x0 and z_full); the adaptive init is the any-shape kernel's wherever the rows are not a WAVE_ROW shape (plan_rows: SPLIT,
    SMALL* and LONG exclude RM_AFINITO_INIT)"""
    return {"grad": grad, "saga_init": saga_init, "finito_init": finito_init, "finito_lists": finito,
            "finito_blocks": finito if finito_blocks is None else finito_blocks, "lfinito_init": grad if lfinito_init is None else lfinito_init,
            "lfinito_pass": grad if lfinito_pass is None else lfinito_pass, "lfinito_lists": lfinito,
            "lfinito_blocks": lfinito if lfinito_blocks is None else lfinito_blocks, "afinito_init": afinito_init}


def all_modes(f, afinito_init=GEN):
    return modes(f, f, f, f, f, afinito_init)


def rows_expect():
    """(class, layout) -> {mode: family}, from plan_rows and wrow_plan.  rows16 := A and the row stride 16-byte aligned, and the table
    in the modes that have one (saga_init, finito_init, the Finito batches, afinito_init)."""
    E = {}
    # WAVE_ROW, K = 1 (64 chunks): no batch goes to SPLIT (64 chunks are not J x 256).  Without rows16 K = 0; 64 chunks are 128 fp64
    # elements -- under 256, so SMALL for the sweeps, rows_wrow_kernel by elements (two per lane) for the batches -- and 256 fp32 elements:
    # SPLIT by single elements.  shift:x1 / shift:x2 STAY: the WAVE_ROW branch does not test x1 / x2, rows_fast_kernel copies them to
    # LDS element by element (rows_kernels.h: lds[e] = a.x1[e]).
    k1 = all_modes(FAST, afinito_init=FAST)
    off = modes(T2(SMALL, SCALAR), T2(SMALL, SCALAR), T2(SMALL, SCALAR), T2(WEL, SCALAR), T2(WEL, SCALAR))
    E["wave_row_k1"] = {"tight": k1, "pad16": k1, "pad3": off, "shift:A": off,
                        "shift:table": modes(FAST, T2(SMALL, SCALAR), T2(SMALL, SCALAR), T2(WEL, SCALAR), FAST),
                        "shift:x1": k1, "shift:x2": k1}
    # WAVE_ROW, K = 4 (256 chunks = J1 exactly): sweeps on rows_multi_kernel, table modes on rows_fast_kernel, batches of up to 16 384
    # rows on rows_split_kernel exact J1 -- which does test x1 / x2: a batch whose x1 (x2) is off alignment stays one wave per row
    # (K > 0 keeps the single-element SPLIT out), the second "stays" of the WAVE_ROW branch.  512 / 1024 elements without rows16: SPLIT scalar.
    k4 = modes(MULTI, FAST, FAST, EXACT, EXACT, afinito_init=FAST)
    off = all_modes(SCALAR)
    E["wave_row_k4"] = {"tight": k4, "pad16": k4, "pad3": off, "shift:A": off,
                        "shift:table": modes(MULTI, SCALAR, SCALAR, SCALAR, EXACT),
                        "shift:x1": modes(MULTI, FAST, FAST, FAST, MULTI, afinito_init=FAST),
                        "shift:x2": modes(MULTI, FAST, FAST, EXACT, MULTI, afinito_init=FAST)}
    # SPLIT with a masked last chunk (150 and 987 chunks: 300 ... 3948 elements, all within the single-element form's 256 .. 4096): any
    # failed conjunct of the 16-byte form -- rows16, x1, x2 in GRAD2 -- gives the single-element form
    m = all_modes(MASKED)
    E["split_masked"] = {"tight": m, "pad16": m, "pad3": all_modes(SCALAR), "shift:A": all_modes(SCALAR),
                         "shift:table": modes(MASKED, SCALAR, SCALAR, SCALAR, MASKED),
                         "shift:x1": all_modes(SCALAR),
                         "shift:x2": modes(MASKED, MASKED, MASKED, MASKED, SCALAR)}
    # SPLIT by single elements (d = 257) and the any-shape kernel (forced, or no shorter kernel takes the shape): no pointer is looked at
    E["split_scalar"] = {k: all_modes(SCALAR) for k in ROWS_LAYOUTS if k != "guarded"}
    E["generic"] = {k: all_modes(GEN) for k in ROWS_LAYOUTS if k != "guarded"}
    # rows of tabular size, d = 52 (13 / 26 chunks) and d = 50 (25 fp64 chunks; no whole fp32 chunks).  Dense aligned rows: the sweeps and
    # inits on the matrix cores (SMALLM: ld == d, A and the table aligned; it does not test x1 -- rowsm_kernels.h copies it element by
    # element: xl[c] = a.x1[c] -- so shift:x1 STAYS), else SMALL.  Batches of 130 rows: rows_wrow_kernel, by chunks where wrow_plan's v16
    # holds (d % VEC, A, ld, the table in the Finito batch, x1, x2 in GRAD2), else by elements.
    for d, w32 in ((52, WCH), (50, WEL)):
        w = T2(WCH, w32)
        t = modes(SMALLM, SMALLM, SMALLM, w, w)
        E[f"small_d{d}"] = {"tight": t, "pad16": modes(SMALL, SMALL, SMALL, w, w), "pad3": modes(SMALL, SMALL, SMALL, WEL, WEL),
                            "shift:A": modes(SMALL, SMALL, SMALL, WEL, WEL), "shift:table": modes(SMALLM, SMALL, SMALL, WEL, w),
                            "shift:x1": modes(SMALLM, SMALLM, SMALLM, WEL, WEL), "shift:x2": modes(SMALLM, SMALLM, SMALLM, w, WEL)}
        # ... with small_wrow = 0: index lists on rows_smallb_kernel (gather), row blocks on the matrix cores where SMALLM holds, else
        # rows_smallb_kernel -- dense when ld == d, gather over a padded stride.  Neither tests x1 / x2 (rows_smallb_kernel reads
        # a.x1[col] by elements): both shifts STAY.
        t = modes(SMALLM, SMALLM, SMALLM, GATHER, GATHER, finito_blocks=SMALLM, lfinito_blocks=SMALLM)
        p = modes(SMALL, SMALL, SMALL, GATHER, GATHER)
        E[f"smallb_d{d}"] = {"tight": t, "pad16": p, "pad3": p,
                             "shift:A": modes(SMALL, SMALL, SMALL, GATHER, GATHER, finito_blocks=DENSE, lfinito_blocks=DENSE),
                             "shift:table": modes(SMALLM, SMALL, SMALL, GATHER, GATHER, finito_blocks=DENSE, lfinito_blocks=SMALLM),
                             "shift:x1": t, "shift:x2": t}
    # SMALLM needs ld == d: guarded and the shifts only (the entries of smallb_d50: same plan, other N and batch)
    E["smallm"] = {k: v for k, v in E["smallb_d50"].items() if k not in ("pad16", "pad3")}
    # LONG (4104 chunks: beyond SPLIT's 4096 chunks and the single-element form's 4096 elements): rows16, x1 and (GRAD2) x2, else the
    # any-shape kernel
    lg = all_modes(LONG)
    E["long"] = {"tight": lg, "pad16": lg, "pad3": all_modes(GEN), "shift:A": all_modes(GEN),
                 "shift:table": modes(LONG, GEN, GEN, GEN, LONG), "shift:x1": all_modes(GEN),
                 "shift:x2": modes(LONG, LONG, LONG, LONG, GEN)}
    # ... and the same rows in batches of two: beyond 8192 elements a batch of up to three rows runs as a chain on several workgroups
    # whatever chain_max_batch says (batch_as_chain, csrc/api_finito.hip), and that chain tests no pointer (CHAIN_EXPECT below): only the
    # sweeps and inits are the rows kernels'
    # complex rows (plan_rows' first branch): rows_csplit_kernel for 64 .. 4096 whole chunks with A, the stride, x1, x2 (GRAD2) and the
    # table (saga_init, finito_init, the Finito batch) aligned, else rows_cplx_kernel, which also takes every adaptive init.  pad2: a
    # stride of d + 2 reals is a multiple of 16 bytes in fp64 and not in fp32.
    CS, CP = r"^rows_csplit_kernel<", r"^rows_cplx_kernel<"
    c, o = all_modes(CS, afinito_init=CP), all_modes(CP, afinito_init=CP)
    E["cplx"] = {"tight": c, "pad16": c, "pad2": {m: T2(c[m], o[m]) for m in c}, "shift:A": o,
                 "shift:table": modes(CS, CP, CP, CP, CS, afinito_init=CP), "shift:x1": o,
                 "shift:x2": modes(CS, CS, CS, CS, CP, afinito_init=CP)}
    E["long_r2"] = {k: dict(v, finito_lists=CHAINW, finito_blocks=CHAINW, lfinito_lists=CHAINW, lfinito_blocks=CHAINW) for k, v in E["long"].items()}
    return E


ROWS_EXPECT = rows_expect()


def rows_class(ctx, ciao, cls, dtype, shapes, opts=None, layouts=ROWS_LAYOUTS, reset=None):
    """One class over all its layouts.  shapes: [(N, d, loss, r)]"""
    for N, d, loss, r in shapes:
        refs, base = {}, None
        for layout in layouts:
            for k, v in (opts or {}).items():
                ctx.set_option(k, v)
            try:
                run = run_modes(ctx, ciao, N, d, dtype, loss, r, layout, refs)
            finally:
                for k in (opts or {}):
                    ctx.set_option(k, (reset or {}).get(k, 0))
            base = base or run
            if layout == "guarded":
                assert run["names"] == base["names"], f"{run['what']}: guards alone changed the kernels: {run['names']} / tight {base['names']}"
            else:
                for mode in MODES:
                    expect_name(ROWS_EXPECT[cls][layout][mode], run["names"][mode], dtype, f"{run['what']} {mode}")
            compare(run, base, ROWS_DEPS, refs, dtype, run["what"], rows_sites)


@DTYPES
@pytest.mark.parametrize("K", [1, 4])
def test_rows_wave_per_row(ctx, ciao, dtype, K):
    rows_class(ctx, ciao, f"wave_row_k{K}", dtype, [(300, K * 64 * vec_of(dtype), "ls" if K == 1 else "logistic", 40)])


@DTYPES
def test_rows_workgroup_per_row_masked_chunks(ctx, ciao, dtype):
    vec = vec_of(dtype)
    rows_class(ctx, ciao, "split_masked", dtype, [(300, 150 * vec, "ls", 40), (60, (4 * 256 - 37) * vec, "logistic", 16)])


@DTYPES
def test_rows_workgroup_per_row_single_elements(ctx, ciao, dtype):
    rows_class(ctx, ciao, "split_scalar", dtype, [(300, 257, "ls", 40)])


@DTYPES
@pytest.mark.parametrize("d", [50, 52])
def test_rows_of_tabular_size(ctx, ciao, dtype, d):
    rows_class(ctx, ciao, f"small_d{d}", dtype, [(900, d, "ls" if d == 50 else "logistic", 130)])


@DTYPES
@pytest.mark.parametrize("d", [50, 52])
def test_rows_of_tabular_size_without_the_wave_per_row_batches(ctx, ciao, dtype, d):
    rows_class(ctx, ciao, f"smallb_d{d}", dtype, [(900, d, "logistic" if d == 50 else "ls", 130)], opts={"small_wrow": 0}, reset={"small_wrow": -1})


@DTYPES
def test_rows_on_the_matrix_cores(ctx, ciao, dtype):
    """N = 1003: a last tile of 11 rows for the sweeps and inits, a last block of 331; N = 1008: three whole blocks of 336"""
    rows_class(ctx, ciao, "smallm", dtype, [(1003, 50, "ls", 336), (1008, 50, "logistic", 336)], opts={"small_wrow": 0}, reset={"small_wrow": -1},
               layouts=tuple(k for k in ROWS_LAYOUTS if k not in ("pad16", "pad3")))


@DTYPES
def test_rows_longer_than_a_workgroup(ctx, ciao, dtype):
    """N = 5 in batches of two (which run as chains: ROWS_EXPECT["long_r2"]); N = 16 in batches of 12, 12, 12, 4 and blocks of 12 and 4"""
    d = (16 * 256 + 8) * vec_of(dtype)
    rows_class(ctx, ciao, "long_r2", dtype, [(5, d, "ls", 2)])
    rows_class(ctx, ciao, "long", dtype, [(16, d, "logistic", 12)])


CPLX_ROWS_LAYOUTS = tuple("pad2" if k == "pad3" else k for k in ROWS_LAYOUTS)


@pytest.mark.parametrize("dtype,n", [(F64, 200), (F32, 200), (F32, 1500)], ids=["c128-200", "c64-200", "c64-1500"])
def test_rows_complex(ctx, ciao, dtype, n):
    """n complex entries are 2n reals: 200 and 100 chunks (one per thread, most of the last wave masked), 750 chunks (J4, a masked tail).
    rows_cplx_kernel takes over on every layout that fails a conjunct."""
    rows_class(ctx, ciao, "cplx", dtype, [(60 if n == 200 else 24, 2 * n, "cplx", 20 if n == 200 else 9)], layouts=CPLX_ROWS_LAYOUTS)


@DTYPES
def test_rows_any_shape(ctx, ciao, dtype):
    rows_class(ctx, ciao, "generic", dtype, [(300, 257, "logistic", 40)], opts={"force_generic": 1})
    # (batches of 12, 12, 12, 4: up to three rows of more than 8192 elements would run as a chain, batch_as_chain of csrc/api_finito.hip)
    rows_class(ctx, ciao, "generic", dtype, [(12, 5001 if dtype == F64 else 9001, "ls", 12)])


# =====================================================================================================================================
# chains
# =====================================================================================================================================
ALGS = ("svrg", "svrg_cached", "saga", "sag", "finito", "lfinito")
USES = {"svrg": ("A", "av", "z", "zf", "w"), "svrg_cached": ("A", "av", "z", "zf", "w"), "saga": ("A", "table", "av", "z"),
        "sag": ("A", "table", "av", "z"), "finito": ("A", "table", "av", "z"), "lfinito": ("A", "av", "z", "zf")}
CHAIN_LAYOUTS = ("tight", "guarded", "pad16", "pad3", "shift:A", "shift:table", "shift:av", "shift:z", "shift:zf", "shift:w")
CHAIN_DEPS = {"svrg": {"w": ["init", "chain"], "z": ["init", "chain"], "av": ["init", "chain"], "zf": ["init", "chain"]},
              # (the cached-dots inner cycle's own name is not shown -- the launcher's last kernel is the full pass that closes the
              # iteration; "svrg" is the name the SVRG run of the same layout reported: the same plan over the same pointers)
              "svrg_cached": {k: ["init", "svrg", "chain"] for k in ("w", "z", "av", "zf")},
              "saga": {k: ["init", "chain"] for k in ("table", "av", "z")}, "sag": {k: ["init", "chain"] for k in ("table", "av", "z")},
              "finito": {k: ["init", "chain"] for k in ("table", "av", "z")},
              "lfinito": {k: ["init", "pass", "chain"] for k in ("av", "z", "zf")}}


def run_chain(ctx, ciao, alg, N, d, dtype, loss, gk, layout, refs, svrg_name=None):
    """One chain of `alg` (run_chain of tests/test_gpu_every_kernel.py, unsharded, batches of one row) with every buffer placed as
    `layout` says -> {names: {init, chain[, pass]}, outs}"""
    from oracle import twin as O
    pl = Placer(layout, dtype)
    op, dp, og, dg, x0, Li = setup(pl, loss, N, d, dtype, N * 31 + d, gk)
    Li = Li + 1e-12
    gx0 = pl.inp("x0", x0)
    st = ciao.IndexStream(N * 1000 + d)
    new = lambda k: pl.out(k, d, role=k)
    names, outs = {}, {}
    fill = alg not in refs
    ref = {}
    what = f"chain {alg} N={N} d={d} {TY[dtype]} {loss} {gk} {layout}"
    if alg in ("svrg", "svrg_cached"):
        gamma = 1.0 / (7 * Li.max())
        av, z, zf, w = new("av"), new("z"), new("zf"), new("w")
        ctx.svrg_init(dp, gx0.view, av.view, z.view, zf.view, w.view)
        names["init"] = ctx.last_kernel()
        idx = st.rand_indices(N, 3 * N + 5)
        idx[4:7] = idx[4]                              # the same row three times in a row
        gidx = pl.inp("idx", idx)
        if alg == "svrg":
            ctx.svrg_inner(dp, dg, gamma, gidx.view, av.view, z.view, zf.view, w.view)
        else:
            names["svrg"] = svrg_name
            for ep in range(2):
                ctx.svrg_iterate(dp, dg, gamma, gidx.view, False, av.view, z.view, zf.view, w.view, reuse_rowdots=True)
        names["chain"] = ctx.last_kernel()
        state = {"w": w, "z": z, "av": av, "zf": zf}
        if fill:
            rav, rz, rzf, rw = O.svrg_init(op, x0)
            if alg == "svrg":
                O.svrg_inner(op, og, dtype(gamma), idx, rav, rz, rzf, rw)
                ref = {"w": rw}
            else:
                for ep in range(2):
                    O.svrg_iterate(op, og, dtype(gamma), idx, False, rav, rz, rzf, rw)
                ref = {"zf": rzf, "av": rav}
    elif alg in ("saga", "sag"):
        gamma = 1.0 / ((16 if alg == "sag" else 3) * Li.max())
        table, av, z = pl.out("table", (N, d), role="table"), new("av"), new("z")
        ctx.saga_init(dp, dg, gamma, gx0.view, table.view, av.view, z.view)
        names["init"] = ctx.last_kernel()
        idx = st.rand_indices(N, 6 * N + 3)
        idx[4:7] = idx[4]
        gidx = pl.inp("idx", idx)
        ctx.saga_steps(dp, dg, gamma, alg == "sag", gidx.view, table.view, av.view, z.view)
        names["chain"] = ctx.last_kernel()
        state = {"table": table, "av": av, "z": z}
        if fill:
            rt, rav, rz = O.saga_init(op, og, dtype(gamma), x0)
            O.saga_steps(op, og, dtype(gamma), alg == "sag", idx, rt, rav, rz)
            ref = {"z": rz, "table": rt}
    else:
        gam = (0.999 * N / Li).astype(dtype)
        ggam = pl.inp("gam", gam)
        hg = ctx.hat_gamma(ggam.view)
        ctx.set_option("chain_max_batch", 64)
        try:
            if alg == "finito":
                table, av, z = pl.out("table", (N, d), role="table"), new("av"), new("z")
                ctx.finito_init(dp, dg, ggam.view, hg, gx0.view, table.view, av.view, z.view)
                names["init"] = ctx.last_kernel()
                batches = [st.sample_without_replacement(N, 1) for _ in range(2 * N + 3)]
                batches[3] = batches[2].copy()         # a batch met again one step later
                bptr = np.arange(len(batches) + 1, dtype=np.int64)
                gidx = pl.inp("idx", np.concatenate(batches))
                ctx.finito_steps(dp, dg, ggam.view, hg, bptr, gidx.view, table.view, av.view, z.view)
                names["chain"] = ctx.last_kernel()
                state = {"table": table, "av": av, "z": z}
                if fill:
                    rt, rav, rz, rhg = O.finito_init(op, og, gam, x0)
                    O.finito_steps(op, og, gam, rhg, batches, rt, rav, rz)
                    ref = {"z": rz, "table": rt}
            else:
                static = [np.arange(j, j + 1, dtype=np.int64) for j in range(N)]
                av, z, zf = new("av"), new("z"), new("zf")
                scratch = pl.out("scratch", d)
                ctx.lfinito_init(dp, hg, gx0.view, av.view, z.view, zf.view)
                names["init"] = ctx.last_kernel()
                ctx.full_gradient(dp, zf.view, scratch.view)   # (the pass that opens an iteration: the same sweep, asked on its own)
                names["pass"] = ctx.last_kernel()
                orders = [np.arange(N), st.randperm(N)]
                bptr = np.arange(N + 1, dtype=np.int64)
                for order in orders:
                    gidx = pl.inp("idx", np.concatenate([static[j] for j in order]))
                    ctx.lfinito_iterate(dp, dg, ggam.view, hg, bptr, gidx.view, av.view, z.view, zf.view)
                names["chain"] = ctx.last_kernel()
                state = {"av": av, "z": z, "zf": zf}
                if fill:
                    rav, rz, rzf, rhg = O.lfinito_init(op, gam, x0)
                    for order in orders:
                        O.lfinito_iterate(op, og, gam, rhg, [static[j] for j in order], rav, rz, rzf)
                    ref = {"zf": rzf, "av": rav}
        finally:
            ctx.set_option("chain_max_batch", -1)
    ctx.synchronize()
    if fill:
        refs[alg] = {k: snap(v) for k, v in ref.items()}
    outs = {k: g.view.clone() for k, g in state.items()}
    pl.check(what)
    no_poison(what, **outs)
    return {"names": names, "outs": outs, "what": what}


def chain_sites(alg):
    def sites(key, out, ref, dtype, what):
        """(6): one stated tolerance per (algorithm, output) of the chains"""
        r, r64 = ref
        if (alg, key) == ("svrg", "w"):
            close(out, r, dtype, scale={64: 150, 32: 200}, what=what, ref64=r64, scale64=230)
        elif (alg, key) == ("svrg_cached", "zf"):
            close(out, r, dtype, scale={64: 120, 32: 160}, what=what, ref64=r64, scale64=230)
        elif (alg, key) == ("svrg_cached", "av"):
            close(out, r, dtype, scale={64: 85, 32: 120}, what=what, ref64=r64, scale64=110)
        elif (alg, key) == ("saga", "z"):
            close(out, r, dtype, scale={64: 79, 32: 110}, what=what, ref64=r64, scale64=370)
        elif (alg, key) == ("saga", "table"):
            close(out, r, dtype, scale={64: 230, 32: 440}, what=what, ref64=r64, scale64=270)
        elif (alg, key) == ("sag", "z"):
            close(out, r, dtype, scale={64: 150, 32: 280}, what=what, ref64=r64, scale64=330)
        elif (alg, key) == ("sag", "table"):
            close(out, r, dtype, scale={64: 120, 32: 130}, what=what, ref64=r64, scale64=260)
        elif (alg, key) == ("finito", "z"):
            close(out, r, dtype, scale={64: 120, 32: 140}, what=what, ref64=r64, scale64=95)
        elif (alg, key) == ("finito", "table"):
            close(out, r, dtype, scale={64: 110, 32: 100}, what=what, ref64=r64, scale64=90)
        elif (alg, key) == ("lfinito", "zf"):
            close(out, r, dtype, scale={64: 96, 32: 98}, what=what, ref64=r64, scale64=65)
        elif (alg, key) == ("lfinito", "av"):
            close(out, r, dtype, scale={64: 190, 32: 150}, what=what, ref64=r64, scale64=100)
        else:
            raise KeyError((alg, key))
    return sites


# ---- the name table (chain_kernel_name of csrc/chain_launch.inc) -----------------------------------------------------------------------
REG = r"^chain_kernel<"
WIDE = r"^chain_wide_kernel<"
BIG = r"^chain_big_kernel<"
# the LDS-DMA ring's classes (plan_chain): row bytes -> (the J the name prints, block, masked); SAGA / SAG on four-wave J1 rows run the
# wave-specialised chain
RING = {1024: (1, 64, False), 1008: (1, 64, True), 2000: (1, 64, True), 4096: (1, 256, False), 4080: (1, 256, True), 8176: (2, 256, True),
        16000: (4, 256, True), 32752: (8, 512, True)}
ALG_NO = {"svrg": 0, "saga": 1, "sag": 1, "finito": 2, "lfinito": 3}   # chain_common.h CA_*


def ring_name(rowb, alg):
    J, block, masked = RING[rowb]
    fam = "chain_ws_kernel" if alg in ("saga", "sag") and block == 256 and J == 1 else "chain_dma_kernel"
    tail = rf"> .* block={block} " if fam == "chain_dma_kernel" else r",issuers\d> "
    return rf"^{fam}<\w+,J{J},alg{ALG_NO[alg]}{',masked' if masked else ''}{tail}"


def chain_expect(cls, layout, alg):
    """(class, layout) -> the family of `alg`'s chain.  The ring (chain_ring_eligible) wants the row stride and every pointer of the call 16-byte
    aligned -- A, av, z, zf, w, and the table where the algorithm keeps one -- else the register ring takes the chain.  The register
    ring, the any-length kernel and the several-workgroup chain test no pointer (the `wide` branch of plan_chain comes before the ring's;
    chain_wide_kernels.h and chain_kernels.h hold no vector cast): every layout STAYS."""
    if cls.startswith("ring"):
        return ring_name(int(cls[4:]), alg) if layout in ("tight", "pad16") else REG
    if cls == "cdma":   # complex rows: the same test over 16 KiB (plan_chain's cplx branch), else the complex register ring (300 entries: two per thread)
        cdma, creg = r"^chain_cdma_kernel<\w+,J\d,alg\d,masked> ", r"^chain_cplx_reg_kernel<\w+,alg\d,EP2> "
        return cdma if layout in ("tight", "pad16") else (T2(cdma, creg) if layout == "pad2" else creg)
    return {"reg": REG, "wide": WIDE, "big": BIG}[cls]


def chain_class(ctx, ciao, cls, dtype, d, loss, opts=None, N=13, algs=ALGS, layouts=CHAIN_LAYOUTS):
    gk = "boxvec" if loss == "logistic" else "l1"
    refs, base = {}, {}
    for layout in layouts:
        svrg_name = None
        for alg in algs:
            if layout.startswith("shift:") and layout[6:] not in USES[alg]:
                continue                                   # (the algorithm has no such buffer: the layout is `guarded`)
            for k, v in (opts or {}).items():
                ctx.set_option(k, v)
            try:
                run = run_chain(ctx, ciao, alg, N, d, dtype, loss, gk, layout, refs, svrg_name)
            finally:
                for k in (opts or {}):
                    ctx.set_option(k, 0)
            if alg == "svrg":
                svrg_name = run["names"]["chain"]
            b = base.setdefault(alg, run)
            if layout == "guarded":
                assert run["names"] == b["names"], f"{run['what']}: guards alone changed the kernels: {run['names']} / tight {b['names']}"
            elif alg != "svrg_cached":
                expect_name(chain_expect(cls, layout, alg), run["names"]["chain"], dtype, run["what"])
            compare(run, b, CHAIN_DEPS[alg], refs[alg], dtype, run["what"], chain_sites(alg))


@DTYPES
@pytest.mark.parametrize("rowb", sorted(RING))
def test_chain_lds_dma_ring(ctx, ciao, dtype, rowb):
    chain_class(ctx, ciao, f"ring{rowb}", dtype, rowb // np.dtype(dtype).itemsize, "ls" if (rowb // 16) % 2 else "logistic")


@DTYPES
@pytest.mark.parametrize("d", [50, 201, 999, 2001])
def test_chain_register_ring(ctx, ciao, dtype, d):
    chain_class(ctx, ciao, "reg", dtype, d, "ls" if d % 2 else "logistic", opts={"chain_no_dma": 1})


@DTYPES
@pytest.mark.parametrize("odd", [0, 1])
def test_chain_on_several_workgroups(ctx, ciao, dtype, odd):
    """three workgroups (five in fp32: 8200 / 2048); the first padded-stride runs of chain_wide_kernel"""
    chain_class(ctx, ciao, "wide", dtype, (4100 if dtype == F64 else 8200) + odd, "logistic" if odd else "ls")


@DTYPES
def test_chain_any_length(ctx, ciao, dtype):
    chain_class(ctx, ciao, "big", dtype, 999, "ls", opts={"chain_big": 1})


@DTYPES
def test_chain_complex_lds_dma_ring(ctx, ciao, dtype):
    """chain_cdma_kernel on 300 complex entries: 4800 bytes (J2, masked) / 2400 bytes (J1, masked).  (No cached-dots SVRG for complex T.)"""
    chain_class(ctx, ciao, "cdma", dtype, 600, "cplx", algs=tuple(a for a in ALGS if a != "svrg_cached"),
                layouts=tuple("pad2" if k == "pad3" else k for k in CHAIN_LAYOUTS))


# =====================================================================================================================================
# adaptive Finito
# =====================================================================================================================================
AF_LAYOUTS = ("tight", "guarded", "pad16", "pad3", "shift:A", "shift:table", "shift:meta", "shift:av", "shift:z")
AF_DMA, AF_REG, AF_WIDE = r"^afinito_dma_kernel<", r"^afinito_chain_kernel<", r"^afinito_wide_kernel<"
AF_DEPS = {k: ["init", "steps"] for k in ("z", "av", "hg", "table", "meta")}


def af_expect(cls, layout):
    """launch_afinito (csrc/chain_launch.inc): the LDS-DMA chain wants ring_eligible over {A, table, meta, av, z} and the row stride; else
    the register chain.  Rows beyond 32 KiB go to afinito_wide_kernel before any pointer is looked at, and a row of 999 elements is no
    whole chunk: those STAY on every layout."""
    if cls == "dma":
        return AF_DMA if layout in ("tight", "pad16") else AF_REG
    return {"reg": AF_REG, "wide": AF_WIDE}[cls]


def run_afinito(ctx, ciao, N, d, dtype, loss, layout, refs):
    from oracle import twin as O
    pl = Placer(layout, dtype)
    A, b, x0 = P.synthetic(loss, N, d, dtype, seed=21 + d)
    lam_f = float(N) if loss == "ls" else 1.0
    op, dp = problem(pl, loss, A, b, lam_f)
    og, dg = prox(pl, "l1", dtype, d)
    alpha, tol_b = 0.999, 1e-9
    idx = ciao.IndexStream(4 + d).rand_indices(N, 3 * N)
    idx[5:8] = idx[5]
    idx[10] = idx[8]
    gx0, gidx = pl.inp("x0", x0), pl.inp("idx", idx)
    table, meta4 = pl.out("table", (N, d), role="table"), pl.out("meta4", (N, 16), role="meta")
    hg, av, z = pl.out("hat_gamma", 1), pl.out("av", d, role="av"), pl.out("z", d, role="z")
    what = f"adaptive Finito N={N} d={d} {TY[dtype]} {loss} {layout}"
    names = {}
    ctx.afinito_init(dp, dg, alpha, gx0.view, table.view, meta4.view, av.view, z.view, hg.view)
    names["init"] = ctx.last_kernel()
    ctx.synchronize()
    done, trials = ctx.afinito_steps(dp, dg, alpha, tol_b, gidx.view, table.view, meta4.view, av.view, z.view, hg.view)
    names["steps"] = ctx.last_kernel()
    ctx.synchronize()
    if not refs:
        rt, rg, rgam, rfi, rav, rz, rhg = O.afinito_init(op, og, dtype(alpha), x0)
        rdone, rhg, rtrials = O.afinito_steps(op, og, dtype(alpha), dtype(tol_b), idx, rt, rg, rgam, rfi, rhg, rav, rz)
        refs.update({"z": snap(rz), "table": snap(rt), "hg": snap(np.asarray([rhg])), "done": rdone, "trials": rtrials})
        if dtype == F32:
            from oracle import twin
            t = twin.twin_of(rhg)
            refs["hg"] = (refs["hg"][0], None if t is None else np.asarray([t], dtype=np.float64))
    outs = {"z": z.view.clone(), "av": av.view.clone(), "hg": hg.view.clone(), "table": table.view.clone(),
            "meta": meta4.view.clone()}                          # (the init writes all four copies of the four per-sample scalars)
    pl.check(what)
    no_poison(what, **outs)
    assert done == refs["done"] == len(idx), (what, done, refs["done"])
    return {"names": names, "outs": outs, "what": what, "done": done, "trials": trials}


def af_sites(trials_equal):
    def sites(key, out, ref, dtype, what):
        r, r64 = ref
        if not trials_equal:     # (Float32 only, within the allowance: every later decision differs with the one that flipped)
            return
        if key == "z":
            close(out, r, dtype, scale={64: 200, 32: 400}, what=what, ref64=r64, scale64=8)
        elif key == "table":
            close(out, r, dtype, scale={64: 170, 32: 380}, what=what, ref64=r64, scale64=8)
        elif key == "hg":
            close(out, r, dtype, scale={64: 430, 32: 410}, what=what, ref64=r64, scale64=8)
        else:
            raise KeyError(key)
    return sites


def af_class(ctx, ciao, cls, dtype, d, loss, opts=None, N=13):
    refs, base = {}, None
    for layout in AF_LAYOUTS:
        for k, v in (opts or {}).items():
            ctx.set_option(k, v)
        try:
            run = run_afinito(ctx, ciao, N, d, dtype, loss, layout, refs)
        finally:
            for k in (opts or {}):
                ctx.set_option(k, 0)
        base = base or run
        if layout == "guarded":
            assert run["names"] == base["names"], f"{run['what']}: guards alone changed the kernels: {run['names']} / tight {base['names']}"
        else:
            expect_name(af_expect(cls, layout), run["names"]["steps"], dtype, run["what"])
        if run["names"] == base["names"]:                  # (5): the decisions too
            assert (run["done"], run["trials"]) == (base["done"], base["trials"]), (run["what"], run["trials"], base["trials"])
        # Float32: a backtracking test that sits on its boundary to within the rounding of the dot products may be decided differently by
        # another kernel (run_afinito of tests/test_gpu_every_kernel.py: the same allowance); Float64 compares unconditionally
        rtr = refs["trials"]
        assert abs(run["trials"] - rtr) <= (0 if dtype == F64 else max(2, rtr // 10)), (run["what"], run["trials"], rtr)
        compare(run, base, AF_DEPS, {k: refs[k] for k in ("z", "table", "hg")}, dtype, run["what"], af_sites(run["trials"] == rtr))


@DTYPES
@pytest.mark.parametrize("rowb", [1008, 4080])
def test_adaptive_finito_lds_dma_chain(ctx, ciao, dtype, rowb):
    af_class(ctx, ciao, "dma", dtype, rowb // np.dtype(dtype).itemsize, "ls" if rowb == 1008 else "logistic")


@DTYPES
def test_adaptive_finito_register_chain(ctx, ciao, dtype):
    af_class(ctx, ciao, "reg", dtype, 999, "ls")


@DTYPES
@pytest.mark.parametrize("odd", [0, 1])
def test_adaptive_finito_on_several_workgroups(ctx, ciao, dtype, odd):
    af_class(ctx, ciao, "wide", dtype, (4100 if dtype == F64 else 8200) + odd, "logistic" if odd else "ls")


# =====================================================================================================================================
# ProShI
# =====================================================================================================================================
PROSHI_LAYOUTS = ("tight", "guarded", "pad16", "pad3", "shift:Q", "shift:q", "shift:table", "shift:x")
PV, PR, PC = r"^proshi_vec_kernel<", r"^proshi_rows_kernel<\w+,\w+,NW4> ", r"^proshi_chain_kernel<"
PROSHI_DEPS = {"init.table": ["init"], "init.av": ["init"], "init.z": ["init"], "init.hg": ["init"],
               "steps.table": ["init", "steps"], "steps.av": ["init", "steps"], "steps.z": ["init", "steps"]}


def proshi_expect(cls, layout):
    """plan_proshi (csrc/rows_launch.inc) -> (init, steps): the vectorised kernel wants whole chunks and Q, q, the table, x (x0 in the
    init, z in a step) and the stride aligned, else the scalar kernel on four waves.  A run of small batches is one launch of
    proshi_chain_kernel, which asks nothing of its pointers (launch_proshi_chain; its LDS-DMA loads are single dwords): it STAYS."""
    if cls == "vec":
        return (PV, PV) if layout in ("tight", "pad16") else (PR, PR)
    return {"rows": (PR, PR), "chain": (PR, PC)}[cls]


def sepquad(pl, Q, q, eta, lo, hi):
    """PackedSepQuad over placed Q and q: the binding takes contiguous tensors only, the C struct a row stride (ciao_sepquad.ld)"""
    from ciaoalgorithms_jl_amd.device import PackedSepQuad, _DT
    import ciaoalgorithms_jl_amd._lib as L
    gQ, gq = pl.inp("Q", Q, role="Q", data=True), pl.inp("q", q, role="q", data=True)
    N, d = q.shape
    ld = int(gQ.view.stride(0))
    f = PackedSepQuad.__new__(PackedSepQuad)
    f.dense, f.Q, f.q, f.eta, f.lo, f.hi, f.N, f.d = False, gQ.view, gq.view, float(eta), float(lo), float(hi), N, d
    f.dtype, f.device, f.N_total, f.row0, f.cyclic = gQ.view.dtype, gQ.view.device, N, 0, None
    f._c = L.SepQuad(_DT[f.dtype], 0, N, d, ld, N, gQ.view.data_ptr(), gq.view.data_ptr(), f.eta, f.lo, f.hi)
    return f


def run_proshi(ctx, ciao, N, d, dtype, batches, chain, layout, refs):
    """proshi_init and a run of batches (test_proshi_steps of tests/test_gpu_parity.py on the problems of
    tests/test_gpu_proshi_dispatch.py), the batches on the batch-parallel kernel or -- chain -- as one coordinate-parallel launch"""
    from oracle import twin as O
    from ciaoalgorithms_jl_amd.device import ProxG
    import ciaoalgorithms_jl_amd._lib as L
    pl = Placer(layout, dtype)
    rng = np.random.default_rng(N + d)
    Q = rng.uniform(-1.0, 3.0, (N, d)).astype(dtype)
    q = rng.standard_normal((N, d)).astype(dtype)
    eta, lo, hi = 3.0 * N, -2.0, 2.0
    x0 = (0.5 * rng.standard_normal(d)).astype(dtype)
    gam = (0.999 * N / (np.abs(Q).max(axis=1) + eta)).astype(dtype)
    g_hi = np.linspace(0.5, 1.5, d).astype(dtype)
    df = sepquad(pl, Q, q, eta, lo, hi)
    ghi, ggam, gx0 = pl.inp("g hi", g_hi), pl.inp("gam", gam), pl.inp("x0", x0, role="x")
    dg = ProxG(L.PROX_BOX, lo=-float("inf"), hi_vec=ghi.view)
    table, av, z, hg = pl.out("table", (N, d), role="table"), pl.out("av", d), pl.out("z", d, role="x"), pl.out("hat_gamma", 1)
    gidx = pl.inp("idx", np.concatenate(batches).astype(np.int64))
    what = f"ProShI N={N} d={d} {TY[dtype]} {layout}"
    names, outs = {}, {}
    ctx.proshi_init(df, dg, ggam.view, gx0.view, table.view, av.view, z.view, hg.view)
    names["init"] = ctx.last_kernel()
    outs.update({"init.table": table.view.clone(), "init.av": av.view.clone(), "init.z": z.view.clone(), "init.hg": hg.view.clone()})
    r = len(batches[0])
    bptr = np.arange(len(batches) + 1, dtype=np.int64) * r
    ctx.set_option("proshi_chain_max_batch", -1 if chain else 0)
    try:
        ctx.proshi_steps(df, dg, ggam.view, float(hg.view.item()), bptr, gidx.view, table.view, av.view, z.view)
    finally:
        ctx.set_option("proshi_chain_max_batch", -1)
    names["steps"] = ctx.last_kernel()
    ctx.synchronize()
    outs.update({"steps.table": table.view.clone(), "steps.av": av.view.clone(), "steps.z": z.view.clone()})
    if not refs:
        of, og = O.SepQuad(Q, q, eta, lo, hi), O.Prox("box", lo=-np.inf, hi=g_hi, dtype=dtype)
        rt, rav, rz, rhg = O.proshi_init(of, og, gam, x0)
        refs.update({"init.table": snap(rt), "init.av": snap(rav), "init.z": snap(rz), "init.zsize": np.abs(rav).max() / abs(float(rhg))})
        O.proshi_steps(of, og, gam, rhg, batches, rt, rav, rz)
        refs.update({"steps.table": snap(rt), "steps.av": snap(rav), "steps.z": snap(rz), "steps.zsize": np.abs(rav).max() / abs(float(rhg))})
    pl.check(what)
    no_poison(what, **outs)
    return {"names": names, "outs": outs, "what": what}


def proshi_sites(refs):
    def sites(key, out, ref, dtype, what):
        """(6).  z = (prox(av) - av) / hat_gamma is a difference of larger quantities: its rounding unit is theirs (`size=`, as
        test_proshi_steps of tests/test_gpu_parity.py states it)"""
        r, r64 = ref
        if key == "init.table":
            close(out, r, dtype, scale=8, what=what, ref64=r64, scale64=8)
        elif key == "init.av":
            close(out, r, dtype, scale=8, what=what, ref64=r64, scale64=8)
        elif key == "init.z":
            close(out, r, dtype, scale=8, what=what, ref64=r64, scale64=8, size=refs["init.zsize"])
        elif key == "steps.table":
            close(out, r, dtype, scale={64: 8.4, 32: 8}, what=what, ref64=r64, scale64=8)
        elif key == "steps.av":
            close(out, r, dtype, scale={64: 8.8, 32: 8}, what=what, ref64=r64, scale64=14)
        elif key == "steps.z":
            close(out, r, dtype, scale=8, what=what, ref64=r64, scale64=8, size=refs["steps.zsize"])
        else:
            raise KeyError(key)
    return sites


def proshi_class(ctx, ciao, cls, dtype, N, d, batches, chain=False):
    refs, base = {}, None
    for layout in PROSHI_LAYOUTS:
        run = run_proshi(ctx, ciao, N, d, dtype, batches, chain, layout, refs)
        base = base or run
        if layout == "guarded":
            assert run["names"] == base["names"], f"{run['what']}: guards alone changed the kernels: {run['names']} / tight {base['names']}"
        else:
            for mode, want in zip(("init", "steps"), proshi_expect(cls, layout)):
                expect_name(want, run["names"][mode], dtype, f"{run['what']} {mode}")
        compare(run, base, PROSHI_DEPS, {k: v for k, v in refs.items() if not k.endswith("zsize")}, dtype, run["what"], proshi_sites(refs))


@DTYPES
def test_proshi_vectorised(ctx, ciao, dtype):
    """one 16-byte chunk per agent row, three agents: two batches of all three"""
    proshi_class(ctx, ciao, "vec", dtype, 3, vec_of(dtype), [np.array([2, 0, 1]), np.array([1, 2, 0])])


@DTYPES
def test_proshi_single_elements(ctx, ciao, dtype):
    proshi_class(ctx, ciao, "rows", dtype, 3, 3, [np.array([2, 0, 1]), np.array([1, 2, 0])])


@DTYPES
def test_proshi_coordinate_parallel_chain(ctx, ciao, dtype):
    proshi_class(ctx, ciao, "chain", dtype, 5, 7, [np.array([0, 1]), np.array([2, 3])] * 3, chain=True)

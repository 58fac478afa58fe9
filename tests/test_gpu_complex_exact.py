"""The complex chain kernels held to EXACT states (tests/complex_exact.py: Gaussian-integer lattice chains on which every association
of every real sum behind every complex operation is exact; tests/test_complex_exact_host.py for the method itself).  Every comparison
with a reference in this file is on integer views, but one: the live complex NormL1 of ONE step, under the bound its kernel states.

  a. every form of complex_exact.FORMS -- chain_cdma_kernel J = 1, 2, 4, exact and masked, and on 64 chunks (one live chunk a lane of
     the first wave); chain_cplx_reg_kernel EP = 1, 2, 4, 8 (through chain_no_dma, and unforced on fp32 rows of an odd complex count;
     last threads that hold fewer than EP entries); chain_cplx_kernel forced and past the register form (2049 entries) -- under SVRG,
     SAGA and SAG with g = Zero, and Finito (batches of 1, 2, 5) and LFinito (1, 2) with the complex NormL1's dead zone (LFinito's ids
     end in "_passthrough": there z = z_full = 0, the two gradients cancel and the ids hold ONLY that the chain leaves the full pass's
     av and z = z_full = 0 in bits -- they do not count as coverage of the LFinito leg's dots, b_i or gamma_i), in both types
     (fp64 alone where the name says so), after 1, 2, DEPTH - 1, DEPTH, DEPTH + 1, 511, 512, 513, 1025 and 1100 steps.  Compared in
     bits: SVRG z and w (z_full and av unchanged); SAGA / SAG / Finito z, av and the WHOLE table; LFinito av, z, z_full.  The launcher's
     report is asserted per call: kernel, type, J / EP, masked, algorithm, grid, block, steps;
  b. one row seven times in a row across step 512 (SAGA, fp64; Finito; SAG: five times, complex_exact.NOT_MADE_EXACT);
  c. fp32: chain_cdma_kernel and chain_cplx_reg_kernel on the same rows give the same bits (both are exact on the lattice);
  d. the live complex NormL1 on one SVRG step of every form of complex_exact.FORMS (J 1, 2, 4 exact and masked, EP 1 .. 8, both any-length shapes): prox_cpair_chain against sign(v) max(|v| - gl, 0) to 50 digits,
     absolute error below 2 eps |v| per part (csrc/ciao_common.h), exactly 0 at n2 == thr, the bits of v at gl = 0;
  e. before every case one chain of the same form and algorithm with NaN targets;
  f. the rows kernels rows_cplx_kernel and rows_csplit_kernel in every mode the plan gives, and finalize_kernel behind them (see the
     tests at the end of the file).

Every state vector and the table sit in guarded buffers (tests/layouts.py); after every call the guards, the inputs, the outputs'
NaN-freeness and the sticky error word are checked, and every call is made twice from the same state: the same bits."""
import numpy as np
import pytest

import complex_exact as E
import rows_exact as X
from layouts import Guarded, bits, has_poison, poison_bits

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
TY = {F64: "f64", F32: "f32"}
BOTH = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]


class Options:
    """library options for a block, put back whatever happens"""

    def __init__(self, ctx, **opts):
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.ctx.set_option(k, E.OPTION_DEFAULTS[k])


def repoison(g):
    bits(g.flat).fill_(poison_bits(g.flat.dtype))


def dev_bits(a, dtype):
    import torch
    return bits(torch.from_numpy(np.ascontiguousarray(X.lossless(a, dtype))).to("cuda"))


def prox_g(lam_g):
    import ciaoalgorithms_jl_amd._lib as L
    from ciaoalgorithms_jl_amd.device import ProxG
    return ProxG(L.PROX_L1_COMPLEX, lam=lam_g) if lam_g is not None else ProxG()


class Device:
    """One complex chain problem on the device: A, b as (re, im) pairs; the inputs once, one set of guarded state buffers per `State`"""

    def __init__(self, ctx, P, dtype):
        from ciaoalgorithms_jl_amd.device import PackedF
        self.ctx, self.P, self.dtype, self.spec = ctx, P, dtype, P.spec
        G = lambda a, name: Guarded(X.lossless(a, dtype), device="cuda", name=name)
        self.A, self.b, self.gam = G(E.pairs(P.A), "A"), G(E.pairs(P.b), "b"), G(P.gam, "gam")
        self.idx = Guarded(P.idx, device="cuda", name="idx")
        self.inputs = [self.A, self.b, self.gam, self.idx]
        self.F = PackedF.least_squares_complex(self.A.view, self.b.view, P.lam, N_total=E.N)
        self.g = prox_g(P.lam_g if self.spec.prox == "dead" else None)
        self.start = {"av": E.pairs(P.av0), "p": E.pairs(P.p0), "z_full": E.pairs(P.zf0), "zsum": E.pairs(P.z0), "table": E.pairs(P.table0)}


class State:
    """a chain's own state buffers, and the call on them"""

    def __init__(self, D):
        self.D = D
        alg, dt = D.spec.alg, D.dtype
        need = {"svrg": ("av", "p", "z_full", "zsum"), "lfinito": ("av", "p", "z_full")}.get(alg, ("av", "p", "table"))
        self.buf = {k: Guarded(X.lossless(D.start[k], dt), device="cuda", name=k) for k in need}
        self.first = {k: g.view.clone() for k, g in self.buf.items()}
        self.outs = {"svrg": {"z": "zsum", "w": "p"}, "lfinito": {"av": "av", "z": "p", "z_full": "z_full"}}.get(alg, {"z": "p", "av": "av", "table": "table"})
        self.kept = ("av", "z_full") if alg == "svrg" else ()

    def reset(self):
        for k, g in self.buf.items():
            g.view.copy_(self.first[k])
        if self.D.spec.alg == "lfinito":                      # written by the call: z = prox(av) of the last batch, z_full = prox(av)
            repoison(self.buf["p"])
            repoison(self.buf["z_full"])

    def call(self, k):
        D, b = self.D, self.buf
        ctx, P, alg, r = D.ctx, D.P, D.spec.alg, D.spec.r
        idx = D.idx.view[:k]
        bptr = np.array(list(range(0, k, r)) + [k], np.int64)
        if alg == "svrg":
            ctx.svrg_inner(D.F, D.g, P.gamma, idx, b["av"].view, b["zsum"].view, b["z_full"].view, b["p"].view)
        elif alg in ("saga", "sag"):
            ctx.saga_steps(D.F, D.g, P.gamma, alg == "sag", idx, b["table"].view, b["av"].view, b["p"].view)
        elif alg == "finito":
            ctx.finito_steps(D.F, D.g, D.gam.view, E.HG, bptr, idx, b["table"].view, b["av"].view, b["p"].view)
        else:
            ctx.lfinito_iterate(D.F, D.g, D.gam.view, E.HG, bptr, idx, b["av"].view, b["p"].view, b["z_full"].view)

    def check(self, what, want):
        """guards, inputs, NaN-freeness, the bits of every compared output"""
        import torch
        for g in self.D.inputs:
            g.check_outside(what)
            g.check_unchanged(what)
        for g in self.buf.values():
            g.check_outside(what)
        for k in self.kept:
            assert torch.equal(bits(self.buf[k].view), bits(self.first[k])), f"{what}: {k} changed"
        for name, k in self.outs.items():
            v = self.buf[k].view.contiguous()
            assert not has_poison(v), f"{what}: NaN in {name}"
            assert torch.equal(bits(v), want[name]), f"{what}: {name} differs from the exact result"


def last_launch_steps(k, r):
    """the steps of the call's LAST chain launch: a short last batch runs as a launch of its own (api_finito.hip same_size_run)"""
    return k if k % r == 0 else k % r


@pytest.fixture(scope="module")
def pollute(ctx):
    """part e: -> pollute(form, alg, dtype): 300 steps of the same form and algorithm on row 0 with every target NaN"""
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF

    def run(form, alg, dtype):
        d, k = 2 * form.n(dtype), 300
        tdt = torch.float64 if dtype == F64 else torch.float32
        A = torch.ones((8, d), dtype=tdt, device="cuda")
        b = torch.full((16,), float("nan"), dtype=tdt, device="cuda")
        F = PackedF.least_squares_complex(A, b, 1.0)
        g = prox_g(None)
        v = lambda: torch.ones(d, dtype=tdt, device="cuda")
        idx = torch.zeros(k, dtype=torch.int64, device="cuda")
        gam = torch.full((8,), 4.0, dtype=tdt, device="cuda")
        table = torch.ones((8, d), dtype=tdt, device="cuda")
        bptr = np.arange(k + 1, dtype=np.int64)
        out = v()
        with Options(ctx, **form.opts(dtype)):
            if alg == "svrg":
                ctx.svrg_inner(F, g, 0.5, idx, v(), v(), v(), out)
            elif alg in ("saga", "sag"):
                ctx.saga_steps(F, g, 0.5, alg == "sag", idx, table, v(), out)
            elif alg == "finito":
                ctx.finito_steps(F, g, gam, 4.0, bptr, idx, table, out, v())
            else:
                ctx.lfinito_iterate(F, g, gam, 4.0, bptr, idx, out, v(), v())
            report = ctx.last_kernel()
        ctx.synchronize()
        expect = form.expect(alg, dtype, k)
        assert E.classify_chain(report) == expect, f"the NaN chain ran as {report}, the form is {expect}"
        assert not bool(torch.isfinite(out).any()), report

    return run


def exact_chain(ctx, pollute, form, alg, r, dtype, spec):
    P, B, ref = E.found(spec)
    assert B.worst() < spec.limit and (spec.limit == X.LIMIT_BITS or dtype == F64), sorted(B.bits.items(), key=lambda kv: -kv[1])[:3]
    E.check_placements(P)
    pollute(form, alg, dtype)
    D = Device(ctx, P, dtype)
    S = State(D)
    with Options(ctx, chain_max_batch=-1, **form.opts(dtype)):
        for k in spec.counts:
            want = {name: dev_bits(v, dtype) for name, v in ref[k].items()}
            expect = form.expect(alg, dtype, last_launch_steps(k, r))
            for rep in range(2):
                S.reset()
                S.call(k)
                report = ctx.last_kernel()
                ctx.synchronize()                               # (raises on the sticky error word)
                what = f"{spec.name} {TY[dtype]}, {k} steps, call {rep} ({report})"
                assert E.classify_chain(report) == expect, f"{what}: the case is written for {expect}"
                S.check(what, want)


# ---- a. every form, every algorithm, every step count ------------------------------------------------------------------------------------------
def _cases():
    return [pytest.param(f, alg, r, dtype, id=f"{f.spec(alg, dtype, r).name}-{TY[dtype]}") for f, alg, r, dtype in E.chain_cases()]


@pytest.mark.parametrize("form,alg,r,dtype", _cases())
def test_every_complex_chain_form_gives_the_exact_state(ctx, ciao, pollute, form, alg, r, dtype):
    exact_chain(ctx, pollute, form, alg, r, dtype, form.spec(alg, dtype, r))


# ---- b. one row many times in a row across step 512 -------------------------------------------------------------------------------------------------
def _runs():
    out = []
    for name in E.RUN_FORMS:
        f = E.FORM_BY_NAME[name]
        for alg, run in E.RUN_ACROSS.items():
            for dtype in (F64, F32):
                s = f.spec(alg, dtype, run=run)
                if dtype == F64 or s.limit == X.LIMIT_BITS:
                    out.append(pytest.param(f, alg, run, dtype, id=f"{s.name}-{TY[dtype]}"))
    return out


@pytest.mark.parametrize("form,alg,run,dtype", _runs())
def test_one_row_many_times_in_a_row_across_step_512(ctx, ciao, pollute, form, alg, run, dtype):
    exact_chain(ctx, pollute, form, alg, 1, dtype, form.spec(alg, dtype, run=run))


# ---- c. fp32: the ring against the register chain ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ["svrg", "saga", "sag", "finito"])
@pytest.mark.parametrize("name", E.RING_VS_REG)
def test_fp32_ring_and_register_chain_give_the_same_bits(ctx, ciao, name, alg):
    """a 16-byte chunk holds TWO fp32 entries, so the two kernels group a dot product's terms differently: on the lattice both are
    exact, and the comparison that runs under a scale of 140 on random data (tests/test_gpu_complex.py) is one of bits"""
    import torch
    form = E.FORM_BY_NAME[name]
    spec = form.spec(alg, F32, 2 if alg == "finito" else 1)
    P, B, ref = E.found(spec)
    assert B.worst() < X.LIMIT_BITS
    D = Device(ctx, P, F32)
    ring, reg = State(D), State(D)
    for k in (E.CCHUNK + 1, spec.nsteps):
        seen = []
        for S, opts in ((ring, {}), (reg, {"chain_no_dma": 1})):
            with Options(ctx, chain_max_batch=-1, **opts):
                S.reset()
                S.call(k)
                seen.append(E.classify_chain(ctx.last_kernel())["kind"])
                ctx.synchronize()
        assert seen == ["cdma", "creg"], seen
        for key in ring.buf:
            assert torch.equal(bits(ring.buf[key].view.contiguous()), bits(reg.buf[key].view.contiguous())), (name, alg, k, key)
        ring.check(f"{spec.name} f32 on the ring, {k} steps", {n_: dev_bits(v, F32) for n_, v in ref[k].items()})


# ---- d. the live complex NormL1 on one step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("name", [f.name for f in E.FORMS])
def test_the_live_complex_norml1_of_one_step_meets_its_stated_bound(ctx, ciao, name, dtype):
    """One SVRG step from a lattice state: the prox argument v = w + gamma (gz - gp - av) is exact (a live row of two entries; av = 0
    and w on the edges of complex_exact.PROX_EDGES everywhere else), so what is measured is prox_cpair_chain's own error.

    Stated bound (csrc/ciao_common.h): absolute error below 2 eps |v| per part.  The largest observed error in eps |v| is printed."""
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    form = E.FORM_BY_NAME[name]
    n = form.n(dtype)
    eps = float(np.finfo(dtype).eps)
    rng = np.random.default_rng(n)
    A = np.zeros((2, n), np.complex128)
    A[0, 0], A[0, n - 1] = 1 + 1j, -1j
    b = np.array([1 - 2j, 0])
    edges = np.array([complex(*e) for e in E.PROX_EDGES])
    w = edges[rng.permutation(n) % len(edges)]
    w[0], w[n - 1] = 3 - 1j, 2 + 2j
    zf = np.zeros(n, np.complex128)
    zf[0], zf[n - 1] = -1 + 2j, 1 + 1j
    gamma = 0.5
    # the step's argument, exact in float64: (conj(a) (a.zf - b) - conj(a) (a.w - b) - av) gamma + w
    v = w + gamma * (np.conj(A[0]) * ((A[0] * zf).sum() - (A[0] * w).sum()))
    vp = E.pairs(v)
    X.lossless(vp, dtype)
    tdt = torch.float64 if dtype == F64 else torch.float32
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(X.lossless(a, dtype))).cuda()
    F = PackedF.least_squares_complex(dev(E.pairs(A)), dev(E.pairs(b)), 1.0, N_total=2)
    idx, zf_dev, worst = np.zeros(1, np.int64), dev(E.pairs(zf)), 0.0
    for gl in (E.PROX_GL, 0.0):
        av, z, w_dev = torch.zeros(2 * n, dtype=tdt, device="cuda"), torch.zeros(2 * n, dtype=tdt, device="cuda"), dev(E.pairs(w))
        g = prox_g(gl / gamma)
        with Options(ctx, **form.opts(dtype)):
            ctx.svrg_inner(F, g, gamma, idx, av, z, zf_dev, w_dev)
            report = ctx.last_kernel()
        ctx.synchronize()
        assert E.classify_chain(report) == form.expect("svrg", dtype, 1), report
        got = w_dev.cpu().numpy().astype(F64)
        assert torch.equal(z, w_dev), "SVRG's sum after one step from 0 is the iterate"
        if gl == 0.0:
            assert np.array_equal(got, vp), "gl = 0: the result is v in bits"
            continue
        dead = 0
        for e in range(n):
            yr, yi, m = E.prox_exact(float(v[e].real), float(v[e].imag), gl)
            if m == 0:                                           # n2 <= thr: exactly 0
                dead += 1
                assert got[2 * e] == 0 and got[2 * e + 1] == 0, (e, v[e], got[2 * e:2 * e + 2])
                continue
            from decimal import Decimal
            err = max(abs(Decimal(float(got[2 * e])) - yr), abs(Decimal(float(got[2 * e + 1])) - yi)) / (Decimal(eps) * m)
            worst = max(worst, float(err))
            assert err < 2, f"{report}: entry {e}, v = {v[e]}: {got[2 * e:2 * e + 2]} against ({float(yr)}, {float(yi)}): {float(err):.3f} eps |v|"
        assert dead >= 4 and any(abs(v[e]) == gl for e in range(n))
    print(f"{report}: the largest error of the live complex NormL1: {worst:.3f} eps |v| (stated: below 2)")


# ---- f. the rows sweeps on complex rows ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def num_cu(ctx):
    import torch
    return int(torch.cuda.get_device_properties(ctx.device).multi_processor_count)


def pollute_rows(ctx, dtype):
    """a complex GRAD sweep whose targets are all NaN: every partial d-vector and raw sum it leaves in the workspace is NaN"""
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    tdt = torch.float64 if dtype == F64 else torch.float32
    A = torch.ones((1100, 512), dtype=tdt, device="cuda")
    b = torch.full((2200,), float("nan"), dtype=tdt, device="cuda")
    av = torch.empty(512, dtype=tdt, device="cuda")
    ctx.full_gradient(PackedF.least_squares_complex(A, b, 1.0), torch.ones(512, dtype=tdt, device="cuda"), av)
    assert bool(torch.isnan(av).all()), ctx.last_kernel()


def same_bits(t, want):
    import torch
    return torch.equal(bits(t.contiguous()), bits(torch.from_numpy(np.ascontiguousarray(want)).to(t.device)))


class Rows:
    """One complex rows problem on the device (rows at stride ld: 2 n, or 2 n + 2 VEC with poisoned padding); sweep(): an entry point
    twice into poisoned outputs, the report, the guards, the inputs and the bits"""

    def __init__(self, ctx, case, P, dtype, padded):
        from ciaoalgorithms_jl_amd.device import PackedF
        self.ctx, self.case, self.P, self.dtype, self.padded, self.PackedF, self.seen = ctx, case, P, dtype, padded, PackedF, []
        G = lambda a, name, **kw: Guarded(X.lossless(a, dtype), device="cuda", name=name, **kw)
        self.A = G(E.pairs(P.A), "A", ld=P.d + 2 * X.vec_of(dtype) if padded else P.d)
        self.b, self.gam, self.x0 = G(E.pairs(P.b), "b"), G(P.gam, "gam"), G(E.pairs(P.x0), "x0")
        self.x_axis, self.z = G(E.pairs(P.x_axis), "x (on the axes)"), G(E.pairs(P.z), "z")
        self.inputs = [self.A, self.b, self.gam, self.x0, self.x_axis, self.z]
        self.b2 = {}

    def finish(self, what, fn, outs, want, k, mode, scalars=None, reset=None, inputs=()):
        """fn() twice from the same state: the report, the guards, the inputs, the bits"""
        ctx, dt = self.ctx, self.dtype
        for rep in range(2):
            if reset:
                reset()
            fn()
            report = ctx.last_kernel()
            c = E.classify_rows(report, k)
            assert (c["kind"], c["dtype"], c["J"], c["mode"]) == (self.case.kind, dt, self.case.J, E.ROW_MODE_NO[mode]), f"{what}: {report}"
            for g in list(outs.values()) + self.inputs + list(inputs):
                g.check_outside(what)
            for g in self.inputs + list(inputs):
                g.check_unchanged(what)
            for name, g in outs.items():
                assert not has_poison(g.view), f"{what}, call {rep}: NaN in {name} ({report})"
                assert same_bits(g.view, X.lossless(want[name], dt)), f"{what}, call {rep}: {name} differs from the exact result ({report})"
            for name, got, exact in (scalars() if scalars else ()):
                assert got == exact, f"{what}, call {rep}: {name} gives {got!r}, exactly {exact!r} ({report})"
        self.seen.append(c)
        return c

    def grad_axis(self, k, want):
        """GRAD at an iterate ON THE AXES with the complex NormL1 as the monitor's g: obj = {F, (1 / N) sum f_i, g(x) = lam sum |x_e|}"""
        import torch
        ctx, P, dt = self.ctx, self.P, self.dtype
        F = self.PackedF.least_squares_complex(self.A.view[:k], self.b.view[:2 * k], P.lam, N_total=P.Nt)
        av = Guarded(shape=(P.d,), dtype=dt, device="cuda", name="av")
        obj = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
        g = prox_g(P.lam_axis)

        def fn():
            ctx.set_monitor(g, obj)
            try:
                ctx.full_gradient(F, self.x_axis.view, av.view)
            finally:
                ctx.set_monitor(None, None)

        what = f"{self.case.name} {TY[dt]} grad at an on-axis iterate rows={k}"
        return self.finish(what, fn, {"av": av}, want, k, "grad", reset=lambda: (repoison(av), obj.fill_(float("nan"))),
                           scalars=lambda: (("the objective", float(obj[1]), float(want["obj"])), ("the NormL1 term", float(obj[2]), float(want["gval"])),
                                            ("F + g", float(obj[0]), float(want["obj"]) + float(want["gval"]))))

    def batch(self, mode, k, kind, want):
        """ONE Finito / LFinito batch of k rows through the rows kernels (chain_max_batch = 0), over an index list or a row block off row 0"""
        ctx, P, dt = self.ctx, self.P, self.dtype
        lists = mode.endswith("lists")
        idx = Guarded(E.batch_rows(P, k, lists), device="cuda", name="index list")
        bptr, first, length = np.array([0, k], np.int64), np.array([E.ROW0], np.int64), np.array([k], np.int64)
        S = lambda a, name: Guarded(X.lossless(a, dt), device="cuda", name=name)
        av, g = S(want["av_in"], "av"), prox_g(P.lam_g(kind))
        what = f"{self.case.name} {TY[dt]} {mode} g={kind} rows={k}{' padded' if self.padded else ''}"
        if mode.startswith("finito"):
            F = self.PackedF.least_squares_complex(self.A.view, self.b.view, P.lam, N_total=P.Nt)
            table, z = S(E.pairs(P.table0), "table"), S(E.pairs(P.z), "z (in / out)")
            if lists:
                fn = lambda: ctx.finito_steps(F, g, self.gam.view, P.hg, bptr, idx.view, table.view, av.view, z.view)
            else:
                fn = lambda: ctx.finito_steps_blocks(F, g, self.gam.view, P.hg, first, length, table.view, av.view, z.view)
            start = [(b, b.view.clone()) for b in (table, av, z)]
            return self.finish(what, fn, {"table": table, "av": av, "z": z}, want, k, mode, inputs=[idx],
                               reset=lambda: [b.view.copy_(t) for b, t in start])
        if kind not in self.b2:
            self.b2[kind] = S(E.pairs(P.b2(kind)), "b (LFinito)")
        F = self.PackedF.least_squares_complex(self.A.view, self.b2[kind].view, P.lam, N_total=P.Nt)
        z, zf = Guarded(shape=(P.d,), dtype=dt, device="cuda", name="z"), Guarded(shape=(P.d,), dtype=dt, device="cuda", name="z_full")
        if lists:
            fn = lambda: ctx.lfinito_iterate(F, g, self.gam.view, P.hg, bptr, idx.view, av.view, z.view, zf.view)
        else:
            fn = lambda: ctx.lfinito_iterate_blocks(F, g, self.gam.view, P.hg, first, length, av.view, z.view, zf.view)
        start = av.view.clone()
        return self.finish(what, fn, {"av": av, "z": z, "z_full": zf}, want, k, mode, inputs=[idx, self.b2[kind]],
                           reset=lambda: (av.view.copy_(start), repoison(z), repoison(zf)))

    def sweep(self, mode, k, want):
        import torch
        ctx, P, d, dt = self.ctx, self.P, self.P.d, self.dtype
        F = self.PackedF.least_squares_complex(self.A.view[:k], self.b.view[:2 * k], P.lam, N_total=P.Nt)
        out = lambda name, shape: Guarded(shape=shape, dtype=dt, device="cuda", name=name)
        obj = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
        if mode == "grad":
            outs = {"av": out("av", (d,))}

            def fn():
                ctx.set_monitor(None, obj)
                try:
                    ctx.full_gradient(F, self.x0.view, outs["av"].view)
                finally:
                    ctx.set_monitor(None, None)
        else:
            outs = {"table": out("table", (k, d)), "av": out("av", (d,)), "z": out("z", (d,))}
            gam = Guarded(X.lossless(P.gam[:k], dt), device="cuda", name="gam (the sweep's rows)")
            if mode == "saga_init":
                fn = lambda: ctx.saga_init(F, prox_g(None), P.saga_gamma, self.x0.view, outs["table"].view, outs["av"].view, outs["z"].view)
            else:
                fn = lambda: ctx.finito_init(F, prox_g(None), gam.view, P.hg, self.x0.view, outs["table"].view, outs["av"].view, outs["z"].view)
        what = f"{self.case.name} {TY[dt]} {mode} rows={k}{' padded' if self.padded else ''}"
        for rep in range(2):
            for g in outs.values():
                repoison(g)
            obj.fill_(float("nan"))
            fn()
            report = ctx.last_kernel()
            c = E.classify_rows(report, k)
            assert (c["kind"], c["dtype"], c["J"], c["mode"]) == (self.case.kind, dt, self.case.J, E.ROW_MODE_NO[mode]), f"{what}: {report}"
            for g in list(outs.values()) + self.inputs:
                g.check_outside(what)
            for g in self.inputs:
                g.check_unchanged(what)
            for name, g in outs.items():
                assert not has_poison(g.view), f"{what}, call {rep}: NaN in {name} ({report})"
                assert same_bits(g.view, X.lossless(want[name], dt)), f"{what}, call {rep}: {name} differs from the exact result ({report})"
            if mode == "grad":
                assert float(obj[1]) == float(want["obj"]), f"{what}, call {rep}: the objective gives {float(obj[1])!r}, exactly {float(want['obj'])!r} ({report})"
        self.seen.append(c)
        return c


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("case", E.ROWS_CASES, ids=lambda c: c.name)
def test_complex_rows_sweeps_at_every_trip_class_exactly(ctx, ciao, num_cu, case, dtype):
    """Every mode the plan gives on rows_cplx_kernel and rows_csplit_kernel: GRAD (av, the LeastSquares objective lam / 2 |res|^2 and,
    at an on-axis iterate, the NormL1 term), SAGA_INIT and FINITO_INIT (the whole table, av, z) with g = Zero; FINITO_BATCH over index
    lists and over row blocks off row 0 with g = Zero, the complex NormL1's dead zone and LIVE on-axis prox arguments (|v| and gl powers
    of two); GRAD2 through lfinito_iterate (lists, blocks) with g = Zero and the dead zone -- one batch a call from a lattice state.  At
    ld = d and under poisoned padding; grids of 1, 2, 3 and the plan's own and the trip classes come from the row counts (complex_exact:
    `sweep_grid` does not reach the complex plans) and are asserted from the reports"""
    pollute_rows(ctx, dtype)
    P, B, seen = case.problem(dtype, num_cu), X.Bounds(), []
    launches = case.launches(num_cu)
    with Options(ctx, **case.opts):
        for padded in (False, True):
            R = Rows(ctx, case, P, dtype, padded)
            for k in (launches if not padded else launches[-1:]):
                want_grid = min(-(-k // 4), num_cu) if case.kind == "cplx" else min(k, num_cu * case.opts.get("split_blocks_per_cu", 1))
                got = [R.sweep(mode, k, E.rows_reference(P, mode, k, B)) for mode in E.ROW_SWEEPS]
                got.append(R.grad_axis(k, E.rows_reference(P, "grad", k, B, x=P.x_axis)))
                # (beyond 8192 reals a batch of up to three rows runs as a chain whatever chain_max_batch says: api_finito.hip batch_as_chain)
                with Options(ctx, chain_max_batch=0):
                    for mode in (E.ROW_BATCHES if P.d <= 8192 or k > 3 else ()):
                        for kind in E.BATCH_PROX[mode.split("_")[0]]:
                            got.append(R.batch(mode, k, kind, E.rows_batch_reference(P, mode, k, B, kind)))
                assert all(c["grid"] == want_grid for c in got), (case.name, k, want_grid, [c["grid"] for c in got])
            seen += R.seen
    ctx.synchronize()
    assert B.worst() < X.LIMIT_BITS, sorted(B.bits.items(), key=lambda kv: -kv[1])[:3]
    reached = set().union(*(E.trip_classes(c) for c in seen))
    assert case.need() <= reached, f"{case.name} on {num_cu} compute units: its launches never reach {sorted(case.need() - reached)}"


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("kind", ["csplit", "cplx"])
def test_finalize_behind_a_complex_sweep_at_every_partial_count(ctx, ciao, num_cu, kind, dtype):
    """rows_csplit_kernel (whole chunks: one partial a row, split_blocks_per_cu = 8) at 1, 2, 33, 64, 65, 257 and 1025 partials; rows_cplx_kernel
    (35 entries: one partial a WAVE, so a multiple of 4) at the nearest counts it reaches, 4 .. 4 min(257, CUs)"""
    pollute_rows(ctx, dtype)
    if kind == "csplit":
        case, opts = E.RowsCase("finalize_csplit", "csplit", chunks=64, J=1), {"split_blocks_per_cu": 8}
        rows = [p for p in E.FINALIZE_PARTS if p <= 8 * num_cu]
        assert rows == list(E.FINALIZE_PARTS) or num_cu < 129
    else:
        case, opts = E.RowsCase("finalize_cplx", "cplx", n=35), {}
        rows = sorted({min(4 * p, 4 * num_cu) for p in (1, 2, 9, 16, 17, 65, 257)})
        assert rows == [4, 8, 36, 64, 68, 260, 1024] or num_cu != 256     # (the counts reached on the 256 CUs of an MI355X)
    P, B = E.RowsProblem(max(rows), case.n(dtype), seed=11), X.Bounds()
    with Options(ctx, **opts):
        R = Rows(ctx, case, P, dtype, False)
        for k in rows:
            c = R.sweep("grad", k, E.rows_reference(P, "grad", k, B))
            assert c["parts"] == k, (k, c)
    ctx.synchronize()
    assert B.worst() < X.LIMIT_BITS

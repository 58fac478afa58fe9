"""The real-typed chain kernels held to EXACT states (tests/chains_exact.py: lattice chains on which every association of every sum of
every step is exact; tests/test_chains_exact_host.py for the method itself).  No tolerance in this file: every comparison is on integer
views.

  a. every kernel form of chains_exact.FORMS -- chain_kernel on one wave and four, masked and full, up to the largest E built;
     chain_big_kernel forced and beyond one workgroup; chain_dma_kernel on one, four and eight waves, J = 1, 2, 4, 8, exact and masked;
     chain_ws_kernel with one and two issuer waves; chain_wide_kernel on three and five workgroups with a last workgroup of one column --
     under SVRG, cached-dots SVRG (chain_dma_kernel's own: a whole svrg_iterate after svrg_init, against the exact state and against the
     same call with the cache refused), SAGA, SAG, Finito (batches of 1, 2 and 5) and LFinito, in both types (fp64 alone where the case's name says so), after
     every step count of the case (1, 2, DEPTH - 1, DEPTH, DEPTH + 1, 1023, 1024, 1025, 2049 and the whole chain; the last ring
     revolution whole, partial and single).  What is compared in bits: SVRG z and w (z_full and av unchanged); SAGA / SAG and Finito z, av
     and the WHOLE table; LFinito av, z and z_full.  The kernel the launcher reports is asserted per call (chains_exact.classify against
     Form.expect): a changed plan fails instead of passing on another kernel;
  b. a chain batch: three chains of 1, 9 and 1025 steps in one launch, each the bits of its exact reference and of the single launch;
     The logistic instantiations of SAGA, SAG and Finito run on rows whose margins per-coordinate bounds lo = hi = 0 hold at 0;
  c. before every test one chain of the same form and algorithm with NaN targets leaves NaN in whatever the kernel keeps between calls
     (LDS, the wide chain's mailbox, the workspace): the exact calls after it must not see any of it.

Every state vector and the table sit in guarded buffers (tests/layouts.py); after every call the guards, the inputs (A, b, idx, gam, the
bounds), the outputs' NaN-freeness and the sticky error word (Context.synchronize raises on it) are checked, and every call is made
twice from the same state: the second must give the same bits.  The bound that makes all of this a statement is computed from the data
and asserted for every case (chains_exact.found)."""
import numpy as np
import pytest

import chains_exact as C
import rows_exact as X
from layouts import Guarded, bits, has_poison, poison_bits

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
TY = {F64: "f64", F32: "f32"}


def _logistic_cases():
    return [pytest.param(C.FORM_BY_NAME[name], alg, dtype, id=f"{C.FORM_BY_NAME[name].spec(alg, dtype, loss='logistic').name}-{TY[dtype]}")
            for name, algs in C.LOGISTIC for alg in algs for dtype in C.FORM_BY_NAME[name].dtypes]


def _cases():
    out = []
    for f in C.FORMS:
        for alg in f.algs:
            for r in (f.r if alg in ("finito", "lfinito") else (1,)):
                for dtype in f.dtypes:
                    spec = f.spec(alg, dtype, r)
                    if dtype == F64 or spec.limit == X.LIMIT_BITS:
                        out.append(pytest.param(f, alg, r, dtype, id=f"{spec.name}-{TY[dtype]}"))
    return out


class Options:
    """library options for a block, put back whatever happens"""

    def __init__(self, ctx, **opts):
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.ctx.set_option(k, C.OPTION_DEFAULTS[k])


def repoison(g):
    bits(g.flat).fill_(poison_bits(g.flat.dtype))


def dev_bits(a, dtype):
    import torch
    return bits(torch.from_numpy(np.ascontiguousarray(X.lossless(a, dtype))).to("cuda"))


class Device:
    """One chain problem on the device: the inputs once, one set of guarded state buffers per `State`"""

    def __init__(self, ctx, P, dtype):
        import ciaoalgorithms_jl_amd._lib as L
        from ciaoalgorithms_jl_amd.device import PackedF, ProxG
        self.ctx, self.P, self.dtype, self.spec = ctx, P, dtype, P.spec
        G = lambda a, name: Guarded(X.lossless(a, dtype), device="cuda", name=name)
        self.A, self.b, self.gam = G(P.A, "A"), G(P.b, "b"), G(P.gam, "gam")
        self.idx = Guarded(P.idx, device="cuda", name="idx")
        self.inputs = [self.A, self.b, self.gam, self.idx]
        if self.spec.loss == "logistic":
            self.F = PackedF.logistic(self.A.view, self.b.view, N_total=C.N)
        else:
            self.F = PackedF.least_squares(self.A.view, self.b.view, P.lam, N_total=C.N)
        if self.spec.prox == "l1":
            self.g = ProxG(L.PROX_L1, lam=P.lam_g)
        elif self.spec.prox == "box":
            self.g = ProxG(L.PROX_BOX, lo=-2.0, hi=2.0)
        else:
            self.lo, self.hi = G(P.lo, "lo"), G(P.hi, "hi")
            self.inputs += [self.lo, self.hi]
            self.g = ProxG(L.PROX_BOX, lo_vec=self.lo.view, hi_vec=self.hi.view)
        self.start = {"av": P.av0, "p": P.p0, "z_full": P.zf0, "zsum": P.z0, "table": P.table0}
        if self.spec.alg == "svrgc":                          # svrg_init's x0
            self.x0 = G(P.zf0, "x0")
            self.inputs.append(self.x0)


class State:
    """a chain's own state buffers, and the call on them"""

    def __init__(self, D):
        self.D = D
        alg, dt, d = D.spec.alg, D.dtype, D.P.d
        need = {"svrg": ("av", "p", "z_full", "zsum"), "svrgc": ("av", "p", "z_full", "zsum"), "lfinito": ("av", "p", "z_full")}.get(alg, ("av", "p", "table"))
        self.buf = {k: Guarded(X.lossless(D.start[k], dt), device="cuda", name=k) for k in need}
        self.first = {k: g.view.clone() for k, g in self.buf.items()}
        # which buffer holds which compared output / which must come back unchanged
        self.outs = {"svrg": {"z": "zsum", "w": "p"}, "svrgc": {"av": "av", "z": "zsum", "z_full": "z_full", "w": "p"},
                     "lfinito": {"av": "av", "z": "p", "z_full": "z_full"}}.get(alg, {"z": "p", "av": "av", "table": "table"})
        self.kept = ("av", "z_full") if alg == "svrg" else ()

    def reset(self):
        for k, g in self.buf.items():
            g.view.copy_(self.first[k])
        if self.D.spec.alg == "lfinito":                      # written by the call: z = prox(av) of the last batch, z_full = prox(av)
            repoison(self.buf["p"])
            repoison(self.buf["z_full"])
        if self.D.spec.alg == "svrgc":                        # svrg_init writes all four
            for g in self.buf.values():
                repoison(g)

    def call(self, n, reuse_rowdots=True):
        D, b = self.D, self.buf
        ctx, P, alg, r = D.ctx, D.P, D.spec.alg, D.spec.r
        idx = D.idx.view[:n]
        bptr = np.array(list(range(0, n, r)) + [n], np.int64)
        if alg == "svrg":
            ctx.svrg_inner(D.F, D.g, P.gamma, idx, b["av"].view, b["zsum"].view, b["z_full"].view, b["p"].view)
        elif alg == "svrgc":
            # the init's full pass caches a_i'x0 for z_full = x0; the iterate's inner cycle then runs on them (api_solvers.hip svrg_inner_t)
            ctx.svrg_init(D.F, D.x0.view, b["av"].view, b["zsum"].view, b["z_full"].view, b["p"].view)
            ctx.svrg_iterate(D.F, D.g, P.gamma, idx, D.spec.plus, b["av"].view, b["zsum"].view, b["z_full"].view, b["p"].view,
                             reuse_rowdots=reuse_rowdots)
        elif alg in ("saga", "sag"):
            ctx.saga_steps(D.F, D.g, P.gamma, alg == "sag", idx, b["table"].view, b["av"].view, b["p"].view)
        elif alg == "finito":
            ctx.finito_steps(D.F, D.g, D.gam.view, C.HG, bptr, idx, b["table"].view, b["av"].view, b["p"].view)
        else:
            ctx.lfinito_iterate(D.F, D.g, D.gam.view, C.HG, bptr, idx, b["av"].view, b["p"].view, b["z_full"].view)

    def check(self, what, want):
        """guards, inputs, NaN-freeness, the bits of every compared output"""
        import torch
        D = self.D
        for g in D.inputs:
            g.check_outside(what)
            g.check_unchanged(what)
        for k, g in self.buf.items():
            g.check_outside(what)
        for k in self.kept:
            assert torch.equal(bits(self.buf[k].view), bits(self.first[k])), f"{what}: {k} changed"
        for name, k in self.outs.items():
            v = self.buf[k].view.contiguous()
            assert not has_poison(v), f"{what}: NaN in {name}"
            assert torch.equal(bits(v), want[name]), f"{what}: {name} differs from the exact result"


def last_launch_steps(n, r):
    """the steps of the call's LAST chain launch: a short last batch runs as a launch of its own (api_finito.hip same_size_run)"""
    return n if n % r == 0 else n % r


@pytest.fixture(scope="module")
def pollute(ctx):
    """part c: -> pollute(form, alg, dtype): 300 steps of the same form and algorithm on row 0 with every target NaN"""
    import torch
    import ciaoalgorithms_jl_amd._lib as L
    from ciaoalgorithms_jl_amd.device import PackedF, ProxG

    def run(form, alg, dtype):
        d, n = form.d(dtype), 300
        tdt = torch.float64 if dtype == F64 else torch.float32
        A = torch.ones((8, d), dtype=tdt, device="cuda")
        b = torch.full((8,), float("nan"), dtype=tdt, device="cuda")
        F = PackedF.least_squares(A, b, 1.0)
        g = ProxG(L.PROX_L1, lam=0.5)
        v = lambda: torch.ones(d, dtype=tdt, device="cuda")
        idx = torch.zeros(n, dtype=torch.int64, device="cuda")
        gam = torch.full((8,), 4.0, dtype=tdt, device="cuda")
        table = torch.ones((8, d), dtype=tdt, device="cuda")
        bptr = np.arange(n + 1, dtype=np.int64)
        with Options(ctx, **form.opts):
            if alg in ("svrg", "svrgc"):
                out = v()
                ctx.svrg_inner(F, g, 0.5, idx, v(), v(), v(), out)
            elif alg in ("saga", "sag"):
                out = v()
                ctx.saga_steps(F, g, 0.5, alg == "sag", idx, table, v(), out)
            elif alg == "finito":
                out = v()
                ctx.finito_steps(F, g, gam, 4.0, bptr, idx, table, out, v())
            else:
                out = v()
                ctx.lfinito_iterate(F, g, gam, 4.0, bptr, idx, out, v(), v())
            report = ctx.last_kernel()
        ctx.synchronize()
        expect = form.expect("svrg" if alg == "svrgc" else alg, dtype, n)
        assert C.classify(report) == expect, f"the NaN chain ran as {report}, the form is {expect}"
        assert not bool(torch.isfinite(out).any()), report       # (NaN, or what the prox makes of it: -inf)

    return run


# ---- a. every form, every algorithm, every step count ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")])
@pytest.mark.parametrize("name", ["dma_4w_j1", "ws_issuers2", "reg_4w_d257", "wide_5"])
def test_one_row_seven_times_in_a_row_across_a_chunk_boundary(ctx, ciao, pollute, name, dtype):
    """SAGA, steps 1021 .. 1027 on one row"""
    form = C.FORM_BY_NAME[name]
    exact_chain(ctx, pollute, form, "saga", 1, dtype, form.spec("saga", dtype, seven=True))


@pytest.mark.parametrize("form,alg,dtype", _logistic_cases())
def test_logistic_rows_at_margin_zero_give_the_exact_state(ctx, ciao, pollute, form, alg, dtype):
    """the LOSS = logistic instantiations of SAGA, SAG and Finito: every margin held at 0 by lo = hi = 0, the coefficient -y / 2"""
    exact_chain(ctx, pollute, form, alg, 1, dtype, form.spec(alg, dtype, loss="logistic"))


@pytest.mark.parametrize("form,alg,r,dtype", _cases())
def test_every_chain_form_gives_the_exact_state(ctx, ciao, pollute, form, alg, r, dtype):
    exact_chain(ctx, pollute, form, alg, r, dtype, form.spec(alg, dtype, r))


def exact_chain(ctx, pollute, form, alg, r, dtype, spec):
    P, B, ref = C.found(spec)
    assert B.worst() < spec.limit and (spec.limit == X.LIMIT_BITS or dtype == F64), sorted(B.bits.items(), key=lambda kv: -kv[1])[:3]
    C.check_placements(P)
    pollute(form, alg, dtype)
    D = Device(ctx, P, dtype)
    S = State(D)
    with Options(ctx, chain_max_batch=-1, **form.opts):
        for n in spec.counts:
            want = {k: dev_bits(v, dtype) for k, v in ref[n].items()}
            expect = form.expect(alg, dtype, last_launch_steps(n, r))
            # cached-dots SVRG: twice on the cached a_i'z_full, then once with the cache refused -- plain SVRG, the same bits
            for rep, reuse in enumerate((True, True, False) if alg == "svrgc" else (True, True)):
                S.reset()
                S.call(n, reuse)
                report = ctx.last_kernel()
                ctx.synchronize()                               # (raises on the sticky error word)
                what = f"{spec.name} {TY[dtype]}, {n} steps, call {rep} ({report})"
                if alg == "svrgc":                              # (the chain's own name is not observable: the epoch tail's full pass writes last)
                    assert report.startswith("rows_"), what
                else:
                    assert C.classify(report) == expect, f"{what}: the case is written for {expect}"
                S.check(what, want)


# ---- b. the chain batch ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")])
@pytest.mark.parametrize("alg", ["svrg", "saga"])
def test_a_chain_batch_of_three_step_counts_gives_each_chains_exact_state(ctx, ciao, pollute, alg, dtype):
    form = C.FORM_BY_NAME["dma_4w_j1"]
    spec = form.spec(alg, dtype)
    P, B, ref = C.found(spec)
    assert B.worst() < X.LIMIT_BITS
    counts = (1, spec.depth + 1, 1025)
    assert set(counts) <= set(spec.counts)
    pollute(form, alg, dtype)
    D = Device(ctx, P, dtype)
    import torch
    chains, alone = [State(D) for _ in counts], [State(D) for _ in counts]
    want = [{k: dev_bits(v, dtype) for k, v in ref[n].items()} for n in counts]
    for T, n, w in zip(alone, counts, want):
        T.reset()
        T.call(n)
        ctx.synchronize()
        T.check(f"{spec.name} {TY[dtype]}: the chain of {n} steps alone", w)
    for rep in range(2):                                        # the batch twice from the same states
        for S in chains:
            S.reset()
        with ctx.chain_batch():
            for S, n in zip(chains, counts):
                S.call(n)
        report = ctx.last_kernel()
        ctx.synchronize()
        c = C.classify(report)
        assert (c["chains"], c["launches"], c["kind"], c["workgroups"], c["threads"]) == (3, 1, "dma", 3, 256), report
        for S, T, n, w in zip(chains, alone, counts, want):
            S.check(f"{spec.name} {TY[dtype]}: the chain of {n} steps in the batch, call {rep} ({report})", w)
            for k in S.buf:
                assert torch.equal(bits(S.buf[k].view.contiguous()), bits(T.buf[k].view.contiguous())), (n, k)

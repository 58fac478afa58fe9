"""ciao_gram_cd_general on the device: coordinate descent with bounds, penalty factors, a ridge and a Gram matrix, u and tol per model
(csrc/gramcdg_kernels.h).

  1. bits: X, R and stat equal host_route.host_gram_cd_general's bit for bit at the pair edges, the 256 / 1024 block switch and the LDS
     cap, in one launch per d that mixes models of several kinds (defaults; non-negative with factors; boxes with both bounds active and
     factors 0 and +inf), each with its own u, ridge (through inv), tol and Gram matrix out of three in scrambled order; cold and warm
     starts, a warm start outside its bounds; four layouts (ldg = d and beyond, odd ldg and set stride, G 8 bytes off 16-byte alignment,
     vector strides beyond d and 0), every padding column and every slot beyond a vector poisoned, every buffer guarded;
  2. the defaults -- left out, and spelled out as tensors -- are Context.gram_cd bit for bit;
  3. independence: a launch permuted, subsets of it, a model alone;
  4. states 3 and 2 end one model only; X and R of a state-3 model keep their sentinels;
  5. every refusal of include/ciao_hip.h launches nothing;
  6. the drivers: gram.lasso_cd with bounds, factors or a ridge on device statistics has the host route's bits; cv.lasso_cv(fused=True)
     is fused=False bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

from layouts import POISON64, Guarded, bits, poisoned

pytestmark = pytest.mark.gpu

D_SIZES = [1, 3, 17, 255, 256, 257, 513, 1024, 1025, 4096]
K_OF = {1: 2, 3: 9, 17: 64, 255: 9, 256: 2, 257: 64, 513: 2, 1024: 9, 1025: 9, 4096: 2}      # tests/test_gpu_gram_cd.py's, and 1024
SWEEPS_OF = {4096: 3, 1025: 6, 1024: 6}                                                       # the numpy mirror runs in seconds
S = 3
INT_MAX = 2 ** 31 - 1


def plan(d, ldg, sg, g_ptr, K, sets):
    """csrc/gramcdg_kernels.h: gramcdg_plan, restated -> what last_kernel must say (sg: 0 with one set)"""
    block = 256 if d <= 1024 else 1024
    vec = g_ptr % 16 == 0 and ldg % 2 == 0 and sg % 2 == 0
    lds = 4 * ((d + 1) // 2 * 2) * 8 + (d + 15) // 16 * 16 + 16
    return f"gramcdg_kernel<{block},{'vec16' if vec else 'elem'}> grid={K} block={block} lds={lds} sets={sets}"


def same(t, a):
    import torch
    return torch.equal(bits(t.contiguous().cpu()), bits(torch.from_numpy(np.ascontiguousarray(a))))


_CASES = {}


def case(d):
    """Three Gram matrices (of three row blocks of one Gaussian matrix with a duplicated and a zero column), K models of mixed kinds,
    and the mirror's answers, made once.  Model k: kind k % 3 (0: boxes of half-width 0.05 around 0 with factors 0, 0.5, 2 and +inf and
    a few one-sided coordinates; 1: non-negative with factors 0.5, 1, 2; 2: the defaults), set (2 k + 1) % 3, u scaled by (1, -1, 0.5)
    [k % 3], ridge (0, 0.3, 2 mean G_jj)[(k // 3) % 3] inside inv, tol (0, 1e-7, 1e-10) sum b^2 [(k + 1) % 3]."""
    if d in _CASES:
        return _CASES[d]
    from ciaoalgorithms_jl_amd.host_route import host_gram_cd_general
    rng = np.random.default_rng(2000 + d)
    N, K = min(d + 3, 96), K_OF[d]
    Gs, us, bb = [], [], 0.0
    for s in range(S):
        A = rng.standard_normal((N, d))
        if d >= 3:
            A[:, 1] = A[:, 0]
        if d >= 2:
            A[:, d - 1] = 0.0
        b = A @ (rng.standard_normal(d) * (rng.random(d) < 0.1)) + 0.1 * rng.standard_normal(N)
        G = A.T @ A
        Gs.append(np.triu(G) + np.triu(G, 1).T)
        us.append(A.T @ b)
        bb += float(b @ b)
    G = np.stack(Gs)
    gsel = ((2 * np.arange(K) + 1) % S).astype(np.int32)
    u = np.stack([us[gsel[k]] * (1.0, -1.0, 0.5)[k % 3] for k in range(K)])
    inv = np.empty((K, d))
    for k in range(K):
        dg = np.diagonal(G[gsel[k]])
        den = dg + (0.0, 0.3, 2.0 * dg.mean())[(k // 3) % 3]
        with np.errstate(divide="ignore"):
            inv[k] = np.where(den > 0, 1.0 / den, 0.0)
    tau = np.abs(u).max(1) * (0.05 + 0.5 * (np.arange(K) + 1.0) / (K + 1.0))
    tol = np.array([(0.0, 1e-7, 1e-10)[(k + 1) % 3] * bb for k in range(K)])
    pf, lo, hi = np.ones((K, d)), np.full((K, d), -np.inf), np.full((K, d), np.inf)
    for k in range(K):
        if k % 3 == 0:
            pf[k] = rng.choice([0.0, 0.5, 2.0, np.inf], d, p=[0.2, 0.4, 0.3, 0.1])
            lo[k], hi[k] = -0.05, 0.05
            one = rng.random(d) < 0.2
            lo[k, one & (np.arange(d) % 2 == 0)] = -0.0
            hi[k, one & (np.arange(d) % 2 == 1)] = 0.0
        elif k % 3 == 1:
            pf[k] = rng.choice([0.5, 1.0, 2.0], d)
            lo[k] = 0.0
    warm = rng.standard_normal((K, d)) * (rng.random((K, d)) < 0.05)
    warm[:, 0] = 0.5                                       # outside the boxes of kind 0
    warm[:, d - 1] = -2.0                                  # ... and below the bound of kind 1, on the zero column
    if d >= 3:
        warm[:, 1] = 0.25
    ms = SWEEPS_OF.get(d, 12)
    c = dict(d=d, K=K, G=G, gsel=gsel, u=u, inv=inv, tau=tau, tol=tol, pf=pf, lo=lo, hi=hi, ms=ms, starts={"cold": np.zeros((K, d)), "warm": warm})
    kw = dict(gsel=gsel, pf=pf, lo=lo, hi=hi)
    c["want"] = {n: host_gram_cd_general(G, u, inv, tau, x0, tol, ms, **kw) for n, x0 in c["starts"].items()}
    # the shared-vector form: one u, inv, pf, lo, hi for all models (the model of kind 0 if there is room for one)
    c["shared"] = {n: host_gram_cd_general(G, u[0], inv[0], tau, x0, tol, ms, gsel=gsel, pf=pf[0], lo=lo[0], hi=hi[0]) for n, x0 in (("warm", warm),)}
    _CASES[d] = c
    return c


def layouts_of(d):
    """(name, off of G, ldg, slack of the set stride, off of the vectors, stride of the per-model vectors, ldx, R given, ldr, shared vectors)"""
    even = d + (d % 2)
    return [("packed", 0, d, 0, 0, d, d, True, d, False),
            ("odd-strides", 0, d + 3 - (d % 2), 0, 1, d + 5, d + 5, False, 0, False),               # odd ldg, odd set stride
            ("off-base", 1, even, 0, 0, d + 2, d + 1, True, d + 2, False),
            ("even-strides-shared", 0, even + 2, 2 + d % 2, 1, 0, d, True, d + 7, True)]             # even ldg, even set stride


class Sets:
    """S matrices of d x d at row stride ldg, sg elements apart, in a poisoned buffer: padding columns, the gaps between the sets and a
    guard band on both sides all carry the poison"""

    def __init__(self, G, off, ldg, slack):
        import torch
        s, d, _ = G.shape
        self.sg = (d - 1) * ldg + d + slack
        guard = 64
        self.flat = poisoned((2 * guard + off + s * self.sg,), torch.float64, "cuda")
        self.view = torch.as_strided(self.flat, (s, d, d), (self.sg, ldg, 1), guard + off)
        self.view.copy_(torch.from_numpy(G))
        self.orig = bits(self.flat).clone()

    def check_unchanged(self, what):
        import torch
        assert torch.equal(bits(self.flat), self.orig), f"{what}: G was written"


def int32_guarded(a):
    import torch
    buf = torch.full((len(a) + 16,), INT_MAX, dtype=torch.int32, device="cuda")
    buf[8:8 + len(a)] = torch.from_numpy(np.asarray(a, np.int32)).cuda()
    return buf, buf[8:8 + len(a)]


def launch(ctx, c, lay, start, G=None, over=None):
    """one call through Context.gram_cd_general, every buffer guarded -> (X, R or None, stat) on the host, after the layout checks"""
    name, goff, ldg, slack, voff, ldv, ldx, with_r, ldr, shared = lay
    d, K = c["d"], c["K"]
    v = dict(c)
    v.update(over or {})
    g = G if G is not None else Sets(v["G"], goff, ldg, slack)

    def vecs(n):
        a = v[n]
        if a is None:
            return None
        if shared:
            return Guarded(a[0] if a.ndim == 2 else a, off=voff, device="cuda", name=n)
        return Guarded(a, off=voff, ld=max(ldv, d), device="cuda", name=n)

    ins = {n: vecs(n) for n in ("u", "inv", "pf", "lo", "hi")}
    small = {n: Guarded(v[n], off=voff, device="cuda", name=n) for n in ("tau", "tol")}
    gbuf, gsel = int32_guarded(v["gsel"])
    X = Guarded(start, off=voff, ld=ldx, device="cuda", name="X")
    R = Guarded(shape=(K, d), dtype=np.float64, off=voff, ld=ldr, device="cuda", name="R") if with_r else None
    stat = Guarded(shape=(K, 4), dtype=np.float64, device="cuda", name="stat")
    view = lambda b: None if b is None else b.view
    ctx.gram_cd_general(g.view, ins["u"].view, ins["inv"].view, small["tau"].view, X.view, small["tol"].view, v["ms"], gsel=gsel,
                        pf=view(ins["pf"]), lo=view(ins["lo"]), hi=view(ins["hi"]), R=R.view if with_r else None, stat=stat.view)
    ctx.synchronize()
    what = f"d={d} {name}: {ctx.last_kernel()}"
    ldg_eff = ldg if d > 1 else d
    assert ctx.last_kernel() == plan(d, ldg_eff, g.sg, g.view.data_ptr(), K, S), what
    g.check_unchanged(what)
    for buf in (*[b for b in ins.values() if b is not None], *small.values()):
        buf.check_unchanged(what)
    assert int((gbuf == INT_MAX).sum()) == 16, what
    for buf in (X, stat) + ((R,) if with_r else ()):
        buf.check_outside(what)
    return X.view.cpu(), R.view.cpu() if with_r else None, stat.view.cpu(), g, R


# ---- 1. bits -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", D_SIZES)
def test_bits_of_the_mirror_in_every_layout(ctx, d):
    c = case(d)
    kinds = set()
    for lay in layouts_of(d):
        g = None
        for sname in (("warm",) if lay[-1] else ("cold", "warm")):
            X, R, stat, g, _ = launch(ctx, c, lay, c["starts"][sname], G=g)
            wX, wR, wS = (c["shared"] if lay[-1] else c["want"])[sname]
            what = (d, lay[0], sname, ctx.last_kernel())
            assert same(stat, wS), (what, stat, wS)
            assert same(X, wX), what
            assert R is None or same(R, wR), what
        kinds.add(ctx.last_kernel().split(">")[0])
    assert len(kinds) == (2 if d > 1 else 1), kinds           # both load kinds ran at this d (one row has no stride: ldg = d = 1)
    # the cases are not trivial: updates happen, nothing is refused or NaN, the warm start is brought inside its bounds, and from d = 17
    # on both bounds of a box are met, a non-negative model sits on its bound, and a one-sided coordinate holds at 0
    wX, _, wS = c["want"]["warm"]
    assert not np.isin(wS[:, 3], (2, 3)).any() and (wS[:, 1] >= 1).all() and not np.isnan(wX).any()
    assert (wX >= c["lo"]).all() and (wX <= c["hi"]).all()
    if d >= 17:
        box = wX[0::3]
        assert (box == 0.05).any() and (box == -0.05).any() and ((box != 0) & (np.abs(box) < 0.05)).any()
        assert (wX[1::3] == 0).any() and (wX[1::3] > 0).any()
        assert (c["want"]["cold"][2][:, 3] == 1).any() or d > 1000


def test_the_defaults_are_gram_cd(ctx):
    """pf, lo, hi left out, or spelled out as tensors of 1, -inf, +inf, with one set: X, R and stat of Context.gram_cd on the same
    inputs, bit for bit"""
    import torch
    for d, K in ((17, 5), (257, 4), (1025, 2)):
        c = case(d)
        G, u = c["G"][0], c["u"][1]
        with np.errstate(divide="ignore"):
            inv = np.where(np.diagonal(G) > 0, 1.0 / np.diagonal(G), 0.0)
        tau = np.abs(u).max() * (0.05 + 0.5 * (np.arange(K) + 1.0) / (K + 1.0))
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        for start in (np.zeros((K, d)), c["starts"]["warm"][:K]):
            tol, ms = 1e-9 * float(np.abs(u).max()) ** 2, 10
            Xo, Ro, So = ctx.gram_cd(dev(G), dev(u), dev(inv), dev(tau), dev(start), tol, ms)
            ctx.synchronize()
            assert ctx.last_kernel().startswith("gramcd_kernel<")
            Xn, Rn, Sn = ctx.gram_cd_general(dev(G), dev(u), dev(inv), dev(tau), dev(start), tol, ms)
            ctx.synchronize()
            assert ctx.last_kernel() == plan(d, d, 0, 0, K, 1)
            ones = lambda v: torch.full((K, d), v, dtype=torch.float64, device="cuda")
            Xs, Rs, Ss = ctx.gram_cd_general(dev(G)[None], dev(np.tile(u, (K, 1))), dev(inv), dev(tau), dev(start), torch.full((K,), tol, dtype=torch.float64, device="cuda"),
                                             ms, gsel=torch.zeros(K, dtype=torch.int32, device="cuda"), pf=ones(1.0), lo=ones(-np.inf), hi=ones(np.inf)[0].contiguous())
            ctx.synchronize()
            for o, n, s in ((Xo, Xn, Xs), (Ro, Rn, Rs), (So, Sn, Ss)):
                assert torch.equal(bits(o), bits(n)) and torch.equal(bits(o), bits(s)), d
            assert float(So[:, 1].max()) >= 1


# ---- 3. independence ---------------------------------------------------------------------------------------------------------------------------
def test_a_model_does_not_depend_on_its_neighbours(ctx):
    import torch
    c = case(257)
    K, d = c["K"], c["d"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    G = dev(c["G"])
    wX, wR, wS = c["want"]["warm"]

    def run(rows, sets=None):
        r = np.asarray(rows)
        X = dev(c["starts"]["warm"][r])
        Gr, sel = (G, c["gsel"][r]) if sets is None else sets
        _, R, st = ctx.gram_cd_general(Gr, dev(c["u"][r]), dev(c["inv"][r]), dev(c["tau"][r]), X, dev(c["tol"][r]), c["ms"], gsel=dev(sel),
                                       pf=dev(c["pf"][r]), lo=dev(c["lo"][r]), hi=dev(c["hi"][r]))
        ctx.synchronize()
        assert same(X, wX[r]) and same(R, wR[r]) and same(st, wS[r]), rows

    run(list(range(K)))
    run(list(range(K)))                                               # a second call
    for k in (0, 31, 63):                                             # alone
        run([k])
    run(np.random.default_rng(4).permutation(K).tolist())             # in another place, among other neighbours
    run([63, 5, 40, 5, 5, 17, 0, 22, 9])                              # nine models, one of them three times
    run([3, 6, 9, 30])                                                # neighbours of one kind only
    # ... and its set in another place among the sets: the matrices reversed, the set numbers with them
    run(list(range(K)), sets=(dev(c["G"][::-1]), (S - 1 - c["gsel"]).astype(np.int32)))
    # one set only, the model's own, for the models that use set 1
    r1 = np.flatnonzero(c["gsel"] == 1)
    run(r1.tolist(), sets=(dev(c["G"][1]), np.zeros(len(r1), np.int32)))


# ---- 4. states 3 and 2 -------------------------------------------------------------------------------------------------------------------------
def test_states_3_and_2_end_one_model_only(ctx):
    from ciaoalgorithms_jl_amd.host_route import host_gram_cd_general
    c = case(17)
    K, d = c["K"], c["d"]
    lay = layouts_of(d)[0]
    wX, wR, wS = c["want"]["warm"]
    warm = c["starts"]["warm"]
    victims = {"gsel low": ("gsel", 4, None, -1), "gsel high": ("gsel", 4, None, S), "pf < 0": ("pf", 7, 16, -1e-300), "pf NaN": ("pf", 7, 0, np.nan),
               "lo > 0": ("lo", 9, 3, 5e-324), "lo NaN": ("lo", 9, 16, np.nan), "hi < 0": ("hi", 12, 8, -5e-324), "hi NaN": ("hi", 12, 1, np.nan),
               "tol < 0": ("tol", 20, None, -1e-300), "tol NaN": ("tol", 20, None, np.nan), "t NaN": ("tau", 3, None, None)}
    for what, (name, k, j, value) in victims.items():
        over = {name: c[name].copy()}
        if what == "t NaN":                                 # 0 inf
            over["tau"][k] = 0.0
            assert np.isinf(c["pf"][k]).any()
        elif j is None:
            over[name][k] = value
        else:
            over[name][k, j] = value
        X, R, stat, _, _ = launch(ctx, c, lay, warm, over=over)
        mX, mR, mS = host_gram_cd_general(c["G"], c["u"], c["inv"], over.get("tau", c["tau"]), warm, over.get("tol", c["tol"]), c["ms"],
                                          gsel=over.get("gsel", c["gsel"]), pf=over.get("pf", c["pf"]), lo=over.get("lo", c["lo"]), hi=over.get("hi", c["hi"]))
        assert mS[k].tolist() == [0.0, 0.0, 0.0, 3.0] and same(stat, mS), what
        assert same(X[k], warm[k]), what                                       # its warm start, untouched
        assert bool((bits(R[k].contiguous()) == POISON64).all()), what                # its row of R: the poison survives
        others = np.delete(np.arange(K), k)
        assert same(X[others], wX[others]) and same(R[others], wR[others]) and same(stat[others], wS[others]), what
    # a NaN in one model's u: state 2 for it alone
    u = c["u"].copy()
    u[10, 5] = np.nan
    X, R, stat, _, _ = launch(ctx, c, lay, warm, over=dict(u=u))
    mX, mR, mS = host_gram_cd_general(c["G"], u, c["inv"], c["tau"], warm, c["tol"], c["ms"], gsel=c["gsel"], pf=c["pf"], lo=c["lo"], hi=c["hi"])
    assert mS[10, 3] == 2 and same(stat, mS) and same(X, mX)
    others = np.delete(np.arange(K), 10)
    assert same(R[others], wR[others]) and same(X[others], wX[others]) and np.isnan(R[10].numpy()).any()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, ciao):
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd.device import PackedF
    f64 = dict(dtype=torch.float64, device="cuda")
    d, K, ns = 8, 3, 2
    G = torch.eye(d, **f64).repeat(ns, 1, 1).contiguous()
    vec = lambda fill: torch.full((K * d + 1,), fill, **f64)
    u, inv, pf, lo, hi = vec(1.0), vec(1.0), vec(1.0), vec(-1.0), vec(1.0)
    tau, tol = torch.ones(K + 1, **f64), torch.full((K + 1,), 1e-9, **f64)
    gsel = torch.zeros(K + 1, dtype=torch.int32, device="cuda")
    X = Guarded(np.zeros((K, d)), device="cuda", name="X")
    R = Guarded(shape=(K, d), dtype=np.float64, device="cuda", name="R")
    stat = Guarded(shape=(K, 4), dtype=np.float64, device="cuda", name="stat")
    x = torch.zeros(d, **f64)
    ctx.full_gradient(PackedF.least_squares(torch.randn((9, d), **f64), torch.randn(9, **f64), 1.0), x, torch.empty_like(x))
    before = ctx.last_kernel()
    assert not before.startswith("gramcd")
    lib, h = ctx.lib, ctx._h
    p = lambda t, byte=0: C.c_void_p(t.data_ptr() + byte)

    def call(ctxh=h, d=d, K=K, G=p(G), ldg=d, sg=d * d, nsets=ns, gsel=p(gsel), u=p(u), ldu=d, inv=p(inv), ldinv=d, tau=p(tau), pf=p(pf), ldpf=d,
             lo=p(lo), ldlo=d, hi=p(hi), ldhi=d, X=p(X.view), ldx=d, tol=p(tol), ms=10, R=p(R.view), ldr=d, stat=p(stat.view)):
        status = lib.ciao_gram_cd_general(ctxh, d, K, G, ldg, sg, nsets, gsel, u, ldu, inv, ldinv, tau, pf, ldpf, lo, ldlo, hi, ldhi, X, ldx, tol, ms, R, ldr, stat)
        if status != L.OK:
            raise L.CiaoError(status, lib.ciao_last_error().decode())

    cases = [("NULL ctx", dict(ctxh=None)), ("NULL G", dict(G=None)), ("NULL u", dict(u=None)), ("NULL inv", dict(inv=None)),
             ("NULL tau", dict(tau=None)), ("NULL X", dict(X=None)), ("NULL stat", dict(stat=None)), ("NULL tol", dict(tol=None)),
             ("d = 0", dict(d=0)), ("d = 4097", dict(d=4097, ldg=4097, sg=4097 * 4097, ldx=4097, ldr=4097, ldu=0, ldinv=0, ldpf=0, ldlo=0, ldhi=0)),
             ("K = 0", dict(K=0)), ("K = 4097", dict(K=4097)),
             ("ldg < d", dict(ldg=d - 1)), ("ldx < d", dict(ldx=d - 1)), ("ldx = 0", dict(ldx=0)), ("ldr < d", dict(ldr=d - 1)), ("ldr = 0", dict(ldr=0)),
             ("ldu in (0, d)", dict(ldu=d - 1)), ("ldinv in (0, d)", dict(ldinv=1)), ("ldpf in (0, d)", dict(ldpf=d - 1)), ("ldlo in (0, d)", dict(ldlo=d - 1)),
             ("ldhi in (0, d)", dict(ldhi=d - 1)), ("ldu < 0", dict(ldu=-d)),
             ("nsets = 0", dict(nsets=0)), ("nsets < 0", dict(nsets=-1)), ("sets overlap", dict(sg=d * d - 1)), ("sg = 0", dict(sg=0)),
             ("G off 4", dict(G=p(G, 4))), ("u off 4", dict(u=p(u, 4))), ("inv off 4", dict(inv=p(inv, 4))), ("tau off 4", dict(tau=p(tau, 4))),
             ("pf off 4", dict(pf=p(pf, 4))), ("lo off 4", dict(lo=p(lo, 4))), ("hi off 4", dict(hi=p(hi, 4))), ("tol off 4", dict(tol=p(tol, 4))),
             ("gsel off 2", dict(gsel=p(gsel, 2))), ("X off 4", dict(X=p(X.view, 4))), ("R off 4", dict(R=p(R.view, 4))), ("stat off 4", dict(stat=p(stat.view, 4))),
             ("max_sweeps = 0", dict(ms=0)), ("max_sweeps = 1025", dict(ms=1025))]
    for what, kw in cases:
        with pytest.raises(L.CiaoError) as e:
            call(**kw)
        assert e.value.status == L.ERR_ARG, what
        assert len(str(e.value)) - len("libciao_hip status -1: ") > 20, (what, str(e.value))
        assert ctx.last_kernel() == before, what
    for buf in (X, R, stat):
        buf.check_unchanged("refused calls")
    # what is accepted: no R (ldr not looked at), NULL gsel / pf / lo / hi with any stride beside them, strides of 0, bases 8 bytes
    # off 16 (gsel: 4 off 8), one set with any set stride
    call(R=None, ldr=0, gsel=None, pf=None, ldpf=3, lo=None, ldlo=-1, hi=None, ldhi=1, u=p(u, 8), ldu=0, inv=p(inv, 8), ldinv=0, tau=p(tau, 8), tol=p(tol, 8))
    ctx.synchronize()
    assert ctx.last_kernel() == plan(d, d, d * d, G.data_ptr(), K, ns)
    R.check_unchanged("R = NULL")
    call(gsel=p(gsel, 4), nsets=1, sg=1)
    ctx.synchronize()
    assert ctx.last_kernel() == plan(d, d, 0, G.data_ptr(), K, 1)
    assert (stat.view[:, 3] == 1).all()
    # the Python layer refuses what it can see before the library does
    t = lambda *s: torch.zeros(s, **f64)
    gd = lambda **kw: ctx.gram_cd_general(kw.pop("G", t(d, d)), kw.pop("u", t(d)), kw.pop("inv", t(d)), kw.pop("tau", t(K)), kw.pop("X", t(K, d)), kw.pop("tol", 0.0), 1, **kw)
    for what, bad in (("X dtype", lambda: gd(X=torch.zeros((K, d), device="cuda"))), ("G shape", lambda: gd(G=t(d, d + 1))), ("G sets shape", lambda: gd(G=t(2, d + 1, d))),
                      ("u length", lambda: gd(u=t(d + 1))), ("u rows", lambda: gd(u=t(K + 1, d))), ("tau length", lambda: gd(tau=t(K + 1))),
                      ("tol length", lambda: gd(tol=t(K + 1))), ("host G", lambda: gd(G=torch.zeros((d, d), dtype=torch.float64))),
                      ("column-major G", lambda: gd(G=t(d, d).t())), ("overlapping sets", lambda: gd(G=t(d, d).expand(2, d, d))),
                      ("gsel dtype", lambda: gd(gsel=torch.zeros(K, dtype=torch.int64, device="cuda"))), ("gsel length", lambda: gd(gsel=torch.zeros(K + 1, dtype=torch.int32, device="cuda"))),
                      ("pf shape", lambda: gd(pf=t(d + 1))), ("lo dtype", lambda: gd(lo=torch.zeros(d, device="cuda"))), ("hi rows", lambda: gd(hi=t(K - 1, d))),
                      ("stat shape", lambda: gd(stat=t(K, 3))), ("no u", lambda: gd(u=None))):
        before2 = ctx.last_kernel()
        with pytest.raises(ValueError):
            bad()
        assert ctx.last_kernel() == before2, what


# ---- 6. the drivers ----------------------------------------------------------------------------------------------------------------------------
def test_lasso_cd_with_constraints_on_device_statistics(ctx):
    """lasso_cd(gram_stats(ctx, F), mus, ctx=ctx, <bounds, factors, a ridge>): converged on the general gap, on the general kernel, with
    the bits of the numpy route fed the same statistics"""
    import torch
    from test_gram_cd_general_host import six_cases
    from test_gram_cd_host import lasso_case
    from ciaoalgorithms_jl_amd import gram as GR
    from ciaoalgorithms_jl_amd.device import PackedF
    N, d = 200, 50
    A, b = lasso_case(N, d)
    F = PackedF.least_squares(torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda(), float(N))
    st = GR.gram_stats(ctx, F)
    mus = [f * GR.mu_max(st) for f in (0.5, 0.1, 0.01)]
    for name, kw in six_cases(d).items():
        if name == "plain":
            continue
        path = GR.lasso_cd(st, mus, gap=1e-9, ctx=ctx, **kw)
        assert ctx.last_kernel().startswith("gramcdg_kernel<256,vec16> ") and ctx.last_kernel().endswith(" sets=1"), name
        host = GR.lasso_cd(st.to("cpu"), mus, gap=1e-9, **kw)
        assert all(path.converged) and path.iterations == host.iterations and path.converged == host.converged, name
        for k in range(len(mus)):
            assert path.x[k].is_cuda and torch.equal(bits(path.x[k].cpu()), bits(host.x[k])), (name, k)
            cd, ch = path.certificates[k], host.certificates[k]
            assert cd.gap <= 1e-9 * max(1.0, cd.objective) and ch.gap <= 1e-9 * max(1.0, ch.objective), (name, k)
        fw = GR.lasso_path(st, mus, gap=1e-9, method="cd", ctx=ctx, **kw)
        assert all(torch.equal(bits(a), bits(w)) for a, w in zip(fw.x, path.x)), name


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_fused_cross_validation_is_the_unfused_one_bit_for_bit(ctx, dtype):
    import torch
    from test_gram_cd_host import lasso_case
    from ciaoalgorithms_jl_amd import cv as CV
    from ciaoalgorithms_jl_amd import gram as GR
    from ciaoalgorithms_jl_amd.device import PackedF
    N, d, folds = 200, 50, 5
    A, b = lasso_case(N, d)
    F = PackedF.least_squares(torch.from_numpy(A.astype(dtype)).cuda(), torch.from_numpy(b.astype(dtype)).cuda(), 1.0)
    mus = [f * GR.mu_max(GR.gram_stats(ctx, F)) for f in (0.5, 0.2, 0.05, 0.01)]
    for kw in ({}, dict(lower=0.0, ridge=0.01)):
        one = CV.lasso_cv(ctx, F, mus, folds=folds, seed=3, fused=False, **kw)
        assert ctx.last_kernel().startswith("gramcdg_kernel<" if kw else "gramcd_kernel<")
        all_ = CV.lasso_cv(ctx, F, mus, folds=folds, seed=3, fused=True, **kw)
        assert ctx.last_kernel().startswith("gramcdg_kernel<256,vec16> ") and ctx.last_kernel().endswith(f" sets={folds + 1}")
        for name in ("mse", "mean", "stderr"):
            assert torch.equal(bits(getattr(one, name).contiguous()), bits(getattr(all_, name).contiguous())), (name, kw)
        assert (one.best, one.one_se, one.floor, one.mus) == (all_.best, all_.one_se, all_.floor, all_.mus)
        assert all(one.path.converged) and one.path.converged == all_.path.converged and one.path.iterations == all_.path.iterations
        assert all(x.is_cuda and x.dtype == (torch.float64 if dtype == np.float64 else torch.float32) and torch.equal(bits(x), bits(y))
                   for x, y in zip(one.path.x, all_.path.x)), kw
        assert not torch.isnan(all_.mse).any() and all_.mse.shape == (folds, len(mus))

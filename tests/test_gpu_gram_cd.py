"""ciao_gram_cd on the device: coordinate descent for the d-space lasso, K models in one launch (csrc/gramcd_kernels.h).

  1. bits: X, R and stat equal host_route.host_gram_cd's bit for bit at every thread / load-round edge and at the LDS cap, cold and warm,
     with tol = 0 under a small sweep budget and with a realistic tol, K = 1, 2, 9, 64; in four hostile layouts (ldg = d and odd
     strides, G 8 bytes off 16-byte alignment, ldx > d, R NULL and given), every buffer Guarded, the padding of G poisoned;
  2. independence: a model alone, among 64 and in another place; a second call; a context with a stream of its own;
  3. last_kernel against the plan restated here;
  4. every refusal of include/ciao_hip.h;
  5. the drivers: gram.lasso_cd on gram_stats, confirmed by Context.certificate on the rows; the same bits as the numpy route;
     newton.logistic_newton(subproblem="cd") on DeviceRows.
"""
import ctypes as C

import numpy as np
import pytest

from layouts import Guarded, bits

pytestmark = pytest.mark.gpu

D_SIZES = [1, 3, 17, 255, 256, 257, 511, 512, 513, 1025, 4096]
K_OF = {1: 2, 3: 9, 17: 64, 255: 9, 256: 2, 257: 64, 511: 1, 512: 9, 513: 2, 1025: 9, 4096: 2}
GAP = 1e-9
U53 = 2.0 ** -53


def plan(d, ldg, g_ptr, K):
    """csrc/gramcd_kernels.h: gramcd_plan, restated -> what last_kernel must say"""
    block = 256 if d <= 1024 else 1024
    vec = g_ptr % 16 == 0 and ldg % 2 == 0
    lds = 3 * ((d + 1) // 2 * 2) * 8
    return f"gramcd_kernel<{block},{'vec16' if vec else 'elem'}> grid={K} block={block} lds={lds}"


_CASES = {}


def case(d):
    """G = A'A of N Gaussian rows with a duplicated column and a zero column, u = A'b, K weights, a sparse warm start that sits on the
    duplicated pair and on the zero column too; and the mirror's answers for the four (start, parameters) combinations.  Made once."""
    if d in _CASES:
        return _CASES[d]
    from ciaoalgorithms_jl_amd.host_route import host_gram_cd
    rng = np.random.default_rng(1000 + d)
    N, K = min(d + 3, 96), K_OF[d]
    A = rng.standard_normal((N, d))
    if d >= 3:
        A[:, 1] = A[:, 0]
    if d >= 2:
        A[:, d - 1] = 0.0
    b = A @ (rng.standard_normal(d) * (rng.random(d) < 0.1)) + 0.1 * rng.standard_normal(N)
    G, u = A.T @ A, A.T @ b
    G = np.triu(G) + np.triu(G, 1).T                     # both triangles the same bits, as ciao_gram writes them
    dg = np.diagonal(G)
    with np.errstate(divide="ignore"):
        inv = np.where(dg > 0, 1.0 / dg, 0.0)
    tau = np.abs(u).max() * (0.05 + 0.9 * (np.arange(K) + 1.0) / (K + 1.0))
    warm = rng.standard_normal((K, d)) * (rng.random((K, d)) < 0.05)
    warm[:, 0] = 0.5
    warm[:, d - 1] = -2.0
    if d >= 3:
        warm[:, 1] = 0.25
    params = {"tol0": (0.0, 3), "real": (1e-7 * float(b @ b), 40)}
    want = {}
    for sname, X0 in (("cold", np.zeros((K, d))), ("warm", warm)):
        for pname, (tol, ms) in params.items():
            want[(sname, pname)] = host_gram_cd(G, u, inv, tau, X0, tol, ms)
    _CASES[d] = dict(d=d, K=K, G=G, u=u, inv=inv, tau=tau, starts={"cold": np.zeros((K, d)), "warm": warm}, params=params, want=want)
    return _CASES[d]


def layouts_of(d):
    """(name, off of G, ldg, off of the vectors, ldx, R given, ldr)"""
    even = d + (d % 2)
    return [("packed", 0, d, 0, d, True, d),
            ("odd-stride", 0, d + 3, 1, d + 5, False, 0),
            ("off-base", 1, even, 0, d + 1, True, d + 2),
            ("even-stride", 0, even + 2, 1, d, True, d + 7)]


def same(t, a):
    import torch
    return torch.equal(bits(t.contiguous().cpu()), bits(torch.from_numpy(np.ascontiguousarray(a))))


def same_but_nan_payloads(t, a):
    """the same bits wherever the mirror holds a number, a NaN wherever it holds a NaN (which NaN an addition returns is the processor's)"""
    t, a = t.contiguous().cpu().numpy(), np.ascontiguousarray(a)
    nan = np.isnan(a)
    return np.array_equal(np.isnan(t), nan) and np.array_equal(t[~nan].view(np.int64), a[~nan].view(np.int64))


def launch(ctx, c, lay, start, tol, ms, G=None):
    """one call through Context.gram_cd with every buffer Guarded -> (X, R or None, stat) as host tensors, after the layout checks"""
    import torch
    name, goff, ldg, voff, ldx, with_r, ldr = lay
    d, K = c["d"], c["K"]
    g = G if G is not None else Guarded(c["G"], off=goff, ld=ldg, device="cuda", name="G")
    ins = [Guarded(c[n], off=voff, device="cuda", name=n) for n in ("u", "inv", "tau")]
    X = Guarded(start, off=voff, ld=ldx, device="cuda", name="X")
    R = Guarded(shape=(K, d), dtype=np.float64, off=voff, ld=ldr, device="cuda", name="R") if with_r else None
    stat = Guarded(shape=(K, 4), dtype=np.float64, device="cuda", name="stat")
    ctx.gram_cd(g.view, ins[0].view, ins[1].view, ins[2].view, X.view, tol, ms, R=R.view if with_r else None, stat=stat.view)
    ctx.synchronize()
    what = f"d={d} {name}: {ctx.last_kernel()}"
    ldg_eff = int(g.view.stride(0)) if d > 1 else d
    assert ctx.last_kernel() == plan(d, ldg_eff, g.view.data_ptr(), K), what
    for buf in (g, *ins):
        buf.check_unchanged(what)
    for buf in (X, stat) + ((R,) if with_r else ()):
        buf.check_outside(what)
    return X.view.cpu(), R.view.cpu() if with_r else None, stat.view.cpu(), g


# ---- 1. bits -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", D_SIZES)
def test_bits_of_the_mirror_in_every_layout(ctx, d):
    c = case(d)
    kinds = set()
    for lay in layouts_of(d):
        g = None
        for sname, start in c["starts"].items():
            for pname, (tol, ms) in c["params"].items():
                X, R, stat, g = launch(ctx, c, lay, start, tol, ms, G=g)
                wX, wR, wS = c["want"][(sname, pname)]
                what = (d, lay[0], sname, pname, ctx.last_kernel())
                assert same(stat, wS), (what, stat, wS)
                assert same(X, wX), what
                assert R is None or same(R, wR), what
        kinds.add(ctx.last_kernel().split(">")[0])
    assert len(kinds) == (2 if d > 1 else 1), kinds        # both load kinds ran at this d (one row has no stride: ldg = d = 1)
    # the cases are not trivial: the realistic parameters converge somewhere, the small budget runs out somewhere (d > 1), updates happen
    states = np.concatenate([c["want"][k][2][:, 3] for k in c["want"]])
    assert 1.0 in states and 2.0 not in states and (d == 1 or 0.0 in states)
    assert c["want"][("cold", "real")][2][:, 1].max() >= 1 and not np.isnan(c["want"][("warm", "real")][0]).any()
    if d >= 2:
        assert not c["want"][("warm", "real")][0][:, d - 1].any()      # the zero column: the warm value is driven to 0


def test_a_nan_ends_one_model_only(ctx):
    """u carries a NaN at one coordinate: every model ends with state 2 there, bit for bit as the mirror; with the NaN in ONE model's warm
    start only, its neighbours are untouched by it."""
    from ciaoalgorithms_jl_amd.host_route import host_gram_cd
    c = dict(case(17))
    u = c["u"].copy()
    u[5] = np.nan
    c["u"] = u
    X, R, stat, _ = launch(ctx, c, layouts_of(17)[0], c["starts"]["cold"], 0.0, 5)
    wX, wR, wS = host_gram_cd(c["G"], u, c["inv"], c["tau"], c["starts"]["cold"], 0.0, 5)
    assert (wS[:, 3] == 2).all() and same(stat, wS) and same(X, wX) and same_but_nan_payloads(R, wR) and np.isnan(wR[:, 5]).all()
    c = case(17)
    warm = c["starts"]["warm"].copy()
    warm[3, 2] = np.nan
    X, R, stat, _ = launch(ctx, c, layouts_of(17)[1], warm, 1e-12, 40)
    wX, _, wS = host_gram_cd(c["G"], c["u"], c["inv"], c["tau"], warm, 1e-12, 40)
    assert wS[3, 3] == 2 and (np.delete(wS[:, 3], 3) != 2).all() and same(stat, wS) and same_but_nan_payloads(X, wX)


# ---- 2. independence ---------------------------------------------------------------------------------------------------------------------------
def test_a_model_does_not_depend_on_its_neighbours(ciao, ctx):
    import torch
    from ciaoalgorithms_jl_amd.device import Context
    c = case(257)
    K, d = c["K"], c["d"]
    assert K == 64
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    G, u, inv, tau = dev(c["G"]), dev(c["u"]), dev(c["inv"]), dev(c["tau"])
    tol, ms = c["params"]["real"]

    def run(on, rows):
        X = dev(c["starts"]["warm"][rows])
        _, R, st = on.gram_cd(G, u, inv, tau[torch.as_tensor(rows, device="cuda")].contiguous(), X, tol, ms)
        on.synchronize()
        return X.cpu(), R.cpu(), st.cpu()

    every = list(range(K))
    X, R, st = run(ctx, every)
    wX, wR, wS = c["want"][("warm", "real")]
    assert same(X, wX) and same(R, wR) and same(st, wS)
    again = run(ctx, every)                                             # a second call
    assert all(torch.equal(bits(a), bits(w)) for a, w in zip(again, (X, R, st)))
    for k in (0, 31, 63):                                               # alone
        one = run(ctx, [k])
        assert all(torch.equal(bits(a[0]), bits(w[k])) for a, w in zip(one, (X, R, st))), k
    perm = np.random.default_rng(4).permutation(K).tolist()            # in another place, among other neighbours
    moved = run(ctx, perm)
    assert all(torch.equal(bits(a), bits(w[perm])) for a, w in zip(moved, (X, R, st)))
    few = run(ctx, [63, 5, 40, 5, 5, 17, 0, 22, 9])                     # nine models, one of them three times
    assert all(torch.equal(bits(a), bits(w[[63, 5, 40, 5, 5, 17, 0, 22, 9]])) for a, w in zip(few, (X, R, st)))
    torch.cuda.synchronize()
    own = Context(0, stream=torch.cuda.Stream())                        # a context with a stream of its own
    try:
        got = run(own, every)
        assert all(torch.equal(bits(a), bits(w)) for a, w in zip(got, (X, R, st)))
    finally:
        own.synchronize()
        own.close()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, ciao):
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    f64 = dict(dtype=torch.float64, device="cuda")
    d, K = 8, 3
    G = Guarded(np.eye(d), device="cuda", name="G")
    u, inv, tau = torch.ones(d + 1, **f64), torch.ones(d + 1, **f64), torch.ones(K + 1, **f64)
    X = Guarded(np.zeros((K, d)), device="cuda", name="X")
    R = Guarded(shape=(K, d), dtype=np.float64, device="cuda", name="R")
    stat = Guarded(shape=(K, 4), dtype=np.float64, device="cuda", name="stat")
    from ciaoalgorithms_jl_amd.device import PackedF
    x = torch.zeros(d, **f64)
    ctx.full_gradient(PackedF.least_squares(torch.randn((9, d), **f64), torch.randn(9, **f64), 1.0), x, torch.empty_like(x))
    before = ctx.last_kernel()
    assert not before.startswith("gramcd")
    lib, h = ctx.lib, ctx._h
    p = lambda t, byte=0: C.c_void_p(t.data_ptr() + byte)

    def call(ctxh=h, d=d, K=K, G=p(G.view), ldg=d, u=p(u), inv=p(inv), tau=p(tau), X=p(X.view), ldx=d, tol=1e-9, ms=10, R=p(R.view), ldr=d,
             stat=p(stat.view)):
        status = lib.ciao_gram_cd(ctxh, d, K, G, ldg, u, inv, tau, X, ldx, tol, ms, R, ldr, stat)
        if status != L.OK:
            raise L.CiaoError(status, lib.ciao_last_error().decode())

    cases = [("NULL ctx", dict(ctxh=None)), ("NULL G", dict(G=None)), ("NULL u", dict(u=None)), ("NULL inv", dict(inv=None)),
             ("NULL tau", dict(tau=None)), ("NULL X", dict(X=None)), ("NULL stat", dict(stat=None)),
             ("d = 0", dict(d=0)), ("d = 4097", dict(d=4097, ldg=4097, ldx=4097, ldr=4097)), ("K = 0", dict(K=0)), ("K = 4097", dict(K=4097)),
             ("ldg < d", dict(ldg=d - 1)), ("ldx < d", dict(ldx=d - 1)), ("ldr < d", dict(ldr=d - 1)),
             ("G off 4", dict(G=p(G.view, 4))), ("u off 4", dict(u=p(u, 4))), ("inv off 4", dict(inv=p(inv, 4))), ("tau off 4", dict(tau=p(tau, 4))),
             ("X off 4", dict(X=p(X.view, 4))), ("R off 4", dict(R=p(R.view, 4))), ("stat off 4", dict(stat=p(stat.view, 4))),
             ("tol < 0", dict(tol=-1e-300)), ("tol NaN", dict(tol=float("nan"))), ("max_sweeps = 0", dict(ms=0)), ("max_sweeps = 1025", dict(ms=1025))]
    for what, kw in cases:
        with pytest.raises(L.CiaoError) as e:
            call(**kw)
        assert e.value.status == L.ERR_ARG, what
        assert len(str(e.value)) - len("libciao_hip status -1: ") > 20, (what, str(e.value))
        assert ctx.last_kernel() == before, what
    # ldr is not looked at without R; bases 8 bytes off 16 are fine
    for buf in (X, R, stat):
        buf.check_unchanged("refused calls")
    call(R=None, ldr=0, u=p(u, 8), inv=p(inv, 8), tau=p(tau, 8))
    ctx.synchronize()
    assert ctx.last_kernel() == plan(d, d, G.view.data_ptr(), K)
    R.check_unchanged("R = NULL")
    # the Python layer refuses what it can see before the library does
    t = lambda *s: torch.zeros(s, **f64)
    for what, bad in (("X dtype", lambda: ctx.gram_cd(t(d, d), t(d), t(d), t(K), torch.zeros((K, d), device="cuda"), 0.0, 1)),
                      ("G shape", lambda: ctx.gram_cd(t(d, d + 1), t(d), t(d), t(K), t(K, d), 0.0, 1)),
                      ("u length", lambda: ctx.gram_cd(t(d, d), t(d + 1), t(d), t(K), t(K, d), 0.0, 1)),
                      ("tau length", lambda: ctx.gram_cd(t(d, d), t(d), t(d), t(K + 1), t(K, d), 0.0, 1)),
                      ("host G", lambda: ctx.gram_cd(torch.zeros((d, d), dtype=torch.float64), t(d), t(d), t(K), t(K, d), 0.0, 1)),
                      ("column-major G", lambda: ctx.gram_cd(t(d, d).t(), t(d), t(d), t(K), t(K, d), 0.0, 1)),
                      ("stat shape", lambda: ctx.gram_cd(t(d, d), t(d), t(d), t(K), t(K, d), 0.0, 1, stat=t(K, 3)))):
        before2 = ctx.last_kernel()
        with pytest.raises(ValueError):
            bad()
        assert ctx.last_kernel() == before2, what


# ---- 5. the drivers ----------------------------------------------------------------------------------------------------------------------------
def lasso_case(N, d):
    from test_gram_cd_host import lasso_case as host_case
    return host_case(N, d)


def rows_noise(A, b, x, lam, dtype):
    """What the rows' own evaluation of F = lam / (2 N) sum_i (a_i'x - b_i)^2 can differ by from the exact value: a residual formed in the
    rows' type carries (d + 2) roundings, |dr_i| <= (d + 2) eps (|a_i|'|x| + |b_i|), and F moves by at most (lam / N) sum_i |r_i| |dr_i|
    (first order); (N + 2) eps F for the sum of squares itself"""
    N, d = A.shape
    eps = float(np.finfo(dtype).eps)
    A, b, x = A.astype(np.float64), b.astype(np.float64), np.asarray(x, np.float64)
    r = A @ x - b
    dr = (d + 2) * eps * (np.abs(A) @ np.abs(x) + np.abs(b))
    return lam / N * float(np.abs(r) @ dr) + (N + 2) * eps * lam / (2 * N) * float(r @ r)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(200, 50), (300, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_lasso_cd_on_device_statistics(ctx, shape, dtype):
    """lasso_cd(gram_stats(ctx, F), mus, ctx=ctx): converged; the certificate GramLasso gives at the returned vector is confirmed by
    Context.certificate on the rows themselves -- the two gaps are the same quantity evaluated two ways, so they differ by no more than the
    two evaluations' own noise: gap_rows <= gap_gram + 4 (rows_noise + stats_noise) + value_floor (the gap is a difference of the primal
    value, the dual value and x'grad, each moved by at most the noise of F's residuals on one side and of the (N + 10) 2^-53 sum |a_i a_j|
    rounding of G, u and sum b^2 on the other; 4 covers the three) -- and, for float64 rows, meets the gap asked for.  The numpy route fed the same statistics returns the same bits."""
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd import gram as GR
    from ciaoalgorithms_jl_amd.device import PackedF, ProxG
    N, d = shape
    A, b = lasso_case(N, d)
    A, b = A.astype(dtype), b.astype(dtype)
    F = PackedF.least_squares(torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda(), float(N))
    st = GR.gram_stats(ctx, F)
    mus = [f * GR.mu_max(st) for f in (0.5, 0.1, 0.01)]
    path = GR.lasso_cd(st, mus, gap=GAP, ctx=ctx)
    assert ctx.last_kernel().startswith("gramcd_kernel<256,vec16> ")
    host = GR.lasso_cd(st.to("cpu"), mus, gap=GAP)
    q = GR.GramLasso(st)
    gamma = 1.0 / GR.smoothness_exact(st)
    assert all(path.converged) and path.iterations == host.iterations and path.converged == host.converged
    for k, mu in enumerate(mus):
        x, c = path.x[k], path.certificates[k]
        assert x.is_cuda and x.dtype == (torch.float64 if dtype == np.float64 else torch.float32) and x.is_contiguous()
        assert torch.equal(bits(x.cpu()), bits(host.x[k])), (shape, k)
        rows = ctx.certificate(F, ProxG(L.PROX_L1, lam=mu), x, gamma)
        xa = x.double().abs()
        stats_noise = (N + 10) * U53 * 0.5 * (float(xa @ (st.G.abs() @ xa)) + 2 * float(st.u.abs() @ xa) + st.sum_bb)   # G, u, sum_bb: host_gram's bound
        noise = 4 * (rows_noise(A, b, x.double().cpu().numpy(), float(N), dtype) + stats_noise) + q.value_floor(x)
        print(f"{shape} {np.dtype(dtype).name} mu {mu:.4g}: gap by GramLasso {c.gap:.3e}, by the rows {rows.gap:.3e}, objective {rows.objective:.10g}, "
              f"allowance {noise:.3e}, asked {GAP * max(1.0, c.objective):.3e}; sweeps (all models) {path.iterations}")
        assert rows.gap <= c.gap + noise
        assert abs(rows.objective - c.objective) <= noise
        if dtype == np.float64:
            assert c.gap <= GAP * max(1.0, c.objective) and rows.gap <= GAP * max(1.0, rows.objective) + noise
    # method="cd" forwards with the context; without one, device statistics are refused rather than solved somewhere else
    fw = GR.lasso_path(st, mus, gap=GAP, method="cd", ctx=ctx)
    assert all(torch.equal(bits(a), bits(w)) for a, w in zip(fw.x, path.x))
    with pytest.raises(L.CiaoError):
        GR.lasso_cd(st, mus)


@pytest.mark.parametrize("shape", [(200, 50, 5), (300, 130, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_newton_with_the_cd_subproblem_on_device_rows(ctx, shape):
    import torch
    from test_gram_weighted_host import logistic_case
    from ciaoalgorithms_jl_amd.device import PackedF
    from ciaoalgorithms_jl_amd.newton import DeviceRows, logistic_newton
    N, d, seed = shape
    A, y, mu_max = logistic_case(N, d, seed)
    F = PackedF.logistic(torch.from_numpy(A).cuda(), torch.from_numpy(y).cuda())
    rows = DeviceRows(ctx, F)
    for frac in (0.5, 0.1):
        mu = frac * mu_max
        r = logistic_newton(rows, mu, gap=GAP, subproblem="cd")
        c = r.certificate
        again = rows.certificate(r.x, mu, 1.0)               # Context.certificate(samples=True) at the returned vector
        ref = logistic_newton(rows, mu, gap=GAP)
        print(f"N={N} d={d} mu={frac} mu_max: cd outer {r.outer} gap {c.gap:.3e} objective {c.objective:.12f} {r.reason}; default outer {ref.outer} "
              f"objective {ref.certificate.objective:.12f}")
        assert r.converged and r.reason == "gap" and c.gap <= GAP * max(1.0, c.objective) and again.gap <= GAP * max(1.0, again.objective)
        assert r.x.is_cuda and r.x.dtype == torch.float64 and r.outer <= 16
        assert ref.converged and abs(c.objective - ref.certificate.objective) <= max(c.gap, ref.certificate.gap) + 1e-13 * c.objective

"""Gap-safe feature screening on the device (ciao_col_sqnorms, ciao_screen, screening.py):
  1. column sums of squares against (A.double()**2).sum(0) at every thread arrangement (rows narrower than a workgroup, one panel, several
     panels, one slab, many slabs), with |out - ref| <= (N + 2) 2^-53 ref, and exactly on small integers;
  2. the same bits for every layout of the same matrix (ld = d, ld = d + pad, a base one element off 16-byte alignment), on a second call
     and from a second Context;
  3. the rule against its numpy restatement, n_kept, and NaN / inf keeping the coordinate;
  4. safety along SVRG runs: no coordinate in the support of a CPU solution (gap <= 1e-12) is ever dropped;
  5. the reduced solve: screen, restrict, solve, expand -- and the certificate of the FULL problem closes;
  6. refusals."""
import math
import types

import numpy as np
import pytest

import problems as P

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53


def tdtype(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


def tname(dtype):
    return "f64" if dtype == np.float64 else "f32"


def bits(t):
    import torch
    return t.view(torch.int64)


def ls_problem(A):
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    return PackedF.least_squares(A, torch.zeros(A.shape[0], dtype=A.dtype, device=A.device), 1.0)


# ---- 1. column sums ------------------------------------------------------------------------------------------------------------------------
D_SIZES = (1, 2, 3, 5, 50, 63, 64, 65, 255, 256, 257, 1000, 1024, 1026, 4096, 5000)
N_SIZES = (1, 2, 17, 300, 2049)


def check_colsq(ctx, A, tag):
    N = A.shape[0]
    out = ctx.col_sqnorms(ls_problem(A))
    assert ctx.last_kernel().startswith("colsq_"), ctx.last_kernel()
    ref = (A.double() ** 2).sum(0)
    err = (out - ref).abs()
    bound = (N + 2) * U53 * ref
    worst = float((err / bound.clamp_min(1e-300)).max())
    assert bool((err <= bound).all()), (tag, worst, ctx.last_kernel())
    return out, worst


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
@pytest.mark.parametrize("d", D_SIZES)
def test_column_sums(ctx, d, dtype):
    import torch
    td = tdtype(dtype)
    gen = torch.Generator(device="cuda").manual_seed(1000 + d)
    worst = 0.0
    for N in N_SIZES:
        A = torch.randn((N, d), dtype=td, device="cuda", generator=gen)
        worst = max(worst, check_colsq(ctx, A, (N, d))[1])
        Ai = torch.randint(-8, 9, (N, d), device="cuda", generator=gen).to(td)     # every square and every sum is an integer < 2^53
        out = ctx.col_sqnorms(ls_problem(Ai))
        assert torch.equal(out, (Ai.double() ** 2).sum(0)), (N, d, ctx.last_kernel())
    print(f"d={d} {tname(dtype)}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
@pytest.mark.parametrize("N,d", [(3, 70000), (40000, 8)])
def test_column_sums_many_panels_and_many_slabs(ctx, N, d, dtype):
    import torch
    td = tdtype(dtype)
    gen = torch.Generator(device="cuda").manual_seed(N + d)
    A = torch.randn((N, d), dtype=td, device="cuda", generator=gen)
    check_colsq(ctx, A, (N, d))
    kernel = ctx.last_kernel()
    panels, slabs = (int(v) for v in kernel.split("grid=")[1].split()[0].split("x"))
    assert (panels > 1) if d == 70000 else (slabs > 1 and "tc=256" not in kernel), kernel
    Ai = torch.randint(-8, 9, (N, d), device="cuda", generator=gen).to(td)
    assert torch.equal(ctx.col_sqnorms(ls_problem(Ai)), (Ai.double() ** 2).sum(0))
    # a logistic problem takes the same pass
    from ciaoalgorithms_jl_amd.device import PackedF
    Fl = PackedF.logistic(A, torch.ones(N, dtype=td, device="cuda"))
    assert torch.equal(bits(ctx.col_sqnorms(Fl)), bits(ctx.col_sqnorms(ls_problem(A))))


# ---- 2. layout independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
@pytest.mark.parametrize("N,d", [(17, 5), (300, 257), (2049, 1024), (300, 1026), (4200, 64)])
def test_the_bits_do_not_depend_on_the_layout(ctx, N, d, dtype):
    import torch
    from ciaoalgorithms_jl_amd.device import Context
    td = tdtype(dtype)
    vec = 16 // (8 if dtype == np.float64 else 4)
    gen = torch.Generator(device="cuda").manual_seed(7 * N + d)
    A = torch.randn((N, d), dtype=td, device="cuda", generator=gen)
    first = ctx.col_sqnorms(ls_problem(A))
    kind = lambda ld: "vec16" if ld % vec == 0 else "elem"             # (torch's allocations are 16-byte aligned)
    assert kind(d) in ctx.last_kernel(), ctx.last_kernel()
    kinds = {kind(d)}
    whole = vec - d % vec                                              # the smallest pad that makes ld whole 16-byte chunks
    for pad in (whole, whole + 1, 3 * vec + 1):                         # ld = d + pad: whole chunks, and not
        wide = torch.full((N, d + pad), float("nan"), dtype=td, device="cuda")
        wide[:, :d] = A
        view = wide[:, :d]
        assert view.stride(0) == d + pad
        assert torch.equal(bits(ctx.col_sqnorms(ls_problem(view))), bits(first)), (pad, ctx.last_kernel())
        assert kind(d + pad) in ctx.last_kernel(), (pad, ctx.last_kernel())
        kinds.add(kind(d + pad))
    flat = torch.full((N * d + vec,), float("nan"), dtype=td, device="cuda")
    off = flat[1:1 + N * d].view(N, d)                                  # the base one element off 16-byte alignment
    off.copy_(A)
    assert off.data_ptr() % 16 == A.element_size()
    assert torch.equal(bits(ctx.col_sqnorms(ls_problem(off))), bits(first))
    assert "elem" in ctx.last_kernel()
    kinds.add("elem")
    assert kinds == {"vec16", "elem"}                                   # both kinds of load were compared
    assert torch.equal(bits(ctx.col_sqnorms(ls_problem(A))), bits(first))              # a second call
    other = Context(0)
    try:
        assert torch.equal(bits(other.col_sqnorms(ls_problem(A))), bits(first))        # a second context
        other.synchronize()
    finally:
        other.close()


# ---- 3. the rule ------------------------------------------------------------------------------------------------------------------------
RULE = dict(s=0.75, kappa=0.3, mu=0.9)      # |grad| ~ |N(0,1)|, colsq ~ U(0, 4): the median of the left side is about 0.9


def rule_data(d, dtype):
    rng = np.random.default_rng(31 * d + (1 if dtype == np.float64 else 0))
    return rng.standard_normal(d).astype(dtype), 4.0 * rng.random(d)


def rule_lhs(grad, colsq):
    return RULE["s"] * np.abs(grad.astype(np.float64)) + RULE["kappa"] * np.sqrt(colsq)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
@pytest.mark.parametrize("d", [1, 7, 1024, 1025, 70000])
def test_the_rule_against_its_restatement(ctx, ciao, d, dtype):
    import torch
    from ciaoalgorithms_jl_amd.screening import host_screen
    grad, colsq = rule_data(d, dtype)
    mu = RULE["mu"]
    near = np.abs(rule_lhs(grad, colsq) - mu) <= 4 * 2.0 ** -52 * mu
    assert not near.any(), "choose another seed: a left side within rounding of mu"     # (so at most 1 % excluded holds with 0 excluded)
    want = host_screen(grad, colsq, **RULE)
    keep, n_kept = ctx.screen(torch.from_numpy(grad).cuda(), torch.from_numpy(colsq).cuda(), **RULE)
    assert ctx.last_kernel().startswith("colsq_screen_kernel"), ctx.last_kernel()
    assert keep.dtype == torch.uint8 and keep.shape == (d,)
    got = keep.cpu().numpy()
    assert set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got.astype(bool), want)
    assert n_kept == int(got.sum()) == int(want.sum())
    if d >= 1024:
        assert 0.3 * d < n_kept < 0.7 * d
    # NaN or inf, in grad or in colsq, keeps the coordinate whatever the rest says
    for where, value in (("grad", np.nan), ("grad", np.inf), ("grad", -np.inf), ("colsq", np.nan), ("colsq", np.inf), ("colsq", -1.0)):
        g2, c2 = grad.copy(), colsq.copy()
        j = (3 * d) // 4
        g2[j], c2[j] = 0.0, 0.0                                       # a coordinate the rule would drop
        assert not host_screen(g2, c2, **RULE)[j]
        (g2 if where == "grad" else c2)[j] = value
        keep2, n2 = ctx.screen(torch.from_numpy(g2).cuda(), torch.from_numpy(c2).cuda(), **RULE)
        got2 = keep2.cpu().numpy().astype(bool)
        assert got2[j], (where, value)
        assert np.array_equal(got2, host_screen(g2, c2, **RULE)) and n2 == int(got2.sum())
    # kappa = +inf keeps everything, also where inf * 0 is NaN
    keep3, n3 = ctx.screen(torch.zeros(d, dtype=tdtype(dtype), device="cuda"), torch.zeros(d, dtype=torch.float64, device="cuda"), 1.0, math.inf, mu)
    assert n3 == d and bool(keep3.all())


# ---- the CPU side of 4 and 5: value, gradient, certificate and a solution to gap <= 1e-12, in float64 -----------------------------------
def value_grad(loss, A, b, lam, x):
    N = A.shape[0]
    z = A @ x
    if loss == "ls":
        r = z - b
        return 0.5 * lam * float(r @ r) / N, lam * (A.T @ r) / N, z
    t = b * z
    e = np.exp(-np.abs(t))
    return (float(np.sum(np.maximum(-t, 0.0) + np.log1p(e))) / N, A.T @ (-b * np.where(t >= 0, e / (1.0 + e), 1.0 / (1.0 + e))) / N, z)


def cpu_certificate(loss, A, b, lam, mu, x):
    from ciaoalgorithms_jl_amd.certificate import assemble
    from ciaoalgorithms_jl_amd.host_route import host_margin_stats
    F, grad, z = value_grad(loss, A, b, lam, x)
    grad_inf = float(np.max(np.abs(grad)))
    if loss == "ls":
        return assemble(F, mu * float(np.abs(x).sum()), 0.0, grad_inf, float(x @ grad), 0.0, mu=mu), grad
    s = 1.0 if grad_inf == 0 else min(1.0, mu / grad_inf)
    return assemble(F, mu * float(np.abs(x).sum()), 0.0, grad_inf, float(x @ grad), 0.0, mu=mu,
                    entropy=host_margin_stats("logistic", z, b, s)[1], n=A.shape[0]), grad


def cpu_solution(loss, A, b, lam, mu, x):
    """Proximal-gradient steps from x until the duality gap is <= 1e-12 (float64)."""
    gamma = A.shape[0] / (np.linalg.norm(A, 2) ** 2 * (lam if loss == "ls" else 0.25))
    for k in range(400000):
        if k % 200 == 0 and cpu_certificate(loss, A, b, lam, mu, x)[0].gap <= 1e-12:
            return x
        w = x - gamma * value_grad(loss, A, b, lam, x)[1]
        x = np.sign(w) * np.maximum(np.abs(w) - gamma * mu, 0.0)
    raise AssertionError("the CPU solution did not reach gap <= 1e-12")


_CASES = {}


def case(name):
    """(loss, A, b, lam, mu, x0, step, support of the CPU solution): computed once, shared, never modified."""
    if name not in _CASES:
        if name == "lasso":
            A, b, Lc, mu, x0, x_star, _ = P.lasso_known_answer(dtype=np.float64)
            loss, lam = "ls", float(A.shape[0])
            start = np.asarray(x_star, np.float64)
        elif name == "logistic":
            A, b, Lc, mu, x0, x_star = P.logistic_fixture(np.float64)
            loss, lam, start = "logistic", 1.0, x_star
        else:
            A, b, _ = P.synthetic("ls", 200, 1000, np.float64, seed=5)
            loss, lam, x0, start = "ls", 1.0, np.zeros(1000), np.zeros(1000)
            Lc = np.sum(A * A, axis=1)
            mu = 0.5 * float(np.max(np.abs(value_grad(loss, A, b, lam, x0)[1])))
        x_cpu = cpu_solution(loss, A, b, lam, float(mu), start.copy())
        for v in (A, b, x0, x_cpu):
            v.setflags(write=False)
        _CASES[name] = (loss, A, b, lam, float(mu), x0, float(1 / (7 * np.max(Lc))), x_cpu != 0)
    return _CASES[name]


def device_case(name, dtype):
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd.device import PackedF, ProxG
    loss, A, b, lam, mu, x0, gamma, support = case(name)
    At, bt = torch.from_numpy(A.astype(dtype)).cuda(), torch.from_numpy(b.astype(dtype)).cuda()
    F = PackedF.least_squares(At, bt, lam) if loss == "ls" else PackedF.logistic(At, bt)
    return F, ProxG(L.PROX_L1, lam=mu), x0.astype(dtype), gamma, support


CHECKPOINTS = {"lasso": (1, 5, 20, 100, 400), "logistic": (1, 10, 50, 200, 1000), "gaussian": (1, 5, 20, 100, 400)}


# ---- 4. safety on the device ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
@pytest.mark.parametrize("name", ["lasso", "logistic", "gaussian"])
def test_no_support_coordinate_is_dropped_along_an_svrg_run(ctx, ciao, name, dtype):
    import ciaoalgorithms_jl_amd.solvers as S
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd.screening import gap_safe, host_screen, mu_max
    F, g, x0, gamma, support = device_case(name, dtype)
    colsq = ctx.col_sqnorms(F)
    if name == "gaussian":
        assert abs(mu_max(ctx, F) - 2 * g.lam) <= 1e-5 * g.lam
    res = None
    for k, st in zip(range(CHECKPOINTS[name][-1]), S.iterator(S.SVRG(dtype, γ=gamma), x0, F=F, g=g, N=F.N, ctx=ctx)):
        if k + 1 not in CHECKPOINTS[name]:
            continue
        x = S.solution(st).clone()
        res = gap_safe(ctx, F, g, x, gamma, colsq=colsq)
        keep = res.keep.cpu().numpy().astype(bool)
        print(f"{name} {tname(dtype)} epoch {k + 1}: gap {res.certificate.gap:.3e} s {res.s:.6f} kappa {res.kappa:.3e} kept {res.n_kept} of {res.d}")
        assert res.d == F.d and res.n_kept == int(keep.sum())
        assert not (support & ~keep).any(), (name, k + 1, np.nonzero(support & ~keep)[0])
        # s and kappa are the section 8.8 formulas on the certificate of THIS problem (its lam, N, mu and the eps of its type)
        c = res.certificate
        G = max(c.gap, 0.0) + 64.0 * float(np.finfo(dtype).eps) * c.objective
        assert res.s == min(1.0, g.lam / c.grad_inf)
        assert res.kappa == (math.sqrt(2.0 * F.lam * G / F.N) if name != "logistic" else math.sqrt(G / (2.0 * F.N)))
    if name == "gaussian":
        # the count is the restatement's at the same x, from the device's own gradient and column sums
        import torch
        grad = torch.empty_like(x)
        ctx.full_gradient(F, x, grad)
        want = host_screen(grad.cpu().numpy(), colsq.cpu().numpy(), res.s, res.kappa, g.lam)
        assert res.n_kept == int(want.sum())
        # without a cached colsq the call makes the column pass itself: the same mask
        again = gap_safe(ctx, F, g, x, gamma)
        assert torch.equal(again.keep, res.keep) and again.n_kept == res.n_kept


# ---- 5. the reduced solve -----------------------------------------------------------------------------------------------------------------
def test_reduced_solve(ctx, ciao):
    import torch
    import ciaoalgorithms_jl_amd.solvers as S
    from ciaoalgorithms_jl_amd.certificate import Certificate, stop_when
    from ciaoalgorithms_jl_amd.screening import expand, gap_safe, restrict
    F, g, x0, gamma, support = device_case("gaussian", np.float64)
    # restrict by all ones is the full problem: bitwise its full gradient
    xr = torch.randn(F.d, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    full, same = torch.empty_like(xr), torch.empty_like(xr)
    ctx.full_gradient(F, xr, full)
    Fall = restrict(F, torch.ones(F.d, dtype=torch.uint8, device="cuda"))
    assert (Fall.N, Fall.d, Fall.N_total, Fall.lam) == (F.N, F.d, F.N_total, F.lam) and Fall.b is F.b
    ctx.full_gradient(Fall, xr, same)
    assert torch.equal(bits(same), bits(full))
    # screen at a checkpoint with gap < 1e-3
    stop = stop_when(Certificate(ctx, F, g, F.N, gamma), gap=1e-3)
    x, it = S.SVRG(np.float64, maxit=1000, γ=gamma)(x0, F=F, g=g, N=F.N, ctx=ctx, stop=stop, check_every=5)
    assert stop.last.gap < 1e-3, (it, stop.last.gap)
    xd = torch.from_numpy(np.asarray(x)).cuda() if not isinstance(x, torch.Tensor) else x
    res = gap_safe(ctx, F, g, xd, gamma)
    keep = res.keep.cpu().numpy().astype(bool)
    assert not (support & ~keep).any() and 0 < res.n_kept < F.d
    Fr = restrict(F, res.keep)
    assert (Fr.N, Fr.d) == (F.N, res.n_kept) and Fr.N_total == F.N_total and Fr.lam == F.lam
    assert torch.equal(Fr.A, F.A[:, torch.from_numpy(keep).cuda()])
    # solve the reduced problem to gap 1e-8, expand, certify on the FULL problem
    stop_r = stop_when(Certificate(ctx, Fr, g, Fr.N, gamma), gap=1e-8)
    x_red, it_r = S.SVRG(np.float64, maxit=4000, γ=gamma)(xd[res.keep.bool()].contiguous(), F=Fr, g=g, N=Fr.N, ctx=ctx, stop=stop_r, check_every=10)
    assert stop_r.last.gap <= 1e-8, (it_r, stop_r.last.gap)
    x_full = expand(x_red if isinstance(x_red, torch.Tensor) else torch.from_numpy(np.asarray(x_red)).cuda(), res.keep)
    assert x_full.shape == (F.d,) and not bool(x_full[~res.keep.bool()].any())
    c = ctx.certificate(F, g, x_full, gamma)
    print(f"screened at gap {stop.last.gap:.3e} after {it} epochs: kept {res.n_kept} of {F.d}; reduced solve {it_r} epochs to gap "
          f"{stop_r.last.gap:.3e}; gap on the full problem {c.gap:.3e}")
    assert 0 <= c.gap <= 1e-6


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, ciao):
    import ctypes as C
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd import operators as ops
    from ciaoalgorithms_jl_amd.device import Context, PackedF, PackedSepQuad, ProxG
    from ciaoalgorithms_jl_amd.screening import gap_safe, mu_max, restrict
    f64 = dict(dtype=torch.float64, device="cuda")
    A = torch.randn((9, 8), **f64)
    F = PackedF.least_squares(A, torch.randn(9, **f64), 1.0)
    Fc = PackedF.least_squares_complex(torch.randn((4, 8), **f64), torch.randn(8, **f64), 4.0)
    Fz = PackedF.zero(4, 8, torch.float64)
    F0 = PackedF.logistic(torch.empty((0, 8), **f64), torch.empty(0, **f64), N_total=4)     # a rank that holds no row
    Fs = PackedSepQuad(torch.ones((3, 4), **f64), torch.ones((3, 4), **f64))
    Fshard = PackedF.least_squares(A, torch.randn(9, **f64), 1.0, N_total=18)
    x, out8, keep8 = torch.zeros(8, **f64), torch.zeros(8, **f64), torch.zeros(8, dtype=torch.uint8, device="cuda")
    g = ProxG(L.PROX_L1, lam=0.25)
    ctx.full_gradient(F, x, torch.empty_like(x))
    before = ctx.last_kernel()
    assert not before.startswith("colsq_")
    lib, h, n = ctx.lib, ctx._h, C.c_int64(0)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def raw(status):
        if status != L.OK:
            raise L.CiaoError(status, lib.ciao_last_error().decode())

    def screen(s=0.5, kappa=0.1, mu=0.5, d=8, grad=out8, colsq=out8, keep=keep8, cnt=n, dtype=L.F64):
        raw(lib.ciao_screen(h, dtype, d, ptr(grad) if grad is not None else None, ptr(colsq) if colsq is not None else None, s, kappa, mu,
                            ptr(keep) if keep is not None else None, C.byref(cnt) if cnt is not None else None))

    # the three kinds of row-sharded context, each a context of its own: an all-reduce hook, a shard table (two shards of F's rows, as
    # the sharded chains take them), peer mailboxes (a world of one over this context's own mailbox: no second process needed)
    hooked, sharded, peered = Context(0), Context(0), Context(0)
    for c in (hooked, sharded, peered):
        c.full_gradient(F, x, torch.empty_like(x))            # (so that each has a last kernel to keep)
        c.synchronize()
    hooked.set_allreduce(lambda buf, count, dtype, stream: 0)
    table = L.ShardTable()
    table.nshards, table.owner = 2, 1
    for k, r0 in enumerate((0, 4)):
        table.row0[k], table.A[k], table.b[k], table.table[k] = r0, F.A[r0:].data_ptr(), F.b[r0:].data_ptr(), None
    table.row0[2] = F.N
    sharded.set_shards(table)
    box = C.c_void_p()
    L.check(lib.ciao_peer_mailbox_create(peered._h, 16, C.byref(box), None))
    peered.set_peers(types.SimpleNamespace(rank=0, world=1, mailboxes=[box.value], max_elems=16))
    others = {"gap_safe hook": hooked, "gap_safe shard table": sharded, "gap_safe peers": peered}
    for c in others.values():
        assert c.is_row_sharded() and c.last_kernel() == before
    assert not ctx.is_row_sharded()
    before_other = {k: c.last_kernel() for k, c in others.items()}
    try:
        cases = [("complex col_sqnorms", lambda: ctx.col_sqnorms(Fc)), ("Zero col_sqnorms", lambda: ctx.col_sqnorms(Fz)),
                 ("sharing col_sqnorms", lambda: ctx.col_sqnorms(Fs)), ("N = 0 col_sqnorms", lambda: ctx.col_sqnorms(F0)),
                 ("NULL problem", lambda: raw(lib.ciao_col_sqnorms(h, None, ptr(out8)))),
                 ("NULL out", lambda: raw(lib.ciao_col_sqnorms(h, F.ref, None))),
                 ("NULL ctx", lambda: raw(lib.ciao_col_sqnorms(None, F.ref, ptr(out8)))),
                 ("s < 0", lambda: screen(s=-0.125)), ("s > 1", lambda: screen(s=1.5)), ("s = nan", lambda: screen(s=math.nan)),
                 ("kappa < 0", lambda: screen(kappa=-1e-300)), ("kappa = nan", lambda: screen(kappa=math.nan)),
                 ("mu = 0", lambda: screen(mu=0.0)), ("mu < 0", lambda: screen(mu=-1.0)), ("mu = inf", lambda: screen(mu=math.inf)),
                 ("mu = nan", lambda: screen(mu=math.nan)), ("d = 0", lambda: screen(d=0)), ("d < 0", lambda: screen(d=-3)),
                 ("dtype", lambda: screen(dtype=7)),
                 ("NULL grad", lambda: screen(grad=None)), ("NULL colsq", lambda: screen(colsq=None)), ("NULL keep", lambda: screen(keep=None)),
                 ("NULL n_kept", lambda: screen(cnt=None)), ("NULL ctx screen", lambda: raw(lib.ciao_screen(None, L.F64, 8, ptr(out8), ptr(out8), 0.5, 0.1, 0.5, ptr(keep8), C.byref(n)))),
                 ("python s", lambda: ctx.screen(out8, out8, 2.0, 0.1, 0.5)),
                 ("gap_safe Zero g", lambda: gap_safe(ctx, F, ProxG(), x, 0.5)), ("gap_safe mu = 0", lambda: gap_safe(ctx, F, ProxG(L.PROX_L1, lam=0.0), x, 0.5)),
                 ("gap_safe box", lambda: gap_safe(ctx, F, ProxG(L.PROX_BOX, lo=-1.0, hi=1.0), x, 0.5)),
                 ("gap_safe operators box", lambda: gap_safe(ctx, F, ops.IndBox(-1.0, 1.0), x, 0.5)),
                 ("gap_safe complex", lambda: gap_safe(ctx, Fc, g, x, 0.5)), ("gap_safe Zero F", lambda: gap_safe(ctx, Fz, g, x, 0.5)),
                 ("gap_safe sharing", lambda: gap_safe(ctx, Fs, g, x, 0.5)), ("gap_safe hook", lambda: gap_safe(hooked, F, g, x, 0.5)),
                 ("gap_safe shard table", lambda: gap_safe(sharded, F, g, x, 0.5)), ("gap_safe peers", lambda: gap_safe(peered, F, g, x, 0.5)),
                 ("gap_safe row shard", lambda: gap_safe(ctx, Fshard, g, x, 0.5)),
                 ("mu_max sharing", lambda: mu_max(ctx, Fs)), ("restrict sharing", lambda: restrict(Fs, keep8))]
        for what, call in cases:
            with pytest.raises(L.CiaoError) as e:
                call()
            assert e.value.status == L.ERR_ARG, what
            assert len(str(e.value)) - len("libciao_hip status -1: ") > 30, (what, str(e.value))
            assert ctx.last_kernel() == before, what
            if what in others:
                assert "row-sharded" in str(e.value) and others[what].last_kernel() == before_other[what], what
        assert "row-sharded" in str(e.value) or "restrict" in str(e.value)
        # kappa = +inf is allowed
        screen(kappa=math.inf)
        assert n.value == 8 and bool(keep8.all())
        with pytest.raises(ValueError):
            restrict(F, torch.zeros(8, dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError):
            ctx.col_sqnorms(F, out=torch.zeros(8, dtype=torch.float32, device="cuda"))
        # with the table, the hook and the peers taken off again the same contexts screen
        sharded.set_shards(None)
        hooked.set_allreduce(None)
        peered.set_peers(None)
        for c in others.values():
            assert not c.is_row_sharded()
            assert gap_safe(c, F, g, x, 0.5).d == 8 and c.last_kernel().startswith("colsq_screen_kernel")
    finally:
        peered.set_peers(None)
        sharded.set_shards(None)
        for c in others.values():
            c.synchronize()
        lib.ciao_peer_mailbox_destroy(peered._h, box)
        for c in others.values():
            c.close()
    ctx.synchronize()

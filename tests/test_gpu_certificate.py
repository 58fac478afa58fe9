"""ciao_certificate on the device: the d-vector reduction against a float64 restatement written HERE (not imported from the package),
with bounds derived from the arithmetic; determinism; the caller's av against the call's own; the lasso duality gap as a bound on
objective(x) - min along an SVRG run on the known-answer fixture; solve to tolerance through the existing stop= keyword; refusals.

Parameters of the restatement cases are exactly representable in float32 (gamma = 3/8, lambda = 5/16, bounds in quarters): kernel and
restatement then see the same parameters, and the bounds below count arithmetic, not the conversion of a parameter to T."""
import math
import os

import numpy as np
import pytest

import problems as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS64 = float(np.finfo(np.float64).eps)
N_ROWS = 64
GAMMA, LAM = 0.375, 0.3125
# csrc/cert_kernels.h: 256 threads, slices of 1024 coordinates up to 512 of them, whole multiples of 1024 beyond
SLICE, FINAL_THREADS, GRID_CAP = 1024, 256, 512
SHAPES = [1, 3, 63, 64, 65, SLICE - 1, SLICE, SLICE + 1, 3 * SLICE + 5,
          FINAL_THREADS * SLICE + 1,      # 257 partial records: more than cert_final_kernel has threads
          GRID_CAP * SLICE + 1]           # beyond the grid cap: the slices grow to 2048
PROXES = ["zero", "l1", "box", "boxvec"]


def bits(res):
    return np.array(tuple(res), dtype=np.float64).view(np.uint64).tolist()


_cache = {}


def problem(loss, dtype, d):
    """(PackedF, x) on the device, shared between the cases of one (loss, dtype, d)."""
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    key = (loss, np.dtype(dtype).name, d)
    if key not in _cache:
        if len(_cache) >= 2:
            _cache.clear()
        td = torch.float64 if dtype == np.float64 else torch.float32
        gen = torch.Generator(device="cuda").manual_seed(1000 + d)
        A = torch.randn((N_ROWS, d), dtype=td, device="cuda", generator=gen) / math.sqrt(d)
        t = torch.randn(N_ROWS, dtype=td, device="cuda", generator=gen)
        x = 0.6 * torch.randn(d, dtype=td, device="cuda", generator=gen)
        if loss == "ls":
            F = PackedF.least_squares(A, t, float(N_ROWS))
        else:
            F = PackedF.logistic(A, torch.where(t >= 0, 1.0, -1.0).to(td))
        _cache[key] = (F, x)
    return _cache[key]


def make_g(kind, dtype, d):
    """(ProxG, lo, hi as float64 numpy or None)"""
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd.device import ProxG
    if kind == "zero":
        return ProxG(L.PROX_ZERO), None, None
    if kind == "l1":
        return ProxG(L.PROX_L1, lam=LAM), None, None
    if kind == "box":
        return ProxG(L.PROX_BOX, lo=-0.25, hi=0.5), np.full(d, -0.25), np.full(d, 0.5)
    k = np.arange(d)
    lo, hi = -0.25 * (1 + k % 3), 0.25 * (1 + k % 5)
    td = torch.float64 if dtype == np.float64 else torch.float32
    return (ProxG(L.PROX_BOX, lo_vec=torch.from_numpy(lo).to("cuda", td), hi_vec=torch.from_numpy(hi).to("cuda", td)), lo, hi)


def restate(x, av, gamma, kind, lam, lo, hi):
    """The five definitions in float64 numpy from the T-typed x and av (exact sums: math.fsum).  g's terms are formed in T, as
    prox_value_elem forms them (one IEEE multiplication: the same value here and there)."""
    T = x.dtype.type
    x64, a64 = x.astype(np.float64), av.astype(np.float64)
    v = x64 - gamma * a64
    if kind == "l1":
        y = np.sign(v) * np.maximum(np.abs(v) - gamma * lam, 0.0)
    elif kind in ("box", "boxvec"):
        y = np.clip(v, lo, hi)
    else:
        y = v
    s0 = math.fsum(((x64 - y) ** 2).tolist())
    s1 = math.fsum((x64 * a64).tolist())
    s2 = math.fsum((T(lam) * np.abs(x)).astype(np.float64).tolist()) if kind == "l1" else 0.0
    m = float(np.max(np.abs(a64)))
    viol = float(max(np.max(lo - x64), np.max(x64 - hi), 0.0)) if lo is not None else 0.0
    return {"residual": math.sqrt(s0) / gamma, "x_dot_grad": s1, "g": s2, "grad_inf": m, "box_violation": viol,
            "abs_dot": math.fsum(np.abs(x64 * a64).tolist()),
            "res_scale": math.sqrt(math.fsum(((np.abs(x64) + gamma * np.abs(a64)) ** 2).tolist())) / gamma}


def check_against_restatement(c, x, av, kind, lo, hi, dtype):
    """grad_inf, box_violation: exact (maxima of T values; the violation a double subtraction of T values on both sides).
    g: d eps64 relative.  x_dot_grad: (d + 1) eps64 sum |x_k av_k|.  residual: per coordinate 2 eps_T (|x_k| + gamma |av_k|) -- the
    product, the subtraction, the prox's own addition and x - y, half an eps_T each of at most |x_k| + gamma |av_k| -- so
    |d residual| <= 2 eps_T || |x| + gamma |av| ||_2 / gamma + d eps64 residual."""
    d, epsT = x.size, float(np.finfo(dtype).eps)
    r = restate(x, av, GAMMA, kind, LAM, lo, hi)
    err = {"grad_inf": abs(c.grad_inf - r["grad_inf"]), "box_violation": abs(c.box_violation - r["box_violation"]),
           "g": abs((c.g if math.isfinite(c.g) else r["g"]) - r["g"]), "x_dot_grad": abs(c.x_dot_grad - r["x_dot_grad"]),
           "residual": abs(c.residual - r["residual"])}
    bound = {"grad_inf": 0.0, "box_violation": 0.0, "g": d * EPS64 * abs(r["g"]), "x_dot_grad": (d + 1) * EPS64 * r["abs_dot"],
             "residual": 2 * epsT * r["res_scale"] + d * EPS64 * r["residual"]}
    print(f"d={d} {np.dtype(dtype).name} {kind}: " + "  ".join(f"{k} err {err[k]:.3e} <= {bound[k]:.3e}" for k in err))
    for k in err:
        assert err[k] <= bound[k], (k, err[k], bound[k], getattr(c, k), r[k])
    # g(x) = +inf exactly when x leaves the box; objective and F stay consistent
    assert (c.g == math.inf) == (r["box_violation"] > 0)
    assert c.objective == c.F + c.g
    return r


@pytest.mark.parametrize("kind", PROXES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
@pytest.mark.parametrize("d", SHAPES)
def test_against_a_restatement(ctx, d, loss, dtype, kind):
    import torch
    from ciaoalgorithms_jl_amd.device import ProxG
    F, x = problem(loss, dtype, d)
    g, lo, hi = make_g(kind, dtype, d)
    av = torch.empty_like(x)
    ctx.full_gradient(F, x, av)                     # the device's own av, downloaded
    c = ctx.certificate(F, g, x, GAMMA)
    assert ctx.last_kernel().startswith("cert_partial_kernel")
    check_against_restatement(c, x.cpu().numpy(), av.cpu().numpy(), kind, lo, hi, dtype)
    # F: bitwise what ciao_objective returns for the same x without its g part
    assert bits([c.F]) == bits([ctx.objective(F, ProxG(), x)])
    if kind == "l1" and loss == "ls":
        s = 1.0 if c.grad_inf == 0 else min(1.0, LAM / c.grad_inf)
        assert c.gap == c.F + c.g - (c.F * (2 * s - s * s) - s * c.x_dot_grad) and c.gap >= 0
    else:
        assert math.isnan(c.gap)


@pytest.mark.parametrize("kind", PROXES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("d", [3, 65, SLICE + 1, 3 * SLICE + 5])
def test_misaligned_x_view(ctx, d, dtype, kind):
    """A contiguous view one element into a buffer is not 16-byte aligned: the element-load path.  Against the restatement, and
    bitwise the aligned vector's result on the same av (which thread adds what does not depend on the alignment)."""
    import torch
    F, x = problem("ls", dtype, d)
    g, lo, hi = make_g(kind, dtype, d)
    big = torch.empty(d + 1, dtype=x.dtype, device="cuda")
    xm = big[1:]
    xm.copy_(x)
    assert xm.data_ptr() % 16 != 0 and xm.is_contiguous()
    c = ctx.certificate(F, g, xm, GAMMA)
    av = torch.empty_like(x)
    ctx.full_gradient(F, xm, av)
    check_against_restatement(c, x.cpu().numpy(), av.cpu().numpy(), kind, lo, hi, dtype)
    f = ctx.objective(F, g, x)
    assert bits(ctx.certificate(F, g, xm, GAMMA, av=av, fval=f)) == bits(ctx.certificate(F, g, x, GAMMA, av=av, fval=f))
    avm = torch.empty(d + 1, dtype=x.dtype, device="cuda")[1:]
    avm.copy_(av)
    assert bits(ctx.certificate(F, g, x, GAMMA, av=avm, fval=f)) == bits(ctx.certificate(F, g, x, GAMMA, av=av, fval=f))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("d", [65, 3 * SLICE + 5, FINAL_THREADS * SLICE + 1])
def test_determinism(ctx, d, dtype):
    """Two calls, and a call on a second context, give bitwise-equal outputs: the grid and every summation order are functions of d."""
    from ciaoalgorithms_jl_amd.device import Context
    F, x = problem("ls", dtype, d)
    g, _, _ = make_g("l1", dtype, d)
    a, b = ctx.certificate(F, g, x, GAMMA), ctx.certificate(F, g, x, GAMMA)
    other = Context(0)
    try:
        c = other.certificate(F, g, x, GAMMA)
    finally:
        other.close()
    assert bits(a) == bits(b) == bits(c)


@pytest.mark.parametrize("kind", PROXES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("loss,d", [("ls", 65), ("logistic", SLICE + 1), ("ls", GRID_CAP * SLICE + 1)])
def test_av_given_equals_av_none(ctx, loss, d, dtype, kind):
    import torch
    from ciaoalgorithms_jl_amd.device import ProxG
    F, x = problem(loss, dtype, d)
    g, _, _ = make_g(kind, dtype, d)
    own = ctx.certificate(F, g, x, GAMMA)
    av = torch.empty_like(x)
    ctx.full_gradient(F, x, av)
    given = ctx.certificate(F, g, x, GAMMA, av=av, fval=ctx.objective(F, ProxG(), x))
    assert bits(own) == bits(given)
    blind = ctx.certificate(F, g, x, GAMMA, av=av)          # F unknown: nan, and with it objective and gap
    assert math.isnan(blind.F) and math.isnan(blind.objective) and math.isnan(blind.gap)
    assert bits(blind[3:7]) == bits(own[3:7])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_two_million_coordinates(ctx, dtype):
    """d = 2 M (the longest row the sweeps serve at speed): 512 slices of 4096.  The reduction alone -- a problem of Zero() terms carries
    no data, the caller's av stands for grad f(x) -- against the restatement."""
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    d = 1 << 21
    td = torch.float64 if dtype == np.float64 else torch.float32
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = 0.6 * torch.randn(d, dtype=td, device="cuda", generator=gen)
    av = torch.randn(d, dtype=td, device="cuda", generator=gen)
    F = PackedF.zero(N_ROWS, d, td)
    g, lo, hi = make_g("l1", dtype, d)
    c = ctx.certificate(F, g, x, GAMMA, av=av, fval=0.0)
    assert ctx.last_kernel() == f"cert_partial_kernel<{'f64' if dtype == np.float64 else 'f32'}> grid=512 block=256"
    check_against_restatement(c, x.cpu().numpy(), av.cpu().numpy(), "l1", lo, hi, dtype)
    assert c.F == 0.0 and math.isnan(c.gap)


# ---- the lasso known-answer fixture ---------------------------------------------------------------------------------------------------
def lasso_fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "lasso_known_answer_f64.npz"))
    A, b, L, lam, x0, x_star, f_star = P.lasso_known_answer(dtype=np.float64)
    assert np.array_equal(A, z["A"]) and np.array_equal(b, z["b"]) and float(z["lam_g"]) == lam     # the fixture IS the generator's problem
    return A, b, L, lam, x0, x_star, f_star


def gap_margin(A, c, x):
    """m = 3 |dF| + |d(x . grad f)| + |dg| + |ds| |dD/ds|: the bounds of the restatement test through gap = F + g - F (2s - s^2) + s x.grad f.
    |dF|: 1e-9 max(1, |F|), the scale of the objective parity test (tests/test_gpu_parity.py).  grad f itself: 81 eps64 ||grad f||_inf,
    the fp64 scale of the full-gradient parity test; it enters x . grad f through ||x||_1 and s = mu / ||grad f||_inf relatively."""
    d = x.size
    dF = 1e-9 * max(1.0, abs(c.F))
    dav = 81 * EPS64 * c.grad_inf
    dxg = float(np.abs(x).sum()) * dav + (d + 1) * EPS64 * float(np.abs(x).sum()) * c.grad_inf
    dg = d * EPS64 * abs(c.g)
    ds = 81 * EPS64
    return 3 * dF + dxg + dg + ds * (2 * abs(c.F) + abs(c.x_dot_grad))


def test_the_gap_is_a_bound(ctx, ciao, tmp_path):
    """gap >= objective(x) - objective(x*) - m at x0 = 0 and along an SVRG run; at x* the gap is within m of 0.  The observed slack
    (gap - suboptimality, and m) is written to the file CIAO_CERT_SLACK_OUT names, or to pytest's temporary directory (profiles/cert_gap_slack.txt is one such run)."""
    import torch
    import ciaoalgorithms_jl_amd.operators as ops
    import ciaoalgorithms_jl_amd.solvers as S
    from ciaoalgorithms_jl_amd.device import PackedF, ProxG
    from ciaoalgorithms_jl_amd import _lib as L
    A, b, Lc, lam, x0, x_star, f_star = lasso_fixture()
    N = A.shape[0]
    F = PackedF.least_squares(torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda(), float(N))
    g = ProxG(L.PROX_L1, lam=lam)
    gamma = float(1 / (7 * np.max(Lc)))
    cost = lambda x: P.lasso_cost(A, b, lam, x)
    lines = ["# point  gap  objective(x)-objective(x*)  slack=gap-subopt  m"]

    def check(tag, xdev):
        c = ctx.certificate(F, g, xdev, gamma)
        x = xdev.cpu().numpy()
        sub, m = cost(x) - cost(x_star), gap_margin(A, c, x)
        lines.append(f"{tag}  {c.gap:.6e}  {sub:.6e}  {c.gap - sub:.6e}  {m:.3e}")
        print(lines[-1])
        assert c.gap >= sub - m, (tag, c.gap, sub, m)
        return c, m

    check("x0", torch.from_numpy(x0).cuda())
    Fo = [ops.LeastSquares(A[i:i + 1, :], b[i:i + 1], float(N)) for i in range(N)]
    for k, st in zip(range(600), S.iterator(S.SVRG(np.float64, γ=gamma), x0, F=Fo, g=ops.NormL1(lam), N=N)):
        if k + 1 in (1, 2, 5, 10, 30, 100, 200, 300, 400, 500, 600):
            check(f"svrg{k + 1}", S.solution(st).clone())
    c, m = check("x_star", torch.from_numpy(x_star).cuda())
    assert abs(c.gap) <= m, (c.gap, m)
    with open(os.environ.get("CIAO_CERT_SLACK_OUT") or str(tmp_path / "cert_gap_slack.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


TAU = 6.057376822354854e-13


def test_solve_to_tolerance(ctx, ciao):
    """SVRG on the known-answer fixture with stop=stop_when(cert, gap=TAU) halts before maxit = 1000 (the count of
    tests/test_gpu_solvers.py::TestLasso) with objective(x) - objective(x*) <= TAU + m; without `stop` all 1000 iterations run.
    TAU = 6.057376822354854e-13 is the gap measured after 500 iterations (half the count) of the unchanged solver, gamma = 1/(7 max L):
    by then the run sits at its fixed point and the gap at its rounding floor (2.1e-5 after 250 iterations, 1.6e-10 after 400)."""
    import ciaoalgorithms_jl_amd.operators as ops
    import ciaoalgorithms_jl_amd.solvers as S
    from ciaoalgorithms_jl_amd.certificate import Certificate, stop_when
    A, b, Lc, lam, x0, x_star, f_star = lasso_fixture()
    N = A.shape[0]
    Fo = [ops.LeastSquares(A[i:i + 1, :], b[i:i + 1], float(N)) for i in range(N)]
    go = ops.NormL1(lam)
    gamma = float(1 / (7 * np.max(Lc)))
    cert = Certificate(ctx, Fo, go, N, gamma)
    stop = stop_when(cert, gap=TAU)
    x, it = S.SVRG(np.float64, maxit=1000, γ=gamma)(x0, F=Fo, g=go, N=N, ctx=ctx, stop=stop, check_every=10)
    print(f"halted after {it} iterations, gap {stop.last.gap:.6e}, residual {stop.last.residual:.3e}")
    assert it < 1000 and stop.last.gap <= TAU
    m = gap_margin(A, stop.last, x)
    assert P.lasso_cost(A, b, lam, x) - P.lasso_cost(A, b, lam, x_star) <= TAU + m
    x2, it2 = S.SVRG(np.float64, maxit=1000, γ=gamma)(x0, F=Fo, g=go, N=N, ctx=ctx)
    assert it2 == 1000
    # a residual bound composes the same way
    x3, it3 = S.SVRG(np.float64, maxit=1000, γ=gamma)(x0, F=Fo, g=go, N=N, ctx=ctx, stop=stop_when(cert, residual=1e-6), check_every=10)
    assert it3 < 1000


def test_refusals(ctx, ciao):
    """gamma <= 0 (or not finite), a complex problem and a sharing problem: CIAO_ERR_ARG with a message, nothing launched."""
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd.device import PackedF, PackedSepQuad, ProxG
    F, x = problem("ls", np.float64, 64)
    g = ProxG(L.PROX_L1, lam=LAM)
    ctx.full_gradient(F, x, torch.empty_like(x))
    before = ctx.last_kernel()
    assert not before.startswith("cert_")
    A2 = torch.randn((4, 8), dtype=torch.float64, device="cuda")
    Fc = PackedF.least_squares_complex(A2, torch.randn(8, dtype=torch.float64, device="cuda"), 4.0)
    Fs = PackedSepQuad(torch.ones((3, 4), dtype=torch.float64, device="cuda"), torch.ones((3, 4), dtype=torch.float64, device="cuda"))
    xs = torch.zeros(8, dtype=torch.float64, device="cuda")
    for what, call in (("gamma = 0", lambda: ctx.certificate(F, g, x, 0.0)), ("gamma < 0", lambda: ctx.certificate(F, g, x, -1.0)),
                       ("gamma = inf", lambda: ctx.certificate(F, g, x, math.inf)), ("gamma = nan", lambda: ctx.certificate(F, g, x, math.nan)),
                       ("complex problem", lambda: ctx.certificate(Fc, ProxG(), xs, 0.5)),
                       ("complex prox", lambda: ctx.certificate(F, ProxG(L.PROX_L1_COMPLEX, lam=1.0), x, 0.5)),
                       ("sharing problem", lambda: ctx.certificate(Fs, ProxG(), xs[:4], 0.5))):
        with pytest.raises(L.CiaoError) as e:
            call()
        assert e.value.status == L.ERR_ARG and len(str(e.value)) > 30, what
        assert ctx.last_kernel() == before, what
    ctx.synchronize()

"""The per-sample side on the device: ciao_row_dots against A64 @ x64 through every sweep family that writes row dots; ciao_margin_stats
against a float64 restatement written HERE (not imported from the package) with bounds derived from the arithmetic; extreme margins;
determinism; ciao_certificate_samples against ciao_certificate and against row_dots + margin_stats; the logistic duality gap as a bound
on objective(x) - min along an SVRG run on the reference's l1-logistic fixture and solve to tolerance; scoring.score; refusals."""
import math
import os

import numpy as np
import pytest

import problems as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS64 = float(np.finfo(np.float64).eps)
N_ROWS = 64
# csrc/mstat_kernels.h reuses csrc/cert_kernels.h: 256 threads, slices of 1024 samples up to 512 of them, whole multiples of 1024 beyond
SLICE, FINAL_THREADS, GRID_CAP = 1024, 256, 512
SIZES = [1, 3, 63, 64, 65, SLICE - 1, SLICE, SLICE + 1, 3 * SLICE + 5,
         FINAL_THREADS * SLICE + 1,      # 257 partial records: more than mstat_final_kernel has threads
         GRID_CAP * SLICE + 1]           # beyond the grid cap: the slices grow to 2048
S_VALUES = [1.0, 0.25, 0.0]


def bits(res):
    return np.array(tuple(res), dtype=np.float64).view(np.uint64).tolist()


def tdtype(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


def tname(dtype):
    return "f64" if dtype == np.float64 else "f32"


# ---- 1. row dots through every sweep family ---------------------------------------------------------------------------------------------
# (dtype, d, the kernel csrc/rows_launch.inc's plan_rows gives a full pass over 64 dense rows of that length)
#   d % (64 chunks) == 0 with 1 chunk per lane      -> one wave per row            rows_fast_kernel (rows_multi_kernel from 2 chunks per lane)
#   whole 16-byte chunks, 64 .. 4096 of them        -> one workgroup per row       rows_split_kernel (masked)
#   256 .. 4096 elements, no 16-byte structure      -> the same, single elements   rows_split_kernel (scalar)
#   at most 16 elements                             -> several rows per wave       rows_small_kernel
#   17 .. 256 elements, dense                       -> matrix-core tiles           rows_smallm_kernel
#   more than 4096 whole chunks                     -> a cluster per row           rows_long_kernel
#   more than 4096 elements, no 16-byte structure   -> any length                  rows_generic_kernel
FAMILY_CASES = [
    (np.float64, 128, ("rows_fast_kernel", "rows_multi_kernel")), (np.float32, 256, ("rows_fast_kernel", "rows_multi_kernel")),
    (np.float64, 512, ("rows_fast_kernel", "rows_multi_kernel")),      # 4 chunks per lane: the two-rows-in-flight form
    (np.float64, 1000, ("rows_split_kernel",)), (np.float32, 1000, ("rows_split_kernel",)),
    (np.float32, 1001, ("rows_split_kernel",)),
    (np.float64, 3, ("rows_small_kernel",)), (np.float32, 3, ("rows_small_kernel",)),
    (np.float64, 50, ("rows_smallm_kernel",)), (np.float32, 50, ("rows_smallm_kernel",)),
    (np.float64, 16384, ("rows_long_kernel",)),
    (np.float64, 4099, ("rows_generic_kernel",)), (np.float32, 4099, ("rows_generic_kernel",)),
]
REQUIRED_FAMILIES = [("rows_fast_kernel", "rows_multi_kernel"), ("rows_split_kernel",), ("rows_small_kernel",), ("rows_smallm_kernel",),
                     ("rows_generic_kernel",), ("rows_long_kernel",)]
assert all(any(c[2] == fam for c in FAMILY_CASES) for fam in REQUIRED_FAMILIES)     # every family is asserted reached by some case below

_rows_cache = {}


def rows_problem(dtype, d):
    """(A, x on the device, exact a_i'x as float64, sum_k |a_ik x_k|): shared by the two losses of one (dtype, d)."""
    import torch
    key = (tname(dtype), d)
    if key not in _rows_cache:
        _rows_cache.clear()
        td = tdtype(dtype)
        gen = torch.Generator(device="cuda").manual_seed(2000 + d)
        A = torch.randn((N_ROWS, d), dtype=td, device="cuda", generator=gen) / math.sqrt(d)
        x = 0.6 * torch.randn(d, dtype=td, device="cuda", generator=gen)
        t = torch.randn(N_ROWS, dtype=td, device="cuda", generator=gen)
        prod = A.cpu().numpy().astype(np.float64) * x.cpu().numpy().astype(np.float64)[None, :]
        exact = np.array([math.fsum(row.tolist()) for row in prod])
        _rows_cache[key] = (A, x, t, exact, np.abs(prod).sum(axis=1))
    return _rows_cache[key]


@pytest.mark.parametrize("loss", ["ls", "logistic"])
@pytest.mark.parametrize("dtype,d,family", FAMILY_CASES, ids=[f"{tname(c[0])}-d{c[1]}-{c[2][0]}" for c in FAMILY_CASES])
def test_row_dots_per_sweep_family(ctx, dtype, d, family, loss):
    """|out_i - a_i'x| <= d eps_T sum_k |a_ik x_k|: the bound gamma_d of a length-d dot product in T, which holds for every order of
    summation and with or without fused multiply-adds (d u / (1 - d u) with u = eps_T / 2; d eps_T is twice that and leaves room for the
    rounding of the float64 products of the restatement, exact for fp32 data and u64 sum |a x| for fp64).  The sums are math.fsum's."""
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    A, x, t, exact, scale = rows_problem(dtype, d)
    td = tdtype(dtype)
    F = (PackedF.least_squares(A, t, float(N_ROWS)) if loss == "ls" else PackedF.logistic(A, torch.where(t >= 0, 1.0, -1.0).to(td)))
    out = torch.full((N_ROWS,), float("nan"), dtype=td, device="cuda")
    got = ctx.row_dots(F, x, out=out)
    name = ctx.last_kernel()
    assert got is out and name.startswith(family), (name, family)
    ctx.synchronize()
    err = np.abs(out.cpu().numpy().astype(np.float64) - exact)
    bound = d * float(np.finfo(dtype).eps) * scale
    print(f"{name}: worst err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound), (name, float(np.max(err / bound)))
    # out=None: a new device vector with the same contents
    out2 = ctx.row_dots(F, x)
    assert out2.shape == (N_ROWS,) and out2.dtype == td and torch.equal(out2, out)


# ---- 2. the statistics against a restatement --------------------------------------------------------------------------------------------
def xlogx(u):
    return np.where(u > 0, u * np.log(np.where(u > 0, u, 1.0)), 0.0)


def restate_logistic(dots, b):
    """The s-independent part, in float64 numpy from the T-typed dots and labels, by the stable evaluation of the kernel."""
    t = b.astype(np.float64) * dots.astype(np.float64)
    e = np.exp(-np.abs(t))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    loss = np.maximum(-t, 0.0) + np.log1p(e)
    return {"t": t, "sneg": np.where(t >= 0, small, big), "spos": np.where(t >= 0, big, small), "loss_sum": math.fsum(loss.tolist()),
            "loss_abs": float(np.sum(np.abs(loss))), "errors": float(np.count_nonzero(t <= 0)), "min_margin": float(np.min(t))}


def restate_entropy(r, s):
    """E(s) and its bound eps64 (16 sum_i [v_i (1 + |log v_i|) + w_i (1 + |log w_i|)] + N sum_i |h_i|)."""
    v, w = s * r["sneg"], (1.0 - s) + s * r["spos"]
    h = xlogx(v) + xlogx(w)
    sens = lambda u: np.where(u > 0, u * (1.0 + np.abs(np.log(np.where(u > 0, u, 1.0)))), 0.0)
    return math.fsum(h.tolist()), EPS64 * (16 * float(np.sum(sens(v) + sens(w))) + h.size * float(np.sum(np.abs(h)))), h


def check_logistic(st, r, s, N, tag):
    """errors, min_margin: exact (a count; a minimum of products both sides round alike).  loss_sum: (N + 8) eps64 sum |term| -- N for
    the additions in any order, 8 for the term itself: exp and log1p within 2 ulp each on either side, one addition.  entropy: the
    terms v log v, w log w move by (1 + log v) dv with dv / v about 2 ulp from exp, 1 from the division, 1 from the product with s,
    and 2 ulp of log itself, on either side: 16 eps64 v (1 + |log v|) covers it; N eps64 sum |h| is the additions."""
    E, Ebound, _ = restate_entropy(r, s)
    err = {"loss_sum": abs(st.loss_sum - r["loss_sum"]), "entropy": abs(st.entropy - E), "errors": abs(st.errors - r["errors"]),
           "min_margin": abs(st.min_margin - r["min_margin"])}
    bound = {"loss_sum": (N + 8) * EPS64 * r["loss_abs"], "entropy": Ebound, "errors": 0.0, "min_margin": 0.0}
    print(f"{tag} s={s}: " + "  ".join(f"{k} err {err[k]:.3e} <= {bound[k]:.3e}" for k in err))
    for k in err:
        assert err[k] <= bound[k], (tag, s, k, err[k], bound[k], getattr(st, k))
    return E


def check_ls(st, dots, b, N, tag):
    """max_abs_r: exact (one double subtraction of T values on both sides).  The sums: (N + 8) eps64 sum |term|."""
    d64, b64 = dots.astype(np.float64), b.astype(np.float64)
    r = d64 - b64
    want = {"sum_r2": math.fsum((r * r).tolist()), "sum_b": math.fsum(b64.tolist()), "sum_b2": math.fsum((b64 * b64).tolist()),
            "max_abs_r": float(np.max(np.abs(r)))}
    scale = {"sum_r2": float(np.sum(r * r)), "sum_b": float(np.sum(np.abs(b64))), "sum_b2": float(np.sum(b64 * b64)), "max_abs_r": 0.0}
    for k in want:
        err, bound = abs(getattr(st, k) - want[k]), (N + 8) * EPS64 * scale[k]
        print(f"{tag}: {k} err {err:.3e} <= {bound:.3e}")
        assert err <= bound, (tag, k, err, bound, getattr(st, k), want[k])


def stats_problem(loss, dtype, dots, b):
    """A d = 1 problem that carries b (the data column is never read by the reduction) and the dots as a device vector."""
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    td = tdtype(dtype)
    bt = torch.from_numpy(b).to("cuda", td)
    A = torch.ones((b.size, 1), dtype=td, device="cuda")
    F = PackedF.least_squares(A, bt, 1.0) if loss == "ls" else PackedF.logistic(A, bt)
    return F, torch.from_numpy(dots).to("cuda", td)


def stats_data(loss, dtype, N):
    rng = np.random.default_rng(3000 + N)
    dots = (4.0 * rng.standard_normal(N)).astype(dtype)
    b = rng.standard_normal(N).astype(dtype) if loss == "ls" else np.where(rng.random(N) < 0.5, 1.0, -1.0).astype(dtype)
    return dots, b


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
@pytest.mark.parametrize("N", SIZES)
def test_statistics_against_a_restatement(ctx, N, loss, dtype):
    dots, b = stats_data(loss, dtype, N)
    F, dd = stats_problem(loss, dtype, dots, b)
    per = -(-N // GRID_CAP)
    slice_ = SLICE if per <= SLICE else -(-per // SLICE) * SLICE          # cert_slice(N)
    grid = -(-N // slice_)
    tag = f"N={N} {tname(dtype)} {loss}"
    if loss == "ls":
        st = ctx.margin_stats(F, dd)
        assert ctx.last_kernel() == f"mstat_partial_kernel<{tname(dtype)},ls> grid={grid} block=256"
        check_ls(st, dots, b, N, tag)
        assert bits(ctx.margin_stats(F, dd, 0.25)) == bits(st)          # s plays no part for LeastSquares rows
        return
    r = restate_logistic(dots, b)
    for s in S_VALUES:
        st = ctx.margin_stats(F, dd, s)
        assert ctx.last_kernel() == f"mstat_partial_kernel<{tname(dtype)},logistic> grid={grid} block=256"
        E = check_logistic(st, r, s, N, tag)
        assert -N * math.log(2) - abs(E) * N * EPS64 <= st.entropy <= 0.0
    assert ctx.margin_stats(F, dd, 0.0).entropy == 0.0                  # s = 0: v = 0, w = 1 for every sample


# ---- 3. extreme margins ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("s", [1.0, 0.5])
def test_extreme_margins(ctx, s, dtype):
    """t in {0, +-1e-30, +-40, +-745, +-1e4} under both labels: exp(-|t|) runs from 1 through the subnormals (745) to 0 (1e4).  Every
    result finite, E in [-N log 2, 0], and the restatement's bounds hold as they stand."""
    ts = np.array([0.0, 1e-30, -1e-30, 40.0, -40.0, 745.0, -745.0, 1e4, -1e4])
    b = np.concatenate([np.ones(ts.size), -np.ones(ts.size)]).astype(dtype)
    dots = (np.concatenate([ts, -ts])).astype(dtype)                      # dot = y t: the margin y dot is t under both labels
    N = b.size
    F, dd = stats_problem("logistic", dtype, dots, b)
    st = ctx.margin_stats(F, dd, s)
    assert all(math.isfinite(v) for v in st), st
    assert -N * math.log(2) <= st.entropy <= 0.0
    r = restate_logistic(dots, b)
    check_logistic(st, r, s, N, f"extreme {tname(dtype)}")
    assert st.errors == 2 * 5 and st.min_margin == -1e4
    assert abs(st.loss_sum - 2 * (3 * math.log(2) + 40 + 745 + 1e4)) <= 1e-9 * 2e4


# ---- 4. determinism and consistency -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
@pytest.mark.parametrize("N", [65, 3 * SLICE + 5, FINAL_THREADS * SLICE + 1])
def test_determinism(ctx, N, loss, dtype):
    """Twice in a row, from a second context, and from a dots view one element into a buffer (not 16-byte aligned: element loads by the
    thread that would have read the chunk): bitwise equal -- the grid and every order of addition are functions of N alone."""
    import torch
    from ciaoalgorithms_jl_amd.device import Context
    dots, b = stats_data(loss, dtype, N)
    F, dd = stats_problem(loss, dtype, dots, b)
    a, a2 = ctx.margin_stats(F, dd, 0.25), ctx.margin_stats(F, dd, 0.25)
    other = Context(0)
    try:
        c = other.margin_stats(F, dd, 0.25)
    finally:
        other.close()
    big = torch.empty(N + 1, dtype=dd.dtype, device="cuda")
    dm = big[1:]
    dm.copy_(dd)
    assert dm.data_ptr() % 16 != 0 and dm.is_contiguous()
    assert bits(a) == bits(a2) == bits(c) == bits(ctx.margin_stats(F, dm, 0.25))


_cert_cache = {}


def cert_problem(loss, dtype, d):
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    key = (loss, tname(dtype), d)
    if key not in _cert_cache:
        td = tdtype(dtype)
        gen = torch.Generator(device="cuda").manual_seed(4000 + d)
        A = torch.randn((N_ROWS, d), dtype=td, device="cuda", generator=gen) / math.sqrt(d)
        t = torch.randn(N_ROWS, dtype=td, device="cuda", generator=gen)
        x = 0.6 * torch.randn(d, dtype=td, device="cuda", generator=gen)
        F = PackedF.least_squares(A, t, float(N_ROWS)) if loss == "ls" else PackedF.logistic(A, torch.where(t >= 0, 1.0, -1.0).to(td))
        _cert_cache[key] = (F, x)
    return _cert_cache[key]


@pytest.mark.parametrize("kind", ["l1", "l1_small", "zero", "box"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("loss,d", [("ls", 65), ("logistic", 65), ("logistic", 1000), ("logistic", 3)])
def test_certificate_with_samples_is_consistent(ctx, loss, d, dtype, kind):
    """certificate(samples=True): its first six numbers are bitwise certificate()'s; its four statistics are bitwise
    margin_stats(F, row_dots(F, x), s) with s formed on the host from its grad_inf as the kernel forms it; its gap is the expression
    of DESIGN 8.7 evaluated from its own fields.  (l1: mu above ||grad f||_inf, s = 1; l1_small: below, s < 1.)"""
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd.device import ProxG
    F, x = cert_problem(loss, dtype, d)
    gamma = 0.375
    plain0 = ctx.certificate(F, ProxG(), x, gamma)
    mu = {"l1": 2.0 * plain0.grad_inf, "l1_small": 0.125 * plain0.grad_inf}.get(kind)
    g = ProxG(L.PROX_L1, lam=mu) if mu is not None else (ProxG() if kind == "zero" else ProxG(L.PROX_BOX, lo=-0.25, hi=0.5))
    plain = ctx.certificate(F, g, x, gamma)
    c, st = ctx.certificate_samples(F, g, x, gamma)
    assert ctx.last_kernel().startswith("mstat_partial_kernel")
    assert bits(ctx.certificate(F, g, x, gamma, samples=True)) == bits(c)
    assert bits(c[:7]) == bits(plain[:7])
    s = 1.0
    if mu is not None:
        s = 1.0 if c.grad_inf == 0 else min(1.0, mu / c.grad_inf)
        assert (s == 1.0) == (kind == "l1")
    assert bits(st) == bits(ctx.margin_stats(F, ctx.row_dots(F, x), s))
    if loss == "logistic" and mu is not None:
        assert c.gap == c.F + c.g + st.entropy / N_ROWS and c.gap >= 0 and math.isnan(plain.gap)
    elif loss == "ls" and mu is not None:
        assert bits([c.gap]) == bits([plain.gap]) and c.gap >= 0
    else:
        assert math.isnan(c.gap) and math.isnan(plain.gap)


# ---- 5. the gap as a bound --------------------------------------------------------------------------------------------------------------
def softplus(u):
    return np.maximum(u, 0.0) + np.log1p(np.exp(-np.abs(u)))


def logistic_cost(A, y, mu, x):
    return float(np.mean(softplus(-y * (A @ x))) + mu * np.abs(x).sum())


# the tolerance and iteration cap of the solve-to-tolerance test: chosen on the host route (tests/test_margins_host.py: the same problem,
# step and index stream halt after 850 iterations there); the fixture's stored x* has gap 5.2e-8
GAP_TOL, MAXIT = 1e-4, 4000


def test_the_gap_is_a_bound(ctx, ciao):
    """SVRG from x0 = ones on the l1-logistic fixture, certificate every 10 iterations: gap >= 0 and gap >= P(x_k) - P(x*) - 1e-9 max(1,
    P(x_k)) with P restated in numpy and x* the fixture's; the last gap is below the first."""
    import torch
    import ciaoalgorithms_jl_amd.operators as ops
    import ciaoalgorithms_jl_amd.solvers as S
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd.device import PackedF, ProxG
    A, y, Lc, mu, x0, x_star = P.logistic_fixture(np.float64)
    N, n = A.shape
    F = PackedF.logistic(torch.from_numpy(A).cuda(), torch.from_numpy(y).cuda())
    g = ProxG(L.PROX_L1, lam=mu)
    gamma = float(1 / (7 * np.max(Lc)))
    p_star = logistic_cost(A, y, mu, x_star)
    gaps = []

    def check(tag, xdev):
        c = ctx.certificate(F, g, xdev, gamma, samples=True)
        pk = logistic_cost(A, y, mu, xdev.cpu().numpy())
        print(f"{tag}  gap {c.gap:.6e}  P - P* {pk - p_star:.6e}")
        assert c.gap >= 0 and c.gap >= pk - p_star - 1e-9 * max(1.0, pk), (tag, c.gap, pk - p_star)
        assert abs(c.objective - pk) <= 1e-9 * max(1.0, pk)
        gaps.append(c.gap)

    check("x0", torch.from_numpy(x0).cuda())
    Fo = [ops.Precompose(ops.LogisticLoss([y[i]], 1.0), A[i].reshape(1, n), 1.0) for i in range(N)]
    for k, st in zip(range(300), S.iterator(S.SVRG(np.float64, γ=gamma), x0, F=Fo, g=ops.NormL1(mu), N=N)):
        if (k + 1) % 10 == 0:
            check(f"svrg{k + 1}", S.solution(st).clone())
    assert gaps[-1] < gaps[0] and 7.5 <= gaps[0] <= 8.0
    check("x_star", torch.from_numpy(x_star).cuda())
    assert gaps[-1] <= 1e-7


def test_solve_to_tolerance(ctx, ciao):
    import ciaoalgorithms_jl_amd.operators as ops
    import ciaoalgorithms_jl_amd.solvers as S
    from ciaoalgorithms_jl_amd.certificate import Certificate, stop_when
    A, y, Lc, mu, x0, x_star = P.logistic_fixture(np.float64)
    N, n = A.shape
    Fo = [ops.Precompose(ops.LogisticLoss([y[i]], 1.0), A[i].reshape(1, n), 1.0) for i in range(N)]
    go = ops.NormL1(mu)
    gamma = float(1 / (7 * np.max(Lc)))
    stop = stop_when(Certificate(ctx, Fo, go, N, gamma, samples=True), gap=GAP_TOL)
    x, it = S.SVRG(np.float64, maxit=MAXIT, γ=gamma)(x0, F=Fo, g=go, N=N, ctx=ctx, stop=stop, check_every=10)
    print(f"halted after {it} iterations, gap {stop.last.gap:.6e}, residual {stop.last.residual:.3e}")
    assert it < MAXIT and 0 <= stop.last.gap <= GAP_TOL
    assert logistic_cost(A, y, mu, x) - logistic_cost(A, y, mu, x_star) <= GAP_TOL
    # without samples the gap stays nan and the same bound never stops the run
    blind = stop_when(Certificate(ctx, Fo, go, N, gamma), gap=GAP_TOL)
    x2, it2 = S.SVRG(np.float64, maxit=50, γ=gamma)(x0, F=Fo, g=go, N=N, ctx=ctx, stop=blind, check_every=10)
    assert it2 == 50 and math.isnan(blind.last.gap)


# ---- 6. scoring ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_score(ctx, dtype):
    """score's fields are their definitions from the raw statistics; it works on a second PackedF (new rows, the same d): the
    prediction path.  Against numpy on the downloaded data the fields move by what the row dots may: delta_i = d eps_T sum_k |a_ik x_k|
    per sample (test 1's bound), through |d r^2| <= 2 |r| delta + delta^2 and the 1-Lipschitz softplus; a label counts as an error for
    certain only where |t_i| > delta_i."""
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    from ciaoalgorithms_jl_amd.scoring import LeastSquaresScore, LogisticScore, score
    td, d = tdtype(dtype), 50
    gen = torch.Generator(device="cuda").manual_seed(77)
    x = torch.randn(d, dtype=td, device="cuda", generator=gen)
    for n_rows in (N_ROWS, 37):            # the "training" rows, then new rows
        A = torch.randn((n_rows, d), dtype=td, device="cuda", generator=gen) / math.sqrt(d)
        b = A @ x + 0.1 * torch.randn(n_rows, dtype=td, device="cuda", generator=gen)
        A64, b64, x64 = A.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64), x.cpu().numpy().astype(np.float64)
        delta = d * float(np.finfo(dtype).eps) * np.abs(A64 * x64[None, :]).sum(axis=1)
        sums = 1 + 64 * EPS64                # the double sums of the reduction and of numpy
        F = PackedF.least_squares(A, b, 1.0)
        sc, st = score(ctx, F, x), ctx.margin_stats(F, ctx.row_dots(F, x))
        assert isinstance(sc, LeastSquaresScore)
        assert sc == (st.sum_r2 / n_rows, 1.0 - st.sum_r2 / (st.sum_b2 - st.sum_b ** 2 / n_rows), st.max_abs_r)
        r = A64 @ x64 - b64
        dmse = float(np.mean(2 * np.abs(r) * delta + delta ** 2))
        tss = float(np.sum((b64 - b64.mean()) ** 2))
        assert abs(sc.mse - np.mean(r * r)) <= dmse * sums + 64 * EPS64 * np.mean(r * r)
        assert abs(sc.max_abs_residual - np.abs(r).max()) <= delta.max() * sums
        assert abs(sc.r2 - (1 - np.sum(r * r) / tss)) <= n_rows * dmse / tss * sums + 1e-12 and sc.r2 > 0.9
        y = torch.where(b >= 0, 1.0, -1.0).to(td)
        y[:3] = -y[:3]                      # three labels flipped
        Fl = PackedF.logistic(A, y)
        sc, st = score(ctx, Fl, x), ctx.margin_stats(Fl, ctx.row_dots(Fl, x))
        assert isinstance(sc, LogisticScore)
        assert sc == (st.loss_sum / n_rows, 1.0 - st.errors / n_rows, st.min_margin)
        t = y.cpu().numpy().astype(np.float64) * (A64 @ x64)
        safe = np.abs(t) > delta * sums
        assert np.count_nonzero((t <= 0) & safe) <= st.errors <= np.count_nonzero((t <= 0) | ~safe)
        assert sc.accuracy == 1.0 - st.errors / n_rows and 0.0 <= sc.accuracy <= 1.0
        assert abs(sc.log_loss - np.mean(softplus(-t))) <= float(np.mean(delta)) * sums + 64 * EPS64 * np.mean(softplus(-t))
        assert abs(sc.min_margin - t.min()) <= delta.max() * sums


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, ciao):
    """Complex problems, Zero() terms, N = 0, s outside [0, 1], samples=True with a caller's av, and a context with an all-reduce hook:
    CIAO_ERR_ARG with a message, nothing launched.  Without samples, logistic rows with NormL1 still give gap = nan."""
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd.device import Context, PackedF, PackedSepQuad, ProxG
    F, x = cert_problem("logistic", np.float64, 65)
    g = ProxG(L.PROX_L1, lam=0.3125)
    dots = ctx.row_dots(F, x)
    assert math.isnan(ctx.certificate(F, g, x, 0.5).gap)
    ctx.full_gradient(F, x, torch.empty_like(x))
    before = ctx.last_kernel()
    assert not before.startswith(("mstat_", "cert_"))
    f64 = dict(dtype=torch.float64, device="cuda")
    Fc = PackedF.least_squares_complex(torch.randn((4, 8), **f64), torch.randn(8, **f64), 4.0)
    Fz = PackedF.zero(4, 8, torch.float64)
    F0 = PackedF.logistic(torch.empty((0, 8), **f64), torch.empty(0, **f64))
    Fs = PackedSepQuad(torch.ones((3, 4), **f64), torch.ones((3, 4), **f64))
    x8, d4, d0 = torch.zeros(8, **f64), torch.zeros(4, **f64), torch.zeros(0, **f64)
    hooked = Context(0)
    hooked.set_allreduce(lambda buf, count, dtype, stream: 0)
    try:
        cases = [("complex row_dots", lambda: ctx.row_dots(Fc, x8)), ("complex margin_stats", lambda: ctx.margin_stats(Fc, d4)),
                 ("complex certificate", lambda: ctx.certificate(Fc, ProxG(), x8, 0.5, samples=True)),
                 ("complex prox", lambda: ctx.certificate(F, ProxG(L.PROX_L1_COMPLEX, lam=1.0), x, 0.5, samples=True)),
                 ("Zero row_dots", lambda: ctx.row_dots(Fz, x8)), ("Zero margin_stats", lambda: ctx.margin_stats(Fz, d4)),
                 ("Zero certificate", lambda: ctx.certificate(Fz, g, x8, 0.5, samples=True)),
                 ("N = 0 margin_stats", lambda: ctx.margin_stats(F0, d0)), ("N = 0 certificate", lambda: ctx.certificate(F0, g, x8, 0.5, samples=True)),
                 ("s < 0", lambda: ctx.margin_stats(F, dots, -0.125)), ("s > 1", lambda: ctx.margin_stats(F, dots, 1.5)),
                 ("s = nan", lambda: ctx.margin_stats(F, dots, math.nan)),
                 ("gamma = 0", lambda: ctx.certificate(F, g, x, 0.0, samples=True)),
                 ("samples with av", lambda: ctx.certificate(F, g, x, 0.5, av=torch.zeros_like(x), samples=True)),
                 ("samples with fval", lambda: ctx.certificate(F, g, x, 0.5, fval=1.0, samples=True)),
                 ("sharing row_dots", lambda: ctx.row_dots(Fs, d4)), ("sharing margin_stats", lambda: ctx.margin_stats(Fs, d4)),
                 ("sharing certificate", lambda: ctx.certificate(Fs, ProxG(), d4, 0.5, samples=True)),
                 ("all-reduce hook", lambda: hooked.certificate(F, g, x, 0.5, samples=True))]
        for what, call in cases:
            with pytest.raises(L.CiaoError) as e:
                call()
            assert e.value.status == L.ERR_ARG and len(str(e.value)) > 30, what
            assert ctx.last_kernel() == before, what
        assert "all-reduce" in str(e.value)
    finally:
        hooked.close()
    ctx.synchronize()

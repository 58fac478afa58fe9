"""K models scored in one pass over the rows (ciao_margin_stats_multi; csrc/mscore_kernels.h).

1. exact cases: integer data whose row dots are exact in either type in any order, so the one-pass kernel must reproduce the library's
   own two-call path ctx.margin_stats(F, ctx.row_dots(F, x_k), s_k) -- LeastSquares bitwise, the logistic count and minimum bitwise,
   the two logistic sums to the reordering of N same-signed terms -- at every shape where the plan changes, under four layouts with
   NaN-poisoned padding and guard bands;
2. independence: a model's four doubles do not depend on K, on its place in the list or on what the other iterates hold (NaN included);
3. general data against the float64 numpy twin with bounds computed from the data;
4. the fallback (rows beyond the kernel's reach, option mscore_off): bitwise the two-call path;
5. refusals, scoring.score_many / best, certificate.gaps_together."""
import math

import numpy as np
import pytest

import layouts as LY
import problems as P

pytestmark = pytest.mark.gpu

PART_TARGET, TILE, MAX_D = 2048, 16, 1024      # csrc/mscore_kernels.h: partitions at most, rows of a tile, longest row of the one-pass kernel
LAYOUTS = [("packed", 0, 0), ("ld>d", 3, 0), ("base+1", 0, 1), ("ld>d,base+1", 3, 1)]   # (name, ld - d, elements off 16-byte alignment)


def part_rows(N):
    """mscore_part_rows: whole tiles, a function of N alone"""
    per = -(-N // PART_TARGET)
    return max(TILE, -(-per // TILE) * TILE)


def bits(vals):
    return np.array([tuple(v) for v in vals], dtype=np.float64).view(np.uint64).tolist()


def tdtype(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


def tname(dtype):
    return "f64" if dtype == np.float64 else "f32"


class Case:
    """A problem under a layout: A, b and the K iterates inside guarded, poisoned buffers (the iterates at their aligned bases: the
    header asks for 16-byte aligned iterates)."""

    def __init__(self, loss, A, b, xs, layout):
        from ciaoalgorithms_jl_amd.device import PackedF
        _, pad, off = layout
        td = tdtype(A.dtype)
        self.loss, self.N, self.d = loss, A.shape[0], A.shape[1]
        self.gA = LY.Guarded(A, off=off, ld=self.d + pad, device="cuda", name="A")
        self.gb = LY.Guarded(b, off=off, device="cuda", name="b")
        self.gx = [LY.Guarded(x, device="cuda", name=f"x[{k}]") for k, x in enumerate(xs)]
        self.xs = [g.view for g in self.gx]
        assert all(x.data_ptr() % 16 == 0 for x in self.xs) and self.gA.view.dtype == td
        self.F = PackedF.least_squares(self.gA.view, self.gb.view, 1.0) if loss == "ls" else PackedF.logistic(self.gA.view, self.gb.view)

    def two_calls(self, ctx, s):
        return [ctx.margin_stats(self.F, ctx.row_dots(self.F, x), sk) for x, sk in zip(self.xs, s)]

    def check_untouched(self, what):
        for g in [self.gA, self.gb] + self.gx:
            g.check_unchanged(what)


def integer_problem(loss, N, d, K, dtype, seed):
    """|a_ij| <= 8, |x_j| <= 4, b integer / +-1: every dot is an integer below 2^24 -- exact in either type in any order"""
    rng = np.random.default_rng(seed)
    A = rng.integers(-8, 9, size=(N, d)).astype(dtype)
    xs = [rng.integers(-4, 5, size=d).astype(dtype) for _ in range(K)]
    b = (rng.integers(-8, 9, size=N) if loss == "ls" else rng.choice([-1, 1], size=N)).astype(dtype)
    return A, b, xs


def kernel_name(dtype, d, loss, K, N, vec16):
    sl = 4 if d <= 64 else 16 if d <= 256 else 32 if d <= 512 else 64
    parts = -(-N // part_rows(N))
    return (f"mscore_partial_kernel<{tname(dtype)},SL{sl},{'logistic' if loss == 'logistic' else 'ls'},{'vec16' if vec16 else 'elem'}> "
            f"grid={8 * -(-K // 16) * -(-parts // 8)} block=256 K={K} partitions={parts}")


# ---- 1. exact cases --------------------------------------------------------------------------------------------------------------------
# every N of {1, 15, 16, 17, 33, 2050} (a partition is one tile of 16 rows up to N = 32768: 15 / 16 / 17 are one below / at / one above
# it), every d of {1, 3, 15, 16, 17, 50, 255, 256, 1000, 1024} and every K of {1, 15, 16, 17, 33}, the corners, the row lengths either
# side of the kernel's three thresholds (64, 256, 512), and partitions of two and three tiles (N beyond 32768 and 65536)
EXACT = [(1, 1, 1), (15, 3, 15), (16, 15, 16), (17, 16, 17), (33, 17, 33), (2050, 50, 1), (16, 255, 15), (17, 256, 16), (33, 1000, 17),
         (15, 1024, 33), (1, 1024, 33), (2050, 1, 33), (2050, 1024, 33), (2050, 1024, 1), (1, 1, 33),
         (33, 64, 17), (33, 65, 17), (33, 257, 17), (33, 512, 17), (33, 513, 17),
         (32768 + 17, 3, 17), (65536 + 33, 17, 5)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
@pytest.mark.parametrize("shape", list(enumerate(EXACT)), ids=[f"N{n}-d{d}-K{k}" for n, d, k in EXACT])
def test_exact_cases(ctx, shape, loss, dtype):
    from ciaoalgorithms_jl_amd import host_route as HR
    idx, (N, d, K) = shape
    layout = LAYOUTS[(idx + (loss == "ls") + 2 * (dtype == np.float64)) % 4]      # every layout meets every loss and type
    A, b, xs = integer_problem(loss, N, d, K, dtype, seed=100 * idx + 7)
    c = Case(loss, A, b, xs, layout)
    s = [(1.0, 0.5, 0.0)[k % 3] for k in range(K)]
    got = ctx.margin_stats_multi(c.F, c.xs, s)
    vec16 = c.gA.view.data_ptr() % 16 == 0 and (c.F.ld * A.itemsize) % 16 == 0
    assert ctx.last_kernel() == kernel_name(dtype, d, loss, K, N, vec16), (ctx.last_kernel(), layout)
    c.check_untouched(f"margin_stats_multi {layout[0]}")
    want = c.two_calls(ctx, s)
    twin = HR.host_margin_stats_multi(loss, A, xs, b, s)
    assert len(got) == K and all(type(g) is type(w) for g, w in zip(got, want))
    if loss == "ls":
        assert bits(got) == bits(want), layout
        assert bits(got) == bits(twin), layout
        return
    for k in range(K):
        g, w = got[k], want[k]
        assert g.errors == w.errors == twin[k][2] and g.min_margin == w.min_margin == twin[k][3], (k, g, w)
        for name in ("loss_sum", "entropy"):
            gv, wv = getattr(g, name), getattr(w, name)
            tol = 2 * N * 2.0 ** -53 * abs(wv)
            assert abs(gv - wv) <= tol, (k, name, gv, wv, abs(gv - wv), tol)
        if s[k] == 0.0:
            assert g.entropy == 0.0


def test_every_layout_meets_every_loss_and_type():
    seen = {(loss, dt, LAYOUTS[(idx + (loss == "ls") + 2 * dt) % 4][0]) for idx in range(len(EXACT)) for loss in ("ls", "logistic") for dt in (0, 1)}
    assert len(seen) == 16


# ---- 2. independence, bitwise --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
def test_a_model_depends_on_nothing_but_itself(ctx, loss, dtype):
    import torch
    N, d, K = 53, 300, 17
    A, b, x0 = P.synthetic(loss, N, d, dtype, seed=5)
    rng = np.random.default_rng(6)
    xs = [x0] + [(0.3 * rng.standard_normal(d)).astype(dtype) for _ in range(K - 1)]
    c = Case(loss, A, b, xs, LAYOUTS[1])
    s = [(1.0, 0.5, 0.0)[k % 3] for k in range(K)]
    all17 = ctx.margin_stats_multi(c.F, c.xs, s)
    assert bits(ctx.margin_stats_multi(c.F, c.xs, s)) == bits(all17)                       # the call repeated
    for k in (0, 7, 16):
        assert bits(ctx.margin_stats_multi(c.F, [c.xs[k]], [s[k]])) == bits([all17[k]]), k   # alone (K = 1: the first column of a block)
    rev = ctx.margin_stats_multi(c.F, c.xs[::-1], s[::-1])
    assert bits(rev[::-1]) == bits(all17)                                                  # another place in the list, another block
    poisoned = list(c.xs)
    poisoned[3] = torch.full_like(c.xs[3], float("nan"))
    got = ctx.margin_stats_multi(c.F, poisoned, s)
    assert bits(got[:3] + got[4:]) == bits(all17[:3] + all17[4:])
    assert math.isnan(got[3][0])
    c.check_untouched("independence")


# ---- 3. general data against the float64 twin ------------------------------------------------------------------------------------------------
def general_bounds(loss, dtype, A64, b64, x64, N, d):
    """delta_i: what a length-d dot in T (and its rounding into T) may move, (d+1) u / (1 - (d+1) u) sum_j |a_ij x_j|; doubled for fp64,
    whose twin rounds too"""
    u = float(np.finfo(dtype).eps) / 2
    delta = (d + 1) * u / (1 - (d + 1) * u) * (np.abs(A64) @ np.abs(x64)) * (2 if dtype == np.float64 else 1)
    dots = A64 @ x64
    if loss == "ls":
        r = dots - b64
        return delta, {"sum_r2": float(np.sum(2 * np.abs(r) * delta + delta ** 2) + 2 * N * 2.0 ** -53 * np.sum(r * r)),
                       "sum_b": 2 * N * 2.0 ** -53 * float(np.sum(np.abs(b64))), "sum_b2": 2 * N * 2.0 ** -53 * float(np.sum(b64 * b64)),
                       "max_abs_r": float(delta.max())}
    return delta, dots * b64


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
@pytest.mark.parametrize("N,d", [(37, 50), (3001, 256), (37, 1000), (3001, 50), (37, 256), (3001, 1000)])
def test_general_data_against_the_float64_twin(ctx, N, d, loss, dtype):
    from ciaoalgorithms_jl_amd import host_route as HR
    K = 5
    A, b, x0 = P.synthetic(loss, N, d, dtype, seed=N + d)
    rng = np.random.default_rng(N * d)
    xs = [x0] + [((0.2 + 0.2 * k) * rng.standard_normal(d)).astype(dtype) for k in range(1, K)]
    c = Case(loss, A, b, xs, LAYOUTS[(N + d) % 4])
    got = ctx.margin_stats_multi(c.F, c.xs)
    assert "mscore_partial_kernel" in ctx.last_kernel() and f"K={K}" in ctx.last_kernel()
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    twin = HR.host_margin_stats_multi(loss, A64, xs, b64)
    for k in range(K):
        x64 = xs[k].astype(np.float64)
        g, w = got[k], twin[k]
        if loss == "ls":
            _, bound = general_bounds(loss, dtype, A64, b64, x64, N, d)
            for i, name in enumerate(("sum_r2", "sum_b", "sum_b2", "max_abs_r")):
                err = abs(g[i] - w[i])
                print(f"N={N} d={d} {tname(dtype)} ls model {k}: {name} err {err:.3e} <= {bound[name]:.3e}")
                assert err <= bound[name], (k, name, g[i], w[i], err, bound[name])
            continue
        delta, t = general_bounds(loss, dtype, A64, b64, x64, N, d)
        sd = float(np.sum(delta))
        bl = sd + 2 * N * 2.0 ** -52 * w[0]
        be = 0.23 * sd + 2 * N * 2.0 ** -52 * abs(w[1])
        print(f"N={N} d={d} {tname(dtype)} logistic model {k}: loss err {abs(g[0] - w[0]):.3e} <= {bl:.3e}  E err {abs(g[1] - w[1]):.3e} <= {be:.3e}")
        assert abs(g.loss_sum - w[0]) <= bl and abs(g.entropy - w[1]) <= be, (k, g, w, bl, be)
        assert np.count_nonzero(t < -delta) <= g.errors <= np.count_nonzero(t <= delta), (k, g.errors)
        assert abs(g.min_margin - w[3]) <= float(delta.max()), (k, g.min_margin, w[3])
    c.check_untouched("general data")


# ---- 4. the fallback -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("loss", ["ls", "logistic"])
@pytest.mark.parametrize("how", ["d=1025", "mscore_off"])
def test_the_fallback_is_the_two_call_path_bitwise(ctx, how, loss, dtype):
    N, d, K = 131, (MAX_D + 1 if how == "d=1025" else 256), 3
    A, b, x0 = P.synthetic(loss, N, d, dtype, seed=11)
    xs = [x0, (2 * x0).astype(dtype), (-x0).astype(dtype)]
    c = Case(loss, A, b, xs, LAYOUTS[0])
    s = [1.0, 0.5, 0.0]
    if how == "mscore_off":
        ctx.set_option("mscore_off", 1)
    try:
        got = ctx.margin_stats_multi(c.F, c.xs, s)
        name = ctx.last_kernel()
    finally:
        ctx.set_option("mscore_off", 0)
    assert "mscore" not in name and name.startswith("mstat_partial_kernel"), name
    assert bits(got) == bits(c.two_calls(ctx, s))
    if how == "mscore_off":                  # the option is off again: the same shape takes the kernel
        ctx.margin_stats_multi(c.F, c.xs, s)
        assert "mscore_partial_kernel" in ctx.last_kernel()


def test_an_unaligned_iterate_takes_the_fallback(ctx):
    import torch
    N, d = 40, 50
    A, b, x0 = P.synthetic("ls", N, d, np.float64, seed=12)
    c = Case("ls", A, b, [x0], LAYOUTS[0])
    big = torch.zeros(d + 1, dtype=torch.float64, device="cuda")
    big[1:].copy_(c.xs[0])
    got = ctx.margin_stats_multi(c.F, [big[1:]])
    assert "mscore" not in ctx.last_kernel()
    assert bits(got) == bits(c.two_calls(ctx, [1.0]))


# ---- 5. refusals and the Python layer ----------------------------------------------------------------------------------------------------
def test_refusals(ctx, ciao):
    import ctypes as C
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd.device import PackedF, PackedSepQuad
    f64 = dict(dtype=torch.float64, device="cuda")
    A = torch.randn((9, 8), **f64)
    F = PackedF.logistic(A, torch.ones(9, **f64))
    x = torch.zeros(8, **f64)
    ctx.full_gradient(F, x, torch.empty_like(x))
    before = ctx.last_kernel()
    assert "mscore" not in before and not before.startswith("mstat_")
    Fc = PackedF.least_squares_complex(torch.randn((4, 8), **f64), torch.randn(8, **f64), 4.0)
    Fz = PackedF.zero(4, 8, torch.float64)
    F0 = PackedF.logistic(torch.empty((0, 8), **f64), torch.empty(0, **f64))
    Fs = PackedSepQuad(torch.ones((3, 8), **f64), torch.ones((3, 8), **f64))
    lib, h = ctx.lib, ctx._h
    tab = (C.c_void_p * 2)(x.data_ptr(), x.data_ptr())
    hole = (C.c_void_p * 2)(x.data_ptr(), None)
    out = (C.c_double * 8)()
    raw = [("NULL ctx", lambda: lib.ciao_margin_stats_multi(None, F.ref, 2, tab, None, out)),
           ("NULL problem", lambda: lib.ciao_margin_stats_multi(h, None, 2, tab, None, out)),
           ("NULL x", lambda: lib.ciao_margin_stats_multi(h, F.ref, 2, None, None, out)),
           ("NULL out", lambda: lib.ciao_margin_stats_multi(h, F.ref, 2, tab, None, None)),
           ("NULL x[1]", lambda: lib.ciao_margin_stats_multi(h, F.ref, 2, hole, None, out))]
    for what, call in raw:
        assert call() == L.ERR_ARG, what
        assert len(lib.ciao_last_error()) > 20 and ctx.last_kernel() == before, what
    cases = [("K = 0", lambda: ctx.margin_stats_multi(F, [])), ("K = 257", lambda: ctx.margin_stats_multi(F, [x] * 257)),
             ("s < 0", lambda: ctx.margin_stats_multi(F, [x, x], [1.0, -0.125])), ("s > 1", lambda: ctx.margin_stats_multi(F, [x, x], [1.5, 1.0])),
             ("s = nan", lambda: ctx.margin_stats_multi(F, [x, x], [0.5, math.nan])),
             ("N = 0", lambda: ctx.margin_stats_multi(F0, [x])), ("Zero", lambda: ctx.margin_stats_multi(Fz, [x])),
             ("complex", lambda: ctx.margin_stats_multi(Fc, [x])), ("sharing", lambda: ctx.margin_stats_multi(Fs, [x])),
             ("s of another length", lambda: ctx.margin_stats_multi(F, [x, x], [1.0]))]
    for what, call in cases:
        with pytest.raises(L.CiaoError) as e:
            call()
        assert e.value.status == L.ERR_ARG and len(str(e.value)) > 20, what
        assert ctx.last_kernel() == before, what
    assert len(ctx.margin_stats_multi(F, [x] * 256)) == 256       # the largest K is taken
    ctx.synchronize()


def test_best():
    from ciaoalgorithms_jl_amd.scoring import LeastSquaresScore, LogisticScore, best
    nan = math.nan
    assert best([LogisticScore(nan, 1.0, 1.0), LogisticScore(0.5, 0.9, 0.1), LogisticScore(0.25, 0.8, 0.1), LogisticScore(0.25, 1.0, 2.0)]) == 2
    assert best([LeastSquaresScore(2.0, 0.1, 1.0), LeastSquaresScore(nan, nan, nan), LeastSquaresScore(2.0, 0.9, 0.5)]) == 0
    with pytest.raises(ValueError):
        best([LogisticScore(nan, 1.0, 1.0)])
    with pytest.raises(ValueError):
        best([])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_score_many_is_score_per_model(ctx, dtype):
    """section 3's bounds carried through _score: mse = sum r^2 / N, log_loss = sum / N; both sides are device paths, each within delta_i
    of the exact dots (the fp64 doubling covers the pair; for fp32 the bound is doubled here)"""
    from ciaoalgorithms_jl_amd.scoring import best, score, score_many
    N, d, K = 200, 50, 4
    pair = 1 if dtype == np.float64 else 2
    for loss in ("ls", "logistic"):
        A, b, x0 = P.synthetic(loss, N, d, dtype, seed=21)
        xs = [((0.5 + 0.5 * k) * x0).astype(dtype) for k in range(K)]
        c = Case(loss, A, b, xs, LAYOUTS[3])
        many = score_many(ctx, c.F, c.xs)
        assert "mscore_partial_kernel" in ctx.last_kernel()
        one = [score(ctx, c.F, x) for x in c.xs]
        A64, b64 = A.astype(np.float64), b.astype(np.float64)
        for k in range(K):
            assert type(many[k]) is type(one[k])
            if loss == "ls":
                delta, bound = general_bounds(loss, dtype, A64, b64, xs[k].astype(np.float64), N, d)
                assert abs(many[k].mse - one[k].mse) <= pair * bound["sum_r2"] / N
                assert abs(many[k].max_abs_residual - one[k].max_abs_residual) <= pair * bound["max_abs_r"]
                # r2 = 1 - sum r^2 / tss, tss = sum b^2 - (sum b)^2 / N from sums that each move by 2 N 2^-53 relative: first order
                tss = float(np.sum((b64 - b64.mean()) ** 2))
                dtss = 2 * N * 2.0 ** -53 * float(np.sum(b64 * b64) + 2 * np.sum(np.abs(b64)) ** 2 / N)
                sr2 = float(np.sum((A64 @ xs[k].astype(np.float64) - b64) ** 2))
                assert abs(many[k].r2 - one[k].r2) <= (pair * bound["sum_r2"] / tss + sr2 * dtss / tss ** 2) * (1 + 1e-6)
            else:
                delta, t = general_bounds(loss, dtype, A64, b64, xs[k].astype(np.float64), N, d)
                assert abs(many[k].log_loss - one[k].log_loss) <= pair * (float(np.sum(delta)) / N + 2 * N * 2.0 ** -52 * one[k].log_loss)
                assert abs(many[k].accuracy - one[k].accuracy) * N <= np.count_nonzero(np.abs(t) <= pair * delta)
                assert abs(many[k].min_margin - one[k].min_margin) <= pair * float(delta.max())
        assert 0 <= best(many) < K


def _entropy(t, s):
    e = np.exp(-np.abs(t))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    v, w = s * np.where(t >= 0, small, big), (1.0 - s) + s * np.where(t >= 0, big, small)
    xlogx = lambda q: np.where(q > 0, q * np.log(np.where(q > 0, q, 1.0)), 0.0)
    return float(np.sum(xlogx(v) + xlogx(w)))


@pytest.mark.parametrize("loss", ["ls", "logistic"])
def test_gaps_together_against_single_certificates(ctx, loss):
    """K certificates from two passes against K single Certificate(samples=True) results (fp64, N = 500, d = 50).  With gap =
    F (1-s)^2 + g + s x.grad (lasso) or F + g + E(s) / N (logistic) the two paths differ by
      * F and E: section 3's bounds on their sums (both sides device paths: the doubled delta covers the pair); for s < 1 the entropy's
        Lipschitz constant in t, sup_t s sigma(t) sigma(-t) |log(u / (1 - u))|, u = s sigma(-t), is taken from a dense grid instead of 0.23;
      * s = min(1, mu / ||grad||_inf) and x.grad: the K-wide gradient agrees with the single pass to tau = 48 eps |grad|_inf per
        coordinate (tests/test_gpu_multi_rhs.py), so |ds| <= s tau / (1 - tau) where s < 1 (mu is chosen away from ||grad||_inf: s is 1
        on both sides or below 1 on both) and |d x.grad| <= tau ||grad||_inf ||x||_1.  E is convex in s: its change over the interval of s
        is the larger of the two ends'."""
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd.certificate import gaps_together
    from ciaoalgorithms_jl_amd.device import PackedF, ProxG
    N, d, K, gamma = 500, 50, 4, 0.25
    A, b, x0 = P.synthetic(loss, N, d, np.float64, seed=31)
    lam = 1.0
    At, bt = torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda()
    F = PackedF.least_squares(At, bt, lam) if loss == "ls" else PackedF.logistic(At, bt)
    xs_h = [((0.25 + 0.5 * k) * x0) for k in range(K)]
    xs = [torch.from_numpy(x).cuda() for x in xs_h]
    ginf = [ctx.certificate(F, ProxG(), x, gamma).grad_inf for x in xs]
    mus = [ginf[k] * (2.0, 0.5, 0.125, 1.5)[k] for k in range(K)]
    gs = [ProxG(L.PROX_L1, lam=mu) for mu in mus]
    got = gaps_together(ctx, F, gs, xs, gamma)
    assert ctx.last_kernel().startswith("mscore_partial_kernel") and len(got) == K
    tau = 48 * float(np.finfo(np.float64).eps)
    grid = np.linspace(-60.0, 60.0, 240001)
    for k in range(K):
        one = ctx.certificate(F, gs[k], xs[k], gamma, samples=True)
        g = got[k]
        x64 = xs_h[k]
        s = min(1.0, mus[k] / one.grad_inf)
        assert (s == 1.0) == (k in (0, 3))
        ds = 0.0 if s == 1.0 else s * tau / (1 - tau)
        dxg = tau * one.grad_inf * float(np.sum(np.abs(x64)))
        if loss == "ls":
            _, bound = general_bounds(loss, np.float64, A, b, x64, N, d)
            dF = 0.5 * lam * bound["sum_r2"] / N + N * 2.0 ** -52 * abs(one.F)
            tol = (1 - s) ** 2 * dF + abs(one.x_dot_grad - 2 * one.F * (1 - s)) * ds + s * dxg + (2 * dF * ds + abs(one.F) * ds * ds + ds * dxg)
        else:
            delta, t = general_bounds(loss, np.float64, A, b, x64, N, d)
            sd = float(np.sum(delta))
            dF = sd / N + 2 * N * 2.0 ** -52 * abs(one.F)
            sp, sn = 1.0 / (1.0 + np.exp(-grid)), 1.0 / (1.0 + np.exp(grid))      # sigma(t), sigma(-t): neither is 0 on the grid
            uu = s * sn
            lip = 1.001 * float(np.max(s * sp * sn * np.abs(np.log(uu / (1.0 - uu))))) if s < 1.0 else 0.23
            E = _entropy(t, s)
            dEs = max(abs(_entropy(t, s + ds) - E), abs(_entropy(t, s - ds) - E)) if ds else 0.0
            tol = dF + (lip * sd + 2 * N * 2.0 ** -52 * abs(E) + dEs) / N
        scale = abs(one.F) + abs(one.g)
        print(f"{loss} model {k}: s = {s:.4f}  gap {g.gap:.12e} vs {one.gap:.12e}  |d gap| / scale {abs(g.gap - one.gap) / scale:.3e} <= {tol / scale:.3e}")
        assert math.isfinite(g.gap) and abs(g.gap - one.gap) / scale <= tol / scale, (k, g.gap, one.gap, tol)
        assert bits([[g.g]]) == bits([[one.g]]) and g.gap >= -tol
        assert abs(g.grad_inf - one.grad_inf) <= tau * one.grad_inf and abs(g.F - one.F) <= dF
    with pytest.raises(L.CiaoError):
        gaps_together(ctx, F, gs[:2], xs, gamma)
    with pytest.raises(L.CiaoError):
        gaps_together(ctx, F, gs, xs, 0.0)

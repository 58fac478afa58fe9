"""Step sizes from the data on the device (ciao_row_sqnorms, Context.row_sqnorms / row_sqnorm_stats, stepsize.py):
  1. the row sums of squares EXACTLY (bitwise) on a matrix of small integers, at every decision of rowsq_plan, in four layouts of the same
     matrix, with guards around the output; and around N = 2048 iterations' worth of rows, where the row loops make more than one trip;
  2. Gaussian rows against math.fsum, |out_i - ref_i| <= (d + 2) 2^-53 ref_i;
  3. the same bits between calls, contexts and layouts, for the vector and the four summary numbers;
  4. the summary: max, argmax (ties, in different workgroups), min, sum; out = NULL; inf; NaN;
  5. complex rows as their 2n reals;
  6. the constants of the two reference fixtures; SAGA and Finito with L= from the device; Finito's step sizes;
  7. smoothness: the Rayleigh quotient from below, the trace bound from above;
  8. refusals.

The thresholds of rowsq_plan (csrc/rowsq_kernels.h), in 16-byte chunks of a row (2 fp64 / 4 fp32 elements): the group width G doubles
at 1, 2, 4, 8, 16, 32 chunks; beyond 64 chunks a lane holds 2 (mode 1), beyond 128 up to 4 (mode 2), beyond 256 any number of chunks
(mode 3), beyond 512 its loop makes a second trip, beyond 1024 a third; beyond 4096 chunks (64 KiB) the four waves share a row.  D_SIZES
has one below, at and one above each of them for both types -- the list the issue suggests, plus 32, 512, 1023, 2047, 2048, 2049,
8191, 8192, 16383, 16384 where this plan's thresholds fall between its entries.  `plan` below restates rowsq_plan; every launch's report
(ctx.last_kernel()) is compared with it, so the thresholds tested are the library's own."""
import ctypes as C
import math

import numpy as np
import pytest

import problems as P

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
GUARD = 64


def tdtype(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


def tname(dtype):
    return "f64" if dtype == np.float64 else "f32"


def vec_of(dtype):
    return 2 if dtype == np.float64 else 4


def bits(t):
    import torch
    return t.view(torch.int64)


def fbits(x):
    return np.float64(x).view(np.int64)


def ls_problem(A):
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    return PackedF.least_squares(A, torch.zeros(A.shape[0], dtype=A.dtype, device=A.device), 1.0)


def plan(N, d, vec):
    """rowsq_plan of csrc/rowsq_kernels.h -> (G, mode, rows_per_wg, grid)"""
    chunks = -(-d // vec)
    if chunks > 4096:
        G, mode, step = 64, 4, 1
    else:
        G = 1
        while G < 64 and G < chunks:
            G *= 2
        trips = -(-chunks // G)
        mode = 0 if trips <= 1 else 1 if trips <= 2 else 2 if trips <= 4 else 3
        step = 4 * (8 >> mode) * (64 // G)
    want = -(-N // 2048)                               # ceil: the rows of a workgroup where 2048 of them share N ...
    per = max(step, -(-want // step) * step)           # ... in whole iterations
    return G, mode, per, -(-N // per)


def check_plan(ctx, N, d, dtype, F=None):
    """The launch's own report against `plan` -> the kind of load it used; with F: the kind its layout calls for"""
    G, mode, per, grid = plan(N, d, vec_of(dtype))
    k = ctx.last_kernel()
    assert k.startswith(f"rowsq_partial_kernel<{tname(dtype)},") and f" grid={grid} " in k and f" G={G} mode={mode} rows_per_wg={per}" in k, (k, G, mode, per, grid)
    kind = k.split(",")[1].split(">")[0]
    if F is not None:
        aligned = F.A.data_ptr() % 16 == 0 and (F.ld * F.A.element_size()) % 16 == 0
        assert kind == ("vec16" if aligned else "elem"), (k, F.ld)
    return kind


def layouts(A, dtype):
    """The same matrix four times: [(name, view)].  torch's allocations are 16-byte aligned, so the third layout takes 16-byte loads
    and the fourth element loads, whatever d is (a single row has no stride: its kind follows from the base alone)."""
    import torch
    N, d = A.shape
    vec = vec_of(dtype)
    nan = float("nan")
    out = [("ld=d", A)]
    wide = torch.full((N, d + 1), nan, dtype=A.dtype, device="cuda")
    wide[:, :d] = A
    out.append(("ld=d+1", wide[:, :d]))
    ldc = (d // vec + 1) * vec                      # whole chunks, and at least one padding column: all of them NaN
    padded = torch.full((N, ldc), nan, dtype=A.dtype, device="cuda")
    padded[:, :d] = A
    out.append(("ld=chunks", padded[:, :d]))
    flat = torch.full((N * d + vec,), nan, dtype=A.dtype, device="cuda")
    off = flat[1:1 + N * d].view(N, d)              # the base one element off 16-byte alignment
    off.copy_(A)
    assert off.data_ptr() % 16 == A.element_size()
    out.append(("base+1", off))
    return out


def guarded_call(ctx, F, N):
    """row_sqnorms into the middle of a NaN-filled buffer -> the N values; the 64 doubles on each side must still be NaN."""
    import torch
    buf = torch.full((N + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    out = ctx.row_sqnorms(F, out=buf[GUARD:GUARD + N])
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + N:]).all()), ("guard overwritten", ctx.last_kernel())
    return out


# ---- 1. exact on integers ------------------------------------------------------------------------------------------------------------------
D_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1000, 1023, 1024, 1025,
           2047, 2048, 2049, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 70001, 262147)
N_SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 257, 1000)
N_SIZES_LONG = (1, 2, 5)                          # d > 16384


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
@pytest.mark.parametrize("d", D_SIZES)
def test_integer_rows_exactly(ctx, d, dtype):
    """A[i,j] = ((7 i + 13 j) mod 11) - 5: every value, square and sum is exact in both types, and the pattern differs along rows and
    columns.  The rows of the smaller N are the first rows of the largest one."""
    import torch
    sizes = N_SIZES if d <= 16384 else N_SIZES_LONG
    Nmax = max(sizes)
    ints = (7 * np.arange(Nmax, dtype=np.int64)[:, None] + 13 * np.arange(d, dtype=np.int64)[None, :]) % 11 - 5
    want = torch.from_numpy((ints * ints).sum(axis=1).astype(np.float64)).cuda()
    A = torch.from_numpy(ints.astype(dtype)).cuda()
    kinds = set()
    for name, view in layouts(A, dtype):
        for N in sizes:
            F = ls_problem(view[:N])
            out = guarded_call(ctx, F, N)
            kinds.add((name, check_plan(ctx, N, d, dtype, F)))
            assert torch.equal(bits(out), bits(want[:N])), (name, N, d, ctx.last_kernel(), (out != want[:N]).nonzero()[:4].tolist())
    assert ("ld=chunks", "vec16") in kinds and ("base+1", "elem") in kinds


# rows_per_wg exceeds one iteration's rows only where N > 2048 iterations' worth: the row loops make a second (third) trip, the summary is
# carried from one trip to the next, and rows_per_wg is rounded up to whole iterations under the cap of 2048 records.  One below, at and
# one above 2048 * step, and one N of three trips, in every mode.
def _trip_cases():
    cases = []
    for d, dtype in ((3, np.float64), (255, np.float64), (1000, np.float32), (513, np.float64), (8193, np.float64)):      # modes 0, 1, 2, 3, split
        step = plan(1, d, vec_of(dtype))[2]
        edge = 2048 * step
        for N in (edge - 1, edge, edge + 1) + ((2 * edge + 2 * step + 1,) if d != 3 else ()):
            cases.append(pytest.param(N, d, dtype, id=f"{N}x{d}-{tname(dtype)}"))
    return cases


@pytest.mark.parametrize("N,d,dtype", _trip_cases())
def test_integer_rows_over_several_trips_of_the_row_loop(ctx, N, d, dtype):
    """The integer matrix again: `out` bitwise, and the summary EXACTLY -- every row sum is an integer and so is their total (< 2^53), so
    the sum has one right value in any order of addition; a row visited twice or skipped by a wrong stride changes it."""
    import torch
    G, mode, per, grid = plan(N, d, vec_of(dtype))
    step = plan(1, d, vec_of(dtype))[2]
    edge = 2048 * step
    assert (per, grid) == ((step, N // step + (N % step > 0)) if N <= edge else (2 * step, -(-N // (2 * step))) if N == edge + 1 else (3 * step, -(-N // (3 * step))))
    assert grid <= 2048
    ints = (7 * np.arange(N, dtype=np.int64)[:, None] + 13 * np.arange(d, dtype=np.int64)[None, :]) % 11 - 5
    rows = (ints * ints).sum(axis=1)
    want = torch.from_numpy(rows.astype(np.float64)).cuda()
    A = torch.from_numpy(ints.astype(dtype)).cuda()
    del ints
    views = layouts(A, dtype)
    for name, view in (views[0], views[3]):                 # ld = d, and the base one element off: both kinds of load at d = 1000, 8193 ...
        F = ls_problem(view)
        out = guarded_call(ctx, F, N)
        check_plan(ctx, N, d, dtype, F)
        assert torch.equal(bits(out), bits(want)), (name, N, d, ctx.last_kernel(), (out != want).nonzero()[:4].tolist())
        st = ctx.row_sqnorm_stats(F)
        assert (st.max, st.argmax, st.min) == (float(rows.max()), int(rows.argmax()), float(rows.min())), (name, st)
        assert st.sum == float(int(rows.sum())) and int(rows.sum()) < 2 ** 53, (name, st.sum, int(rows.sum()))
        ref = math.fsum(out.tolist())
        assert abs(st.sum - ref) <= (N + 2) * U53 * ref


# ---- 2. Gaussian rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
@pytest.mark.parametrize("N,d", [(65, 1), (65, 3), (65, 50), (33, 255), (33, 257), (33, 1000), (33, 1024), (33, 1025), (9, 4097), (9, 8193),
                                 (5, 16385), (3, 70001)])
def test_gaussian_rows_against_fsum(ctx, N, d, dtype):
    """|out_i - ref_i| <= (d + 2) 2^-53 ref_i, ref_i = math.fsum of the float64 squares: the terms are non-negative, there are d - 1
    additions in double and one rounding per square in fp64 (none in fp32), whatever the order of addition."""
    import torch
    rng = np.random.default_rng(1000 * d + N)
    A = rng.standard_normal((N, d)).astype(dtype)
    sq = A.astype(np.float64) ** 2
    ref = np.array([math.fsum(row) for row in sq])
    out = guarded_call(ctx, ls_problem(torch.from_numpy(A).cuda()), N).cpu().numpy()
    check_plan(ctx, N, d, dtype)
    frac = np.abs(out - ref) / ((d + 2) * U53 * ref)
    print(f"N={N} d={d} {tname(dtype)}: worst error / bound {frac.max():.4f}")
    assert (frac <= 1.0).all(), (N, d, float(frac.max()), ctx.last_kernel())


# ---- 3. the same bits ----------------------------------------------------------------------------------------------------------------------
def raw_both(ctx, F, out):
    """ciao_row_sqnorms with the vector AND the summary -> the four numbers"""
    from ciaoalgorithms_jl_amd import _lib as L
    stats = (C.c_double * 4)()
    L.check(ctx.lib.ciao_row_sqnorms(ctx._h, F.ref, C.c_void_p(out.data_ptr()), stats))
    return tuple(stats)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
@pytest.mark.parametrize("N,d", [(1100, 1000), (300, 1001), (3, 70001)])      # whole chunks (16-byte loads at ld = d); not; a row beyond 64 KiB
def test_the_bits_do_not_depend_on_call_context_or_layout(ctx, N, d, dtype):
    import torch
    from ciaoalgorithms_jl_amd.device import Context
    A = torch.from_numpy(np.random.default_rng(7 * N + d).standard_normal((N, d)).astype(dtype)).cuda()
    first = ctx.row_sqnorms(ls_problem(A))
    first_stats = ctx.row_sqnorm_stats(ls_problem(A))
    kinds = set()
    for name, view in layouts(A, dtype):
        F = ls_problem(view)
        assert torch.equal(bits(ctx.row_sqnorms(F)), bits(first)), (name, ctx.last_kernel())
        kinds.add(check_plan(ctx, N, d, dtype, F))
        st = ctx.row_sqnorm_stats(F)
        assert [fbits(v) for v in st] == [fbits(v) for v in first_stats], (name, st, first_stats)
    assert kinds == {"vec16", "elem"}
    assert torch.equal(bits(ctx.row_sqnorms(ls_problem(A))), bits(first))                 # a second call
    other = Context(0)
    try:
        assert torch.equal(bits(other.row_sqnorms(ls_problem(A))), bits(first))           # a second context
        st = other.row_sqnorm_stats(ls_problem(A))
        assert [fbits(v) for v in st] == [fbits(v) for v in first_stats]
        other.synchronize()
    finally:
        other.close()


# ---- 4. the summary ------------------------------------------------------------------------------------------------------------------------
def summary_sizes(dtype):
    """d = 3: one workgroup takes `per` rows at the least.  1, 255, 256, 257 (inside one workgroup: lanes, waves and iterations of it);
    one below, at and one above the first workgroup boundary; several workgroups; and 256 records + 1, one more than a single pass of
    rowsq_final_kernel's 256 threads."""
    per = plan(1, 3, vec_of(dtype))[2]
    return (1, 255, 256, 257, per - 1, per, per + 1, 3 * per + 5, 256 * per + 1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
@pytest.mark.parametrize("k", range(9))
def test_summary(ctx, k, dtype):
    import torch
    d = 3
    N = summary_sizes(dtype)[k]
    per = plan(N, d, vec_of(dtype))[2]
    A = np.random.default_rng(50 + k).standard_normal((N, d)).astype(dtype)
    # the maximum three times: in the first workgroup, in the last, and between them where there is room -- never first in its workgroup
    big = np.array([10.0, -10.0, 10.0], dtype)
    ties = sorted({min(N - 1, per // 3), min(N - 1, per + 7), N - 1})
    A[ties] = big
    At = torch.from_numpy(A).cuda()
    F = ls_problem(At)
    out = ctx.row_sqnorms(F)
    check_plan(ctx, N, d, dtype)
    st = ctx.row_sqnorm_stats(F)                                                          # out = NULL
    assert "+final" in ctx.last_kernel()
    if k == 8:
        assert plan(N, d, vec_of(dtype))[3] == 257
    assert fbits(st.max) == fbits(float(out.max())) == fbits(300.0)
    assert fbits(st.min) == fbits(float(out.min()))
    assert st.argmax == ties[0] == int((out == out.max()).nonzero()[0])
    ref = math.fsum(out.tolist())
    print(f"N={N} {tname(dtype)}: sum error / bound {abs(st.sum - ref) / ((N + 2) * U53 * ref):.4f}")
    assert abs(st.sum - ref) <= (N + 2) * U53 * ref
    # with the vector: the same four numbers, bitwise, and the same vector
    out2 = torch.empty_like(out)
    both = raw_both(ctx, F, out2)
    assert [fbits(v) for v in both] == [fbits(st.max), fbits(float(st.argmax)), fbits(st.min), fbits(st.sum)]
    assert torch.equal(bits(out2), bits(out))
    # the tie moved: only the later rows hold the maximum
    if len(ties) > 1:
        A2 = At.clone()
        A2[ties[0]] = 0.0
        st2 = ctx.row_sqnorm_stats(ls_problem(A2))
        assert st2.argmax == ties[1] and st2.max == 300.0 and st2.min == 0.0
    # one row holding inf: max = inf, only that row
    j = (2 * N) // 3
    Ai = At.clone()
    Ai[j, d - 1] = float("-inf")
    oi, si = ctx.row_sqnorms(ls_problem(Ai)), ctx.row_sqnorm_stats(ls_problem(Ai))
    assert si.max == math.inf and si.argmax == j and si.sum == math.inf and math.isinf(float(oi[j]))
    keep = torch.ones(N, dtype=torch.bool, device="cuda")
    keep[j] = False
    assert torch.equal(bits(oi[keep]), bits(out[keep]))
    # one NaN: max and sum NaN, and only that row of out
    An = At.clone()
    An[j, 0] = float("nan")
    on, sn = ctx.row_sqnorms(ls_problem(An)), ctx.row_sqnorm_stats(ls_problem(An))
    assert math.isnan(sn.max) and math.isnan(sn.sum) and sn.argmax == j
    assert bool(torch.isnan(on[j])) and torch.equal(bits(on[keep]), bits(out[keep]))


# ---- 5. complex rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
@pytest.mark.parametrize("N,n", [(7, 3), (70, 129), (5, 1000)])
def test_complex_rows_are_their_reals(ctx, N, n, dtype):
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    rng = np.random.default_rng(N + n)
    pairs = torch.from_numpy(rng.standard_normal((N, 2 * n)).astype(dtype)).cuda()
    Fc = PackedF.least_squares_complex(pairs, torch.zeros(2 * N, dtype=pairs.dtype, device="cuda"), 2.0)
    got = ctx.row_sqnorms(Fc)
    assert torch.equal(bits(got), bits(ctx.row_sqnorms(ls_problem(pairs))))
    z = pairs.double().cpu().numpy()
    ref = np.array([math.fsum(r) for r in z * z])
    assert (np.abs(got.cpu().numpy() - ref) <= (2 * n + 2) * U53 * ref).all()


# ---- 6. the constants, and through the solvers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
def test_constants_of_the_reference_fixtures(ctx, ciao, dtype):
    """Within 4 eps of the dtype, relative: both sides round a sum of a few terms and one product (fp32: the fixture's L comes from the
    float64 matrix, the device's from its float32 rounding, 2^-24 per element)."""
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    from ciaoalgorithms_jl_amd.host_route import host_lipschitz
    from ciaoalgorithms_jl_amd.stepsize import lipschitz, lipschitz_max, lipschitz_range
    eps = float(np.finfo(dtype).eps)
    A, b, Lc, lam, x0, x_star, f_star = P.lasso_known_answer(dtype=dtype)
    N = A.shape[0]
    F = PackedF.least_squares(torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda(), float(N))      # test_lasso.jl:52-54, lam = N
    got = lipschitz(ctx, F)
    assert got.dtype == tdtype(dtype) and got.shape == (N,) and got.is_cuda
    assert (np.abs(got.cpu().numpy().astype(np.float64) - Lc.astype(np.float64)) <= 4 * eps * Lc.astype(np.float64)).all()
    twin = host_lipschitz("ls", A, float(N))
    assert (np.abs(got.cpu().numpy().astype(np.float64) - twin) <= 4 * eps * twin).all()
    r = lipschitz_range(ctx, F)
    full = (ctx.row_sqnorms(F) * float(N)).cpu().numpy()
    assert r.max == full.max() == lipschitz_max(ctx, F) and r.min == full.min() and r.argmax == int(full.argmax())
    A, y, Lc, lam, x0, x_star = P.logistic_fixture(dtype)
    F = PackedF.logistic(torch.from_numpy(A).cuda(), torch.from_numpy(y).cuda())
    got = lipschitz(ctx, F).cpu().numpy()
    assert got.dtype == dtype
    assert (np.abs(got.astype(np.float64) - Lc.astype(np.float64)) <= 4 * eps * Lc.astype(np.float64)).all()
    # a complex LeastSquares problem: lam times the sum over the 2n reals
    Ac, bc, _ = P.synthetic_complex(9, 5, np.complex128 if dtype == np.float64 else np.complex64)
    pairs = torch.view_as_real(torch.from_numpy(Ac).cuda()).reshape(9, 10).contiguous()
    Fc = PackedF.least_squares_complex(pairs, torch.view_as_real(torch.from_numpy(bc).cuda()).reshape(18).contiguous(), 9.0)
    ref = host_lipschitz("ls", Ac, 9.0)
    assert (np.abs(lipschitz(ctx, Fc).cpu().numpy().astype(np.float64) - ref) <= (10 + 4) * eps * ref).all()    # 10 terms a side, one product, one cast


def test_saga_and_finito_with_L_from_the_device(ctx, ciao):
    """The lasso fixture in fp64 with nothing computed on the host: iteration count and tolerance of the same fixture's tests,
    tests/test_gpu_solvers.py:162 (maxit, tol = 1000, 1e-4 on cost(x) - f_star; :168-169 Finito, :249-250 SAGA)."""
    import torch
    import ciaoalgorithms_jl_amd.operators as ops
    import ciaoalgorithms_jl_amd.solvers as S
    from ciaoalgorithms_jl_amd.device import PackedF
    from ciaoalgorithms_jl_amd.stepsize import lipschitz, lipschitz_max
    maxit, tol = 1000, 1e-4
    A, b, Lc, lam, x0, x_star, f_star = P.lasso_known_answer(dtype=np.float64)
    N = A.shape[0]
    Fp = PackedF.least_squares(torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda(), float(N))
    cost = lambda x: P.lasso_cost(A, b, lam, x)
    Ld = lipschitz(ctx, Fp)
    x, it = S.SAGA(np.float64, maxit=maxit)(x0, F=Fp, g=ops.NormL1(lam), L=lipschitz_max(ctx, Fp), N=N, ctx=ctx)
    print(f"SAGA: cost - f_star {cost(x) - f_star:.3e}, |x - x_star| {np.abs(x - x_star).max():.3e}")
    assert cost(x) - f_star < tol and x.dtype == np.float64
    x, it = S.Finito(np.float64, maxit=maxit)(x0, F=Fp, g=ops.NormL1(lam), L=Ld, N=N, ctx=ctx)
    print(f"Finito: cost - f_star {cost(x) - f_star:.3e}, |x - x_star| {np.abs(x - x_star).max():.3e}")
    assert cost(x) - f_star < tol and x.dtype == np.float64
    # Finito's step sizes are alpha N / L_i, formed from the device vector
    alpha = 0.999
    state = next(iter(S.iterator(S.Finito(np.float64, α=alpha), x0, F=Fp, g=ops.NormL1(lam), L=Ld, N=N, ctx=ctx)))
    assert state.γ.is_cuda and torch.equal(state.γ, (np.float64(alpha) * np.float64(N)) / Ld)
    assert torch.equal(Ld, lipschitz(ctx, Fp))                                           # (the solver did not write into it)


def test_a_context_on_a_stream_of_its_own(ciao, ctx):
    """torch's multiply / cast / dot in stepsize.py follow the library's kernels on the context's stream, not on torch's current one"""
    import torch
    from ciaoalgorithms_jl_amd.device import Context
    from ciaoalgorithms_jl_amd.stepsize import lipschitz, smoothness
    A = torch.from_numpy(np.random.default_rng(77).standard_normal((20000, 260))).cuda()
    F = ls_problem(A)
    want, (est, upper) = lipschitz(ctx, F), smoothness(ctx, F)
    torch.cuda.synchronize()
    own = Context(0, stream=torch.cuda.Stream())
    try:
        got = lipschitz(own, F)
        own.synchronize()
        assert torch.equal(bits(got), bits(want))
        assert smoothness(own, F) == (est, upper)
    finally:
        own.synchronize()
        own.close()


# ---- 7. smoothness ----------------------------------------------------------------------------------------------------------------------------
def planted(dtype, seed=0):
    """A = 3 u v' + Gaussian / sqrt(d) at (N, d) = (200, 40), u a unit vector, v standard normal"""
    N, d = 200, 40
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(N)
    u /= np.linalg.norm(u)
    v = rng.standard_normal(d)
    return (3.0 * np.outer(u, v) + rng.standard_normal((N, d)) / np.sqrt(d)).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
@pytest.mark.parametrize("loss", ["ls", "logistic"])
def test_smoothness(ctx, ciao, loss, dtype):
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    from ciaoalgorithms_jl_amd.stepsize import smoothness
    A = planted(dtype)
    N, d = A.shape
    w = np.linalg.eigvalsh(A.astype(np.float64).T @ A.astype(np.float64))
    assert w[-2] / w[-1] <= 0.5, "choose another seed: the second eigenvalue of A'A is too close to the first"    # a condition on the input
    At = torch.from_numpy(A).cuda()
    if loss == "ls":
        lam = 2.5
        F, c = PackedF.least_squares(At, torch.ones(N, dtype=At.dtype, device="cuda"), lam), lam / N
    else:
        F, c = PackedF.logistic(At, torch.ones(N, dtype=At.dtype, device="cuda")), 0.25 / N
    true = c * w[-1]
    rtol = 1e-6
    est, upper = smoothness(ctx, F, iters=50, rtol=rtol, seed=0)
    eps = float(np.finfo(dtype).eps)
    print(f"{loss} {tname(dtype)}: estimate / true - 1 = {est / true - 1:.3e}, upper / true = {upper / true:.3f}")
    assert est <= true * (1 + 8 * eps * d)
    assert est >= true * (1 - 10 * rtol)
    assert upper >= true
    assert upper == c * ctx.row_sqnorm_stats(F).sum


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, ciao):
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd.device import Context, PackedF, PackedSepQuad
    from ciaoalgorithms_jl_amd.stepsize import lipschitz, lipschitz_max, smoothness
    f64 = dict(dtype=torch.float64, device="cuda")
    A = torch.randn((9, 8), **f64)
    F = PackedF.least_squares(A, torch.randn(9, **f64), 1.0)
    Fc = PackedF.least_squares_complex(torch.randn((4, 8), **f64), torch.randn(8, **f64), 4.0)
    Fz = PackedF.zero(4, 8, torch.float64)
    F0 = PackedF.logistic(torch.empty((0, 8), **f64), torch.empty(0, **f64), N_total=4)     # a rank that holds no row
    Fs = PackedSepQuad(torch.ones((3, 4), **f64), torch.ones((3, 4), **f64))
    Fshard = PackedF.least_squares(A, torch.randn(9, **f64), 1.0, N_total=18)
    x, out9 = torch.zeros(8, **f64), torch.zeros(9, **f64)
    ctx.full_gradient(F, x, torch.empty_like(x))
    before = ctx.last_kernel()
    assert not before.startswith("rowsq_")
    lib, h = ctx.lib, ctx._h
    stats = (C.c_double * 4)()

    def raw(status):
        if status != L.OK:
            raise L.CiaoError(status, lib.ciao_last_error().decode())

    hooked = Context(0)
    hooked.full_gradient(F, x, torch.empty_like(x))
    hooked.synchronize()
    hooked.set_allreduce(lambda buf, count, dtype, stream: 0)
    before_hooked = hooked.last_kernel()
    try:
        cases = [("Zero", lambda: ctx.row_sqnorms(Fz)), ("Zero stats", lambda: ctx.row_sqnorm_stats(Fz)),
                 ("sharing", lambda: ctx.row_sqnorms(Fs)), ("sharing stats", lambda: ctx.row_sqnorm_stats(Fs)),
                 ("N = 0", lambda: ctx.row_sqnorms(F0)), ("N = 0 stats", lambda: ctx.row_sqnorm_stats(F0)),
                 ("both NULL", lambda: raw(lib.ciao_row_sqnorms(h, F.ref, None, None))),
                 ("NULL problem", lambda: raw(lib.ciao_row_sqnorms(h, None, C.c_void_p(out9.data_ptr()), stats))),
                 ("NULL ctx", lambda: raw(lib.ciao_row_sqnorms(None, F.ref, C.c_void_p(out9.data_ptr()), stats))),
                 ("lipschitz Zero", lambda: lipschitz(ctx, Fz)), ("lipschitz sharing", lambda: lipschitz(ctx, Fs)),
                 ("lipschitz_max sharing", lambda: lipschitz_max(ctx, Fs)),
                 ("smoothness complex", lambda: smoothness(ctx, Fc)), ("smoothness Zero", lambda: smoothness(ctx, Fz)),
                 ("smoothness sharing", lambda: smoothness(ctx, Fs)), ("smoothness row shard", lambda: smoothness(ctx, Fshard)),
                 ("smoothness hook", lambda: smoothness(hooked, F))]
        for what, call in cases:
            with pytest.raises(L.CiaoError) as e:
                call()
            assert e.value.status == L.ERR_ARG, what
            assert ctx.last_kernel() == before and hooked.last_kernel() == before_hooked, what
        assert "row-sharded" in str(e.value)
        with pytest.raises(ValueError):
            ctx.row_sqnorms(F, out=torch.zeros(9, dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError):
            ctx.row_sqnorms(F, out=torch.zeros(8, **f64))
        assert ctx.last_kernel() == before
        # on the context with the hook the row pass itself works, on the local rows
        want = ctx.row_sqnorms(F)
        assert torch.equal(bits(hooked.row_sqnorms(F)), bits(want)) and hooked.last_kernel().startswith("rowsq_")
        assert hooked.row_sqnorm_stats(Fshard) == ctx.row_sqnorm_stats(F)
        # ... and with the hook taken off the same context estimates
        hooked.set_allreduce(None)
        est, upper = smoothness(hooked, F)
        assert 0 < est <= upper * (1 + 1e-12)
    finally:
        hooked.synchronize()
        hooked.close()
    ctx.synchronize()

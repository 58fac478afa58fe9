"""Column standardisation on the device (ciao_col_moments, ciao_scale_columns, Context.col_moments / scale_columns, standardize.py;
DESIGN.md section 8.10):
  1. the shifted column sums EXACTLY (bitwise) on integer matrices, |a| <= 64, against numpy int64 arithmetic, with an integer shift and
     with shift = NULL, one below / at / one above every threshold of colmom_plan, in four layouts of the same matrix, NaN in every
     padding column and NaN guards around both outputs; the launch's own report against a restatement of the plan;
  2. Gaussian columns (one with mean 10^6 sigma, one whose first row is 10^8) against math.fsum and fractions.Fraction with the derived
     bounds |s1 - exact| <= (N + 2) 2^-53 sum|a - c|, |s2 - exact| <= (N + 3) 2^-53 sum (a - c)^2; the refinement rule; var after it;
  3. the scaling bitwise against numpy's ((A.astype(f64) - c) * s).astype(T) for Gaussian and integer matrices at the same thresholds and
     layouts: out of place with ld_out != ld, in place, NULL center / NULL scale, padding columns and guards untouched;
  4. standardize / Scaler through the public interface; 5. refusals.

The thresholds of colmom_plan (csrc/colmom_kernels.h) in 16-byte chunks of a row (VEC = 2 fp64 / 4 fp32 elements): the column threads tc
of a workgroup double at 1, 2, ..., 128 chunks and stay 256 beyond; past 256 chunks a row takes a second panel, past 512 a third.  A
workgroup holds tr = 256 / tc row groups of 8 rows in flight: N = 8 tr is one unrolled trip, a slab is 32 tr rows at the least."""
import ctypes as C
import math
from fractions import Fraction

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
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def problem(A, kind="ls"):
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    b = torch.ones(A.shape[0], dtype=A.dtype, device=A.device)
    return PackedF.least_squares(A, b, 1.0) if kind == "ls" else PackedF.logistic(A, b)


def plan(N, d, vec):
    """colmom_plan of csrc/colmom_kernels.h -> (tc, panels, slab, nslab)"""
    chunks = -(-d // vec)
    tc = 1
    while tc < 256 and tc < chunks:
        tc *= 2
    panels = -(-chunks // tc)
    step = (256 // tc) * 8
    want = max(1, min(2048 // panels, (32 << 20) // (16 * d)))
    slab = max(4 * step, -(-(-(-N // want)) // step) * step)
    return tc, panels, slab, max(1, -(-N // slab))


def d_sizes(dtype):
    vec = vec_of(dtype)
    ds = {1, 2, 3, 256 * vec + 1, 2 * 256 * vec + 1}
    for k in range(9):
        ds |= {vec * 2 ** k - 1, vec * 2 ** k, vec * 2 ** k + 1}
    return sorted(v for v in ds if v >= 1)


def n_sizes(d, dtype):
    """1; one below, at, one above one unrolled trip; one slab, two slabs; 33 slabs (the final kernel's unrolled loop, all four quarters)"""
    tc = plan(1, d, vec_of(dtype))[0]
    step = (256 // tc) * 8
    ns = sorted({1, step - 1, step, step + 1, 4 * step, 4 * step + 1, 128 * step + 1})
    assert [plan(n, d, vec_of(dtype))[3] for n in ns[-3:]] == [1, 2, 33]
    return ns


def cases():
    return [pytest.param(d, dt, id=f"{d}-{tname(dt)}") for dt in (np.float32, np.float64) for d in d_sizes(dt)]


class Layout:
    """An (N, d) matrix inside a NaN-filled flat buffer: GUARD elements on either side, row stride ld, the base `off` elements past a
    16-byte boundary.  view[:n] is the first n rows in the same layout."""

    def __init__(self, M, ld, off, name):
        import torch
        N, d = M.shape
        self.name, self.ld, self.N, self.d = name, ld, N, d
        self.flat = torch.full((2 * GUARD + off + N * ld,), float("nan"), dtype=M.dtype, device="cuda")
        self.view = torch.as_strided(self.flat, (N, d), (ld, 1), GUARD + off)
        self.view.copy_(M)
        assert self.view.data_ptr() % 16 == (off * M.element_size()) % 16

    def rows(self, n):
        return self.view[:n]


def layouts(M, dtype):
    d, vec = M.shape[1], vec_of(dtype)
    return [Layout(M, d, 0, "ld=d"), Layout(M, d + 3, 0, "ld=d+3"), Layout(M, d, 1, "base+1"), Layout(M, (d // vec + 1) * vec, 0, "ld=chunks")]


def kind_of(F):
    return "vec16" if F.A.data_ptr() % 16 == 0 and (F.ld * F.A.element_size()) % 16 == 0 else "elem"


def check_report(ctx, what, N, d, dtype, kind, tail):
    tc, panels, slab, nslab = plan(N, d, vec_of(dtype))
    want = f"{what}<{tname(dtype)},{kind}> grid={panels}x{nslab} block=256 tc={tc} slab={slab}{tail}"
    assert ctx.last_kernel() == want, (ctx.last_kernel(), want)


def guarded_moments(ctx, F, shift):
    """col_moments into the middle of two NaN-filled buffers -> (s1, s2); the 64 doubles on either side of both must still be NaN"""
    import torch
    d = F.d
    buf = torch.full((2, d + 2 * GUARD), float("nan"), dtype=torch.float64, device="cuda")
    s1, s2 = ctx.col_moments(F, shift, s1=buf[0, GUARD:GUARD + d], s2=buf[1, GUARD:GUARD + d])
    assert bool(torch.isnan(buf[:, :GUARD]).all()) and bool(torch.isnan(buf[:, GUARD + d:]).all()), ("guard overwritten", ctx.last_kernel())
    return s1, s2


def int_matrix(N, d):
    """A[i,j] = ((7 i + 13 j) mod 129) - 64: |a| <= 64, the pattern differs along rows and columns"""
    return (7 * np.arange(N, dtype=np.int64)[:, None] + 13 * np.arange(d, dtype=np.int64)[None, :]) % 129 - 64


# ---- 1. exact on integers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dtype", cases())
def test_integer_columns_exactly(ctx, d, dtype):
    import torch
    sizes = n_sizes(d, dtype)
    ints = int_matrix(sizes[-1], d)
    cint = np.arange(d, dtype=np.int64) % 7 - 3
    shift = torch.from_numpy(cint.astype(np.float64)).cuda()
    want = {}
    for N in sizes:
        for key, c in (("given", cint), ("row0", ints[0])):
            t = ints[:N] - c[None, :]
            s2 = (t * t).sum(axis=0)
            assert int(s2.max()) < 2 ** 53
            want[N, key] = tuple(torch.from_numpy(v.astype(np.float64)).cuda() for v in (t.sum(axis=0), s2))
    M = torch.from_numpy(ints.astype(dtype)).cuda()
    kinds = set()
    for lay in layouts(M, dtype):
        for N in sizes:
            F = problem(lay.rows(N))
            for key, sh in (("given", shift), ("row0", None)):
                s1, s2 = guarded_moments(ctx, F, sh)
                check_report(ctx, "colmom_partial_kernel", N, d, dtype, kind_of(F), f" shift={key}")
                assert torch.equal(bits(s1), bits(want[N, key][0])), (lay.name, N, d, key, ctx.last_kernel())
                assert torch.equal(bits(s2), bits(want[N, key][1])), (lay.name, N, d, key, ctx.last_kernel())
            kinds.add((lay.name, kind_of(F)))
    assert ("ld=chunks", "vec16") in kinds and ("base+1", "elem") in kinds


def test_a_logistic_problem_a_second_call_and_a_second_context_give_the_same_bits(ctx):
    import torch
    from ciaoalgorithms_jl_amd.device import Context
    A = torch.from_numpy(np.random.default_rng(5).standard_normal((2100, 70)).astype(np.float32)).cuda()
    first = ctx.col_moments(problem(A))
    for again in (ctx.col_moments(problem(A)), ctx.col_moments(problem(A, "logistic"))):
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again, first))
    other = Context(0)
    try:
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(other.col_moments(problem(A)), first))
        other.synchronize()
    finally:
        other.close()


# ---- 2. Gaussian columns -------------------------------------------------------------------------------------------------------------------
ROUND_N = 4099
EXACT_COLS = lambda d: (0, 1, 2, d // 2, d - 1)     # Gaussian, mean 10^6 sigma, first row 10^8, Gaussian, the last (partial) chunk
_GAUSS = {}


def gauss_case(d, dtype):
    """(plain, spike, reference): plain = Gaussian columns, column 1 with mean 10^6 sigma; spike = plain with A[0, 2] = 10^8.  reference:
    for the spike matrix and c = its first row, per column fsum of the double terms, and for EXACT_COLS the exact rational sums and the
    exact population variance.  Computed once, shared, never modified."""
    if (d, dtype) not in _GAUSS:
        rng = np.random.default_rng(4099 + d)
        plain = rng.standard_normal((ROUND_N, d))
        plain[:, 1] += 1e6
        plain = plain.astype(dtype)
        spike = plain.copy()
        spike[0, 2] = 1e8
        A = spike.astype(np.float64)
        t = A - A[0][None, :]
        ref = dict(s1=np.array([math.fsum(col) for col in t.T.tolist()]), s2=np.array([math.fsum(col) for col in (t * t).T.tolist()]),
                   abs1=np.abs(t).sum(axis=0), exact={})
        for j in EXACT_COLS(d):
            col = [Fraction(v) for v in A[:, j].tolist()]
            diff = [v - col[0] for v in col]
            mean = sum(col) / ROUND_N
            ref["exact"][j] = (sum(diff), sum(v * v for v in diff), sum((v - mean) ** 2 for v in col) / ROUND_N)
        for v in (plain, spike):
            v.setflags(write=False)
        _GAUSS[d, dtype] = (plain, spike, ref)
    return _GAUSS[d, dtype]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
@pytest.mark.parametrize("d", [50, 257])
def test_gaussian_columns_against_fsum_and_fractions(ctx, d, dtype):
    """The bounds are derived: a - c is rounded once, there are N - 1 additions in double (s2: one more rounding for the square), whatever
    the order of addition; second-order terms are far below the slack of 2 / 3 units."""
    import torch
    plain, spike, ref = gauss_case(d, dtype)
    N = ROUND_N
    F = problem(torch.from_numpy(spike.copy()).cuda())
    s1, s2 = (v.cpu().numpy() for v in guarded_moments(ctx, F, None))
    check_report(ctx, "colmom_partial_kernel", N, d, dtype, kind_of(F), " shift=row0")
    b1, b2 = (N + 2) * U53 * ref["abs1"], (N + 3) * U53 * ref["s2"]
    f1, f2 = np.abs(s1 - ref["s1"]) / b1.clip(1e-300), np.abs(s2 - ref["s2"]) / b2.clip(1e-300)
    for j, (e1, e2, _) in ref["exact"].items():
        x1 = float(abs(Fraction(float(s1[j])) - e1) / Fraction(float(b1[j]))) if b1[j] else 0.0
        x2 = float(abs(Fraction(float(s2[j])) - e2) / Fraction(float(b2[j]))) if b2[j] else 0.0
        f1[j], f2[j] = max(f1[j], x1), max(f2[j], x2)
    print(f"N={N} d={d} {tname(dtype)}: worst |s1 - exact| / bound {f1.max():.3e}, worst |s2 - exact| / bound {f2.max():.3e}")
    assert (f1 <= 1.0).all() and (f2 <= 1.0).all(), (float(f1.max()), float(f2.max()), ctx.last_kernel())


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
@pytest.mark.parametrize("d", [50, 257])
def test_refinement(ctx, d, dtype):
    import torch
    from ciaoalgorithms_jl_amd.standardize import column_moments, host_column_moments
    plain, spike, ref = gauss_case(d, dtype)
    Fp, Fs = problem(torch.from_numpy(plain.copy()).cuda()), problem(torch.from_numpy(spike.copy()).cuda())
    assert column_moments(ctx, Fp).passes == 1                      # Gaussian columns and the one with mean 10^6 sigma: s2 / M2 is 1 - 3
    m = column_moments(ctx, Fs)
    assert m.passes == 2 and m.n == ROUND_N                          # the first row of column 2 is 10^8: s2 / M2 is about N
    assert column_moments(ctx, Fs, refine=False).passes == 1 and column_moments(ctx, Fp, refine=True).passes == 2
    assert host_column_moments(plain).passes == 1 and host_column_moments(spike).passes == 2
    var, mean = m.var.cpu().numpy(), m.mean.cpu().numpy()
    worst = 0.0
    for j, (_, _, v) in ref["exact"].items():
        rel = float(abs(Fraction(float(var[j])) - v) / v)
        worst = max(worst, rel)
        assert rel <= 64 * U53, (j, rel / U53)
    print(f"d={d} {tname(dtype)}: var after refinement, worst relative error {worst / U53:.2f} x 2^-53")
    h = host_column_moments(spike)
    assert np.allclose(mean, h.mean, rtol=1e-14, atol=1e-12) and np.allclose(var, h.var, rtol=1e-12)
    # a given shift: the same moments as the default one to rounding
    sh = torch.from_numpy(spike.astype(np.float64).mean(axis=0)).cuda()
    g = column_moments(ctx, Fs, shift=sh)
    assert g.passes == 1 and np.allclose(g.var.cpu().numpy(), var, rtol=1e-12)


# ---- 3. the scaling ------------------------------------------------------------------------------------------------------------------------
def scale_inputs(kind, N, d, dtype):
    rng = np.random.default_rng(100 * d + (1 if dtype == np.float64 else 0))
    A = int_matrix(N, d).astype(dtype) if kind == "int" else rng.standard_normal((N, d)).astype(dtype)
    return A, rng.standard_normal(d), np.exp(rng.standard_normal(d))


@pytest.mark.parametrize("kind", ["gauss", "int"])
@pytest.mark.parametrize("d,dtype", cases())
def test_scaling_bitwise(ctx, d, dtype, kind):
    import torch
    sizes = n_sizes(d, dtype)
    A, c, s = scale_inputs(kind, sizes[-1], d, dtype)
    ref = torch.from_numpy(((A.astype(np.float64) - c) * s).astype(dtype)).cuda()
    cd, sd = torch.from_numpy(c).cuda(), torch.from_numpy(s).cuda()
    M = torch.from_numpy(A).cuda()
    nan = float("nan")
    for lay in layouts(M, dtype):
        orig = lay.flat.clone()
        target = Layout(M, d + 5, 0, "out")                          # ld_out != ld, NaN in its padding and guards
        for N in sizes:
            F = problem(lay.rows(N))
            # out of place: the first N rows of `target` become the reference, nothing else of its buffer changes (its rows held A)
            expect = target.flat.clone()
            torch.as_strided(expect, (N, d), (target.ld, 1), GUARD).copy_(ref[:N])
            out = ctx.scale_columns(F, cd, sd, out=target.rows(N))
            both16 = kind_of(F) == "vec16" and (N == 1 or ((d + 5) * M.element_size()) % 16 == 0)
            check_report(ctx, "colscale_kernel", N, d, dtype, "vec16" if both16 else "elem", "")
            assert out.data_ptr() == target.view.data_ptr()
            assert torch.equal(bits(target.flat), bits(expect)), (lay.name, N, d, ctx.last_kernel())
            assert torch.equal(bits(lay.flat), bits(orig)), "the input was written"
            target.view[:N].copy_(M[:N])
            # in place: the same bits over A itself; rows beyond N, padding columns and guards keep theirs
            expect = orig.clone()
            torch.as_strided(expect, (N, d), (lay.ld, 1), lay.view.storage_offset()).copy_(ref[:N])
            got = ctx.scale_columns(F, cd, sd, inplace=True)
            check_report(ctx, "colscale_kernel", N, d, dtype, kind_of(F), " in place")
            assert got.data_ptr() == F.A.data_ptr()
            assert torch.equal(bits(lay.flat), bits(expect)), (lay.name, N, d, ctx.last_kernel())
            lay.flat.copy_(orig)
        # NULL center / NULL scale / both, at the largest N
        F = problem(lay.view)
        A64 = A.astype(np.float64)
        for cc, ss, want in ((None, sd, (A64 * s)), (cd, None, (A64 - c)), (None, None, A64)):
            got = ctx.scale_columns(F, cc, ss)
            assert got.shape == (sizes[-1], d) and got.is_contiguous()
            assert torch.equal(bits(got), bits(torch.from_numpy(want.astype(dtype)).cuda())), (lay.name, cc is None, ss is None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
def test_a_constant_column_centred_is_exactly_zero(ctx, dtype):
    import torch
    from ciaoalgorithms_jl_amd.standardize import standardize
    rng = np.random.default_rng(3)
    A = rng.standard_normal((2053, 9)).astype(dtype)
    A[:, 4] = dtype(0.1) * 3                                         # not representable as a short binary fraction
    A[:, 7] = 0.0
    A[0, 2] = 1e8                                                    # forces the second pass for the whole matrix
    F = problem(torch.from_numpy(A).cuda())
    F_std, sc = standardize(ctx, F)
    out = F_std.A.cpu().numpy()
    assert not out[:, 4].any() and not out[:, 7].any() and not np.signbit(out[:, 4]).any()
    assert sc.scale[4].item() == 1.0 and sc.scale[7].item() == 1.0 and sc.mean[4].item() == float(A[0, 4])
    assert np.isfinite(out).all()


# ---- 4. through the public interface -------------------------------------------------------------------------------------------------
_LASSO = {}


def lasso_case(dtype):
    """A (1000, 50) lasso problem of tests/problems.py whose columns have different scales and offsets (so that standardising it does
    something), and its float64 numpy standardisation.  Shared, never modified."""
    if dtype not in _LASSO:
        from ciaoalgorithms_jl_amd.host_route import host_standardize
        A, b, _ = P.synthetic("ls", 1000, 50, np.float64, seed=11)
        rng = np.random.default_rng(12)
        A = (A * np.exp(2.0 * rng.standard_normal(50))[None, :] + rng.standard_normal(50)[None, :]).astype(dtype)
        b = (b + 3.0).astype(dtype)
        host = host_standardize(A.astype(np.float64), b.astype(np.float64))
        for v in (A, b) + tuple(h for h in host if isinstance(h, np.ndarray)):
            v.setflags(write=False)
        _LASSO[dtype] = (A, b, host)
    return _LASSO[dtype]


def device_lasso(dtype):
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    A, b, host = lasso_case(dtype)
    return PackedF.least_squares(torch.from_numpy(A.copy()).cuda(), torch.from_numpy(b.copy()).cuda(), 1.0), host


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
def test_standardize(ctx, ciao, dtype):
    import torch
    from ciaoalgorithms_jl_amd.host_route import host_standardize
    from ciaoalgorithms_jl_amd.standardize import standardize
    eps = float(np.finfo(dtype).eps)
    F, _ = device_lasso(dtype)
    A, b, _ = lasso_case(dtype)
    N, d = A.shape
    A_before = F.A.clone()
    F_std, sc = standardize(ctx, F)
    assert torch.equal(bits(F.A), bits(A_before)) and F_std.A.data_ptr() != F.A.data_ptr()
    assert (F_std.loss, F_std.lam, F_std.N, F_std.d, F_std.N_total, F_std.row0, F_std.cyclic, F_std.padded_from) == \
           (F.loss, F.lam, N, d, F.N_total, F.row0, F.cyclic, F.padded_from)
    S = F_std.A.double().cpu().numpy()
    # a column's mean is within 8 eps_T of 0 relative to the column's max |a_ij|, in the units of the output (times scale_j): the mean
    # itself is a double (half a unit of |mean_j| <= max |a_ij|), a_ij - mean_j is rounded once in double and the product once to T
    amax = np.abs(A.astype(np.float64)).max(axis=0) * sc.scale.cpu().numpy()
    frac = np.abs(S.mean(axis=0)) / (8 * eps * amax)
    print(f"{tname(dtype)}: worst |column mean| / bound {frac.max():.3f}")
    assert (frac <= 1.0).all()
    # ... and its sum of squares within N times 2 (eps_T / 2) a^2 summed, i.e. eps_T relative, of N; 8 eps_T asked, whatever d is
    colsq = ctx.col_sqnorms(F_std).cpu().numpy()
    print(f"{tname(dtype)}: worst |colsq - N| / bound {float(np.abs(colsq - N).max() / (8 * eps * N)):.3f}")
    assert (np.abs(colsq - N) <= 8 * eps * N).all()
    b64 = b.astype(np.float64)
    assert abs(sc.b_mean - b64.mean()) <= 8 * 2.0 ** -52 * np.abs(b64).mean()
    assert np.array_equal(F_std.b.cpu().numpy(), (b64 - sc.b_mean).astype(dtype)) and F_std.b.data_ptr() != F.b.data_ptr()
    # the numpy twin (same dtype in): the same moments to rounding, and from the device's mean and scale the same bits
    hA, hb, hmean, hscale, hb_mean = host_standardize(A, b)
    assert np.allclose(sc.mean.cpu().numpy(), hmean, rtol=1e-13, atol=1e-13) and np.allclose(sc.scale.cpu().numpy(), hscale, rtol=1e-12)
    want = ((A.astype(np.float64) - sc.mean.cpu().numpy()) * sc.scale.cpu().numpy()).astype(dtype)
    assert np.array_equal(F_std.A.cpu().numpy().view(np.int64 if dtype == np.float64 else np.int32), want.view(np.int64 if dtype == np.float64 else np.int32))
    # transform of the training rows reproduces F_std.A bitwise (and centres b the same way); on a logistic view the labels stay
    again = sc.transform(ctx, F)
    assert torch.equal(bits(again.A), bits(F_std.A)) and torch.equal(bits(again.b), bits(F_std.b))
    from ciaoalgorithms_jl_amd.device import PackedF
    labels = torch.ones(N, dtype=F.dtype, device="cuda")
    Fl = sc.transform(ctx, PackedF.logistic(F.A, labels))
    assert torch.equal(bits(Fl.A), bits(F_std.A)) and Fl.b is labels
    # center / scale alone
    Fc, scc = standardize(ctx, F, scale=False)
    assert bool((scc.scale == 1).all()) and torch.equal(bits(Fc.A), bits(ctx.scale_columns(F, sc.mean, None)))
    Fs, scs = standardize(ctx, F, center=False)
    assert bool((scs.mean == 0).all()) and scs.b_mean == 0.0 and Fs.b is F.b
    assert torch.equal(bits(Fs.A), bits(ctx.scale_columns(F, None, sc.scale)))
    # in place: bitwise the out-of-place result, over F.A's own storage
    F_in, sc_in = standardize(ctx, F, inplace=True)
    assert F_in.A.data_ptr() == F.A.data_ptr() and F_in.A.untyped_storage().data_ptr() == F.A.untyped_storage().data_ptr()
    assert torch.equal(bits(F.A), bits(F_std.A)) and torch.equal(bits(F_in.b), bits(F_std.b))
    assert torch.equal(bits(sc_in.mean), bits(sc.mean)) and torch.equal(bits(sc_in.scale), bits(sc.scale))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
def test_coefficients_give_the_same_predictions(ctx, ciao, dtype):
    """a_std_i'x_std + b_mean = a_i'coef + intercept for every row, to (d + 2) eps_T sum_j |a_ij coef_j|: the derived bound of a length-d dot
    product in T."""
    import torch
    from ciaoalgorithms_jl_amd.standardize import standardize
    eps = float(np.finfo(dtype).eps)
    F, _ = device_lasso(dtype)
    A, b, _ = lasso_case(dtype)
    d = F.d
    F_std, sc = standardize(ctx, F)
    x_std = torch.from_numpy(np.random.default_rng(8).standard_normal(d).astype(dtype)).cuda()
    coef, intercept = sc.coefficients(x_std)
    assert coef.dtype == x_std.dtype and isinstance(intercept, float)
    lhs = ctx.row_dots(F_std, x_std).double().cpu().numpy() + sc.b_mean
    rhs = ctx.row_dots(F, coef).double().cpu().numpy() + intercept
    c64 = coef.double().cpu().numpy()
    mag = np.abs(A.astype(np.float64)) @ np.abs(c64)
    frac = np.abs(lhs - rhs) / ((d + 2) * eps * mag)
    print(f"{tname(dtype)}: worst |difference| / bound {frac.max():.3f}")
    assert (frac <= 1.0).all()
    back = sc.to_standardized(coef)
    assert torch.allclose(back.double(), x_std.double(), rtol=4 * eps, atol=0)
    xn, icn = sc.coefficients(x_std.cpu().numpy())                    # numpy in, numpy out
    assert isinstance(xn, np.ndarray) and xn.dtype == dtype and np.array_equal(xn, coef.cpu().numpy()) and abs(icn - intercept) <= 1e-12 * (1 + abs(intercept))


def test_svrg_on_the_standardised_problem(ctx, ciao):
    """SVRG with stop_when(cert, gap=...) reaches the asked gap on F_std as the same call does on the problem standardised in numpy
    float64 and packed."""
    import torch
    import ciaoalgorithms_jl_amd.solvers as S
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd.certificate import Certificate, stop_when
    from ciaoalgorithms_jl_amd.device import PackedF, ProxG
    from ciaoalgorithms_jl_amd.screening import mu_max
    from ciaoalgorithms_jl_amd.standardize import standardize
    from ciaoalgorithms_jl_amd.stepsize import lipschitz_max
    F, (hA, hb, hmean, hscale, hb_mean) = device_lasso(np.float64)
    F_std, sc = standardize(ctx, F)
    F_host = PackedF.least_squares(torch.from_numpy(hA.copy()).cuda(), torch.from_numpy(hb.copy()).cuda(), 1.0)
    target, runs = 1e-6, []
    for G in (F_std, F_host):
        g = ProxG(L.PROX_L1, lam=0.1 * mu_max(ctx, G))
        gamma = 1.0 / (7.0 * lipschitz_max(ctx, G))
        stop = stop_when(Certificate(ctx, G, g, G.N, gamma), gap=target)
        x, it = S.SVRG(np.float64, maxit=2000, γ=gamma)(np.zeros(G.d), F=G, g=g, N=G.N, ctx=ctx, stop=stop, check_every=5)
        runs.append((stop.last.gap, it, g.lam))
    print(f"device-standardised: gap {runs[0][0]:.3e} after {runs[0][1]} epochs; numpy-standardised: gap {runs[1][0]:.3e} after {runs[1][1]}")
    assert 0 <= runs[0][0] <= target and 0 <= runs[1][0] <= target
    assert abs(runs[0][2] - runs[1][2]) <= 1e-10 * runs[1][2]


def test_a_context_on_a_stream_of_its_own(ciao, ctx):
    """torch's own operations in standardize.py follow the library's kernels on the context's stream, not on torch's current one"""
    import torch
    from ciaoalgorithms_jl_amd.device import Context
    from ciaoalgorithms_jl_amd.standardize import standardize
    A = torch.from_numpy(np.random.default_rng(77).standard_normal((20000, 260)) * 3.0 + 2.0).cuda()
    A[0, 5] = 1e8
    F = problem(A)
    want, sc = standardize(ctx, F)
    torch.cuda.synchronize()
    own = Context(0, stream=torch.cuda.Stream())
    try:
        got, sc2 = standardize(own, F)
        own.synchronize()
        assert torch.equal(bits(got.A), bits(want.A)) and torch.equal(bits(got.b), bits(want.b))
        assert torch.equal(bits(sc2.mean), bits(sc.mean)) and torch.equal(bits(sc2.scale), bits(sc.scale)) and sc2.b_mean == sc.b_mean
    finally:
        own.synchronize()
        own.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, ciao):
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd.device import Context, PackedF, PackedSepQuad
    from ciaoalgorithms_jl_amd.standardize import column_moments, standardize
    f64 = dict(dtype=torch.float64, device="cuda")
    A = torch.randn((9, 8), **f64)
    F = PackedF.least_squares(A, torch.randn(9, **f64), 1.0)
    Fc = PackedF.least_squares_complex(torch.randn((4, 8), **f64), torch.randn(8, **f64), 4.0)
    Fz = PackedF.zero(4, 8, torch.float64)
    F0 = PackedF.logistic(torch.empty((0, 8), **f64), torch.empty(0, **f64), N_total=4)     # a rank that holds no row
    Fs = PackedSepQuad(torch.ones((3, 4), **f64), torch.ones((3, 4), **f64))
    Fshard = PackedF.least_squares(A, torch.randn(9, **f64), 1.0, N_total=18)
    x, v8, w8 = torch.zeros(8, **f64), torch.ones(8, **f64), torch.ones(8, **f64)
    out = torch.empty((9, 8), **f64)
    big = torch.zeros(200, **f64)
    ctx.full_gradient(F, x, torch.empty_like(x))
    before = ctx.last_kernel()
    assert not before.startswith("col")
    lib, h = ctx.lib, ctx._h
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def raw(status):
        if status != L.OK:
            raise L.CiaoError(status, lib.ciao_last_error().decode())

    def overlapping(shift_elems, ld):
        Fo = PackedF.least_squares(torch.as_strided(big, (9, 8), (10, 1), 16), torch.randn(9, **f64), 1.0)
        return lambda: raw(lib.ciao_scale_columns(h, Fo.ref, None, None, C.c_void_p(Fo.A.data_ptr() + 8 * shift_elems), ld))

    hooked = Context(0)
    hooked.full_gradient(F, x, torch.empty_like(x))
    hooked.synchronize()
    hooked.set_allreduce(lambda buf, count, dtype, stream: 0)
    before_hooked = hooked.last_kernel()
    try:
        cases = [("complex moments", lambda: ctx.col_moments(Fc)), ("Zero moments", lambda: ctx.col_moments(Fz)),
                 ("sharing moments", lambda: ctx.col_moments(Fs)),
                 ("complex scale", lambda: raw(lib.ciao_scale_columns(h, Fc.ref, None, None, ptr(out), 8))),
                 ("Zero scale", lambda: raw(lib.ciao_scale_columns(h, Fz.ref, None, None, ptr(out), 8))),
                 ("sharing scale", lambda: ctx.scale_columns(Fs)),
                 ("NULL ctx", lambda: raw(lib.ciao_col_moments(None, F.ref, None, ptr(v8), ptr(w8)))),
                 ("NULL problem", lambda: raw(lib.ciao_col_moments(h, None, None, ptr(v8), ptr(w8)))),
                 ("NULL s1", lambda: raw(lib.ciao_col_moments(h, F.ref, None, None, ptr(w8)))),
                 ("NULL s2", lambda: raw(lib.ciao_col_moments(h, F.ref, None, ptr(v8), None))),
                 ("NULL ctx scale", lambda: raw(lib.ciao_scale_columns(None, F.ref, None, None, ptr(out), 8))),
                 ("NULL problem scale", lambda: raw(lib.ciao_scale_columns(h, None, None, None, ptr(out), 8))),
                 ("NULL out", lambda: raw(lib.ciao_scale_columns(h, F.ref, None, None, None, 8))),
                 ("ld_out < d", lambda: raw(lib.ciao_scale_columns(h, F.ref, None, None, ptr(out), 7))),
                 ("out = A, another ld", overlapping(0, 12)), ("out one row down", overlapping(10, 10)),
                 ("out one element up", overlapping(-1, 10)), ("out in A's last row", overlapping(80, 10)),
                 ("standardize complex", lambda: standardize(ctx, Fc)), ("standardize Zero", lambda: standardize(ctx, Fz)),
                 ("standardize sharing", lambda: standardize(ctx, Fs)), ("standardize N = 0", lambda: standardize(ctx, F0)),
                 ("column_moments complex", lambda: column_moments(ctx, Fc)),
                 ("standardize row shard", lambda: standardize(ctx, Fshard)), ("standardize hook", lambda: standardize(hooked, F))]
        for what, call in cases:
            with pytest.raises(L.CiaoError) as e:
                call()
            assert e.value.status == L.ERR_ARG, what
            assert len(str(e.value)) - len("libciao_hip status -1: ") > 30, (what, str(e.value))
            assert ctx.last_kernel() == before and hooked.last_kernel() == before_hooked, what
        assert "row-sharded" in str(e.value)
        for bad in (lambda: ctx.col_moments(F, shift=torch.zeros(8, dtype=torch.float32, device="cuda")), lambda: ctx.col_moments(F, shift=torch.zeros(7, **f64)),
                    lambda: ctx.scale_columns(F, center=torch.zeros(9, **f64)), lambda: ctx.scale_columns(F, out=torch.empty((9, 8), dtype=torch.float32, device="cuda")),
                    lambda: ctx.scale_columns(F, out=torch.empty((8, 9), **f64)), lambda: standardize(ctx, F, refine="maybe")):
            with pytest.raises(ValueError):
                bad()
        assert ctx.last_kernel() == before
        assert not bool(big.any())                                     # no refused call wrote
        # N = 0: zeros, nothing launched
        s1, s2 = ctx.col_moments(F0, s1=v8, s2=w8)
        assert not bool(s1.any()) and not bool(s2.any()) and ctx.last_kernel() == before
        assert ctx.scale_columns(F0, v8, w8).shape == (0, 8) and ctx.last_kernel() == before
        # on the context with the hook both passes work, on the local rows
        want = ctx.col_moments(F)
        got = hooked.col_moments(Fshard)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, want)) and hooked.last_kernel().startswith("colmom_")
        assert torch.equal(bits(hooked.scale_columns(Fshard, want[0], None)), bits(ctx.scale_columns(F, want[0], None)))
        # ... and with the hook taken off the same context standardises
        hooked.set_allreduce(None)
        assert standardize(hooked, F)[0].A.shape == (9, 8)
    finally:
        hooked.synchronize()
        hooked.close()
    ctx.synchronize()

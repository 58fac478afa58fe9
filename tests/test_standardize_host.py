"""The host side of column standardisation (standardize.py, host_route.host_col_moments / host_standardize),
without a GPU: the numpy twins against math.fsum, the refinement rule on its three cases, the coefficient map and its inverse, the
zero-variance rule, the new prototypes as plain C, and that solvers.py stays untouched by it."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U53 = 2.0 ** -53
N = 4099


def three_cases(dtype, d=6):
    """Gaussian columns; the same with mean 10^6 sigma; the same with a first row of 10^8"""
    rng = np.random.default_rng(17)
    g = rng.standard_normal((N, d))
    shifted = (g + 1e6).astype(dtype)
    spike = g.astype(dtype)
    spike[0] = 1e8
    return g.astype(dtype), shifted, spike


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_col_moments_against_fsum(ciao, dtype):
    """The device test's bounds: one rounding of a - c, N - 1 additions in double (s2: one more rounding, of the square)."""
    from ciaoalgorithms_jl_amd.host_route import host_col_moments
    for A in three_cases(dtype):
        for shift in (None, np.arange(A.shape[1], dtype=np.float64) - 2.0):
            s1, s2 = host_col_moments(A, shift)
            assert s1.dtype == s2.dtype == np.float64 and s1.shape == s2.shape == (A.shape[1],)
            t = A.astype(np.float64) - (A[0].astype(np.float64) if shift is None else shift)[None, :]
            r1 = np.array([math.fsum(c) for c in t.T.tolist()])
            r2 = np.array([math.fsum(c) for c in (t * t).T.tolist()])
            assert (np.abs(s1 - r1) <= (N + 2) * U53 * np.abs(t).sum(axis=0)).all()
            assert (np.abs(s2 - r2) <= (N + 3) * U53 * r2).all()
    ints = np.random.default_rng(1).integers(-64, 65, (300, 7))
    s1, s2 = host_col_moments(ints.astype(dtype), np.full(7, 3.0))
    assert np.array_equal(s1, (ints - 3).sum(axis=0)) and np.array_equal(s2, ((ints - 3) ** 2).sum(axis=0))
    with pytest.raises(ValueError):
        host_col_moments(np.zeros((3, 2), np.complex128))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_refinement_rule_on_its_three_cases(ciao, dtype):
    """s2 / M2 is 1 - 3 for Gaussian columns shifted by their first row, whatever their mean; about N where the first row is an outlier:
    only that takes the second pass, after which the variance is exact to a few units."""
    from ciaoalgorithms_jl_amd.host_route import host_col_moments
    from ciaoalgorithms_jl_amd.standardize import REFINE_RATIO, _needs_refinement, host_column_moments
    assert REFINE_RATIO == 1024.0
    gauss, shifted, spike = three_cases(dtype)
    for A, passes in ((gauss, 1), (shifted, 1), (spike, 2)):
        s1, s2 = host_col_moments(A)
        amp = s2 / (s2 - s1 * s1 / N)
        assert (amp < 16).all() if passes == 1 else (amp > 0.9 * N).all()
        assert _needs_refinement(s1, s2, N).all() == (passes == 2)
        m = host_column_moments(A)
        assert m.passes == passes and m.n == N
        A64 = A.astype(np.float64)
        mean = np.array([math.fsum(c) for c in A64.T.tolist()]) / N
        var = np.array([math.fsum(c) for c in ((A64 - mean) ** 2).T.tolist()]) / N
        assert (np.abs(m.var - var) <= 1e-12 * var).all() and (np.abs(m.mean - mean) <= 1e-15 * np.abs(A64).max()).all()
        assert host_column_moments(A, refine=False).passes == 1 and host_column_moments(A, refine=True).passes == 2
    # cancellation that leaves M2 <= 0 under a positive s2 asks for the second pass too; an all-constant column does not
    assert _needs_refinement(np.array([4.0, 0.0]), np.array([4.0, 0.0]), 4).tolist() == [True, False]
    with pytest.raises(ValueError):
        host_column_moments(gauss, refine="maybe")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_standardize_and_the_zero_variance_rule(ciao, dtype):
    from ciaoalgorithms_jl_amd.host_route import host_standardize
    rng = np.random.default_rng(2)
    A = (rng.standard_normal((500, 8)) * np.exp(rng.standard_normal(8)) + rng.standard_normal(8)).astype(dtype)
    A[:, 3] = dtype(0.1) * 3
    A[:, 6] = 0.0
    b = (rng.standard_normal(500) + 4.0).astype(dtype)
    A_std, b_std, mean, scale, b_mean = host_standardize(A, b)
    assert A_std.dtype == dtype and b_std.dtype == dtype and mean.dtype == scale.dtype == np.float64
    assert not A_std[:, 3].any() and not A_std[:, 6].any()                   # a constant column centred is exactly zero ...
    assert scale[3] == 1.0 and scale[6] == 1.0 and mean[3] == float(A[0, 3])  # ... and is not scaled
    eps = float(np.finfo(dtype).eps)
    live = [0, 1, 2, 4, 5, 7]
    S = A_std.astype(np.float64)[:, live]
    assert (np.abs(S.mean(axis=0)) <= 8 * eps * np.abs(S).max(axis=0)).all()
    assert (np.abs((S * S).sum(axis=0) - 500) <= 8 * eps * 500).all()
    assert abs(b_mean - b.astype(np.float64).mean()) <= 1e-15 * 5 and np.array_equal(b_std, (b.astype(np.float64) - b_mean).astype(dtype))
    assert np.array_equal(A_std, ((A.astype(np.float64) - mean) * scale).astype(dtype))
    # center / scale alone; logistic labels (b = None)
    Ac, _, mc, sc, bm = host_standardize(A, None, scale=False)
    assert (sc == 1).all() and bm == 0.0 and np.array_equal(Ac, (A.astype(np.float64) - mean).astype(dtype))
    As, bs, ms, ss, bm = host_standardize(A, b, center=False)
    assert (ms == 0).all() and bm == 0.0 and np.array_equal(bs, b) and np.array_equal(As, (A.astype(np.float64) * scale).astype(dtype))


def test_coefficients_and_to_standardized_are_inverse(ciao):
    """The maps use nothing of the device but the two vectors: stand-ins with .cpu().numpy() serve."""
    from ciaoalgorithms_jl_amd.standardize import Scaler

    class Vec:
        def __init__(self, v):
            self.v = v

        def cpu(self):
            return self

        def numpy(self):
            return self.v

    rng = np.random.default_rng(4)
    mean, scale = rng.standard_normal(12), np.exp(rng.standard_normal(12))
    sc = Scaler(Vec(mean), Vec(scale), 2.5, True, True)
    for dtype in (np.float32, np.float64):
        x_std = rng.standard_normal(12).astype(dtype)
        x, intercept = sc.coefficients(x_std)
        assert x.dtype == dtype and isinstance(intercept, float)
        assert np.array_equal(x, (x_std.astype(np.float64) * scale).astype(dtype))
        assert intercept == 2.5 - float((mean * x.astype(np.float64)).sum())
        back = sc.to_standardized(x)
        eps = float(np.finfo(dtype).eps)
        assert back.dtype == dtype and (np.abs(back - x_std) <= 2 * eps * np.abs(x_std)).all()
        again, _ = sc.coefficients(back)
        assert (np.abs(again - x) <= 2 * eps * np.abs(x)).all()
        # the predictions agree: (a - mean) scale . x_std + b_mean = a . x + intercept
        a = rng.standard_normal(12)
        lhs = float(((a - mean) * scale) @ x_std.astype(np.float64)) + sc.b_mean
        rhs = float(a @ x.astype(np.float64)) + intercept
        assert abs(lhs - rhs) <= 14 * eps * float(np.abs(a) @ np.abs(x.astype(np.float64)) + np.abs(mean) @ np.abs(x.astype(np.float64)))


def test_the_solvers_do_not_import_the_module(ciao):
    src = open(os.path.join(ROOT, "ciaoalgorithms.jl_amd", "solvers.py")).read()
    assert not re.search(r"import.*\bstandardize\b|\bstandardize\s+import|col_moments|scale_columns|standardi", src)
    import ciaoalgorithms_jl_amd.standardize as st
    for name in ("column_moments", "standardize", "host_column_moments", "Scaler", "ColumnMoments"):
        assert callable(getattr(st, name))
    import ciaoalgorithms_jl_amd.host_route as hr
    assert callable(hr.host_col_moments) and callable(hr.host_standardize)
    for name, nargs in (("ciao_col_moments", 5), ("ciao_scale_columns", 6)):
        assert name in ciao._lib.SIGNATURES and len(ciao._lib.SIGNATURES[name][1]) == nargs
    assert ciao._lib.ABI_VERSION == 3


def test_the_new_prototypes_are_plain_c(tmp_path):
    """include/ciao_hip.h as C11, pedantic, with a caller that passes NULL for shift, center and scale."""
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n#include "ciao_hip.h"\n'
                   "int32_t (*fm)(ciao_ctx *, const ciao_problem *, const double *, double *, double *) = ciao_col_moments;\n"
                   "int32_t (*fs)(ciao_ctx *, const ciao_problem *, const double *, const double *, void *, int64_t) = ciao_scale_columns;\n"
                   "int32_t all(ciao_ctx *c, const ciao_problem *p, double *s1, double *s2, void *out) {\n"
                   "    return ciao_col_moments(c, p, NULL, s1, s2) + ciao_col_moments(c, p, s1, s1, s2) + ciao_scale_columns(c, p, NULL, NULL, out, p->d)\n"
                   "         + ciao_scale_columns(c, p, s1, NULL, out, p->d) + ciao_scale_columns(c, p, NULL, s2, (void *)p->A, p->ld); }\n")
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(tmp_path / "s.o")], check=True)

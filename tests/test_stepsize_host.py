"""The host side of the step sizes from the data (stepsize.py, host_route.host_row_sqnorms / host_lipschitz),
without a GPU: the numpy twins against math.fsum and the reference fixtures' own constants, the power iteration's arithmetic against
numpy.linalg.eigvalsh, the new prototype as plain C, and that solvers.py stays untouched by it."""
import math
import os
import subprocess

import numpy as np
import pytest

import problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U53 = 2.0 ** -53


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N,d", [(5, 1), (7, 3), (9, 50), (4, 1025), (2, 70001)])
def test_host_row_sqnorms_against_fsum(ciao, N, d, dtype):
    """The device test's bound: d - 1 additions of non-negative terms in double, one rounding per square in fp64, none in fp32."""
    from ciaoalgorithms_jl_amd.host_route import host_row_sqnorms
    A = np.random.default_rng(100 * d + N).standard_normal((N, d)).astype(dtype)
    sq = A.astype(np.float64) ** 2
    ref = np.array([math.fsum(row) for row in sq])
    got = host_row_sqnorms(A)
    assert got.dtype == np.float64 and got.shape == (N,)
    assert (np.abs(got - ref) <= (d + 2) * U53 * ref).all()


def test_host_row_sqnorms_of_complex_rows(ciao):
    from ciaoalgorithms_jl_amd.host_route import host_row_sqnorms
    A, _, _ = P.synthetic_complex(6, 11, np.complex128)
    pairs = np.ascontiguousarray(A).view(np.float64).reshape(6, 22)
    assert np.array_equal(host_row_sqnorms(A), host_row_sqnorms(pairs))
    ref = np.array([math.fsum(r) for r in pairs * pairs])
    assert (np.abs(host_row_sqnorms(A) - ref) <= 24 * U53 * ref).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_lipschitz_gives_the_fixtures_constants(ciao, dtype):
    """tests/problems.py: N sum(A^2, axis=1) (test_lasso.jl:52-56) and 0.25 sum(XS^2, axis=1) (test_logistic_l1.jl:39); within 4 eps."""
    from ciaoalgorithms_jl_amd.host_route import host_lipschitz
    eps = float(np.finfo(dtype).eps)
    A, b, Lc, lam, x0, x_star, f_star = P.lasso_known_answer(dtype=dtype)
    got = host_lipschitz("ls", A, float(A.shape[0]))
    assert got.dtype == np.float64
    assert (np.abs(got - Lc.astype(np.float64)) <= 4 * eps * Lc.astype(np.float64)).all()
    A, y, Lc, lam, x0, x_star = P.logistic_fixture(dtype)
    got = host_lipschitz("logistic", A)
    assert (np.abs(got - Lc.astype(np.float64)) <= 4 * eps * Lc.astype(np.float64)).all()
    with pytest.raises(ValueError):
        host_lipschitz("zero", A)


def planted(seed=0):
    """The matrix of tests/test_gpu_stepsize.py: A = 3 u v' + Gaussian / sqrt(d) at (200, 40), u a unit vector, v standard normal"""
    N, d = 200, 40
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(N)
    u /= np.linalg.norm(u)
    v = rng.standard_normal(d)
    return 3.0 * np.outer(u, v) + rng.standard_normal((N, d)) / np.sqrt(d)


@pytest.mark.parametrize("kind", ["ls", "logistic"])
def test_power_iteration_against_eigvalsh(ciao, kind):
    from ciaoalgorithms_jl_amd.host_route import host_row_sqnorms
    from ciaoalgorithms_jl_amd.stepsize import _power, host_smoothness
    A = planted()
    N, d = A.shape
    w = np.linalg.eigvalsh(A.T @ A)
    assert w[-2] / w[-1] <= 0.5, "choose another seed"
    lam = 2.5
    c = (lam if kind == "ls" else 0.25) / N
    true = c * w[-1]
    rtol = 1e-6
    est, upper = host_smoothness(kind, A, lam, iters=50, rtol=rtol, seed=0)
    eps = float(np.finfo(np.float64).eps)
    assert true * (1 - 10 * rtol) <= est <= true * (1 + 8 * eps * d)
    assert upper >= true and upper == ((lam if kind == "ls" else 0.25) / N) * float(np.sum(host_row_sqnorms(A)))
    # the quotient rises monotonically and the iteration stops early: far fewer than 50 applications at a ratio <= 0.5
    calls = []

    def apply(v):
        calls.append(float(v @ (A.T @ (A @ v))))
        return A.T @ (A @ v)

    rho, n = _power(apply, np.random.default_rng(0).standard_normal(d), 50, rtol, lambda a, b: float(a @ b))
    assert n == len(calls) < 50 and rho <= w[-1] * (1 + 8 * eps * d)
    assert all(b >= a * (1 - 8 * eps * d) for a, b in zip(calls, calls[1:]))
    # one iteration is allowed and gives a lower bound too
    assert 0 < host_smoothness(kind, A, lam, iters=1)[0] <= true * (1 + 8 * eps * d)
    with pytest.raises(ValueError):
        host_smoothness(kind, A, lam, iters=0)


def test_the_solvers_do_not_import_the_module(ciao):
    src = open(os.path.join(ROOT, "ciaoalgorithms.jl_amd", "solvers.py")).read()
    import re
    assert not re.search(r"import.*\bstepsize\b|\bstepsize\s+import|row_sqnorm|lipschitz", src)
    import ciaoalgorithms_jl_amd.stepsize as st
    for name in ("lipschitz", "lipschitz_max", "lipschitz_range", "smoothness", "host_smoothness"):
        assert callable(getattr(st, name))
    assert "ciao_row_sqnorms" in ciao._lib.SIGNATURES


def test_the_new_prototype_is_plain_c(tmp_path):
    """include/ciao_hip.h as C11, pedantic, with a caller of ciao_row_sqnorms that passes NULL for either output."""
    src = tmp_path / "r.c"
    src.write_text('#include <stddef.h>\n#include "ciao_hip.h"\n'
                   "int32_t (*fp)(ciao_ctx *, const ciao_problem *, double *, double *) = ciao_row_sqnorms;\n"
                   "int32_t both(ciao_ctx *c, const ciao_problem *p, double *out) { double s[4]; return ciao_row_sqnorms(c, p, out, s) + "
                   "ciao_row_sqnorms(c, p, NULL, s) + ciao_row_sqnorms(c, p, out, NULL); }\n")
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(tmp_path / "r.o")], check=True)

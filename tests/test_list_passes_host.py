"""The host twins of the row-list passes (host_route.host_list_dots / host_list_combine) and newton.HostRows(rows=); DESIGN.md section 8.16.

  * on integer data (|a| <= 64, |x| <= 8, |c| <= 8) every sum is exact: the twins equal numpy's int64 result, for lists with repeats, a
    reversed list, an empty list and no list;
  * the refusals follow host_gram(rows=);
  * HostRows(A, y, rows=idx) is HostRows(A[idx], y[idx]) bit for bit through a whole logistic_newton solve."""
import numpy as np
import pytest


def int_data(N=37, d=11):
    rng = np.random.default_rng(21)
    return rng.integers(-64, 65, (N, d)), rng.integers(-8, 9, d)


LISTS = {"repeats": lambda N: np.random.default_rng(22).integers(0, N, 2 * N + 3), "reversed": lambda N: np.arange(N - 1, -1, -1),
         "stride": lambda N: np.arange(1, N, 3), "empty": lambda N: np.zeros(0, np.int64), "none": lambda N: None}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(LISTS))
def test_the_twins_on_integers(ciao, dtype, name):
    from ciaoalgorithms_jl_amd.host_route import host_list_combine, host_list_dots
    A, x = int_data()
    rows = LISTS[name](A.shape[0])
    if name == "repeats":
        assert len(np.unique(rows)) < len(rows)
    g = A if rows is None else A[rows]
    c = (5 * np.arange(g.shape[0])) % 9 - 4
    dots = host_list_dots(A.astype(dtype), x.astype(dtype), rows)
    comb = host_list_combine(A.astype(dtype), c.astype(np.float64), rows)
    assert dots.dtype == np.float64 and comb.dtype == np.float64 and dots.shape == (g.shape[0],) and comb.shape == (A.shape[1],)
    assert np.array_equal(dots, (g @ x).astype(np.float64)) and np.array_equal(comb, (g.T @ c).astype(np.float64))
    if name == "empty":
        assert not comb.any()


def test_refusals(ciao):
    from ciaoalgorithms_jl_amd.host_route import host_list_combine, host_list_dots
    A, x = int_data()
    A, x = A.astype(np.float64), x.astype(np.float64)
    N, d = A.shape
    for bad in (np.array([0, N]), np.array([-1, 2]), np.array([0.0, 1.0]), np.zeros((2, 2), np.int64)):
        with pytest.raises(ValueError):
            host_list_dots(A, x, bad)
        with pytest.raises(ValueError):
            host_list_combine(A, np.ones(bad.size), bad)
    with pytest.raises(ValueError):
        host_list_dots(A, x[:-1])
    with pytest.raises(ValueError):
        host_list_dots(A + 0j, x)
    with pytest.raises(ValueError):
        host_list_dots(A[0], x)
    with pytest.raises(ValueError):
        host_list_combine(A, np.ones(N - 1))
    with pytest.raises(ValueError):
        host_list_combine(A, np.ones(3), np.array([0, 1]))
    with pytest.raises(ValueError):
        host_list_combine(A, np.ones(N) + 0j)


@pytest.mark.parametrize("dtype,gap", [(np.float64, 1e-9), (np.float32, 1e-5)])
@pytest.mark.parametrize("subproblem", ["cd", "fista"])
def test_host_rows_over_a_list_are_the_gathered_rows(ciao, dtype, gap, subproblem):
    from ciaoalgorithms_jl_amd.newton import HostRows, logistic_mu_max, logistic_newton
    rng = np.random.default_rng(23)
    N, d = 120, 17
    A = rng.standard_normal((N, d)).astype(dtype)
    xt = np.zeros(d)
    xt[:4] = (2.0, -1.5, 1.0, 0.5)
    y = np.where(A @ xt + 0.5 * rng.standard_normal(N) >= 0, 1.0, -1.0).astype(dtype)
    idx = rng.integers(0, N, 90)
    assert len(np.unique(idx)) < len(idx)
    a, b = HostRows(A, y, rows=idx), HostRows(A[idx], y[idx])
    assert (a.N, a.d) == (b.N, b.d) == (90, d)
    mu = 0.1 * logistic_mu_max(b)
    assert logistic_mu_max(a) == logistic_mu_max(b)
    ra, rb = (logistic_newton(r, mu, gap=gap, subproblem=subproblem) for r in (a, b))
    assert ra.converged and ra.reason == "gap"
    assert np.array_equal(np.asarray(ra.x).view(np.uint8), np.asarray(rb.x).view(np.uint8))
    assert ra.certificate == rb.certificate and (ra.outer, ra.passes, ra.converged, ra.reason) == (rb.outer, rb.passes, rb.converged, rb.reason)
    import torch
    assert HostRows(A, y, rows=torch.from_numpy(idx)).N == 90
    for bad in (np.array([0, N]), np.array([-1]), np.zeros(0, np.int64), np.array([0.5])):
        with pytest.raises(ValueError):
            HostRows(A, y, rows=bad)

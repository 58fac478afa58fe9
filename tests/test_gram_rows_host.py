"""The host side of the Gram statistics over a list of rows (host_route.host_gram(rows=), gram.host_gram_stats(rows=), gram.add_stats,
gram.mse), without a GPU:

  1. host_gram(rows=) is host_gram of the gathered arrays, bit for bit: lists with repeats, with weights by list position, an empty list;
     refusals;
  2. add_stats: sums in list order, N and the sums of b included; refusals (weighted statistics, another d, lam or kind);
  3. mse on integer rows with an integer x equals sum((A x - b)^2) / M exactly: every term is an integer below 2^53.
"""
import numpy as np
import pytest


def case(N=40, d=7, seed=0, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, d)).astype(dtype), rng.standard_normal(N).astype(dtype)


def int_case(N=90, d=11, seed=1):
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, (N, d)).astype(np.float64), rng.integers(-20, 21, N).astype(np.float64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_host_gram_over_a_list_is_host_gram_of_the_gathered_arrays(ciao, dtype):
    from ciaoalgorithms_jl_amd.host_route import host_gram
    A, b = case(dtype=dtype)
    rng = np.random.default_rng(2)
    rows = rng.integers(0, 40, 55)
    assert len(np.unique(rows)) < 55
    w = rng.standard_normal(55)
    for weights in (None, w):
        got = host_gram(A, b, weights, rows)
        want = host_gram(A[rows], b[rows], weights)
        assert len(got) == 4 and got[3].shape == ((2,) if weights is None else (3,))
        assert all(g.dtype == np.float64 and np.array_equal(g.view(np.int64), e.view(np.int64)) for g, e in zip(got, want))
    # the identity list: the matrix itself; any integer type; a list, not an array
    assert all(np.array_equal(g, e) for g, e in zip(host_gram(A, b, rows=np.arange(40, dtype=np.int32)), host_gram(A, b)))
    assert all(np.array_equal(g, e) for g, e in zip(host_gram(A, b, rows=[3, 3, 0]), host_gram(A[[3, 3, 0]], b[[3, 3, 0]])))
    # an empty list: zeros of the right shapes
    for weights, nb in ((None, 2), (np.empty(0), 3)):
        got = host_gram(A, b, weights, np.empty(0, np.int64))
        assert [g.shape for g in got] == [(7, 7), (7,), (7,), (nb,)] and not any(g.any() for g in got)


def test_host_gram_refuses_a_bad_list(ciao):
    from ciaoalgorithms_jl_amd.host_route import host_gram
    A, b = case()
    for bad in ([-1, 2], [0, 40], np.array([0.0, 1.0]), np.zeros((2, 2), np.int64)):
        with pytest.raises(ValueError):
            host_gram(A, b, rows=bad)
    with pytest.raises(ValueError):
        host_gram(A, b, np.ones(40), [0, 1, 2])      # one weight per list position, not per row


def test_host_gram_stats_over_a_list(ciao):
    import torch
    from ciaoalgorithms_jl_amd import gram as GR
    A, b = int_case()
    rows = np.array([5, 5, 17, 89, 0])
    st = GR.host_gram_stats(A, b, lam=2.0, rows=rows)
    ref = GR.host_gram_stats(A[rows], b[rows], lam=2.0)
    assert st.N == 5 and st.d == 11 and st.lam == 2.0 and st.kind == "ls" and st.sum_w is None
    assert torch.equal(st.G, ref.G) and torch.equal(st.u, ref.u) and torch.equal(st.colsum, ref.colsum) and (st.sum_b, st.sum_bb) == (ref.sum_b, ref.sum_bb)
    wst = GR.host_gram_stats(A, b, weights=np.arange(5.0), rows=rows)
    assert wst.N == 5 and wst.sum_w == 10.0


def test_add_stats(ciao):
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd import gram as GR
    A, b = int_case()
    parts = [np.arange(0, 30), np.arange(30, 31), np.arange(31, 90)]
    stats = [GR.host_gram_stats(A, b, lam=3.0, rows=r) for r in parts]
    whole = GR.host_gram_stats(A, b, lam=3.0)
    tot = GR.add_stats(stats)
    assert tot.N == 90 and (tot.d, tot.lam, tot.kind, tot.sum_w, tot.dtype) == (11, 3.0, "ls", None, torch.float64)
    assert torch.equal(tot.G, whole.G) and torch.equal(tot.u, whole.u) and torch.equal(tot.colsum, whole.colsum)      # integers: exact
    assert (tot.sum_b, tot.sum_bb) == (whole.sum_b, whole.sum_bb)
    # list order: ((s0 + s1) + s2), on Gaussian rows too
    Ag, bg = case(90, 11, seed=3)
    sg = [GR.host_gram_stats(Ag, bg, rows=r) for r in parts]
    tg = GR.add_stats(sg)
    assert torch.equal(tg.G, (sg[0].G + sg[1].G) + sg[2].G) and tg.sum_bb == (sg[0].sum_bb + sg[1].sum_bb) + sg[2].sum_bb
    one = GR.add_stats(stats[:1])
    assert torch.equal(one.G, stats[0].G) and one.G.data_ptr() != stats[0].G.data_ptr()
    # a generator is taken too; the parts are left as they were
    assert GR.add_stats(s for s in stats).N == 90 and stats[0].N == 30
    with pytest.raises(ValueError):
        GR.add_stats([])
    others = (GR.host_gram_stats(A, b, lam=3.0, weights=np.ones(90)),                 # weighted
              GR.host_gram_stats(A[:, :10], b, lam=3.0),                             # another d
              GR.host_gram_stats(A, b, lam=2.0),                                      # another lam
              GR.host_gram_stats(A, np.sign(b + 0.5), kind="logistic"))               # another kind
    for other in others:
        with pytest.raises(L.CiaoError) as e:
            GR.add_stats([stats[0], other])
        assert e.value.status == L.ERR_ARG


def test_mse_on_integers_is_exact(ciao):
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd import gram as GR
    A, b = int_case()
    rng = np.random.default_rng(4)
    rows = rng.permutation(90)[:37]
    st = GR.host_gram_stats(A, b, rows=rows)
    X = rng.integers(-5, 6, (11, 4)).astype(np.float64)
    X[:, 3] = 0
    Af, bf = A[rows], b[rows]
    v, fl = GR.mse(st, X)
    assert v.shape == (4,) and fl.shape == (4,) and v.dtype == torch.float64
    for k in range(4):
        r = Af @ X[:, k] - bf
        want = np.sum(r ** 2) / 37
        assert float(v[k]) == want, k
        q = X[:, k] @ (Af.T @ Af) @ X[:, k]
        assert float(fl[k]) == 4 * 2.0 ** -53 * (q + 2 * abs((Af.T @ bf) @ X[:, k]) + np.sum(bf ** 2)) / 37
    one_v, one_fl = GR.mse(st, torch.from_numpy(X[:, 1]))
    assert isinstance(one_v, float) and (one_v, one_fl) == (float(v[1]), float(fl[1]))
    # the floor is GramLasso.value_floor on the scale of the mean squared residual: value = lam mse / 2
    q = GR.GramLasso(st)
    assert torch.allclose(q.value(torch.from_numpy(X)), 0.5 * st.lam * v, rtol=1e-15, atol=0) and torch.allclose(q.value_floor(torch.from_numpy(X)), 0.5 * st.lam * fl, rtol=1e-15, atol=0)
    for bad in (GR.host_gram_stats(A, np.sign(b + 0.5), kind="logistic"), GR.host_gram_stats(A, b, weights=np.ones(90))):
        with pytest.raises(L.CiaoError):
            GR.mse(bad, X)

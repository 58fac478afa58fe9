"""K-fold cross-validation of the lasso path in d-space (cv.py), without a GPU: the folds' statistics come from
host_route.host_gram(rows=), everything after them is the code the device route runs.

  1. fold_lists: a partition of 0 .. N-1 into sorted lists whose sizes differ by at most one; the seed decides, and only the seed;
  2. lasso_cv_from_stats on Gaussian rows, (N, d) = (200, 50): every entry of the table against the direct numpy residual of the model
     that produced it, under a derived bound; best and one_se from the table by their definitions; a NaN column never wins; path is
     lasso_cd on the summed statistics; FISTA in place of coordinate descent; refusals.

The bound of item 2.  mse[f, k] is (x'G_f x - 2 u_f'x + sum b_f^2) / M from statistics that carry host_gram's own rounding; the
reference is mean((A_f x - b_f)^2) in numpy.  With t_n = |a_n|'|x| + |b_n| and S = sum_n t_n^2 over the M rows of the fold:
  - evaluating the three terms from given statistics: at most the floor gram.mse reports beside the value, 4 * 2^-53 (x'Gx + 2 |u'x| +
    sum b^2) / M (GramLasso.value_floor on this scale);
  - the statistics themselves (section 8.12): every entry of G_f, u_f and sum b_f^2 is within (M + 8) 2^-53 of its exact value times the
    sum of the absolute products, which moves the quadratic form by at most (M + 8) 2^-53 S / M;
  - the direct sum: a residual is a dot product of d + 1 terms, off by at most (d + 2) 2^-53 t_n, so its square by 2 (d + 2) 2^-53 t_n^2
    to first order; squaring and adding M of them adds (M + 1) roundings, and 1 more covers the second-order terms: (2 (d + 2) + M + 2)
    2^-53 S / M.
Together: |mse - direct| <= floor + (2 M + 2 d + 14) 2^-53 S / M.  The factor 2 M + 2 d + 14 comes from these bounds, not from what
the code gives."""
import numpy as np
import pytest

U53 = 2.0 ** -53


def gauss_case(N=200, d=50, seed=21):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, d))
    x_true = np.zeros(d)
    x_true[rng.choice(d, 8, replace=False)] = rng.standard_normal(8)
    return A, A @ x_true + 0.5 * rng.standard_normal(N)


@pytest.mark.parametrize("N,folds", [(200, 5), (203, 5), (7, 7), (10, 3)])
def test_fold_lists_partition_the_rows(ciao, N, folds):
    import torch
    from ciaoalgorithms_jl_amd.cv import fold_lists
    lists = fold_lists(N, folds, seed=4)
    assert len(lists) == folds and all(r.dtype == torch.int64 and r.dim() == 1 and r.is_contiguous() and r.device.type == "cpu" for r in lists)
    assert torch.equal(torch.sort(torch.cat(lists)).values, torch.arange(N))
    sizes = [len(r) for r in lists]
    assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)
    assert all(bool((r[1:] > r[:-1]).all()) for r in lists)
    again = fold_lists(N, folds, seed=4)
    assert all(torch.equal(a, b) for a, b in zip(lists, again))
    if N >= 200:
        other = fold_lists(N, folds, seed=5)
        assert any(not torch.equal(a, b) for a, b in zip(lists, other))
        assert not torch.equal(lists[0], torch.arange(len(lists[0])))      # random folds, not contiguous ones


def test_fold_lists_refusals(ciao):
    from ciaoalgorithms_jl_amd.cv import fold_lists
    for N, folds in ((10, 1), (3, 4), (0, 2)):
        with pytest.raises(ValueError):
            fold_lists(N, folds)


@pytest.fixture(scope="module")
def cv_case(ciao):
    from ciaoalgorithms_jl_amd import cv as CV
    from ciaoalgorithms_jl_amd import gram as GR
    A, b = gauss_case()
    lists = CV.fold_lists(200, 5, seed=9)
    stats = CV.fold_stats(None, (A, b), lists)
    whole = GR.add_stats(stats)
    mus = [f * GR.mu_max(whole) for f in (0.6, 0.3, 0.1, 0.03, 0.003)]
    return A, b, lists, stats, mus, CV.lasso_cv_from_stats(stats, mus)


def test_the_table_against_direct_residuals(ciao, cv_case):
    import torch
    from ciaoalgorithms_jl_amd import gram as GR
    A, b, lists, stats, mus, res = cv_case
    N, d = A.shape
    assert res.mus == mus and tuple(res.mse.shape) == (5, len(mus)) and res.mse.dtype == torch.float64
    worst, floors = 0.0, []
    for f, rows in enumerate(lists):
        rows = rows.numpy()
        Af, bf, M = A[rows], b[rows], len(rows)
        train = GR.add_stats([s for g, s in enumerate(stats) if g != f])
        fit = GR.lasso_cd(train, mus, gap=1e-6)                      # the models of this fold, as the driver fits them
        V, FL = GR.mse(stats[f], torch.stack(fit.x, dim=1))
        assert torch.equal(V, res.mse[f])
        for k, x in enumerate(fit.x):
            x = x.numpy()
            direct = np.mean((Af @ x - bf) ** 2)
            v, floor = float(V[k]), float(FL[k])
            S = np.sum((np.abs(Af) @ np.abs(x) + np.abs(bf)) ** 2)
            bound = floor + (2 * M + 2 * d + 14) * U53 * S / M
            worst = max(worst, abs(v - direct) / bound)
            floors.append(floor)
            assert abs(v - direct) <= bound, (f, k, v, direct, bound)
    print(f"worst |mse - direct| / bound {worst:.3e}; floor {res.floor:.3e}")
    assert res.floor == max(floors)
    assert torch.equal(res.mean, res.mse.mean(0))
    # (five terms, a handful of roundings each way: 16 units of the last place are ample)
    assert np.allclose(res.stderr.numpy(), np.std(res.mse.numpy(), axis=0, ddof=1) / np.sqrt(5), rtol=16 * 2.0 ** -52, atol=0)


def test_best_and_one_se_by_their_definitions(ciao, cv_case):
    from ciaoalgorithms_jl_amd.cv import choose
    A, b, lists, stats, mus, res = cv_case
    mean, se = res.mean.tolist(), res.stderr.tolist()
    assert res.best == int(np.argmin(mean)) and 0 < res.best            # the largest mu underfits at this noise level
    within = [k for k in range(len(mus)) if mean[k] <= mean[res.best] + se[res.best]]
    assert res.one_se == max(within, key=lambda k: mus[k]) and mus[res.one_se] >= mus[res.best]
    # by hand: the order of the mus does not matter, a NaN never wins and never is within one standard error, ties go to the first
    assert choose([1.0, 2.0, 3.0], [0.5, 0.4, 0.45], [0.1, 0.06, 0.1]) == (1, 2)
    assert choose([3.0, 2.0, 1.0], [0.45, 0.4, 0.5], [0.1, 0.06, 0.1]) == (1, 0)
    assert choose([1.0, 2.0, 3.0], [0.5, 0.4, 0.47], [0.1, 0.06, 0.1]) == (1, 1)
    nan = float("nan")
    assert choose([1.0, 2.0, 3.0], [nan, 0.4, nan], [nan, 0.06, nan]) == (1, 1)
    assert choose([1.0, 2.0, 3.0], [0.4, nan, 0.4], [0.0, nan, 0.0]) == (0, 2)
    assert choose([1.0, 2.0], [0.4, 0.3], [0.1, nan]) == (1, 1)
    with pytest.raises(ValueError):
        choose([1.0, 2.0], [nan, nan], [nan, nan])


def test_the_refitted_path_and_the_methods(ciao, cv_case):
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd import cv as CV
    from ciaoalgorithms_jl_amd import gram as GR
    A, b, lists, stats, mus, res = cv_case
    ref = GR.lasso_cd(GR.add_stats(stats), mus, gap=1e-6)
    assert all(res.path.converged) and res.path.iterations == ref.iterations
    assert all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(res.path.x, ref.x))
    # FISTA in place of coordinate descent: a table of its own, chosen from by the same rule
    fista = CV.lasso_cv_from_stats(stats, mus[:3], method="fista")
    assert bool(torch.isfinite(fista.mse).all()) and fista.best == int(np.argmin(fista.mean.tolist())) and all(fista.path.converged)
    # refusals: one fold, no mu, logistic statistics, something that is no GramStats
    with pytest.raises(ValueError):
        CV.lasso_cv_from_stats(stats[:1], mus)
    with pytest.raises(ValueError):
        CV.lasso_cv_from_stats(stats, [])
    with pytest.raises(ValueError):
        CV.lasso_cv_from_stats(stats, [0.1, -1.0])
    logi = [GR.host_gram_stats(A, np.sign(b), kind="logistic", rows=r.numpy()) for r in lists]
    with pytest.raises(L.CiaoError):
        CV.lasso_cv_from_stats(logi, mus)
    with pytest.raises(TypeError):
        CV.lasso_cv_from_stats([stats[0], None], mus)
    with pytest.raises(L.CiaoError):
        CV.lasso_cv(None, (A, b), mus)                # the device driver takes a PackedF


def test_solvers_import_nothing_from_cv():
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ciaoalgorithms.jl_amd", "solvers.py")).read()
    assert "cv" not in [w for line in src.splitlines() if line.lstrip().startswith(("import ", "from ")) for w in line.replace(",", " ").replace(".", " ").split()]

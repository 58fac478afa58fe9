"""Constrained, weighted and batched coordinate descent on Gram matrices, without a GPU (host_route.host_gram_cd_general,
gram.constrained_gaps, the keywords of gram.lasso_cd / lasso_path, cv.lasso_cv_from_stats(fused=)):

  1. the general mirror with the defaults -- left out, and spelled out as arrays -- is host_gram_cd bit for bit (X, R, stat);
  2. six problems (plain, non-negative, a box, mixed factors with two unpenalised bounded coordinates, elastic net, elastic net +
     non-negative + an unpenalised coordinate) at two shapes: lasso_cd meets gap <= 1e-9 max(1, objective) by constrained_gaps, and
     that gap bounds objective - (the objective an independent solver reaches) from above: projected FISTA, 20 000 iterations, in
     numpy here.  Every constrained case has a coordinate AT a bound and one strictly inside;
  3. elastic net is the plain mirror on G + ridge I (1e-12 relative in x);
  4. state 3 for every input a model cannot run on, state 2 for a NaN in one model's u: the neighbours keep their bits;
  5. the driver's refusals, the forwarding of lasso_path, the certificates;
  6. lasso_cv_from_stats(fused=True) is fused=False bit for bit on statistics of integer rows, plain and constrained.
"""
import os

import numpy as np
import pytest

from test_gram_cd_host import lasso_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(200, 50), (300, 130)]
GAP = 1e-9
FISTA_ITERATIONS = 20000


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def gram_case(d, seed=0, K=3):
    rng = np.random.default_rng(100 * d + seed)
    N = d + 5
    A = rng.standard_normal((N, d))
    if d >= 3:
        A[:, 1] = A[:, 0]
    b = A @ (rng.standard_normal(d) * (rng.random(d) < 0.3)) + 0.1 * rng.standard_normal(N)
    G, u = A.T @ A, A.T @ b
    G = np.triu(G) + np.triu(G, 1).T
    inv = 1.0 / np.diagonal(G)
    tau = np.abs(u).max() * np.array([0.5, 0.1, 0.01])[:K]
    warm = rng.standard_normal((K, d)) * (rng.random((K, d)) < 0.3)
    return G, u, inv, tau, warm, float(b @ b)


# ---- 1. the defaults ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 17, 130])
def test_the_mirror_with_defaults_is_host_gram_cd(ciao, d):
    from ciaoalgorithms_jl_amd.host_route import host_gram_cd, host_gram_cd_general
    G, u, inv, tau, warm, bb = gram_case(d)
    K = len(tau)
    for X0 in (np.zeros((K, d)), warm):
        for tol, ms in ((0.0, 3), (1e-7 * bb, 40)):
            want = host_gram_cd(G, u, inv, tau, X0, tol, ms)
            got = host_gram_cd_general(G, u, inv, tau, X0, tol, ms)
            spelled = host_gram_cd_general(G[None], np.tile(u, (K, 1)), np.tile(inv, (K, 1)), tau, X0, np.full(K, tol), ms, gsel=np.zeros(K, np.int32),
                                           pf=np.ones(d), lo=np.full((K, d), -np.inf), hi=np.full(d, np.inf))
            for w, g, s in zip(want, got, spelled):
                assert same(w, g) and same(w, s), (d, tol, ms)
            assert want[2][:, 1].max() >= 1 or d == 1


# ---- 2. the six problems -----------------------------------------------------------------------------------------------------------------------
def six_cases(d):
    pfm = np.ones(d)
    pfm[::3] = 0.3
    pfm[[4, 7]] = 0.0
    lom, him = np.full(d, -np.inf), np.full(d, np.inf)
    lom[4], him[4], lom[7], him[7] = -0.02, 0.02, -0.01, 0.01
    pfe = np.ones(d)
    pfe[2] = 0.0
    return {"plain": {}, "non-negative": dict(lower=0.0), "box": dict(lower=-0.5, upper=0.7),
            "mixed": dict(penalty_factor=pfm, lower=lom, upper=him), "elastic-net": dict(ridge=0.05),
            "elastic-net+": dict(ridge=0.05, lower=0.0, penalty_factor=pfe)}


def projected_fista(G, u, sum_bb, c, mu, pf, lo, hi, ridge, iterations):
    """min (c/2)(x'Gx - 2u'x + sum_bb) + sum mu pf_j |x_j| + (ridge/2)|x|^2 over the box, by FISTA on the smooth part with the exact prox
    of the rest (soft threshold, shrink by 1 / (1 + step ridge), clamp: the prox of a separable convex function plus an interval's
    indicator is the clamp of the unconstrained prox).  Shares nothing with the package."""
    d = len(u)
    step = 1.0 / (c * np.linalg.eigvalsh(G)[-1])
    x = np.zeros(d)
    y, t = x.copy(), 1.0
    thr = step * mu * pf
    for _ in range(iterations):
        z = y - step * c * (G @ y - u)
        xn = np.clip(np.sign(z) * np.maximum(np.abs(z) - thr, 0.0) / (1.0 + step * ridge), lo, hi)
        tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        y = xn + ((t - 1.0) / tn) * (xn - x)
        x, t = xn, tn
    return x


def objective(G, u, sum_bb, c, mu, pf, ridge, x):
    return 0.5 * c * (x @ (G @ x) - 2.0 * (u @ x) + sum_bb) + mu * float(pf @ np.abs(x)) + 0.5 * ridge * float(x @ x)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_six_problems_reach_a_gap_that_bounds_the_distance_to_an_independent_solver(ciao, shape):
    import torch
    from ciaoalgorithms_jl_amd import gram as GR
    N, d = shape
    A, b = lasso_case(N, d)
    st = GR.host_gram_stats(A, b, lam=float(N))
    q = GR.GramLasso(st)
    mu = 0.1 * GR.mu_max(st)
    G, u, c = st.G.numpy(), st.u.numpy(), st.lam / st.N
    for name, kw in six_cases(d).items():
        p = GR.lasso_cd(st, [mu], gap=GAP, **kw)
        x = p.x[0].numpy()
        cert = p.certificates[0]
        pf = np.broadcast_to(np.asarray(kw.get("penalty_factor", 1.0), np.float64), (d,))
        lo = np.broadcast_to(np.asarray(kw.get("lower", -np.inf), np.float64), (d,))
        hi = np.broadcast_to(np.asarray(kw.get("upper", np.inf), np.float64), (d,))
        ridge = kw.get("ridge", 0.0)
        gp, obj = GR.constrained_gaps(st, p.x[0][:, None], [mu], **kw)
        gp, obj = float(gp[0]), float(obj[0])
        xr = projected_fista(G, u, st.sum_bb, c, mu, pf, lo, hi, ridge, FISTA_ITERATIONS)
        obj_r = objective(G, u, st.sum_bb, c, mu, pf, ridge, xr)
        mine = objective(G, u, st.sum_bb, c, mu, pf, ridge, x)
        floor = 2.0 * (q.value_floor(x) + q.value_floor(xr))       # what the rounding of the two evaluated objectives can amount to
        print(f"{shape} {name}: sweeps {p.iterations} gap {gp:.3e} objective {obj:.12g} fista {obj_r:.12g} difference {obj - obj_r:.3e} "
              f"floor {floor:.1e} nnz {int((x != 0).sum())}")
        assert p.converged == [True] and gp <= GAP * max(1.0, obj), name
        assert (x >= lo).all() and (x <= hi).all() and abs(mine - obj) <= floor, name
        assert gp >= obj - obj_r - floor, name                      # the gap bounds objective - optimum, and optimum <= the FISTA value
        assert obj_r - obj <= 1e-6 * max(1.0, obj), name            # ... which is itself near the optimum: the comparison means something
        if name == "plain":
            g0, o0 = GR._path_gaps(q, torch.tensor([mu], dtype=torch.float64), p.x[0][:, None])
            assert abs(float(g0[0]) - gp) <= floor and abs(float(o0[0]) - obj) <= floor      # lasso_path's gap, up to rounding
            ref = GR.lasso_cd(st, [mu], gap=GAP, penalty_factor=None, lower=None, upper=None, ridge=0.0)
            assert same(ref.x[0].numpy(), x) and ref.certificates == p.certificates
        else:
            assert cert.gap == gp and cert.objective == obj and np.isnan(cert.residual) and cert.box_violation == 0.0, name
        if "lower" in kw or "upper" in kw:
            # at a bound: x_j on a non-zero bound, or held at a zero bound that binds (without it the coordinate would leave 0:
            # the gradient beats the l1 weight towards the closed side)
            grad = c * (G @ x - u)
            at = ((x == lo) & (lo < 0)) | ((x == hi) & (hi > 0)) | ((x == 0) & (lo == 0) & (grad > mu * pf)) | ((x == 0) & (hi == 0) & (grad < -mu * pf))
            inside = (x > lo) & (x < hi) & (x != 0)
            assert at.any() and inside.any(), f"{name}: a broken case: no coordinate at a bound, or none strictly inside"


# ---- 3. elastic net --------------------------------------------------------------------------------------------------------------------------
def test_elastic_net_is_the_plain_mirror_on_the_shifted_matrix(ciao):
    from ciaoalgorithms_jl_amd.host_route import host_gram_cd, host_gram_cd_general
    rng = np.random.default_rng(5)
    d, N = 17, 60
    A = rng.standard_normal((N, d))
    b = A @ (rng.standard_normal(d) * (rng.random(d) < 0.4)) + 0.1 * rng.standard_normal(N)
    G, u = A.T @ A, A.T @ b
    ridges = np.array([0.5, 3.0, 20.0])
    tau = np.abs(u).max() * np.array([0.3, 0.1, 0.02])
    inv = 1.0 / (np.diagonal(G)[None, :] + ridges[:, None])
    X, _, st = host_gram_cd_general(G, u, inv, tau, np.zeros((3, d)), 1e-26, 1000)
    assert (st[:, 3] == 1).all()
    for k, rg in enumerate(ridges):
        Gs = G + rg * np.eye(d)
        Xp, _, sp = host_gram_cd(Gs, u, 1.0 / np.diagonal(Gs), tau[k:k + 1], np.zeros((1, d)), 1e-26, 1000)
        assert sp[0, 3] == 1 and (Xp != 0).any()
        assert np.abs(X[k] - Xp[0]).max() <= 1e-12 * np.abs(Xp).max(), (k, np.abs(X[k] - Xp[0]).max())


# ---- 4. states 3 and 2 -------------------------------------------------------------------------------------------------------------------------
def test_what_a_model_cannot_run_on_ends_that_model_only(ciao):
    from ciaoalgorithms_jl_amd.host_route import host_gram_cd_general
    d, K = 17, 4
    G, u, inv, tau, warm, bb = gram_case(d, seed=1, K=3)
    tau = np.append(tau, tau[0] * 0.7)
    warm = np.vstack([warm, warm[:1]])
    G3 = np.stack([G, 2.0 * G, 0.5 * G])
    inv3 = np.stack([inv, inv / 2.0, inv * 2.0])
    gsel = np.array([2, 0, 1, 0], np.int32)
    base = dict(gsel=gsel, pf=np.full((K, d), 0.8), lo=np.full((K, d), -0.6), hi=np.full((K, d), 0.9))
    tol = np.full(K, 1e-9 * bb)
    U, INV = np.tile(u, (K, 1)), inv3[gsel]
    want = host_gram_cd_general(G3, U, INV, tau, warm, tol, 40, **base)
    assert np.isin(want[2][:, 3], (0, 1)).all() and (want[2][:, 1] > 0).all()

    def spoil(name, value, j=5):
        kw = {k: v.copy() for k, v in base.items()}
        t = tol.copy()
        if name == "tol":
            t[1] = value
        elif name == "gsel":
            kw["gsel"][1] = value
        else:
            kw[name][1, j] = value
        return kw, t

    bad = [("gsel", -1), ("gsel", 3), ("pf", -1e-300), ("pf", np.nan), ("lo", 1e-300), ("lo", np.nan), ("hi", -1e-300), ("hi", np.nan),
           ("tol", -1e-300), ("tol", np.nan)]
    for name, value in bad:
        kw, t = spoil(name, value)
        X, R, st = host_gram_cd_general(G3, U, INV, tau, warm, t, 40, **kw)
        assert st[1].tolist() == [0.0, 0.0, 0.0, 3.0], (name, value)
        assert same(X[1], warm[1]) and np.isnan(R[1]).all(), (name, value)
        for k in (0, 2, 3):
            assert same(X[k], want[0][k]) and same(R[k], want[1][k]) and same(st[k], want[2][k]), (name, value, k)
    # t_kj = tau_k pf_kj NaN: 0 inf
    kw, t = spoil("pf", np.inf)
    tz = tau.copy()
    tz[1] = 0.0
    _, _, st = host_gram_cd_general(G3, U, INV, tz, warm, t, 40, **kw)
    assert st[1, 3] == 3 and same(np.delete(st, 1, 0), np.delete(want[2], 1, 0))
    # what IS allowed: zero bounds of either sign, pf = 0 and +inf, a warm start outside its bounds (it is brought inside)
    kw, t = spoil("pf", np.inf)
    kw["pf"][1, 6] = 0.0
    kw["lo"][1, :3] = -0.0
    kw["hi"][1, 3:5] = 0.0
    out = warm.copy()
    out[1, 8] = 7.0
    X, _, st = host_gram_cd_general(G3, U, INV, tau, out, t, 200, **kw)
    assert st[1, 3] == 1 and X[1, 5] == 0 and (X[1, :3] >= 0).all() and (X[1, 3:5] <= 0).all() and -0.6 <= X[1, 8] <= 0.9
    # a NaN in ONE model's u: state 2 for it, the others as they were
    Un = U.copy()
    Un[2, 4] = np.nan
    X, R, st = host_gram_cd_general(G3, Un, INV, tau, warm, tol, 40, **base)
    assert st[2, 3] == 2 and np.isnan(R[2, 4])
    for k in (0, 1, 3):
        assert same(X[k], want[0][k]) and same(R[k], want[1][k]) and same(st[k], want[2][k])
    for wrong in (lambda: host_gram_cd_general(G3, U, INV, tau, warm, tol, 0), lambda: host_gram_cd_general(G3, U[:, :-1], INV, tau, warm, tol, 5),
                  lambda: host_gram_cd_general(G3, U, INV, tau, warm, tol[:-1], 5), lambda: host_gram_cd_general(G3[:, :-1], U, INV, tau, warm, tol, 5)):
        with pytest.raises(ValueError):
            wrong()


def test_a_model_does_not_depend_on_its_neighbours(ciao):
    from ciaoalgorithms_jl_amd.host_route import host_gram_cd_general
    d, K = 17, 3
    G, u, inv, tau, warm, bb = gram_case(d, seed=2)
    G3 = np.stack([G, 2.0 * G, 0.5 * G])
    gsel = np.array([1, 2, 0], np.int32)
    rng = np.random.default_rng(3)
    pf, lo, hi = rng.random((K, d)) * 2, -rng.random((K, d)), rng.random((K, d))
    lo[0], hi[2] = -np.inf, np.inf
    U = u[None, :] * np.array([1.0, -1.0, 0.5])[:, None]
    INV = np.stack([inv / 2.0, inv * 2.0, inv])
    tol = np.array([1e-9, 0.0, 1e-6]) * bb
    want = host_gram_cd_general(G3, U, INV, tau, warm, tol, 25, gsel=gsel, pf=pf, lo=lo, hi=hi)
    for order in ([2, 0, 1], [1], [0, 0, 2]):
        o = np.array(order)
        got = host_gram_cd_general(G3, U[o], INV[o], tau[o], warm[o], tol[o], 25, gsel=gsel[o], pf=pf[o], lo=lo[o], hi=hi[o])
        assert all(same(g, w[o]) for g, w in zip(got, want)), order


# ---- 5. the drivers ----------------------------------------------------------------------------------------------------------------------------
def test_driver_refusals_and_forwarding(ciao):
    import torch
    from ciaoalgorithms_jl_amd import gram as GR
    A, b = lasso_case(200, 50)
    st = GR.host_gram_stats(A, b, lam=200.0)
    mus = [0.3 * GR.mu_max(st), 0.05 * GR.mu_max(st)]
    free = np.ones(50)
    free[3] = 0.0
    one_side = np.full(50, -np.inf)
    one_side[3] = -1.0
    for kw in (dict(penalty_factor=free), dict(penalty_factor=free, lower=one_side), dict(penalty_factor=free, upper=1.0)):
        with pytest.raises(ValueError, match="Bound the coordinate.*add a ridge.*standardized"):
            GR.lasso_cd(st, mus, **kw)
    # ... bounded on both sides, or with a ridge, it runs
    assert all(GR.lasso_cd(st, mus, penalty_factor=free, lower=one_side, upper=1.0).converged)
    assert all(GR.lasso_cd(st, mus, penalty_factor=free, ridge=0.01).converged)
    for kw in (dict(penalty_factor=-1.0), dict(penalty_factor=np.full(50, np.nan)), dict(lower=0.5), dict(upper=-0.5), dict(lower=np.nan),
               dict(ridge=-1.0), dict(ridge=np.inf), dict(lower=np.zeros(49))):
        with pytest.raises(ValueError):
            GR.lasso_cd(st, mus, **kw)
    with pytest.raises(ValueError, match="method='cd'"):
        GR.lasso_path(st, mus, lower=0.0)
    a, f = GR.lasso_cd(st, mus, lower=0.0, ridge=0.01), GR.lasso_path(st, mus, lower=0.0, ridge=0.01, method="cd")
    assert a.iterations == f.iterations and all(torch.equal(x, y) for x, y in zip(a.x, f.x)) and all(a.converged)
    # an excluded coordinate stays out; a model is the same alone as among others; float32 output
    out = np.ones(50)
    out[0] = np.inf
    e = GR.lasso_cd(st, mus, penalty_factor=out, x0=np.ones(50))
    assert all(e.converged) and all(float(x[0]) == 0.0 for x in e.x) and all(c.gap <= 1e-9 * max(1.0, c.objective) for c in e.certificates)
    assert torch.equal(GR.lasso_cd(st, mus[1:], lower=0.0, ridge=0.01).x[0], a.x[1])
    assert GR.lasso_cd(st, mus, lower=0.0, dtype=torch.float32).x[0].dtype == torch.float32
    short = GR.lasso_cd(st, [mus[1]], gap=1e-13, max_sweeps=2, lower=0.0)
    assert short.converged == [False] and short.iterations == 2
    assert ciao.constrained_gaps is GR.constrained_gaps


# ---- 6. fused cross-validation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, dict(lower=0.0, ridge=0.25), dict(penalty_factor=0.5, upper=2.0)], ids=["plain", "nn-ridge", "factor-upper"])
def test_fused_cross_validation_is_the_unfused_one_bit_for_bit(ciao, kw):
    import torch
    from ciaoalgorithms_jl_amd import cv as CV
    from ciaoalgorithms_jl_amd import gram as GR
    rng = np.random.default_rng(16)
    N, d, folds = 300, 24, 3
    A = rng.integers(-8, 9, (N, d)).astype(np.float64)
    xt = np.zeros(d)
    xt[:6] = rng.integers(-3, 4, 6)
    b = A @ xt + rng.integers(-4, 5, N)
    stats = CV.fold_stats(None, (A, b, 1.0), CV.fold_lists(N, folds, seed=5))
    whole = GR.add_stats(stats)
    mus = [f * GR.mu_max(whole) for f in (0.5, 0.2, 0.05, 0.01)]
    one = CV.lasso_cv_from_stats(stats, mus, fused=False, **kw)
    all_ = CV.lasso_cv_from_stats(stats, mus, fused=True, **kw)
    assert all(one.path.converged) and all(all_.path.converged)
    # every model of every fold converged, far from the sweep budget (the premise of the equality)
    for f in range(folds):
        fit = GR.lasso_cd(GR.add_stats([s for g, s in enumerate(stats) if g != f]), mus, gap=1e-6, **kw)
        assert all(fit.converged) and fit.iterations < 1000
    for name in ("mse", "mean", "stderr"):
        assert same(getattr(one, name).numpy(), getattr(all_, name).numpy()), name
    assert (one.best, one.one_se, one.floor, one.mus) == (all_.best, all_.one_se, all_.floor, all_.mus)
    assert one.path.iterations == all_.path.iterations and one.path.converged == all_.path.converged
    assert all(same(x.numpy(), y.numpy()) for x, y in zip(one.path.x, all_.path.x))
    assert one.path.certificates == all_.path.certificates or kw     # (NaN fields of the general certificates do not compare equal)
    assert [c.gap for c in one.path.certificates] == [c.gap for c in all_.path.certificates]
    with pytest.raises(ValueError, match="method='cd'"):
        CV.lasso_cv_from_stats(stats, mus, fused=True, method="fista")


def test_the_four_general_kernels_have_no_scratch_and_no_spills(ciao):
    """The built library holds exactly four general coordinate-descent kernels (two block sizes x two load kinds), none with scratch
    memory or spilled registers, beside the four of ciao_gram_cd."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    lib = os.path.join(ROOT, "ciaoalgorithms.jl_amd", "libciao_hip.so")
    assert os.path.exists(lib), "build the library first (__graft_entry__.build())"
    mine = [r for r in kernel_meta.library_kernels(lib) if "ciao::gramcdg_kernel<" in r["name"]]
    assert sorted(r["name"].split("(")[0].split("gramcdg_kernel")[1].replace(" ", "") for r in mine) == ["<1024,false>", "<1024,true>", "<256,false>", "<256,true>"]
    for r in mine:
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r.get("sgpr_spill", 0) == 0, r

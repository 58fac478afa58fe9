"""Coordinate descent for the d-space lasso, without a GPU (host_route.host_gram_cd, gram.lasso_cd, lasso_path(method="cd"),
logistic_newton(subproblem="cd")):

  1. the numpy mirror -- the specification of ciao_gram_cd -- against closed forms: d = 1, a diagonal G (soft-thresholding), G_jj = 0,
     a NaN in u (state 2, x untouched there), max_sweeps = 1 (state 0), the residual it returns;
  2. lasso_cd on host_gram_stats at four shapes (one with d > N and a singular G) and three l1 weights: every model converged, its
     certificate confirms the gap, and its objective agrees with lasso_path's within what two certified gaps allow:
         |objective_cd - objective_fista| <= 2 gap max(1, objective) + value_floor_cd + value_floor_fista
     (both objectives lie within their own gap above the same minimum; each value is known up to its floor);
  3. weighted statistics are accepted, method="cd" forwards, bad arguments are refused;
  4. logistic_newton(HostRows, subproblem="cd") reaches the gap the default reaches, at the shapes of tests/test_gram_weighted_host.py;
  5. lasso_path's default is what it was: the same bits as method="fista" given explicitly, and as a result recorded from the parent
     commit under tests/golden/.
"""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(6, 3), (200, 50), (300, 130), (150, 257)]
MU_FRACTIONS = (0.5, 0.1, 0.01)
NEWTON_SHAPES = [(6, 3, 2), (200, 50, 5), (300, 130, 7)]
GAP = 1e-9


def lasso_case(N, d, seed=None):
    """Gaussian rows with a near-collinear column pair (correlation 0.995) and targets from a sparse vector plus noise"""
    rng = np.random.default_rng(d if seed is None else seed)
    A = rng.standard_normal((N, d))
    A[:, 1] = A[:, 0] + 0.1 * rng.standard_normal(N)
    xt = rng.standard_normal(d) * (rng.random(d) < 0.2)
    return A, A @ xt + 0.1 * rng.standard_normal(N)


def cd(G, u, tau, X=None, tol=0.0, max_sweeps=100):
    from ciaoalgorithms_jl_amd.host_route import host_gram_cd
    G, u = np.asarray(G, np.float64), np.asarray(u, np.float64)
    dg = np.diagonal(G)
    with np.errstate(divide="ignore"):
        inv = np.where(dg > 0, 1.0 / dg, 0.0)
    tau = np.atleast_1d(np.asarray(tau, np.float64))
    X = np.zeros((len(tau), len(u))) if X is None else X
    return host_gram_cd(G, u, inv, tau, X, tol, max_sweeps)


def soft(v, t):
    return np.sign(v) * np.maximum(np.abs(v) - t, 0.0)


def test_mirror_against_closed_forms(ciao):
    # d = 1: x = soft(u, tau) / g in one update (numbers whose products are exact)
    for g, u, tau in ((2.0, 3.0, 1.0), (2.0, -3.0, 1.0), (2.0, 0.5, 1.0), (0.25, 7.0, 0.0)):
        X, R, st = cd([[g]], [u], [tau])
        want = np.copysign(max(abs(u) - tau, 0.0), u) * (1.0 / g)
        assert X[0, 0] == want and R[0, 0] == u - g * want
        moved = want != 0
        # (moved: the full sweep, an active sweep that moves nothing, the full sweep that confirms; the last full sweep's change is 0)
        assert st[0].tolist() == [3.0 if moved else 1.0, 1.0 if moved else 0.0, 0.0, 1.0]
    # a diagonal G: every coordinate is its own problem; K models at once; a warm start ends where the cold one does
    rng = np.random.default_rng(0)
    d = 7
    g, u = rng.random(d) + 0.5, rng.standard_normal(d)
    taus = np.array([0.0, 0.3, 0.8, 10.0])
    X, R, st = cd(np.diag(g), u, taus)
    for k, t in enumerate(taus):
        want = np.array([np.copysign(max(abs(v) - t, 0.0), v) * (1.0 / gj) for v, gj in zip(u, g)])
        # (tol = 0 iterates to the fixed point of the rounded update: rho = r_j + g_j x_j returns u_j up to two roundings)
        assert np.abs(X[k] - want).max() <= 4 * 2.0 ** -53 * np.abs(want).max() and st[k, 3] == 1
        assert np.abs(R[k] - (u - g * want)).max() <= 2 * 2.0 ** -53 * np.abs(u).max()
    assert not X[3].any() and st[3].tolist() == [1.0, 0.0, 0.0, 1.0]
    # (a tolerance of 0 asks for a fixed point to the bit, which a warm start may circle in the last place: 1e-30 bounds delta by 1e-15)
    Xw, _, stw = cd(np.diag(g), u, taus, X=rng.standard_normal((4, d)), tol=1e-30)
    assert np.abs(Xw - X).max() <= 1e-14 and (stw[:, 3] == 1).all()
    # the input is not written
    X0 = rng.standard_normal((1, d))
    keep = X0.copy()
    cd(np.diag(g), u, [0.1], X=X0)
    assert np.array_equal(X0, keep)
    # G_jj = 0 (a zero column: u_j = 0 too, inv_j = 0): a warm x_j is driven to 0, a cold one stays
    G = np.diag([1.0, 0.0, 2.0])
    X, R, st = cd(G, [1.0, 0.0, -3.0], [0.5], X=np.array([[0.0, 4.0, 0.0]]))
    assert X[0].tolist() == [0.5, 0.0, -1.25] and st[0, 3] == 1
    # a NaN in u: the coordinate's delta is not finite -> state 2 at once, x unchanged there, the coordinates before it updated
    X, R, st = cd(np.diag([1.0, 1.0, 1.0]), [2.0, np.nan, 2.0], [0.5], X=np.array([[0.0, 0.25, 0.0]]))
    assert st[0, 3] == 2 and st[0, 0] == 1 and X[0].tolist() == [1.5, 0.25, 0.0] and np.isnan(R[0, 1])
    # max_sweeps = 1 on a coupled problem: the budget is spent -> state 0, one sweep made; more sweeps converge
    A, b = lasso_case(40, 5, 1)
    G, u = A.T @ A, A.T @ b
    X1, _, st1 = cd(G, u, [0.1 * np.abs(u).max()], max_sweeps=1)
    assert st1[0, 3] == 0 and st1[0, 0] == 1 and st1[0, 1] >= 1 and st1[0, 2] > 0
    X2, R2, st2 = cd(G, u, [0.1 * np.abs(u).max()], tol=1e-20, max_sweeps=500)
    assert st2[0, 3] == 1 and 2 <= st2[0, 0] < 500
    # the optimality conditions of the lasso at the converged point: |r_j| <= tau off the support, r_j = tau sign(x_j) on it
    tau = 0.1 * np.abs(u).max()
    r = u - G @ X2[0]
    assert np.abs(R2[0] - r).max() <= 1e-12 * np.abs(u).max()
    on = X2[0] != 0
    assert on.any() and np.abs(r[on] - tau * np.sign(X2[0][on])).max() <= 1e-8 * tau and (np.abs(r[~on]) <= tau * (1 + 1e-8)).all()
    # two launches of one sweep each are one launch of two sweeps while no active sweep intervenes ... and relaunching from a
    # converged point moves nothing
    X3, _, st3 = cd(G, u, [tau], X=X2, tol=1e-20)
    assert st3[0, 3] == 1 and np.abs(X3 - X2).max() <= 1e-12
    with pytest.raises(ValueError):
        cd(G, u, [tau], tol=-1.0)
    with pytest.raises(ValueError):
        cd(G, u, [tau], max_sweeps=0)
    with pytest.raises(ValueError):
        cd(G, u[:-1], [tau])


@pytest.fixture(scope="module")
def solved(ciao):
    """lasso_cd and lasso_path at every shape, once"""
    from ciaoalgorithms_jl_amd import gram as GR
    out = {}
    for N, d in SHAPES:
        A, b = lasso_case(N, d)
        st = GR.host_gram_stats(A, b, lam=float(N))
        mus = [f * GR.mu_max(st) for f in MU_FRACTIONS]
        out[(N, d)] = (st, mus, GR.lasso_cd(st, mus, gap=GAP), GR.lasso_path(st, mus, gap=GAP, maxit=100000))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_lasso_cd_reaches_the_gap_and_agrees_with_fista(ciao, solved, shape):
    import torch
    from ciaoalgorithms_jl_amd import gram as GR
    st, mus, pc, pf = solved[shape]
    q = GR.GramLasso(st)
    assert all(pf.converged), "the FISTA reference did not reach its gap"
    assert isinstance(pc, GR.LassoPath) and len(pc.x) == len(mus) and pc.iterations >= len(mus)
    for k, mu in enumerate(mus):
        cc, cf = pc.certificates[k], pf.certificates[k]
        print(f"{shape} mu {MU_FRACTIONS[k]} mu_max: cd gap {cc.gap:.3e} objective {cc.objective:.12g} nnz {int((pc.x[k] != 0).sum())}; "
              f"fista gap {cf.gap:.3e} objective {cf.objective:.12g}; sweeps (all models) {pc.iterations}, fista iterations {pf.iterations}")
        assert pc.converged[k] and pc.x[k].dtype == torch.float64 and pc.x[k].shape == (shape[1],)
        assert cc.gap <= GAP * max(1.0, cc.objective)
        # the certificate is the one GramLasso gives at the returned vector
        assert cc.gap == q.certificate(pc.x[k], mu, 1.0).gap
        bound = 2 * GAP * max(1.0, cc.objective) + q.value_floor(pc.x[k]) + q.value_floor(pf.x[k])
        assert abs(cc.objective - cf.objective) <= bound, (cc.objective, cf.objective, bound)


def test_weighted_statistics_forwarding_and_refusals(ciao):
    import torch
    from ciaoalgorithms_jl_amd import gram as GR
    A, b = lasso_case(200, 50)
    w = np.random.default_rng(1).random(200) + 0.5
    st = GR.host_gram_stats(A, b, lam=200.0, weights=w)
    assert st.sum_w is not None
    mus = [0.3 * GR.mu_max(st), 0.05 * GR.mu_max(st)]
    pc = GR.lasso_cd(st, mus, gap=GAP)
    assert all(pc.converged) and all(c.gap <= GAP * max(1.0, c.objective) for c in pc.certificates)
    # ... the weighted problem is the plain one on the rows scaled by sqrt(w)
    sw = np.sqrt(w)
    ps = GR.lasso_cd(GR.host_gram_stats(sw[:, None] * A, sw * b, lam=200.0), mus, gap=GAP)
    for a, c in zip(pc.certificates, ps.certificates):
        assert abs(a.objective - c.objective) <= 2 * GAP * max(1.0, a.objective) + 1e-12 * a.objective
    # method="cd" forwards: the same bits as lasso_cd, warm starts and dtype included
    fw = GR.lasso_path(st, mus, gap=GAP, method="cd")
    assert fw.iterations == pc.iterations and all(torch.equal(a, c) for a, c in zip(fw.x, pc.x))
    warm = GR.lasso_path(st, mus, x0=pc.x, gap=GAP, method="cd", dtype=torch.float32)
    assert all(warm.converged) and warm.x[0].dtype == torch.float32 and warm.iterations <= 2 * len(mus)
    one = GR.lasso_cd(st, mus[:1], x0=pc.x[0], gap=GAP)
    assert one.converged == [True] and one.iterations == 1
    # a model is the same alone as among others
    assert torch.equal(GR.lasso_cd(st, mus[1:], gap=GAP).x[0], pc.x[1])
    # beyond mu_max: x = 0 after one sweep
    z = GR.lasso_cd(st, [1.5 * GR.mu_max(st)], gap=GAP)
    assert z.converged == [True] and not z.x[0].any() and z.iterations == 1
    for bad in (lambda: GR.lasso_cd(st, []), lambda: GR.lasso_cd(st, [0.0]), lambda: GR.lasso_cd(st, [0.1, 0.2], x0=[np.zeros(50)]),
                lambda: GR.lasso_cd(st, [0.1], gap=0.0), lambda: GR.lasso_cd(st, [0.1], max_sweeps=0),
                lambda: GR.lasso_path(st, [0.1], method="newton")):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ciao._lib.CiaoError):
        GR.lasso_cd(GR.host_gram_stats(A, np.sign(b), kind="logistic"), [0.1])
    # the sweep budget: a model that has not met its gap when it is spent is reported, not hidden
    short = GR.lasso_cd(st, [mus[1]], gap=1e-13, max_sweeps=2)
    assert short.converged == [False] and short.iterations == 2


@pytest.mark.parametrize("shape", NEWTON_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_newton_with_the_cd_subproblem_reaches_the_gap(ciao, shape):
    from test_gram_weighted_host import logistic_case
    from ciaoalgorithms_jl_amd.newton import HostRows, logistic_newton, logistic_path
    N, d, seed = shape
    A, y, mu_max = logistic_case(N, d, seed)
    rows = HostRows(A, y)
    for frac in (0.5, 0.1):
        mu = frac * mu_max
        r = logistic_newton(rows, mu, gap=GAP, subproblem="cd")
        r0 = logistic_newton(rows, mu, gap=GAP)
        c, c0 = r.certificate, r0.certificate
        print(f"N={N} d={d} mu={frac} mu_max: cd outer {r.outer} gap {c.gap:.3e} objective {c.objective:.12f} {r.reason}; "
              f"fista outer {r0.outer} gap {c0.gap:.3e} objective {c0.objective:.12f}")
        assert r.converged and r.reason == "gap" and c.gap <= GAP * max(1.0, c.objective)
        assert r0.converged and abs(c.objective - c0.objective) <= max(c.gap, c0.gap) + 1e-13 * c.objective
        assert isinstance(r.x, np.ndarray) and r.x.dtype == np.float64
    if shape == NEWTON_SHAPES[1]:
        path = logistic_path(rows, [0.5 * mu_max, 0.25 * mu_max], gap=GAP, subproblem="cd")
        assert [p.converged for p in path] == [True, True]
        with pytest.raises(ValueError):
            logistic_newton(rows, 0.1 * mu_max, subproblem="lars")


def test_the_default_of_lasso_path_is_unchanged(ciao):
    """The default method is FISTA as on the parent commit: the same bits as method="fista", and as the result recorded from the parent's
    code (tests/golden/lasso_path_fista_6x3_f64.json: x, iterations, converged, gaps, objectives of lasso_case(6, 3), lam = 6, the three
    l1 weights)."""
    import torch
    from ciaoalgorithms_jl_amd import gram as GR
    A, b = lasso_case(6, 3)
    st = GR.host_gram_stats(A, b, lam=6.0)
    mus = [f * GR.mu_max(st) for f in MU_FRACTIONS]
    p = GR.lasso_path(st, mus, gap=GAP)
    e = GR.lasso_path(st, mus, gap=GAP, method="fista")
    assert p.iterations == e.iterations and p.converged == e.converged
    assert all(torch.equal(a.view(torch.int64), c.view(torch.int64)) for a, c in zip(p.x, e.x))
    with open(os.path.join(ROOT, "tests", "golden", "lasso_path_fista_6x3_f64.json")) as fh:
        g = json.load(fh)
    assert p.iterations == g["iterations"] and p.converged == g["converged"]
    assert [[float(v).hex() for v in x.tolist()] for x in p.x] == g["x"]
    assert [float(c.gap).hex() for c in p.certificates] == g["gap"] and [float(c.objective).hex() for c in p.certificates] == g["objective"]
    # a warm start and a single vector for all go the same way
    A2, b2 = lasso_case(200, 50)
    st2 = GR.host_gram_stats(A2, b2, lam=200.0)
    m2 = [0.1 * GR.mu_max(st2)]
    a1, a2 = GR.lasso_path(st2, m2, x0=np.ones(50), maxit=50), GR.lasso_path(st2, m2, x0=np.ones(50), maxit=50, method="fista")
    assert torch.equal(a1.x[0].view(torch.int64), a2.x[0].view(torch.int64)) and a1.certificates == a2.certificates


def test_the_four_kernels_have_no_scratch_and_no_spills(ciao):
    """The built library holds exactly four coordinate-descent kernels (two block sizes x two load kinds), none with scratch memory or
    spilled registers (tools/kernel_meta.py reads the gfx950 code objects of libciao_hip.so, as tests/test_kernel_resources.py does)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    lib = os.path.join(ROOT, "ciaoalgorithms.jl_amd", "libciao_hip.so")
    assert os.path.exists(lib), "build the library first (__graft_entry__.build())"
    mine = [r for r in kernel_meta.library_kernels(lib) if "ciao::gramcd_kernel<" in r["name"]]
    assert sorted(r["name"].split("(")[0].split("gramcd_kernel")[1].replace(" ", "") for r in mine) == ["<1024,false>", "<1024,true>", "<256,false>", "<256,true>"]
    for r in mine:
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r.get("sgpr_spill", 0) == 0, r

"""Gram statistics on the device (ciao_gram, Context.gram, gram.py; csrc/gram_kernels.h).

  1. exact on integers: |a| <= 64, so every partial sum is an integer below 2^53 and ANY order of addition must give numpy's int64 result:
     all five outputs, fp64 and fp32 rows, at every threshold of gram_plan, in four layouts of the same matrix, NaN around and inside every
     buffer, the launch's own report against a restatement of the plan;
  2. bits: symmetry, a second call, the layouts, fp32 rows against their .double() copy, every NULL output;
  3. Gaussian rows against exact sums under a derived bound;
  4. the siblings: col_sqnorms, col_moments, full_gradient;
  5. the Python layer: smoothness_exact, GramLasso against Context.certificate, lasso_path, standardized, score_many;
  6. refusals.

The thresholds of gram_plan (csrc/gram_kernels.h).  Columns: a block is 128 columns, so the number of blocks changes at every multiple of 128
and the tiles are the pairs (ib, jb >= ib): one value just above every multiple of 128 up to 1024 -- 129, 257, 385, 513, 641, 769, 897, 1025:
3, 6, 10, 15, 21, 28, 36, 45 tiles -- with 127 | 128 and 255 | 256 below and at.  From 28 tiles on the 256 MiB workspace caps the partitions
asked for.  Every further multiple of 128 runs the same tile decoding with a smaller cap; those sizes are left to tools/gram_time.py (at
d = 4096 G alone is 128 MiB).  Rows: an MFMA step is 4 rows, a staged chunk 16, a partition `per` rows = whole chunks:
16 rows until N exceeds 16 * want, so N = 16 | 17 is one | two partitions, N = 128 | 129 is 8 (the XCD map) | 9 (the plain map), and
N = 16 * want + 1 is the first with two chunks a partition: 32129 at d <= 17 (with it a thousand records for the final kernel's loop, which
has no other branch) and 769 at d >= 897 (the capped plan); between those d the matrix would exceed a few MB.  Large N goes with small d and the other way round: no matrix here is larger than a few MB."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from layouts import Guarded, bits, has_poison

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
T, KC, REC, WG_TARGET, WS = 128, 16, 128 * 128 + 2 * 128 + 8, 2048, 256 << 20


def tdtype(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


def tname(dtype):
    return "f64" if dtype == np.float64 else "f32"


def want_of(d):
    """the partitions gram_plan asks for -> (ntiles, want)"""
    nb = -(-d // T)
    ntiles = nb * (nb + 1) // 2
    cap = WS // (ntiles * REC * 8)
    want = min(-(-(-(-WG_TARGET // ntiles)) // 8) * 8, cap)
    return ntiles, want // 8 * 8 if want >= 8 else want


def plan(N, d):
    """gram_plan of csrc/gram_kernels.h -> (ntiles, per, P, xcd, workspace bytes)"""
    ntiles, want = want_of(d)
    per = max(KC, -(-(-(-N // want)) // KC) * KC)
    P = -(-N // per)
    return ntiles, per, P, P % 8 == 0, ntiles * P * REC * 8


D_SIZES = [1, 2, 3, 15, 16, 17, 50, 127, 128, 129, 255, 256, 257, 385, 513, 641, 769, 897, 1024, 1025]
N_SMALL = [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 127, 128, 129]


def n_sizes(d):
    ns = list(N_SMALL)
    if d <= 17 or d >= 897:                      # one below, at, one above the first two-chunk partition
        w = want_of(d)[1]
        ns += [16 * w - 1, 16 * w, 16 * w + 1]
        assert [plan(n, d)[1] for n in ns[-3:]] == [16, 16, 32] and (plan(ns[-1], d)[2] > 1000 or d >= 897)
    assert [plan(n, d)[2:4] for n in (16, 17, 128, 129)] == [(1, False), (2, False), (8, True), (9, False)]
    return ns


def kind_of(F):
    return "vec16" if F.A.data_ptr() % 16 == 0 and (F.ld * F.A.element_size()) % 16 == 0 else "elem"


def check_report(ctx, N, d, dtype, kind):
    ntiles, per, P, xcd, ws = plan(N, d)
    want = (f"gram_partial_kernel<{tname(dtype)},{kind}> grid={ntiles * P} block=256 tile=128x128 chunk=16 tiles={ntiles} partitions={P} "
            f"rows={per} map={'xcd' if xcd else 'plain'} workspace={ws}")
    assert ctx.last_kernel() == want, (ctx.last_kernel(), want)
    assert ws <= WS


def input_layouts(M, b, dtype):
    """the same matrix and targets four ways: (name, A, b) with A, b Guarded"""
    d, vec = M.shape[1], (2 if dtype == np.float64 else 4)
    mk = lambda name, ld, off: (name, Guarded(M, off=off, ld=ld, device="cuda", name=f"A {name}"), Guarded(b, off=off, device="cuda", name=f"b {name}"))
    return [mk("ld=d", d, 0), mk("ld=d+1", d + 1, 0), mk("padding", (d // vec + 2) * vec, 0), mk("base+1", d, 1)]


def problem(A, b, kind="ls", lam=1.0):
    from ciaoalgorithms_jl_amd.device import PackedF
    return PackedF.least_squares(A, b, lam) if kind == "ls" else PackedF.logistic(A, b)


class Outputs:
    """G (row stride d + 3), u, colsum, bsum, each inside a poisoned buffer of its own"""

    def __init__(self, d):
        self.G = Guarded(shape=(d, d), dtype=np.float64, ld=d + 3, device="cuda", name="G")
        self.u, self.cs, self.bs = (Guarded(shape=(n,), dtype=np.float64, device="cuda", name=nm) for n, nm in ((d, "u"), (d, "colsum"), (2, "bsum")))

    def run(self, ctx, F, u=True, colsum=True, bsum=True):
        got = ctx.gram(F, G=self.G.view, u=self.u.view if u else None, colsum=self.cs.view if colsum else None, bsum=self.bs.view if bsum else None)
        for g in (self.G, self.u, self.cs, self.bs):
            g.check_outside(ctx.last_kernel())
        return got


def int_matrix(N, d):
    """A[i,j] = ((7 i + 13 j) mod 129) - 64 and b_i = ((11 i) mod 129) - 64: |a|, |b| <= 64"""
    i = np.arange(N, dtype=np.int64)
    return (7 * i[:, None] + 13 * np.arange(d, dtype=np.int64)[None, :]) % 129 - 64, (11 * i) % 129 - 64


_INT_REF = {}


def int_gram(a):
    """a'a in int64, by slabs of 32 rows (numpy's integer product walks a long transposed operand slowly)"""
    G = np.zeros((a.shape[1], a.shape[1]), np.int64)
    for k in range(0, a.shape[0], 32):
        G += np.ascontiguousarray(a[k:k + 32].T) @ a[k:k + 32]
    return G


def int_reference(d):
    """{N: the four outputs as float64 arrays holding exact integers} in numpy int64 arithmetic, one slab of rows after the other; computed
    once per d, shared by the two types, never modified"""
    if d not in _INT_REF:
        sizes = n_sizes(d)
        ints, bi = int_matrix(sizes[-1], d)
        want, prev, acc = {}, 0, [np.zeros((d, d), np.int64), np.zeros(d, np.int64), np.zeros(d, np.int64), np.zeros(2, np.int64)]
        for N in sizes:
            a, bb = ints[prev:N], bi[prev:N]
            acc = [acc[0] + int_gram(a), acc[1] + a.T @ bb, acc[2] + a.sum(axis=0), acc[3] + np.array([bb.sum(), (bb * bb).sum()])]
            prev = N
            assert all(v.dtype == np.int64 for v in acc) and max(int(np.abs(v).max()) for v in acc) < 2 ** 53
            want[N] = [v.astype(np.float64) for v in acc]
            for v in want[N]:
                v.setflags(write=False)
        _INT_REF[d] = want
    return _INT_REF[d]


# ---- 1. exact on integers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dtype", [pytest.param(d, dt, id=f"{d}-{tname(dt)}") for dt in (np.float32, np.float64) for d in D_SIZES])
def test_integer_rows_exactly(ctx, d, dtype):
    import torch
    sizes = n_sizes(d)
    ints, bi = int_matrix(sizes[-1], d)
    want = {N: [torch.from_numpy(v.copy()).cuda() for v in ref] for N, ref in int_reference(d).items()}
    out = Outputs(d)
    kinds = set()
    for name, GA, Gb in input_layouts(torch.from_numpy(ints.astype(dtype)), torch.from_numpy(bi.astype(dtype)), dtype):
        for N in sizes:
            F = problem(GA.view[:N], Gb.view[:N])
            got = out.run(ctx, F)
            check_report(ctx, N, d, dtype, kind_of(F))
            for g, w, what in zip(got, want[N], ("G", "u", "colsum", "bsum")):
                assert torch.equal(bits(g.contiguous()), bits(w)), (what, name, N, d, ctx.last_kernel())
            kinds.add((name, kind_of(F)))
        GA.check_unchanged(name)
        Gb.check_unchanged(name)
    assert ("padding", "vec16") in kinds and ("base+1", "elem") in kinds


# ---- 2. bits ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
def test_the_same_bits(ctx, dtype):
    """G symmetric to the bit; a second call, the four layouts, a logistic view of the same rows, the .double() copy of fp32 rows and every
    NULL output leave every bit where it was.  N = 700, d = 150: three tiles, several partitions, a partial last chunk."""
    import torch
    rng = np.random.default_rng(11)
    N, d = 700, 150
    M = torch.from_numpy(rng.standard_normal((N, d)).astype(dtype))
    b = torch.from_numpy(np.sign(rng.standard_normal(N)).astype(dtype))
    out = Outputs(d)
    first = None
    for name, GA, Gb in input_layouts(M, b, dtype):
        for kind in ("ls", "logistic"):
            for rep in range(2):
                got = [g.contiguous().clone() for g in out.run(ctx, problem(GA.view, Gb.view, kind))]
                assert not any(has_poison(g) for g in got), name
                assert torch.equal(bits(got[0]), bits(got[0].T.contiguous())), "G is not symmetric to the bit"
                if first is None:
                    first = got
                assert all(torch.equal(bits(a), bits(w)) for a, w in zip(got, first)), (name, kind, rep)
    if dtype == np.float32:
        wide = [g.contiguous() for g in out.run(ctx, problem(M.double().cuda(), b.double().cuda()))]
        assert ctx.last_kernel().startswith("gram_partial_kernel<f64,")
        assert all(torch.equal(bits(a), bits(w)) for a, w in zip(wide, first)), "fp32 rows and their double copy differ"
    F = problem(M.cuda(), b.cuda())
    for mask in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0)):
        fresh = Outputs(d)
        got = fresh.run(ctx, F, *map(bool, mask))
        assert torch.equal(bits(got[0].contiguous()), bits(first[0]))
        for k, (on, g, held) in enumerate(zip(mask, got[1:], (fresh.u, fresh.cs, fresh.bs))):
            if on:
                assert torch.equal(bits(g), bits(first[1 + k]))
            else:
                assert g is None and not held.outside_touched() and bool((bits(held.view) == bits(held.flat[:1])).all())   # still the poison


# ---- 3. Gaussian rows -----------------------------------------------------------------------------------------------------------------------
GN, GD = 1000, 20
_GAUSS = {}


def gauss_case(dtype):
    """(A, b, exact, scale): Gaussian rows, column 1 with mean 10^6 sigma; exact = the four outputs correctly rounded from exact sums
    (Fractions for fp64 data; for fp32 data every product is a double, so math.fsum of the products is exact); scale = the sums of
    absolute products the bounds multiply.  Computed once, shared, never modified."""
    if dtype not in _GAUSS:
        rng = np.random.default_rng(1000)
        A = rng.standard_normal((GN, GD))
        A[:, 1] += 1e6
        A, b = A.astype(dtype), rng.standard_normal(GN).astype(dtype)
        A64, b64 = A.astype(np.float64), b.astype(np.float64)
        aug = np.concatenate([A64, b64[:, None], np.ones((GN, 1))], axis=1)
        m = GD + 2
        E = np.zeros((m, m))
        if dtype == np.float32:
            for i in range(m):
                for j in range(i, m):
                    E[i, j] = E[j, i] = math.fsum((aug[:, i] * aug[:, j]).tolist())
        else:
            cols = [[Fraction(v) for v in aug[:, i].tolist()] for i in range(m)]
            for i in range(m):
                for j in range(i, m):
                    E[i, j] = E[j, i] = float(sum(x * y for x, y in zip(cols[i], cols[j])))
        S = np.abs(aug).T @ np.abs(aug)
        for v in (A, b, E, S):
            v.setflags(write=False)
        _GAUSS[dtype] = (A, b, E, S)
    return _GAUSS[dtype]


def split(E):
    """the augmented (d + 2) x (d + 2) matrix of [a, b, 1] -> (G, u, colsum, bsum)"""
    d = E.shape[0] - 2
    return E[:d, :d], E[:d, d], E[:d, d + 1], np.array([E[d, d + 1], E[d, d]])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
def test_gaussian_rows_against_exact_sums(ctx, dtype):
    """Derived: every product is rounded once (not at all for fp32 data) and passes through at most N additions in double, whatever their
    order: |G_ij - exact| <= (N + 8) 2^-53 sum_n |a_ni a_nj|, the 8 covering the rounding of the reference and the second-order terms."""
    import torch
    A, b, E, S = gauss_case(dtype)
    F = problem(torch.from_numpy(A.copy()).cuda(), torch.from_numpy(b.copy()).cuda())
    got = [g.cpu().numpy() for g in Outputs(GD).run(ctx, F)]
    check_report(ctx, GN, GD, dtype, kind_of(F))
    for g, e, s, what in zip(got, split(E), split(S), ("G", "u", "colsum", "bsum")):
        ratio = np.abs(g - e) / ((GN + 8) * U53 * s)
        print(f"{tname(dtype)} {what}: worst |got - exact| / bound {ratio.max():.3e}")
        assert (ratio <= 1).all(), what


# ---- 4. the siblings --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
def test_agreement_with_the_siblings(ctx, dtype):
    """Both sides lie within their own bound of the exact value (sections 8.8, 8.10: (N + 3) 2^-53 sum a^2, (N + 2) 2^-53 sum |a|; the full
    gradient: its d-vector is formed in the rows' type, so one rounding of that type on top)."""
    import torch
    A, b, E, S = gauss_case(dtype)
    lam = 3.0
    F = problem(torch.from_numpy(A.copy()).cuda(), torch.from_numpy(b.copy()).cuda(), lam=lam)
    G, u, cs, _ = (g.cpu().numpy() for g in ctx.gram(F))
    SG, Su, Scs, _ = split(S)
    sq = ctx.col_sqnorms(F).cpu().numpy()
    assert (np.abs(np.diag(G) - sq) <= (2 * GN + 11) * U53 * np.diag(SG)).all()
    s1, _ = ctx.col_moments(F, torch.zeros(GD, dtype=torch.float64, device="cuda"))
    assert (np.abs(cs - s1.cpu().numpy()) <= (2 * GN + 10) * U53 * Scs).all()
    x = torch.zeros(GD, dtype=tdtype(dtype), device="cuda")
    av = torch.empty_like(x)
    ctx.full_gradient(F, x, av)
    eps = float(np.finfo(dtype).eps)
    want = -lam * u / GN
    tol = (lam / GN) * ((GN + 8) * U53 * Su + (GN + 8) * eps * Su) + eps * np.abs(want)
    assert (np.abs(av.double().cpu().numpy() - want) <= tol).all()


# ---- 5. the Python layer ----------------------------------------------------------------------------------------------------------------------
def test_smoothness_exact_lies_inside_the_bracket(ctx):
    import torch
    from ciaoalgorithms_jl_amd import gram as GR
    from ciaoalgorithms_jl_amd.stepsize import smoothness
    rng = np.random.default_rng(21)
    A = torch.from_numpy(rng.standard_normal((600, 40)) * np.exp(rng.standard_normal(40))).cuda()
    y = torch.from_numpy(np.sign(rng.standard_normal(600))).cuda()
    for F in (problem(A, y, lam=600.0), problem(A, y, "logistic")):
        est, upper = smoothness(ctx, F)
        exact = GR.smoothness_exact(GR.gram_stats(ctx, F))
        print(f"estimate {est:.12e} exact {exact:.12e} upper {upper:.12e}")
        assert est <= exact * (1 + 1e-12) and exact <= upper * (1 + 1e-12)


def cert_bounds(A, b, lam, x, mu, c, floor):
    """What two evaluations of the certificate at x may differ by, field by field: the Gram side is exact up to value_floor and the entry
    bound of item 3 through G x - u; the device side forms r = A x - b and A'r in double: (d + 2) roundings a residual, N + 8 a sum."""
    N, d = A.shape
    absr = np.abs(A) @ np.abs(x) + np.abs(b)
    gb = (lam / N) * 2 * (N + d + 10) * U53 * (np.abs(A).T @ absr)            # per coordinate of the gradient, both sides together
    Fb = floor + (lam / (2 * N)) * 2 * (N + d + 10) * U53 * float(absr @ absr)
    ginf = float(gb.max())
    xdg = float(np.abs(x) @ gb) + 2 * (d + 2) * U53 * float(np.abs(x) @ np.abs(lam / N * (A.T @ (A @ x - b))))
    s = 1.0 if c.grad_inf == 0 else min(1.0, mu / c.grad_inf)
    ds = mu * ginf / (c.grad_inf - ginf) ** 2 if c.grad_inf > 2 * ginf else 1.0      # (min(1, .) is 1-Lipschitz: also across the kink)
    gapb = Fb * (1 + abs(2 * s - s * s)) + xdg + ds * (abs(c.F) * 2 + abs(c.x_dot_grad)) + 8 * U53 * (abs(c.F) + abs(c.g) + abs(c.x_dot_grad))
    return dict(F=Fb, g=4 * (d + 2) * U53 * abs(c.g), objective=Fb + 4 * (d + 2) * U53 * abs(c.g), residual=float(np.linalg.norm(gb)) + 8 * d * U53 * c.residual,
                grad_inf=ginf, x_dot_grad=xdg, box_violation=0.0, gap=gapb)


def test_gram_lasso_against_the_device_certificate(ctx):
    import torch
    import problems as P
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd import gram as GR
    from ciaoalgorithms_jl_amd.certificate import stop_when
    from ciaoalgorithms_jl_amd.device import ProxG
    N, n, p = 200, 50, 5
    A, b, _, mu, _, x_star, _ = P.lasso_known_answer(N, n, p)
    F = problem(torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda(), lam=float(N))
    st = GR.gram_stats(ctx, F)
    q, g = GR.GramLasso(st), ProxG(L.PROX_L1, lam=mu)
    gamma = 1.0 / GR.smoothness_exact(st)
    solved = GR.lasso_path(st.to("cpu"), [mu]).x[0].numpy()
    for x in (np.random.default_rng(3).standard_normal(n), solved, x_star):
        xt = torch.from_numpy(x).cuda()
        dev, mine = ctx.certificate(F, g, xt, gamma), q.certificate(xt, mu, gamma)
        tol = cert_bounds(A, b, float(N), x, mu, dev, q.value_floor(xt))
        for field in dev._fields:
            a, m = getattr(dev, field), getattr(mine, field)
            print(f"{field}: device {a:.17g} gram {m:.17g} |diff| {abs(a - m):.3e} bound {tol[field]:.3e}")
            assert abs(a - m) <= tol[field], field
    stop = stop_when(q.as_certificate(mu, gamma), gap=1e-6)
    assert callable(stop) and stop.last is None


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=tname)
@pytest.mark.parametrize("shape", [(6, 3, 2), (200, 50, 5), (300, 130, 7)])
def test_lasso_path_reaches_the_known_answer(ctx, shape, dtype):
    """The statistics come from the device; the d x d iteration runs where its tensors are put (here the host, and for the smallest problem
    the device too).  The inequalities and the allowance for fp32 data are those of tests/test_gram_host.py."""
    import torch
    import problems as P
    import test_gram_host as H
    from ciaoalgorithms_jl_amd import gram as GR
    from ciaoalgorithms_jl_amd.scoring import score, score_many
    N, n, p = shape
    A64, b64, _, lam, _, x_star, f_star = P.lasso_known_answer(N, n, p)
    A, b = A64.astype(dtype), b64.astype(dtype)
    F = problem(torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda(), lam=float(N))
    st = GR.gram_stats(ctx, F)
    assert st.dtype == tdtype(dtype) and st.G.is_cuda
    H.check_path(P, GR, st.to("cpu"), A64, b64, A, b, x_star, f_star)
    if N == 6:
        path = H.check_path(P, GR, st, A64, b64, A, b, x_star, f_star, mus_extra=(0.5,))
        # the iterates go through score_many as they are: device vectors of the rows' type
        assert all(x.is_cuda and x.dtype == tdtype(dtype) and x.is_contiguous() for x in path.x)
        many, one = score_many(ctx, F, path.x), [score(ctx, F, x) for x in path.x]
        assert len(many) == 2 and all(abs(a.mse - o.mse) <= 1e-5 * max(o.mse, 1e-30) for a, o in zip(many, one))


def test_standardized_against_the_standardised_matrix(ctx):
    """G_std from (G, A'1, N) against the Gram statistics of standardize()'s matrix: each entry within the reported amplification times the
    bound of item 3 (both sides, and one rounding of every entry of the standardised matrix)."""
    import torch
    from ciaoalgorithms_jl_amd import gram as GR
    from ciaoalgorithms_jl_amd.standardize import standardize
    rng = np.random.default_rng(31)
    N, d = 500, 12
    A = rng.standard_normal((N, d)) * np.exp(rng.standard_normal(d)) + 2.0 * rng.standard_normal(d)
    b = rng.standard_normal(N) + 0.5
    F = problem(torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda(), lam=float(N))
    st = GR.gram_stats(ctx, F)
    mine, sc = st.standardized()
    F_std, sc_ref = standardize(ctx, F)
    ref = GR.gram_stats(ctx, F_std)
    amp = sc.amplification.cpu().numpy()
    assert (amp >= 1).all() and (amp < GR.AMPLIFICATION_LIMIT).all()
    scale = sc_ref.scale.cpu().numpy()
    absA, absS = np.abs(A), np.abs(F_std.A.cpu().numpy())
    tolG = 4 * (N + 8) * U53 * np.sqrt(np.outer(amp, amp)) * ((absA.T @ absA) * np.outer(scale, scale) + absS.T @ absS)
    diff = (mine.G - ref.G).abs().cpu().numpy()
    print(f"worst |G_std - reference| / tolerance {np.max(diff / tolG):.3e}; amplification up to {amp.max():.3f}")
    assert (diff <= tolG).all() and torch.equal(bits(mine.G.contiguous()), bits(mine.G.T.contiguous()))
    tolu = 4 * (N + 8) * U53 * np.sqrt(amp) * scale * (absA.T @ np.abs(b) + np.abs(sc_ref.mean.cpu().numpy()) * np.abs(b).sum())
    assert ((mine.u - ref.u).abs().cpu().numpy() <= tolu).all()
    assert abs(sc.b_mean - sc_ref.b_mean) <= 4 * U53 * np.abs(b).max() and mine.sum_b == 0.0
    assert abs(mine.sum_bb - ref.sum_bb) <= 4 * (N + 8) * U53 * float(b @ b)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, ciao):
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd import gram as GR
    from ciaoalgorithms_jl_amd.device import Context, PackedF, PackedSepQuad
    f64 = dict(dtype=torch.float64, device="cuda")
    A = torch.randn((9, 8), **f64)
    F = PackedF.least_squares(A, torch.randn(9, **f64), 1.0)
    Fc = PackedF.least_squares_complex(torch.randn((4, 8), **f64), torch.randn(8, **f64), 4.0)
    Fz = PackedF.zero(4, 8, torch.float64)
    F0 = PackedF.logistic(torch.empty((0, 8), **f64), torch.empty(0, **f64), N_total=4)     # a rank that holds no row
    Fs = PackedSepQuad(torch.ones((3, 4), **f64), torch.ones((3, 4), **f64))
    Fshard = PackedF.least_squares(A, F.b, 1.0, N_total=18)
    Fwide = PackedF.least_squares(torch.zeros((1, 4097), **f64), torch.zeros(1, **f64), 1.0)
    x = torch.zeros(8, **f64)
    out = Guarded(shape=(8, 8), dtype=np.float64, ld=8, device="cuda", name="G")
    v = Guarded(shape=(8,), dtype=np.float64, device="cuda", name="u")
    wide = torch.zeros(8, **f64)                       # (never written: every call that names it is refused first)
    ctx.full_gradient(F, x, torch.empty_like(x))
    before = ctx.last_kernel()
    assert not before.startswith("gram")
    lib, h = ctx.lib, ctx._h
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def raw(status):
        if status != L.OK:
            raise L.CiaoError(status, lib.ciao_last_error().decode())

    hooked = Context(0)
    hooked.full_gradient(F, x, torch.empty_like(x))
    hooked.synchronize()
    hooked.set_allreduce(lambda buf, count, dtype, stream: 0)
    before_hooked = hooked.last_kernel()
    try:
        cases = [("complex", lambda: raw(lib.ciao_gram(h, Fc.ref, ptr(out.view), 8, None, None, None))),
                 ("Zero", lambda: raw(lib.ciao_gram(h, Fz.ref, ptr(out.view), 8, None, None, None))),
                 ("sharing", lambda: ctx.gram(Fs)),
                 ("NULL ctx", lambda: raw(lib.ciao_gram(None, F.ref, ptr(out.view), 8, None, None, None))),
                 ("NULL problem", lambda: raw(lib.ciao_gram(h, None, ptr(out.view), 8, None, None, None))),
                 ("NULL G", lambda: raw(lib.ciao_gram(h, F.ref, None, 8, ptr(v.view), None, None))),
                 ("ldg < d", lambda: raw(lib.ciao_gram(h, F.ref, ptr(out.view), 7, None, None, None))),
                 ("d > 4096", lambda: raw(lib.ciao_gram(h, Fwide.ref, ptr(wide), 4097, None, None, None))),
                 ("gram_stats complex", lambda: GR.gram_stats(ctx, Fc)), ("gram_stats Zero", lambda: GR.gram_stats(ctx, Fz)),
                 ("gram_stats sharing", lambda: GR.gram_stats(ctx, Fs)), ("gram_stats N = 0", lambda: GR.gram_stats(ctx, F0)),
                 ("gram_stats row shard", lambda: GR.gram_stats(ctx, Fshard)), ("gram_stats hook", lambda: GR.gram_stats(hooked, F))]
        for what, call in cases:
            with pytest.raises(L.CiaoError) as e:
                call()
            assert e.value.status == L.ERR_ARG, what
            assert len(str(e.value)) - len("libciao_hip status -1: ") > 30, (what, str(e.value))
            assert ctx.last_kernel() == before and hooked.last_kernel() == before_hooked, what
        assert "row-sharded" in str(e.value)
        for bad in (lambda: ctx.gram(F, G=torch.empty((8, 8), dtype=torch.float32, device="cuda")), lambda: ctx.gram(F, G=torch.empty((8, 9), **f64)),
                    lambda: ctx.gram(F, u=torch.zeros(7, **f64)), lambda: ctx.gram(F, bsum=torch.zeros(3, **f64))):
            with pytest.raises(ValueError):
                bad()
        assert ctx.last_kernel() == before
        out.check_outside("refused calls")
        v.check_outside("refused calls")
        assert bool((bits(out.view.contiguous()) == bits(out.flat[:1])).all()) and not bool(wide.any())      # no refused call wrote
        # N = 0: zeros, nothing launched
        got = ctx.gram(F0)
        assert all(not bool(g.any()) for g in got) and got[0].shape == (8, 8) and ctx.last_kernel() == before
        # on the context with the hook the call works, on the local rows
        want = ctx.gram(F)
        got = hooked.gram(Fshard)
        assert all(torch.equal(bits(a.contiguous()), bits(b.contiguous())) for a, b in zip(got, want)) and hooked.last_kernel().startswith("gram_")
    finally:
        hooked.synchronize()
        hooked.close()

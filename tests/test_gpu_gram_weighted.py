"""Weighted Gram statistics on the device and the proximal Newton driver on device rows (ciao_gram_weighted, Context.gram(weights=),
newton.py; csrc/gram_kernels.h).

  1. exact on integers: |a| <= 64 and integer weights w_n = (5 n) mod 9 in [0, 8], zeros included: every partial sum is an integer far
     below 2^53, so all five outputs must equal numpy's int64 result bit for bit: fp64 and fp32 rows, one tile / a diagonal plus
     off-diagonal tiles / the capped plan, every row threshold of gram_plan, four layouts of the matrix, w inside a poisoned buffer at
     offset 0 and at offset 1 (8 bytes off 16-byte alignment) that ends at w[N - 1], every output guarded, the launch's report against
     a restatement of the plan;
  2. bits: w = 1 against ciao_gram, symmetry under weights of both signs, a second call, the layouts, fp32 rows against their .double()
     copy, a logistic view, every NULL output;
  3. folds: the five 0/1-weighted results add up exactly to the unweighted one;
  4. Gaussian rows against exact sums under the bound of section 8.13;
  5. refusals;
  6. the driver: logistic_newton / logistic_path on DeviceRows.

The bound of item 4.  One operand of every product is w_n a, rounded once; the product is rounded once; the sum passes through at most N
additions in double: |got - exact| <= (N + 10) 2^-53 sum_n |w_n a_ni a_nj| -- the (N + 8) of section 8.12 plus the rounding of w a and
its second-order term."""
import ctypes as C

import numpy as np
import pytest

from layouts import Guarded, bits, has_poison
from test_gpu_gram import GD, GN, gauss_case, input_layouts, int_matrix, kind_of, n_sizes, plan, problem, tname
from test_gram_weighted_host import MU_FRACTIONS, SHAPES, logistic_case, split, weighted_exact

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
WS = 256 << 20
D_INT = [1, 3, 17, 128, 129, 257, 1025]


def check_report(ctx, N, d, dtype, kind):
    ntiles, per, P, xcd, ws = plan(N, d)
    want = (f"gram_partial_kernel<{tname(dtype)},{kind},w> grid={ntiles * P} block=256 tile=128x128 chunk=16 tiles={ntiles} partitions={P} "
            f"rows={per} map={'xcd' if xcd else 'plain'} workspace={ws}")
    assert ctx.last_kernel() == want, (ctx.last_kernel(), want)
    assert ws <= WS


class Outputs:
    """G (row stride d + 3), u, colsum, bsum (three elements), each inside a poisoned buffer of its own"""

    def __init__(self, d):
        self.G = Guarded(shape=(d, d), dtype=np.float64, ld=d + 3, device="cuda", name="G")
        self.u, self.cs, self.bs = (Guarded(shape=(n,), dtype=np.float64, device="cuda", name=nm) for n, nm in ((d, "u"), (d, "colsum"), (3, "bsum")))

    def run(self, ctx, F, w, u=True, colsum=True, bsum=True):
        got = ctx.gram(F, G=self.G.view, u=self.u.view if u else None, colsum=self.cs.view if colsum else None, bsum=self.bs.view if bsum else None,
                       weights=w)
        for g in (self.G, self.u, self.cs, self.bs):
            g.check_outside(ctx.last_kernel())
        return got


def int_weights(N):
    return (5 * np.arange(N, dtype=np.int64)) % 9


_INT_REF = {}


def int_reference(d):
    """{N: the four weighted outputs as float64 arrays holding exact integers} in numpy int64 arithmetic, one slab of rows after the other;
    computed once per d, shared by the two types, never modified"""
    if d not in _INT_REF:
        sizes = n_sizes(d)
        ints, bi = int_matrix(sizes[-1], d)
        wi = int_weights(sizes[-1])
        want, prev = {}, 0
        acc = [np.zeros((d, d), np.int64), np.zeros(d, np.int64), np.zeros(d, np.int64), np.zeros(3, np.int64)]
        for N in sizes:
            a, bb, w = ints[prev:N], bi[prev:N], wi[prev:N]
            wa = w[:, None] * a
            G = np.zeros((d, d), np.int64)
            for k in range(0, a.shape[0], 32):
                G += np.ascontiguousarray(a[k:k + 32].T) @ wa[k:k + 32]
            acc = [acc[0] + G, acc[1] + a.T @ (w * bb), acc[2] + a.T @ w, acc[3] + np.array([(w * bb).sum(), (w * bb * bb).sum(), w.sum()])]
            prev = N
            assert all(v.dtype == np.int64 for v in acc) and max(int(np.abs(v).max()) for v in acc) < 2 ** 53
            want[N] = [v.astype(np.float64) for v in acc]
            for v in want[N]:
                v.setflags(write=False)
        _INT_REF[d] = want
    return _INT_REF[d]


# ---- 1. exact on integers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dtype", [pytest.param(d, dt, id=f"{d}-{tname(dt)}") for dt in (np.float32, np.float64) for d in D_INT])
def test_integer_rows_and_integer_weights_exactly(ctx, d, dtype):
    import torch
    sizes = n_sizes(d)
    ints, bi = int_matrix(sizes[-1], d)
    wi = int_weights(sizes[-1]).astype(np.float64)
    want = {N: [torch.from_numpy(v.copy()).cuda() for v in ref] for N, ref in int_reference(d).items()}
    # the weights of the first N rows in a buffer of their own that ends at w[N - 1], at both alignments: poison on either side
    Gw = {(N, off): Guarded(torch.from_numpy(wi[:N].copy()), off=off, device="cuda", name=f"w N={N} off={off}") for N in sizes for off in (0, 1)}
    out = Outputs(d)
    kinds, offs = set(), set()
    for li, (name, GA, Gb) in enumerate(input_layouts(torch.from_numpy(ints.astype(dtype)), torch.from_numpy(bi.astype(dtype)), dtype)):
        for ni, N in enumerate(sizes):
            off = (li + ni) % 2                  # every N meets both offsets, every layout both
            w = Gw[(N, off)]
            assert w.view.data_ptr() % 16 == 8 * off
            F = problem(GA.view[:N], Gb.view[:N])
            got = out.run(ctx, F, w.view)
            check_report(ctx, N, d, dtype, kind_of(F))
            for g, e, what in zip(got, want[N], ("G", "u", "colsum", "bsum")):
                assert torch.equal(bits(g.contiguous()), bits(e)), (what, name, N, d, off, ctx.last_kernel())
            kinds.add((name, kind_of(F)))
            offs.add((N, off))
        GA.check_unchanged(name)
        Gb.check_unchanged(name)
    for w in Gw.values():
        w.check_unchanged("weights")
    assert ("padding", "vec16") in kinds and ("base+1", "elem") in kinds and len(offs) == 2 * len(sizes)


# ---- 2. bits ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
def test_the_same_bits(ctx, dtype):
    """N = 700, d = 150: three tiles, several partitions, a partial last chunk."""
    import torch
    rng = np.random.default_rng(11)
    N, d = 700, 150
    M = torch.from_numpy(rng.standard_normal((N, d)).astype(dtype))
    b = torch.from_numpy(np.sign(rng.standard_normal(N)).astype(dtype))
    F = problem(M.cuda(), b.cuda())
    # w = 1: ciao_gram's bits, and the row count
    plain = [g.contiguous() for g in ctx.gram(F)]
    assert ctx.last_kernel().startswith(f"gram_partial_kernel<{tname(dtype)},{kind_of(F)}> ")
    ones = [g.contiguous() for g in ctx.gram(F, weights=torch.ones(N, dtype=torch.float64, device="cuda"))]
    assert ctx.last_kernel().startswith(f"gram_partial_kernel<{tname(dtype)},{kind_of(F)},w> ")
    assert all(torch.equal(bits(a), bits(p)) for a, p in zip(ones[:3], plain[:3])) and torch.equal(bits(ones[3][:2]), bits(plain[3]))
    assert float(ones[3][2]) == 700.0
    # Gaussian weights of both signs
    wv = torch.from_numpy(rng.standard_normal(N))
    assert bool((wv < 0).any()) and bool((wv > 0).any())
    out = Outputs(d)
    first = None
    for li, (name, GA, Gb) in enumerate(input_layouts(M, b, dtype)):
        w = Guarded(wv, off=li % 2, device="cuda", name=f"w {name}")
        for kind in ("ls", "logistic"):
            for rep in range(2):
                got = [g.contiguous().clone() for g in out.run(ctx, problem(GA.view, Gb.view, kind), w.view)]
                assert not any(has_poison(g) for g in got), name
                assert torch.equal(bits(got[0]), bits(got[0].T.contiguous())), "G is not symmetric to the bit"
                if first is None:
                    first = got
                assert all(torch.equal(bits(a), bits(e)) for a, e in zip(got, first)), (name, kind, rep)
        w.check_unchanged(name)
    w = wv.cuda()
    if dtype == np.float32:
        wide = [g.contiguous() for g in out.run(ctx, problem(M.double().cuda(), b.double().cuda()), w)]
        assert ctx.last_kernel().startswith("gram_partial_kernel<f64,vec16,w> ")      # (150 doubles a row: whole 16-byte chunks)
        assert all(torch.equal(bits(a), bits(e)) for a, e in zip(wide, first)), "fp32 rows and their double copy differ"
    for mask in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        fresh = Outputs(d)
        got = fresh.run(ctx, F, w, *map(bool, mask))
        assert torch.equal(bits(got[0].contiguous()), bits(first[0]))
        for k, (on, g, held) in enumerate(zip(mask, got[1:], (fresh.u, fresh.cs, fresh.bs))):
            if on:
                assert torch.equal(bits(g), bits(first[1 + k]))
            else:
                assert g is None and not held.outside_touched() and bool((bits(held.view) == bits(held.flat[:1])).all())   # still the poison


# ---- 3. folds --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
def test_folds_add_up_to_the_whole(ctx, dtype):
    """0/1 weights give the statistics of a row subset without copying rows: fold id n mod 5, integer rows, so the five results add up
    exactly to the unweighted one, and each equals ciao_gram on the gathered rows."""
    import torch
    N, d = 1000, 129
    ints, bi = int_matrix(N, d)
    A, b = torch.from_numpy(ints.astype(dtype)).cuda(), torch.from_numpy(bi.astype(dtype)).cuda()
    F = problem(A, b)
    whole = [g.clone() for g in ctx.gram(F)]
    fold = torch.arange(N, device="cuda") % 5
    total = None
    for f in range(5):
        keep = fold == f
        part = [g.clone() for g in ctx.gram(F, weights=keep.double())]
        sub = ctx.gram(problem(A[keep].contiguous(), b[keep].contiguous()))
        assert all(torch.equal(p, s) for p, s in zip(part[:3], sub[:3])) and torch.equal(part[3][:2], sub[3]) and float(part[3][2]) == float(keep.sum())
        total = part if total is None else [t + p for t, p in zip(total, part)]
    assert all(torch.equal(bits(t.contiguous()), bits(e.contiguous())) for t, e in zip(total[:3], whole[:3]))
    assert torch.equal(bits(total[3][:2].contiguous()), bits(whole[3])) and float(total[3][2]) == float(N)


# ---- 4. Gaussian rows ------------------------------------------------------------------------------------------------------------------------
_GAUSS_W = {}


def gauss_weighted(dtype):
    """(A, b, w, exact, scale): test_gpu_gram.gauss_case's rows with weights uniform in [0, 1/4]; exact = the weighted outputs correctly
    rounded from sums of Fractions (the weights as the doubles they are); computed once, shared, never modified"""
    if dtype not in _GAUSS_W:
        A, b, _, _ = gauss_case(dtype)
        w = np.random.default_rng(2000).random(GN) * 0.25
        E, S = weighted_exact(A, b, w)
        E = np.array([[float(v) for v in row] for row in E])
        for v in (w, E, S):
            v.setflags(write=False)
        _GAUSS_W[dtype] = (A, b, w, E, S)
    return _GAUSS_W[dtype]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=tname)
def test_gaussian_rows_against_exact_sums(ctx, dtype):
    import torch
    A, b, w, E, S = gauss_weighted(dtype)
    F = problem(torch.from_numpy(A.copy()).cuda(), torch.from_numpy(b.copy()).cuda())
    got = [g.cpu().numpy() for g in Outputs(GD).run(ctx, F, torch.from_numpy(w.copy()).cuda())]
    check_report(ctx, GN, GD, dtype, kind_of(F))
    for g, e, s, what in zip(got, split(E), split(S), ("G", "u", "colsum", "bsum")):
        ratio = np.abs(g - e.astype(np.float64)) / ((GN + 10) * U53 * s.astype(np.float64))
        print(f"{tname(dtype)} {what}: worst |got - exact| / bound {ratio.max():.3e}")
        assert (ratio <= 1).all(), what


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, ciao):
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd.device import PackedF
    f64 = dict(dtype=torch.float64, device="cuda")
    A = torch.randn((9, 8), **f64)
    F = PackedF.least_squares(A, torch.randn(9, **f64), 1.0)
    Fc = PackedF.least_squares_complex(torch.randn((4, 8), **f64), torch.randn(8, **f64), 4.0)
    Fz = PackedF.zero(4, 8, torch.float64)
    F0 = PackedF.logistic(torch.empty((0, 8), **f64), torch.empty(0, **f64), N_total=4)     # a rank that holds no row
    Fwide = PackedF.least_squares(torch.zeros((1, 4097), **f64), torch.zeros(1, **f64), 1.0)
    x = torch.zeros(8, **f64)
    out = Guarded(shape=(8, 8), dtype=np.float64, ld=8, device="cuda", name="G")
    wide = torch.zeros(8, **f64)                       # (never written: every call that names it is refused first)
    w = torch.ones(9, **f64)
    ctx.full_gradient(F, x, torch.empty_like(x))
    before = ctx.last_kernel()
    assert not before.startswith("gram")
    lib, h = ctx.lib, ctx._h
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def raw(status):
        if status != L.OK:
            raise L.CiaoError(status, lib.ciao_last_error().decode())

    cases = [("NULL w", lambda: raw(lib.ciao_gram_weighted(h, F.ref, None, ptr(out.view), 8, None, None, None))),
             ("complex", lambda: raw(lib.ciao_gram_weighted(h, Fc.ref, ptr(w), ptr(out.view), 8, None, None, None))),
             ("Zero", lambda: raw(lib.ciao_gram_weighted(h, Fz.ref, ptr(w), ptr(out.view), 8, None, None, None))),
             ("NULL ctx", lambda: raw(lib.ciao_gram_weighted(None, F.ref, ptr(w), ptr(out.view), 8, None, None, None))),
             ("NULL problem", lambda: raw(lib.ciao_gram_weighted(h, None, ptr(w), ptr(out.view), 8, None, None, None))),
             ("NULL G", lambda: raw(lib.ciao_gram_weighted(h, F.ref, ptr(w), None, 8, None, None, None))),
             ("ldg < d", lambda: raw(lib.ciao_gram_weighted(h, F.ref, ptr(w), ptr(out.view), 7, None, None, None))),
             ("d > 4096", lambda: raw(lib.ciao_gram_weighted(h, Fwide.ref, ptr(w), ptr(wide), 4097, None, None, None)))]
    for what, call in cases:
        with pytest.raises(L.CiaoError) as e:
            call()
        assert e.value.status == L.ERR_ARG, what
        assert len(str(e.value)) - len("libciao_hip status -1: ") > 30, (what, str(e.value))
        assert ctx.last_kernel() == before, what
    for what, bad in (("length", torch.ones(8, **f64)), ("dtype", torch.ones(9, dtype=torch.float32, device="cuda")), ("device", torch.ones(9, dtype=torch.float64)),
                      ("shape", torch.ones((9, 1), **f64)), ("stride", torch.ones(18, **f64)[::2]), ("type", np.ones(9))):
        with pytest.raises(ValueError):
            ctx.gram(F, weights=bad)
        assert ctx.last_kernel() == before, what
    with pytest.raises(ValueError):
        ctx.gram(F, weights=w, bsum=torch.zeros(2, **f64))       # three sums with weights
    assert ctx.last_kernel() == before
    out.check_outside("refused calls")
    assert bool((bits(out.view.contiguous()) == bits(out.flat[:1])).all()) and not bool(wide.any())      # no refused call wrote
    # N = 0: zeros (three sums), nothing launched
    got = ctx.gram(F0, weights=torch.empty(0, **f64))
    assert all(not bool(g.any()) for g in got) and got[0].shape == (8, 8) and got[3].shape == (3,) and ctx.last_kernel() == before


# ---- 6. the driver ---------------------------------------------------------------------------------------------------------------------------
def device_case(shape, dtype):
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    N, d, seed = shape
    A, y, mu_max = logistic_case(N, d, seed, dtype)
    return A, y, mu_max, PackedF.logistic(torch.from_numpy(A).cuda(), torch.from_numpy(y).cuda())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_newton_on_float64_device_rows(ctx, shape):
    """converged, gap <= 1e-9 max(1, objective) by the returned certificate AND by a fresh Context.certificate(samples=True) of the
    returned vector; outer <= 16: twice the worst count of the method's numpy restatement (2 to 8 from x = 0 at these shapes)."""
    import torch
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd.device import ProxG
    from ciaoalgorithms_jl_amd.newton import DeviceRows, logistic_mu_max, logistic_newton
    from ciaoalgorithms_jl_amd.scoring import score_many
    A, y, mu_max, F = device_case(shape, np.float64)
    rows = DeviceRows(ctx, F)
    assert abs(logistic_mu_max(rows) - mu_max) <= 1e-12 * mu_max
    xs = []
    for frac in MU_FRACTIONS:
        mu = frac * mu_max
        r = logistic_newton(rows, mu, gap=1e-9)
        c = r.certificate
        fresh = ctx.certificate(F, ProxG(L.PROX_L1, lam=mu), r.x, 0.5, samples=True)
        print(f"N={shape[0]} d={shape[1]} mu={frac} mu_max: outer {r.outer} passes {tuple(r.passes)} gap {c.gap:.3e} fresh gap {fresh.gap:.3e} "
              f"objective {c.objective:.12f} {r.reason}")
        assert r.converged and r.reason == "gap"
        assert c.gap <= 1e-9 * max(1.0, c.objective) and fresh.gap <= 1e-9 * max(1.0, fresh.objective)
        assert r.outer <= 16 and r.passes.gram == r.outer and r.passes.first_order >= r.outer + 2
        assert r.x.is_cuda and r.x.dtype == torch.float64 and r.x.is_contiguous() and tuple(r.x.shape) == (shape[1],)
        xs.append(r.x)
    # the returned vectors go through score_many as they are
    many = score_many(ctx, F, xs)
    assert len(many) == len(xs)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_newton_on_float32_device_rows(ctx, shape):
    """The driver returns -- converged, or stalled at the noise of float32 dots -- and what it returns is as good as the float64 solution
    of the same (float32-valued) rows rounded to float32, both objectives evaluated the same way (row_dots + margin_stats on the float32
    rows), up to 8 (d + 2) eps32 mean_i sum_j |a_ij x_j|: (d + 2) roundings a dot, 8 for the two evaluations and the log-loss's slope <= 1."""
    import torch
    from ciaoalgorithms_jl_amd.device import PackedF
    from ciaoalgorithms_jl_amd.newton import DeviceRows, logistic_newton
    from ciaoalgorithms_jl_amd.scoring import score_many
    A, y, mu_max, F = device_case(shape, np.float32)
    rows = DeviceRows(ctx, F)
    rows64 = DeviceRows(ctx, PackedF.logistic(torch.from_numpy(A.astype(np.float64)).cuda(), torch.from_numpy(y.astype(np.float64)).cuda()))
    d = shape[1]
    xs = []
    for frac in MU_FRACTIONS:
        mu = frac * mu_max
        r = logistic_newton(rows, mu, gap=1e-9, max_outer=30)
        assert (r.converged and r.reason == "gap") or r.reason == "stalled", r.reason
        assert r.outer < 30 and r.x.is_cuda and r.x.dtype == torch.float32 and r.x.is_contiguous()
        r64 = logistic_newton(rows64, mu, gap=1e-9)
        assert r64.converged
        x64 = r64.x.float().contiguous()
        phi = lambda x: rows.loss(rows.dots(x))[0] + mu * float(x.double().abs().sum())
        allow = 8 * (d + 2) * float(np.finfo(np.float32).eps) * float(np.mean(np.abs(A.astype(np.float64)) @ np.abs(x64.double().cpu().numpy())))
        o32, o64 = phi(r.x), phi(x64)
        print(f"N={shape[0]} d={d} mu={frac} mu_max: outer {r.outer} {r.reason} gap {r.certificate.gap:.3e}; objective {o32:.10f} against {o64:.10f} "
              f"(float64 solve rounded), allowance {allow:.3e}, used {(o32 - o64) / allow if allow > 0 else 0.0:.3f}")
        assert o32 <= o64 + allow
        xs.append(r.x)
    assert len(score_many(ctx, F, xs)) == len(xs)


def test_path_warm_starts_on_device_rows(ctx):
    from ciaoalgorithms_jl_amd import _lib as L
    from ciaoalgorithms_jl_amd.device import PackedF
    from ciaoalgorithms_jl_amd.newton import DeviceRows, logistic_newton, logistic_path
    A, y, mu_max, F = device_case((200, 50, 5), np.float64)
    rows = DeviceRows(ctx, F)
    mus = [0.5 * mu_max, 0.25 * mu_max, 0.125 * mu_max]
    path = logistic_path(rows, mus, gap=1e-9)
    cold = [logistic_newton(rows, m, gap=1e-9) for m in mus]
    print("outer iterations along the path", [r.outer for r in path], "cold", [r.outer for r in cold])
    assert all(r.converged for r in path) and all(r.converged for r in cold)
    assert path[0].outer == cold[0].outer and all(p.outer <= c.outer for p, c in zip(path[1:], cold[1:]))
    for p, c in zip(path, cold):
        assert abs(p.certificate.objective - c.certificate.objective) <= max(p.certificate.gap, c.certificate.gap) + 1e-13
    # refused: LeastSquares rows, a rank's shard
    for bad in (PackedF.least_squares(F.A, F.b, 1.0), PackedF.logistic(F.A, F.b, N_total=400)):
        with pytest.raises(L.CiaoError) as e:
            DeviceRows(ctx, bad)
        assert e.value.status == L.ERR_ARG


def test_a_context_on_a_stream_of_its_own(ciao, ctx):
    """torch's operations between the library's calls (the casts, sigma(-t)(1 - sigma(-t)), G x, the trial points of the line search) follow
    the kernels on the context's stream, not on torch's current one: the solve on a Context that owns its stream gives the bits, the
    iteration count and the passes of the solve on the session's context.  N = 20000, d = 260: kernels long enough to be overtaken."""
    import torch
    from ciaoalgorithms_jl_amd.device import Context
    from ciaoalgorithms_jl_amd.newton import DeviceRows, logistic_mu_max, logistic_newton
    A, y, mu_max, F = device_case((20000, 260, 77), np.float64)
    want_mu = logistic_mu_max(DeviceRows(ctx, F))
    want = logistic_newton(DeviceRows(ctx, F), 0.1 * want_mu, gap=1e-9)
    assert want.converged and abs(want_mu - mu_max) <= 1e-12 * mu_max
    torch.cuda.synchronize()
    own = Context(0, stream=torch.cuda.Stream())
    try:
        rows = DeviceRows(own, F)
        assert logistic_mu_max(rows) == want_mu
        got = logistic_newton(rows, 0.1 * want_mu, gap=1e-9)
        own.synchronize()
        assert got.converged and (got.outer, got.passes, got.reason) == (want.outer, want.passes, want.reason)
        assert torch.equal(bits(got.x), bits(want.x)) and got.certificate == want.certificate
    finally:
        own.synchronize()
        own.close()

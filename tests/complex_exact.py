"""Exact lattice problems for the complex kernels (CIAO_LOSS_LS_COMPLEX, vectors as (re, im) pairs): the chains chain_cdma_kernel
(csrc/chain_dma_kernels.h), chain_cplx_reg_kernel and chain_cplx_kernel (chain_reg_kernels.h), and the rows kernels rows_cplx_kernel and
rows_csplit_kernel with finalize_kernel behind them (rows_kernels.h): the method of tests/rows_exact.py and tests/chains_exact.py on a
GAUSSIAN-INTEGER lattice.

Every sum the device forms -- the two (four) real sums behind a complex dot product, the residual's two parts, both parts of every
coordinate's update, SVRG's running sum, the partial d-vectors and finalize -- is a sum of multiples of one power of two whose ABSOLUTE
values add up to less than 2^24 of them (2^53 where the case's name ends in "_f64only").  Every association of such a sum is exact, so
the state does not depend on how the (re, im) pairs are dealt to chunks, lanes and waves, and it is compared in BITS.  The real products
behind a complex product are recorded term by term (`split`): on random data a dropped cross term, a conjugation sign, re and im swapped
in one wave's share or the imaginary half of b_i taken from the neighbouring slot are a few hundred eps; here they change bits.

The chains' data.  256 rows, N_total = 256, lam = 1.  Rows 0 .. 239 are live: two entries on the case's MARKED complex entries
(chains_exact.marked_columns counted in complex entries, plus both entries of every marked 16-byte chunk in fp32, where a chunk holds
two), the first from {+-1 +-i}, the second from {+-1, +-i, +-1 +-i}, dealt so that the rows the steps take have disjoint supports while
the entries last; b a Gaussian integer with parts in {-2 .. 2} (live rows: both parts non-zero on every second row).  The iterates are
Gaussian integers with BOTH parts non-zero on every marked entry: all four real products of every complex product count.  Rows 240 ..
255 are idle (all zero, b = 0).  The chain is 1100 steps; chain_cdma_kernel stages indices, the pair b_i, gamma_i and the stale flags
CDMA_CHUNK = 512 steps at a time, so the marks are 512 and 1024 and the compared step counts 1, 2, DEPTH - 1, DEPTH, DEPTH + 1, 511,
512, 513, 1025 and 1100.  Live steps, repeats (distances 1 .. DEPTH + 1, each once inside a chunk and once across step 512) and the
differing slot 0 of the second chunk are placed by the real harness's own functions.

A complex problem takes g = Zero or the complex NormL1: there is no box to bound a lattice iterate.
  SVRG (gamma = 1/2), SAGA and SAG (gamma = 1/4): g = Zero.  What refines their lattice is the 1 / N of the aggregate and gamma, up to 10
  bits a visit of a row's coordinates: with disjoint supports and the designed repeats they stay below 2^24; where the live rows share
  entries (fewer than 160) and where one row comes seven times in a row across step 512 (SAGA: 2^37 .. 2^42) they hold in fp64 only.  SAG's
  seven-fold row is beyond 2^53 (NOT_MADE_EXACT); its run across step 512 is FIVE visits long.
  Finito, LFinito: g = complex NormL1 with the threshold hat_gamma lam_g = 2^12, every prox argument in the DEAD ZONE (|v| <= 2^11:
  `Chain` asserts it for every prox of the chain) -- the design the issue names; no bounded live-iterate design was found (without a clamp
  hat_gamma = N / 2 is no contraction).  The iterate is 0 after each prox; the table rows, av, the pair b_i, gamma_i, the stale-row
  logic and the batches (r = 1, 2, 5) are live, and with r > 1 the first batch's dots run on the non-zero start iterate.  The dots of
  every later batch are all zero.  LFinito's z_full = prox(av) is 0 as well, so its two gradients cancel in av coordinate by coordinate
  (both are formed and added: exact) and what its chain holds is b_i and the (re, im) order of the pair, not the dots.
  The LIVE complex NormL1 is held on ONE step (`PROX_EDGES`, `prox_exact`): prox_cpair_chain's 1 - gl rsqrt(n2) is not exact at any lattice.

The rows half (at the end of the module): every mode the plan gives on dense lattice rows -- GRAD with the LeastSquares objective (and the
NormL1 term at an on-axis iterate), SAGA_INIT, FINITO_INIT, FINITO_BATCH (g = Zero, the dead zone, live on-axis prox arguments) and GRAD2
through lfinito_iterate (Zero, the dead zone), one batch a call; ROWS_NOT_COVERED names what is left, with the reason.

A plain module: tests/test_complex_exact_host.py holds the restatement against the oracle in bits, asserts the bound and plants the
defects; tests/test_gpu_complex_exact.py runs the cases on the device."""
import re

import numpy as np

from chains_exact import MARKED, ChainBounds, _NoBounds, dma_depth, live_steps, marked_columns, place_repeats
from rows_exact import Bounds, lossless, quantum  # noqa: F401  (Bounds, quantum: the rows half and the host file)

F64, F32 = np.float64, np.float32
C128 = np.complex128
N, NLIVE = 256, 240
CCHUNK = 512                                            # chain_dma_kernels.h CDMA_CHUNK
NSTEPS = 1100
HG = N / 2.0
DEAD_GL = 2.0 ** 12                                     # Finito / LFinito: the complex NormL1's threshold hat_gamma lam_g
SHARED_BELOW = 160                                      # complex entries below which the live rows cannot have disjoint supports
ALGS = ("svrg", "saga", "sag", "finito", "lfinito")
TABLE_ALGS = ("saga", "sag", "finito")
ALG_NO = {"svrg": 0, "saga": 1, "sag": 1, "finito": 2, "lfinito": 3}
RUN_ACROSS = {"saga": 7, "sag": 5, "finito": 7}         # one row that many times in a row across step 512 (SAG: NOT_MADE_EXACT)

NOT_MADE_EXACT = {
    "one row seven times in a row across step 512 under SAG":
        "SAG's iterate moves by the refined aggregate alone: 2^60.8, 2^62.5 and 2^62.8 quanta on the three seeds tried at 300 entries, beyond "
        "fp64; a run of five holds in fp64 (2^44.8 .. 2^52.3: sag_run5_f64only).  SAGA's seven-fold row holds in fp64 (2^37.3 .. 2^41.9)",
    "a live complex NormL1 in a chain": "prox_cpair_chain multiplies by 1 - gl rsqrt(n2): not exact on any lattice; held on one step under its own bound",
    "adaptive Finito on complex rows": "its backtracking divides by data-dependent norms; it stays on fitted scales (tests/test_gpu_complex.py)",
}


def pc_of(dtype):
    """complex entries per 16-byte chunk"""
    return 8 // np.dtype(dtype).itemsize


def pairs(v):
    """complex128 -> interleaved (re, im) float64"""
    return np.ascontiguousarray(np.asarray(v, C128)).view(F64).reshape(np.shape(v)[:-1] + (-1,))


def cpx(v):
    """interleaved (re, im) pairs -> complex128"""
    return np.ascontiguousarray(np.asarray(v, F64)).view(C128)


def split(x, y):
    """the complex product x y as the device forms it: its two real products per part, as two complex terms (x.re y, i x.im y)"""
    return [x.real * y, 1j * x.imag * y]


def _ri(t):
    return np.concatenate([np.real(t), np.imag(t)])


def unit(rng, both):
    """an entry of A: {+-1 +-i} (both parts non-zero), or one of the eight {+-1, +-i, +-1 +-i}"""
    if both or rng.integers(2):
        return complex(rng.choice([-1.0, 1.0]), rng.choice([-1.0, 1.0]))
    return complex(rng.choice([-1.0, 1.0])) * (1j if rng.integers(2) else 1.0)


def gauss(rng, n, lo, hi, nonzero=False):
    vals = [v for v in range(lo, hi + 1) if v or not nonzero]
    return rng.choice(vals, n).astype(F64) + 1j * rng.choice(vals, n).astype(F64)


def marked_entries(n, pc):
    """chains_exact.marked_columns in complex entries; in fp32 (pc = 2) BOTH entries of the first, the last and the last whole chunk --
    the second entry of a chunk is its own edge there"""
    c = set(int(x) for x in marked_columns(n, pc))
    if pc == 2:
        for e in (0, n - 1, (n - 1) // 2 * 2, max(n - 2, 0)):
            c |= {e, min(e ^ 1, n - 1)}
    c = sorted(c)
    while len(c) > MARKED:                              # (the spread gives way, never an edge)
        del c[len(c) // 2]
    return np.array(c, np.int64)


# ---- the chains ---------------------------------------------------------------------------------------------------------------------------
class Spec:
    """One chain case.  n: complex entries of a row; depth: the kernel's look-ahead; run: one row that many times in a row across step
    512; pc: complex entries per chunk (the marked entries); limit: 24, or 53 (fp64 only)."""

    def __init__(self, name, alg, n, depth=8, r=1, repeats=None, run=0, pc=1, nsteps=NSTEPS, marks=(CCHUNK, 2 * CCHUNK), seed0=0, limit=None):
        if limit is None:
            # SAGA / SAG where the live rows share entries, or one row comes many times in a row: 10 bits a visit (module docstring)
            limit = 53 if alg in ("saga", "sag") and (n < SHARED_BELOW or run) else 24
        self.alg, self.n, self.depth, self.r, self.run, self.pc, self.nsteps, self.seed0, self.limit = alg, int(n), int(depth), int(r), int(run), pc, int(nsteps), seed0, limit
        self.name = name + ("_f64only" if limit == 53 else "")
        self.table = alg in TABLE_ALGS
        self.marks = tuple(m for m in marks if m < nsteps)
        self.repeats = tuple(repeats if repeats is not None else (range(1, depth + 2) if self.table and not run else ()))
        self.prox = "dead" if alg in ("finito", "lfinito") else "zero"
        c = (1, 2, depth - 1, depth, depth + 1, CCHUNK - 1, CCHUNK, CCHUNK + 1, 2 * CCHUNK + 1)
        self.counts = tuple(sorted({k for k in c if 1 <= k < self.nsteps} | {self.nsteps}))


class Chain:
    """A Spec's data for one seed: complex A (N x n), b, gam, idx, the live mask, the start state (complex128 everywhere)"""

    def __init__(self, spec, seed):
        rng = np.random.default_rng(seed)
        s, n = spec, spec.n
        self.spec, self.seed, self.n, self.d = s, seed, n, 2 * n
        self.cols = marked_entries(n, s.pc)
        nc = len(self.cols)
        self.A = np.zeros((N, n), C128)
        order = rng.permutation(nc)
        order = np.concatenate([[nc - 1, 0], order[(order != nc - 1) & (order != 0)]])[:nc]      # row 0: the last and the first entry (step 1's row)
        for i in range(NLIVE):
            mine = self.cols[[order[(i * 2 + q) % nc] for q in range(min(2, nc))]]
            self.A[i, mine] = [unit(rng, q == 0) for q in range(len(mine))]
        self.b = np.zeros(N, C128)
        self.b[:NLIVE] = gauss(rng, NLIVE, -2, 2)
        self.b[:NLIVE:2] = gauss(rng, len(self.b[:NLIVE:2]), -2, 2, nonzero=True)
        self.gam = rng.choice([N / 4.0, N / 2.0], N)
        self.lam = 1.0
        self.gamma = 0.5 if s.alg == "svrg" else 0.25
        self.lam_g = DEAD_GL / HG if s.prox == "dead" else 0.0

        def on_cols(lo, hi, nonzero=False):
            v = np.zeros(n, C128)
            v[self.cols] = gauss(rng, nc, lo, hi, nonzero)
            return v

        self.av0, self.z0 = on_cols(-1, 1), on_cols(-2, 2)
        self.p0 = on_cols(-2, 2, nonzero=True)          # both parts non-zero on every marked entry
        self.zf0 = -self.p0
        self.table0 = np.zeros((N, n), C128)
        if s.alg in ("saga", "sag"):
            self.av0[:] = 0                              # (the drift p -= gamma av over the idle steps starts with a row's first visit)
        for i in range(NLIVE):
            nz = np.nonzero(self.A[i])[0]
            self.table0[i, nz] = np.conj(self.A[i, nz]) * (rng.choice([-5.0, -3.0, 3.0, 5.0]) + 1j * rng.choice([-5.0, -3.0, 3.0, 5.0]))   # (parts 3 and 5: never Finito's own (gam_i / N) conj(a_i) b_i)
        # the steps
        k = s.nsteps
        live = np.zeros(k, bool)
        live[live_steps(k, s.depth, s.marks, s.counts)] = True
        idx = rng.integers(NLIVE, N, k).astype(np.int64)
        fresh = list(range(NLIVE - 1, 0, -1))
        self.placed = {}
        if s.repeats:
            self.placed = place_repeats(idx, live, list(s.marks), s.repeats, fresh, inside_at=40, chunks=(CCHUNK,))
        if s.run:
            a = CCHUNK - s.run // 2
            idx[a:a + s.run] = fresh.pop()
            live[a:a + s.run] = True
        idx[1] = 0
        for j in np.nonzero(live)[0]:
            if idx[j] >= NLIVE:
                idx[j] = fresh.pop()
        # slot 0 of the first chunk and of the second hold different b_i (both parts) and gamma_i
        at = self.b[idx[CCHUNK]]
        other = [q for q in reversed(fresh) if self.b[q].real != at.real and self.b[q].imag != at.imag and self.gam[q] != self.gam[idx[CCHUNK]]]
        idx[0] = other[0]
        fresh.remove(other[0])
        self.idx, self.live = idx, live
        visits = np.bincount(idx[idx < NLIVE], minlength=NLIVE)
        designed = sum(len(v) for v in self.placed.values()) + (s.run - 1 if s.run else 0)
        assert visits.sum() - np.count_nonzero(visits) == designed, "a live row is taken by two steps that are no designed repeat"
        for j in np.nonzero(live)[0]:                    # every live row: an entry with both parts non-zero on an iterate entry with both non-zero
            a = self.A[idx[j]]
            e = np.nonzero((a.real != 0) & (a.imag != 0))[0]
            assert len(e) and (self.p0[e].real != 0).all() and (self.p0[e].imag != 0).all()

    def batches(self, k):
        r = self.spec.r
        return [self.idx[j:min(j + r, k)] for j in range(0, k, r)]


def check_placements(P):
    """every repeat distance once inside a chunk and once across a staging boundary -- step 512 while its neighbourhood has two free
    steps at that distance, step 1024 then (the pairs share no step: distances 1 and 2 cannot both straddle one boundary); the run"""
    s = P.spec
    assert set(P.placed) == set(s.repeats), (s.name, sorted(P.placed))
    for k, places in P.placed.items():
        assert {m is not None for a, b, m in places} == {True, False}, (s.name, k, places)
        assert all(m in (None, CCHUNK, 2 * CCHUNK) for a, b, m in places), (s.name, k, places)
        for a, b, m in places:
            assert b - a == k and P.idx[a] == P.idx[b] < NLIVE and (m is None or a < m <= b), (s.name, k, a, b, m)
            assert m is not None or (a - 1) // CCHUNK == b // CCHUNK, (s.name, k, a, b)
    if s.run:
        a = CCHUNK - s.run // 2
        assert len(set(P.idx[a:a + s.run])) == 1 and P.idx[a] < NLIVE and a < CCHUNK < a + s.run
    assert P.b[P.idx[0]].real != P.b[P.idx[CCHUNK]].real and P.b[P.idx[0]].imag != P.b[P.idx[CCHUNK]].imag and P.gam[P.idx[0]] != P.gam[P.idx[CCHUNK]]


def R2(v):
    """complex -> its two parts as a real array (2, ...): what every step below works on, part by part as the kernels do (numpy's own
    complex product and conj() give other SIGNS OF ZERO than a r.re + a.im r.im, and a table row's zeros are compared in bits too)"""
    v = np.asarray(v, C128)
    return np.stack([v.real, v.imag])


def as_pairs2(v):
    """(2, n) or (2, N, n) parts -> interleaved (re, im) pairs (n 2) or (N, n 2)"""
    return np.ascontiguousarray(np.moveaxis(v, 0, -1)).reshape(v.shape[1:-1] + (-1,))


def cgrad(a, r, lam, conj=True):
    """cgrad_elem (csrc/ciao_common.h): (conj(a) res) lam = ((a.re r.re + a.im r.im) lam, (a.re r.im - a.im r.re) lam); -> the value and
    its two real products per part"""
    sg = 1.0 if conj else -1.0
    t1, t2 = np.stack([a[0] * r[0], a[0] * r[1]]), np.stack([sg * (a[1] * r[1]), -sg * (a[1] * r[0])])
    return (t1 + t2) * lam, [t1 * lam, t2 * lam]


def run(P, B=None, D=None, counts=None, keep=None, resume=None):
    """The chain of P.spec.alg over P.idx from P's start state: the steps of chain_cplx_kernel (chain_reg_kernels.h), which are those of
    the oracle (oracle/ciao_oracle_impl.inc, loss 3), on (re, im) parts in the kernels' own operation order.  -> {k: outputs after k
    steps, as (re, im) pairs}.  B: a ChainBounds that records every real sum.  D: planted defects (the host file): {"skip": k} |
    {"stale": k} | {"b_im_from": (k, j)} (step k takes the imaginary part of step j's b) | {"b_from": (k, j)} | {"gam_from": (k, j)} |
    {"no_conj": k} (the gradient a res for conj(a) res) | {"conj_dot": k} | {"drop_cross": k} (a.im x.re missing from the dot's imaginary
    part) | {"swap": (k, entries)} (re and im of those entries' share of the dot exchanged) | {"dot": (k, entries, factor)} |
    {"swap_sag": k} | {"no_last_prox": True}; k None: every step.  keep / resume as in chains_exact.run."""
    s, n, c = P.spec, P.n, P.cols
    A = np.stack([P.A.real, P.A.imag], axis=1)               # (N, 2, n)
    B = B if B is not None else _NoBounds()
    D = D or {}
    counts = set(counts if counts is not None else s.counts)
    alg = s.alg
    invN, LAM, GAMMA = 1.0 / N, P.lam, P.gamma
    av, p, zf, zs = R2(P.av0), R2(P.p0), R2(P.zf0), R2(P.z0)
    table = np.stack([P.table0.real, P.table0.imag], axis=1)
    before, out = {}, {}
    at = lambda key, k: key in D and (D[key] if not isinstance(D[key], tuple) else D[key][0]) in (k, None)

    def upd(name, *terms):
        B.update(name, *[np.broadcast_to(t, (2, n))[:, c].ravel() for t in terms])

    def prox(v, name="prox"):
        if s.prox == "zero":
            return v
        # the dead zone: n2 <= thr whatever rounds (a factor 4 inside it), the result exactly 0 (prox_cpair_chain; prox_cpair's hypot)
        assert (v[0] ** 2 + v[1] ** 2 <= (DEAD_GL / 2) ** 2).all(), f"{s.name}: {name}: an argument leaves the dead zone"
        return np.zeros((2, n))

    def dot(k, a, x, name):
        """s1r += a.re x.re - a.im x.im; s1i += a.re x.im + a.im x.re, from +0"""
        if any(at(key, k) for key in ("conj_dot", "drop_cross", "swap", "dot")):
            ai = -a[1] if at("conj_dot", k) else a[1]
            t = np.stack([a[0] * x[0] - ai * x[1], a[0] * x[1] + (0.0 if at("drop_cross", k) else ai * x[0])])
            if at("swap", k):
                e = D["swap"][1]
                t[:, e] = t[::-1, e]
            if at("dot", k):
                t[:, D["dot"][1]] *= D["dot"][2]
            return 0.0 + t.sum(axis=1)
        ac, xc = a[:, c], x[:, c]
        return 0.0 + np.array([B.dot(name + " (re)", np.concatenate([ac[0] * xc[0], -(ac[1] * xc[1])])),
                               B.dot(name + " (im)", np.concatenate([ac[0] * xc[1], ac[1] * xc[0]]))])

    def res(k, dd, i, name):
        bi = P.b[i]
        if at("b_from", k):
            bi = P.b[P.idx[D["b_from"][1]]]
        if at("b_im_from", k):
            bi = bi.real + 1j * P.b[P.idx[D["b_im_from"][1]]].imag
        bi = np.array([bi.real, bi.imag])
        B.update(name, dd, -bi)
        return dd - bi

    def grad(k, a, r):
        g, t = cgrad(a, r[:, None], LAM, conj=not at("no_conj", k))
        return g, t

    if alg == "lfinito":                                     # api_finito.hip lfinito_iterate_t: z_full = prox(av); the full pass
        zf = prox(av, "LFinito z_full")
        cc = HG * invN
        gs = [cgrad(A[i], (0.0 + (np.stack([A[i, 0] * zf[0] - A[i, 1] * zf[1], A[i, 0] * zf[1] + A[i, 1] * zf[0]])).sum(axis=1) - np.array([P.b[i].real, P.b[i].imag]))[:, None], LAM)
              for i in range(N)]
        upd("LFinito full pass", zf, *[-cc * t for g, ts in gs[:NLIVE] for t in ts])
        av = zf.copy()
        for g, ts in gs:
            av = av - cc * g
    inb, k0, skip = 0, 0, D.get("skip")
    if resume is not None:
        k0, (av, p, zf, zs, table, inb) = resume[0], [v.copy() if isinstance(v, np.ndarray) else v for v in resume[1]]
        skip = k0
    for k in range(k0, s.nsteps):
        i = int(P.idx[k])
        a = A[i]
        last = (inb + 1 == s.r)
        if keep is not None and P.live[k]:
            keep[k] = (av.copy(), p.copy(), zf.copy(), zs.copy(), table.copy(), inb)
        if skip == k:
            pass
        elif alg == "svrg":                                  # SVRG_basic.jl:74-81
            gz, tz = grad(k, a, res(k, dot(k, a, zf, "a.z_full"), i, "residual (z_full)"))
            gp, tp = grad(k, a, res(k, dot(k, a, p, "a.w"), i, "residual"))
            upd("SVRG update", *[GAMMA * t for t in tz], *[-GAMMA * t for t in tp], -GAMMA * av, p)
            t = gz - gp
            t = t - av
            t = t * GAMMA
            t = t + p
            p = prox(t)
            upd("SVRG sum", zs, p)
            zs = zs + p
        elif alg in ("saga", "sag"):                         # SAGA_basic.jl:56-65
            gn, tn = grad(k, a, res(k, dot(k, a, p, "a.z"), i, "residual"))
            sk = before[i] if D.get("stale") == k else table[i]
            dl = (gn - sk) * invN
            upd("SAGA update", *[GAMMA * t for t in tn], -GAMMA * sk, GAMMA * av, GAMMA * dl, p)
            upd("SAGA av", av, *[t * invN for t in tn], -sk * invN)
            if (alg == "sag") != at("swap_sag", k):
                av = av + dl
                wv = p - GAMMA * av
            else:
                wv = p - GAMMA * ((gn - sk) + av)
                av = av + dl
            p = prox(wv)
            if keep is not None and np.any(dl != 0):
                keep.setdefault("moved", []).append(k)
            before[i] = table[i].copy()
            table[i] = gn
        elif alg == "finito":                                # Finito_basic.jl:110-118
            gi = P.gam[P.idx[D["gam_from"][1]]] if at("gam_from", k) else P.gam[i]
            g, tg = grad(k, a, res(k, dot(k, a, p, "a.z"), i, "residual"))
            sk = before[i] if D.get("stale") == k else table[i]
            t = p - (gi * invN) * g
            rr = HG / gi
            upd("Finito update", rr * p, *[-rr * (gi * invN) * x for x in tg], -rr * sk, av)
            av = av + (t - sk) * rr
            before[i] = table[i].copy()
            table[i] = t
            if last:
                p = prox(av)
        else:                                                # Finito_LFinito.jl:92-98
            if inb == 0:
                p = prox(av)
            gi = P.gam[P.idx[D["gam_from"][1]]] if at("gam_from", k) else P.gam[i]
            cc, rr = HG * invN, HG / gi
            gz, tz = grad(k, a, res(k, dot(k, a, zf, "a.z_full"), i, "residual (z_full)"))
            gp, tp = grad(k, a, res(k, dot(k, a, p, "a.z"), i, "residual"))
            upd("LFinito update", av, *[cc * x for x in tz], *[-cc * x for x in tp], rr * p, -rr * zf)
            av = av + cc * gz
            av = av - cc * gp
            av = av + rr * (p - zf)
        inb = 0 if last else inb + 1
        if k + 1 in counts:
            if alg == "svrg":
                o = {"z": zs, "w": p}
            elif alg == "lfinito":
                o = {"av": av, "z": p, "z_full": zf}
            else:
                z = p
                if alg == "finito" and not last and not D.get("no_last_prox"):
                    z = prox(av, "prox (short last batch)")
                o = {"z": z, "av": av, "table": np.moveaxis(table, 1, 0)}
            out[k + 1] = {name: as_pairs2(v) for name, v in o.items()}
    return out


def found(spec, tries=24):
    """the CPU search: the first seed whose chain meets the condition -> (Chain, ChainBounds, reference)"""
    worst = []
    for seed in range(spec.seed0, spec.seed0 + tries):
        P, B = Chain(spec, seed), ChainBounds()
        ref = run(P, B)
        if B.worst() < spec.limit:
            return P, B, ref
        worst.append(round(B.worst(), 1))
    raise AssertionError(f"{spec.name}: no seed in {spec.seed0} .. {spec.seed0 + tries - 1} keeps every sum below 2^{spec.limit} quanta ({worst})")


# ---- the launcher's reports -------------------------------------------------------------------------------------------------------------------
CHAIN_REPORT = re.compile(r"^chain_(cdma_kernel|cplx_reg_kernel|cplx_kernel)<(f64|f32)((?:,\w+)*)> grid=(\d+) block=(\d+) steps=(\d+)$")


def classify_chain(report):
    """-> dict(kind "cdma" | "creg" | "cbig", dtype, J, EP, alg, masked, grid, threads, steps)"""
    m = CHAIN_REPORT.match(report)
    assert m, report
    tags = [t for t in m.group(3).split(",") if t]
    num = lambda pre: next((int(t[len(pre):]) for t in tags if re.fullmatch(pre + r"\d+", t)), None)
    return dict(kind={"cdma_kernel": "cdma", "cplx_reg_kernel": "creg", "cplx_kernel": "cbig"}[m.group(1)], dtype=F64 if m.group(2) == "f64" else F32,
                J=num("J"), EP=num("EP"), alg=num("alg"), masked="masked" in tags, grid=int(m.group(4)), threads=int(m.group(5)), steps=int(m.group(6)))


def T2(f64, f32):
    return {F64: f64, F32: f32}


def _of(v, dtype):
    return v[dtype] if isinstance(v, dict) and dtype in v else v


class Form:
    """One complex chain kernel form: the shape and options that select it (chain_launch.inc plan_chain) and what the launcher reports"""

    def __init__(self, name, n, kind, algs, opts=None, J=None, EP=None, masked=False, r=(1,)):
        self.name, self._n, self.kind, self.algs, self._opts, self._J, self._EP, self.masked, self.r = name, n, kind, tuple(algs), opts or {}, J, EP, masked, r

    def n(self, dtype):
        return _of(self._n, dtype)

    def opts(self, dtype):
        return dict(_of(self._opts, dtype))

    def depth(self, alg):
        return dma_depth(self._J, alg in TABLE_ALGS) if self.kind == "cdma" else 1      # (creg: the next row one step ahead; cbig: none)

    def expect(self, alg, dtype, steps):
        return dict(kind=self.kind, dtype=dtype, J=self._J, EP=_of(self._EP, dtype), alg=ALG_NO[alg], masked=self.masked, grid=1,
                    threads=1024 if self.kind == "cbig" else 256, steps=steps)

    def spec(self, alg, dtype, r=1, run=0):
        """(LFinito's ids say "_passthrough": in the dead zone its chain must leave the full pass's av and z = z_full = 0 -- no step, b_i
        or gamma_i of it is live; the module docstring)"""
        dep = self.depth(alg)
        n = self.n(dtype)
        rep = None if self.kind == "cdma" else ((1, 2, 3) if alg in TABLE_ALGS and not run else ())
        return Spec(f"{self.name}_{alg}{'_passthrough' if alg == 'lfinito' else ''}{'_r%d' % r if r > 1 else ''}{'_run%d' % run if run else ''}", alg, n, depth=dep, r=r, repeats=rep, run=run,
                    pc=pc_of(dtype))


_S3, _B2 = ("svrg", "saga", "sag"), ("finito", "lfinito")
_NODMA = {"chain_no_dma": 1}
FORMS = [
    # chain_cdma_kernel: rows of whole 16-byte chunks up to 16 KiB; J = the row's 4 KiB class; masked: the row ends short of it
    Form("cdma_j1", T2(256, 512), "cdma", _S3 + _B2, J=1, r=(1, 2, 5)),
    Form("cdma_j1_masked", T2(250, 500), "cdma", _S3 + _B2, J=1, masked=True, r=(1, 2, 5)),
    Form("cdma_j2", T2(512, 1024), "cdma", _S3, J=2),
    Form("cdma_j2_masked", T2(510, 1020), "cdma", _S3, J=2, masked=True),
    Form("cdma_j4", T2(1024, 2048), "cdma", _S3, J=4),
    Form("cdma_j4_masked", T2(1022, 2044), "cdma", _S3, J=4, masked=True),
    # 64 chunks: one live chunk for every lane of the first wave, three waves (and every further chunk) dead
    Form("cdma_64_chunks", T2(64, 128), "cdma", _S3 + ("finito",), J=1, masked=True),
    # chain_cplx_reg_kernel: EP complex entries a thread.  fp64 rows are whole chunks always (chain_no_dma); fp32 rows of an odd count are not
    Form("creg_ep1_255", 255, "creg", _S3, T2(_NODMA, {}), EP=1),                                   # the last thread holds no entry
    Form("creg_ep2_300", 300, "creg", _S3 + _B2, _NODMA, EP=2, r=(1, 2, 5)),                        # threads 44 .. 255 hold one of two
    Form("creg_ep4_1001", 1001, "creg", _S3, T2(_NODMA, {}), EP=4),                                 # odd; the last thread holds three of four
    Form("creg_ep8_2048", 2048, "creg", _S3, _NODMA, EP=8),
    # chain_cplx_kernel: forced, and past the register form
    Form("cbig_forced_300", 300, "cbig", _S3 + _B2, {"chain_big": 1}, r=(1, 2, 5)),
    Form("cbig_2049", 2049, "cbig", _S3, {}),
]
FORM_BY_NAME = {f.name: f for f in FORMS}
OPTION_DEFAULTS = {"chain_no_dma": 0, "chain_big": 0, "chain_max_batch": -1, "force_generic": 0, "sweep_grid": 0, "split_blocks_per_cu": 0}
# the run of one row across step 512 (RUN_ACROSS visits; SAGA and SAG in fp64 alone)
RUN_FORMS = ("cdma_j1", "cdma_j2_masked", "creg_ep2_300", "cbig_forced_300")
# fp32: the ring and the register chain on the same rows give the same bits (both are exact)
RING_VS_REG = ("cdma_j1", "cdma_j1_masked", "cdma_j2", "cdma_j4_masked")


def chain_cases():
    """(form, alg, r, dtype) of the device file; fp32 where the case's limit is 24"""
    out = []
    for f in FORMS:
        for alg in f.algs:
            rs = f.r if alg == "finito" else tuple(r for r in f.r if r <= 2) if alg == "lfinito" else (1,)
            for r in rs:
                for dtype in (F64, F32):
                    if dtype == F64 or f.spec(alg, dtype, r).limit == 24:
                        out.append((f, alg, r, dtype))
    return out


HOST_SPECS = ([Spec(f"host_{alg}_n300{'_r%d' % r if r > 1 else ''}", alg, 300, r=r, pc=2) for alg in ALGS for r in ((1, 2, 5) if alg == "finito" else (1, 2) if alg == "lfinito" else (1,))]
              + [Spec(f"host_{alg}_n64", alg, 64) for alg in ("svrg", "saga", "finito")]
              + [Spec("host_svrg_n1001_depth1", "svrg", 1001, depth=1, pc=2), Spec("host_saga_n300_depth1", "saga", 300, depth=1, repeats=(1, 2, 3)),
                 Spec("host_saga_n300_run7", "saga", 300, run=7), Spec("host_sag_n300_run5", "sag", 300, run=5),
                 Spec("host_finito_n300_run7", "finito", 300, run=7)])


# ---- the live complex NormL1 on one step ------------------------------------------------------------------------------------------------------
PROX_GL = 4.0
PROX_EDGES = [(4.0, 0.0), (0.0, -4.0), (4.0, 2.0 ** -8), (3.0, 3.0), (4.0, 1.0), (8.0, 0.0), (0.0, -8.0), (3.0, 4.0), (-5.0, 12.0), (2.0, 2.0),
              (-4.0, 4.0), (1.0, -1.0), (0.0, 0.0), (16.0, -2.0 ** -6), (-0.5, 4.0), (2.0 ** -10, 2.0 ** -10)]


def prox_exact(vr, vi, gl):
    """sign(v) max(|v| - gl, 0) to 50 digits (decimal: the square root is bracketed far below either type's rounding)"""
    from decimal import Decimal, getcontext
    getcontext().prec = 60
    r, i, g = Decimal(vr), Decimal(vi), Decimal(gl)
    n2 = r * r + i * i
    if n2 <= g * g:
        return 0.0, 0.0, Decimal(0)
    m = n2.sqrt()
    sc = 1 - g / m
    return r * sc, i * sc, m


# ---- the rows kernels: the sweeps ----------------------------------------------------------------------------------------------------------------
# rows_cplx_kernel (wave w = 4 block + wave-in-block takes rows w, w + 4 grid, ...: one partial d-vector per WAVE) and rows_csplit_kernel
# (workgroup b takes rows b, b + grid, ...: one partial per workgroup), finalize_kernel behind both.  plan_rows returns from its complex
# branch before `sweep_grid` is applied (rows_launch.inc), so the grid follows from the row count alone: min(ceil(n / 4), CUs) and, with
# split_blocks_per_cu = B, min(n, B CUs) -- the trip classes are reached through row counts sized from the CU count.
ROW_SWEEPS = ("grad", "saga_init", "finito_init")
ROWS_REPORT = re.compile(r"^rows_(cplx|csplit)_kernel<(f64|f32)(?:,J(\d+))?,mode(\d)>(?: \(cplx\))? grid=(\d+) block=(\d+)$")
ROW_BATCHES = ("finito_lists", "finito_blocks", "lfinito_lists", "lfinito_blocks")
ROW_MODE_NO = {"grad": 0, "saga_init": 2, "finito_init": 3, "finito_lists": 4, "finito_blocks": 4, "lfinito_lists": 1, "lfinito_blocks": 1}
ROW0 = 4                                                # first row of a row block: off row 0
ROWS_DEAD_GL = 2.0 ** 20                                # the rows' dead zone: a batch of 5000 rows sums to 2^17 and more
AXIS_GL = 2.0                                           # the live on-axis prox arguments' threshold hat_gamma lam_g
# g of a batch's epilogue (prox_cpair: hypot and two divisions): Zero; the complex NormL1's dead zone (exactly 0); LIVE arguments on an
# axis with |v| and gl powers of two (hypot(x, 0) = |x|, x / |x| = +-1: exact in the type) -- FINITO_BATCH's av is steered onto them
# by the incoming av.  GRAD2 (lfinito_iterate) takes z_full and z from prox(av): Zero and the dead zone
BATCH_PROX = {"finito": ("zero", "dead", "axis"), "lfinito": ("zero", "dead")}
ROWS_NOT_COVERED = {
    "the row dots a GRAD leg stores": "ciao_row_dots refuses complex problems (api_analysis.hip: 'covers real problems only'): no entry point reaches rowdot_out on complex rows",
    "rows_cplx_kernel behind finalize at partial counts that are no multiple of 4": "one partial a wave, four waves a workgroup",
    "a second batch of the same call": "after a batch z is too fine for fp32 (as in tests/rows_exact.py)",
    "live on-axis prox arguments under GRAD2": "its z_full = prox(av) and z = prox(av) feed the dots: an on-axis av after the full pass cannot be steered (FINITO_BATCH's can)",
}


class RowsProblem:
    """Np rows of n complex lattice entries: A dense in {0, +-1, +-i, +-1 +-i}, x0 and b Gaussian integers with parts in {-2 .. 2}, lam in
    {1, 1/2}, N_total a power of two, gam_i in {N_total / 4, N_total / 2}, hat_gamma = N_total / 2; g = Zero"""

    def __init__(self, Np, n, seed):
        rng = np.random.default_rng(seed)
        self.Np, self.n, self.d = int(Np), int(n), 2 * int(n)
        self.Nt = max(64, 1 << int(np.ceil(np.log2(self.Np))))
        self.lam = (1.0, 0.5)[seed % 2]
        self.A = gauss(rng, (Np, n), -1, 1)
        self.x0 = gauss(rng, n, -2, 2)
        self.x0[::3] = gauss(rng, len(self.x0[::3]), -2, 2, nonzero=True)
        self.b = gauss(rng, Np, -2, 2)
        self.gam = rng.choice([self.Nt / 4.0, self.Nt / 2.0], Np)
        self.hg, self.saga_gamma = self.Nt / 2.0, 0.5
        # the batches' lattice state: z, the incoming av, a table handed in; an ON-AXIS iterate for the objective's NormL1 term
        self.z, self.av, self.table0 = gauss(rng, n, -2, 2), gauss(rng, n, -2, 2), gauss(rng, (Np, n), -2, 2)
        self.z[::3] = gauss(rng, len(self.z[::3]), -2, 2, nonzero=True)
        ax = rng.integers(-2, 3, n).astype(F64)
        self.x_axis = np.where(rng.integers(0, 2, n) == 0, ax + 0j, 1j * ax)
        self.lam_axis = 0.5
        self.e = gauss(rng, Np, -2, 2) * (np.arange(Np) % 8 == 0)            # LFinito: b2 = A z_full - e (tests/rows_exact.py)
        self._b2 = {}

    def lam_g(self, kind):
        return {"zero": None, "dead": ROWS_DEAD_GL / self.hg, "axis": AXIS_GL / self.hg}[kind]

    def zfull(self, kind):
        return prox_pair(R2(self.av), None if kind == "zero" else ROWS_DEAD_GL, kind)

    def b2(self, kind):
        if kind not in self._b2:
            zf = self.zfull(kind)
            self._b2[kind] = (self.A * (zf[0] + 1j * zf[1])).sum(axis=1) - self.e
        return self._b2[kind]


def prox_pair(v, gl, kind):
    """prox_cpair on (2, n) parts: ax = hypot(re, im); (re / ax) m, (im / ax) m with m = ax - gl where ax > gl, else 0.  Exact where it is
    asked: g = Zero; the dead zone (a factor 2 inside it: whatever hypot rounds); on-axis arguments with |v| and gl powers of two"""
    if kind == "zero":
        return v
    ax = np.hypot(v[0], v[1])
    if kind == "dead":
        assert (ax <= gl / 2).all(), "a prox argument leaves the dead zone"
        return np.zeros_like(v)
    on_axis = (v[0] == 0) | (v[1] == 0)
    m, e = np.frexp(ax)
    assert on_axis.all() and ((m == 0.5) | (ax == 0)).all(), "a live prox argument is not on an axis with |v| a power of two"
    live = ax > gl
    safe = np.where(live, ax, 1.0)
    return np.where(live, (v / safe) * (ax - gl), 0.0)


def _dots(A, x):
    """(k, n) complex rows, x (2, n) -> the two real sums of every row's dot, from +0, and their terms"""
    a0, a1 = A.real, A.imag
    tr, ti = np.concatenate([a0 * x[0], -(a1 * x[1])], axis=1), np.concatenate([a0 * x[1], a1 * x[0]], axis=1)
    return tr, ti


def _row_grads(P, A, b, x, B, tag=""):
    """-> g (2, k, n) = cgrad_elem of every row at x, the real products behind each part, the residual's parts"""
    a0, a1 = A.real, A.imag
    tr, ti = _dots(A, x)
    dr, di = 0.0 + B.total("row dots (re)" + tag, tr, 1), 0.0 + B.total("row dots (im)" + tag, ti, 1)
    rr, ri = B.value("residual" + tag, dr - b.real), B.value("residual" + tag, di - b.imag)
    t = [a0 * rr[:, None], a1 * ri[:, None], a0 * ri[:, None], -(a1 * rr[:, None])]
    g = np.stack([(t[0] + t[1]) * P.lam, (a0 * ri[:, None] - a1 * rr[:, None]) * P.lam])
    return g, [np.concatenate([t[0], t[1]]) * P.lam, np.concatenate([t[2], t[3]]) * P.lam], rr, ri


def batch_rows(P, k, lists):
    """the k rows of a batch: a row block off row 0, or an index list -- distinct, unsorted, from all Np rows"""
    if not lists:
        return np.arange(ROW0, ROW0 + k, dtype=np.int64)
    return np.random.default_rng(1000 + k).permutation(P.Np)[:k].astype(np.int64)


def rows_batch_reference(P, mode, k, B, kind):
    """ONE batch of k rows from the lattice state, in the kernels' order (rows_kernels.h rows_cplx_kernel; epilogue_pre of ciao_common.h)
    -> outputs as (re, im) pairs, and "av_in": the incoming av the call takes.
    finito_*: t_i = z - (gam_i / N) grad f_i(z); av = sum_i (t_i - table_i) hat_gamma / gam_i + av_in; table_i = t_i; z = prox(av).
    lfinito_*: z_full = prox(av_in); the full pass av1 = -(hat_gamma / N) sum_i grad f_i(z_full) + z_full over ALL rows; z = prox(av1);
    av = (hat_gamma / N) sum_i (grad f_i(z_full) - grad f_i(z)) + av1 + E z - E z_full, E = sum_i hat_gamma / gam_i (targets b2)"""
    rows = batch_rows(P, k, mode.endswith("lists"))
    A, gam = P.A[rows], P.gam[rows]
    gl = {"zero": None, "dead": ROWS_DEAD_GL, "axis": AXIS_GL}[kind]
    if mode.startswith("finito"):
        z = R2(P.z)
        g, gt, rr, ri = _row_grads(P, A, P.b[rows], z, B)
        t = B.value("FINITO_BATCH table", z[:, None, :] - (gam / P.Nt)[None, :, None] * g)
        t0 = np.stack([P.table0.real, P.table0.imag])
        diff = B.value("FINITO_BATCH difference", t - t0[:, rows]) * (P.hg / gam)[None, :, None]
        S = np.stack([0.0 + B.total("FINITO_BATCH sum", diff[q], 0) for q in (0, 1)])
        if kind == "axis":                                   # the incoming av steers the sum onto axis points of modulus 2, 4, 8 (2: n2 == thr)
            j = np.arange(P.n)
            target = np.where(j % 2 == 0, 1.0, 1j) * np.where(j % 4 < 2, 1.0, -1.0) * 2.0 ** (1 + j % 3)
            av_in = B.value("FINITO_BATCH incoming av", R2(target) - S)
        else:
            av_in = R2(P.av)
        av = B.value("FINITO_BATCH av", S + av_in)
        table = t0.copy()
        table[:, rows] = t
        return {"table": as_pairs2(table), "av": as_pairs2(av), "z": as_pairs2(prox_pair(av, gl, kind)), "av_in": as_pairs2(av_in)}
    zf, b2 = P.zfull(kind), P.b2(kind)
    gall, gallt, _, _ = _row_grads(P, P.A, b2, zf, B, " (full pass)")
    S1 = np.stack([0.0 + (B.total("LFinito pass sum", gallt[q], 0), gall[q].sum(axis=0))[1] for q in (0, 1)])
    av1 = B.value("LFinito pass av", (-(P.hg / P.Nt)) * S1 + zf)
    z = prox_pair(av1, gl, kind)
    g1, g1t, _, _ = _row_grads(P, A, b2[rows], zf, B)
    g2, g2t, _, _ = _row_grads(P, A, b2[rows], z, B, " (z)")
    S2 = np.stack([0.0 + (B.total("GRAD2 sum", np.concatenate([g1t[q], -g2t[q]]), 0), (g1[q] - g2[q]).sum(axis=0))[1] for q in (0, 1)])
    extra = B.total("GRAD2 extra", P.hg / gam, 0)
    a = B.value("GRAD2 av", (P.hg / P.Nt) * S2)
    a = B.value("GRAD2 av", a + av1)
    a = B.value("GRAD2 av", a + B.value("GRAD2 av", extra * z))
    a = B.value("GRAD2 av", a + B.value("GRAD2 av", (-extra) * zf))
    return {"av": as_pairs2(a), "z": as_pairs2(z), "z_full": as_pairs2(zf), "av_in": as_pairs2(R2(P.av)), "extra": extra}


def rows_reference(P, mode, k, B, D=None, x=None):
    """the sweep over rows [0, k), part by part in the kernels' operation order (cgrad_elem) -> outputs as (re, im) pairs.  D:
    {"drop_partial": (parts, j)}: partial j of `parts` (rows j, j + parts, ...) missing from finalize"""
    A, b = P.A[:k], P.b[:k]
    x = P.x0 if x is None else x
    a0, a1, xr, xi = A.real, A.imag, x.real, x.imag
    dr = 0.0 + B.total("row dots (re)", np.concatenate([a0 * xr, -(a1 * xi)], axis=1), 1)
    di = 0.0 + B.total("row dots (im)", np.concatenate([a0 * xi, a1 * xr], axis=1), 1)
    rr, ri = B.value("residual", dr - b.real), B.value("residual", di - b.imag)
    t = [a0 * rr[:, None], a1 * ri[:, None], a0 * ri[:, None], -(a1 * rr[:, None])]
    g = np.stack([(t[0] + t[1]) * P.lam, (a0 * ri[:, None] - a1 * rr[:, None]) * P.lam])                 # (2, k, n)
    gterms = [np.concatenate([t[0], t[1]]) * P.lam, np.concatenate([t[2], t[3]]) * P.lam]             # the real products behind each part
    keep = np.ones(k, bool)
    if D and "drop_partial" in D:
        parts, j = D["drop_partial"]
        keep[j::parts] = False
    total = lambda name, terms, v: (B.total(name, terms, 0), 0.0 + v[keep].sum(axis=0))[1]
    if mode == "grad":
        S = np.stack([total("GRAD sum", gterms[q], g[q]) for q in (0, 1)])
        f = np.concatenate([(P.lam / 2.0) * rr * rr, (P.lam / 2.0) * ri * ri])
        B.value("objective term", f)
        extra = B.total("objective", f, 0)
        return {"av": as_pairs2(B.value("GRAD av", S / P.Nt)), "obj": extra * (1.0 / P.Nt), "gval": P.lam_axis * float(np.abs(x.real).sum() + np.abs(x.imag).sum())}
    if mode == "saga_init":
        S = np.stack([total("SAGA_INIT sum", gterms[q], g[q]) for q in (0, 1)])
        return {"table": as_pairs2(g), "av": as_pairs2(B.value("SAGA_INIT av", S / P.Nt)), "z": as_pairs2(R2((1.0 - P.saga_gamma) * P.x0))}
    gam = P.gam[:k]
    x = R2(P.x0)[:, None, :]
    table = B.value("FINITO_INIT table", x - (gam / P.Nt)[None, :, None] * g)
    S = np.stack([total("FINITO_INIT sum", np.concatenate([np.broadcast_to(x[q], (k, P.n)) / gam[:, None], -gterms[q][:k] / P.Nt, -gterms[q][k:] / P.Nt]),
                        table[q] * (1.0 / gam)[:, None]) for q in (0, 1)])
    av = B.value("FINITO_INIT av", P.hg * S)
    return {"table": as_pairs2(table), "av": as_pairs2(av), "z": as_pairs2(av)}


def classify_rows(report, k):
    """-> dict(kind "cplx" | "csplit", dtype, J, mode, grid, workers, parts, trips)"""
    m = ROWS_REPORT.match(report)
    assert m, report
    kind, grid = m.group(1), int(m.group(5))
    assert int(m.group(6)) == 256, report
    workers = grid * (4 if kind == "cplx" else 1)
    trips = sorted(max(0, -(-(k - w) // workers)) for w in range(workers))
    return dict(kind=kind, dtype=F64 if m.group(2) == "f64" else F32, J=int(m.group(3)) if m.group(3) else None, mode=int(m.group(4)), grid=grid,
                workers=workers, parts=workers, trips=trips)


def trip_classes(c):
    t, out = set(c["trips"]), set()
    if 0 in t:
        out.add("an idle worker")
    for q in (1, 2, 3):
        if q in t:
            out.add(f"{q} trip{'s' if q > 1 else ''}")
    if max(t) >= 5:
        out.add(">= 5 trips")
    return out


class RowsCase:
    """name; chunks: 16-byte chunks of a row (csplit), or n: complex entries by type (cplx); deep: also run at 2, 3 and >= 5 trips"""

    def __init__(self, name, kind, chunks=None, n=None, J=None, opts=None, deep=False, two=True):
        self.name, self.kind, self.chunks, self._n, self.J, self.opts, self.deep, self.two = name, kind, chunks, n, J, dict(opts or {}), deep, two

    def n(self, dtype):
        return self.chunks * pc_of(dtype) if self.chunks else _of(self._n, dtype)

    def launches(self, num_cu):
        """row counts: an idle worker beside one trip (cplx: 3 rows on four waves); 1 trip; and for the deep cases 2 and 1, 3 and 2, 6 and 5"""
        W = num_cu * (4 if self.kind == "cplx" else self.opts.get("split_blocks_per_cu", 1))
        small = [1, 2, 3, 7] if self.kind == "csplit" else [3, 4, 8]          # grids of 1, 2, 3 (csplit: a workgroup a row), 1, 1, 2 (cplx)
        return small + ([W + 1, 2 * W + 2, 5 * W + 1] if self.deep else [W + 1] if self.kind == "csplit" and self.two else [])

    def problem(self, dtype, num_cu):
        return RowsProblem(max(self.launches(num_cu)) + ROW0, self.n(dtype), seed=len(self.name) + self.n(dtype))

    def need(self):
        need = {"1 trip", "2 trips"} if (self.kind == "csplit" and self.two) or self.deep else {"1 trip"}
        if self.deep:
            need |= {"3 trips", ">= 5 trips"}
        if self.kind == "cplx":
            need.add("an idle worker")                   # (rows_csplit_kernel's plan gives min(rows, ...) workgroups: none idle)
        return need


_SPLIT1 = {"split_blocks_per_cu": 1}
ROWS_CASES = [
    RowsCase("cplx_3", "cplx", n=3, deep=True),
    RowsCase("cplx_35", "cplx", n=35, deep=True),                                        # an odd count: no fp32 row is whole chunks
    RowsCase("cplx_forced_64_chunks", "cplx", chunks=64, opts={"force_generic": 1}),
    RowsCase("csplit_64_chunks", "csplit", chunks=64, J=1, opts=_SPLIT1, deep=True),     # the smallest eligible row
    RowsCase("csplit_j1", "csplit", chunks=256, J=1, opts=_SPLIT1),
    RowsCase("csplit_j1_two_a_cu", "csplit", chunks=256, J=1, opts={"split_blocks_per_cu": 2}),      # grid = min(rows, 2 CUs)
    RowsCase("csplit_j2", "csplit", chunks=512, J=2, opts=_SPLIT1),
    RowsCase("csplit_j4_dead_chunks", "csplit", chunks=1000, J=4, opts=_SPLIT1),         # the last group of 256 chunks: 232 live, 24 dead
    RowsCase("csplit_j8", "csplit", chunks=2048, J=8, opts=_SPLIT1, two=False),         # (32 and 64 KiB rows: 3 and 7 rows, one trip)
    RowsCase("csplit_j16", "csplit", chunks=4096, J=16, opts=_SPLIT1, two=False),
]
FINALIZE_PARTS = (1, 2, 33, 64, 65, 257, 1025)                                          # rows_csplit_kernel: one workgroup and one partial a row

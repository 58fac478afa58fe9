"""Exact lattice problems for the real-typed chain kernels (csrc/chain_reg_kernels.h chain_kernel / chain_big_kernel, chain_dma_kernels.h,
chain_ws_kernels.h, chain_wide_kernels.h, the chain batch): the method of tests/rows_exact.py carried to the sequential hot path.

On the data below every sum a chain step forms -- the two dot products, the residual, every coordinate's update, the prox's shift, SVRG's
running sum -- is a sum of multiples of one power of two whose ABSOLUTE values add up to less than 2^24 of them (2^53 for the cases that
only fp64 can hold: their names end in "_f64only").  Every association of such a sum is exact in the type, so the state after any number
of steps does not depend on how a row is dealt to lanes, waves and workgroups, on contraction or on re-association, and it is compared in
BITS.  A stale table row, a b_i or gamma_i of the wrong step, a chunk, wave or workgroup missing from a dot product, a step missing from
SVRG's sum all change the bits.  `ChainBounds` (rows_exact.Bounds with per-coordinate quanta) computes the condition from the data, per
case; tests/test_chains_exact_host.py and the device test assert it -- a condition, not a tolerance.

The data.  Least squares, 256 rows, N_total = 256.  A chain's lattice gets finer with every step that does something, so a chain is made
of LIVE steps and IDLE steps.  Rows 0 .. 239 are live: two +-1 each on the case's MARKED columns (`marked_columns`: the first and last
element, the last valid 16-byte chunk of a masked row, both ends of every workgroup's 2048 columns -- a last workgroup's single column --
and a spread over every wave's share), dealt so that the rows the steps take have DISJOINT supports while the columns last (d >= 160;
below that the table algorithms' chains hold in fp64 only and their names end in "_f64only"), and b in {-2 .. 2}.  Every live step and
every repeat takes a row no other step takes.  Rows 240 .. 255 are idle: all zero, b = 0, a zero table row (Finito: the start iterate, see below): they add exact zeros to the
dot products and leave every quantum where it is (the iterate still moves by gamma av in an idle SAGA step: on the lattice it already
has).  lam = 1.  SVRG: gamma = 1/2 -- with two non-zeros a step annihilates the row's residual and the lattice stays put -- and NormL1 with
threshold 1/2.  SAGA / SAG: gamma = 1 (the row's residual is reflected), IndBox [-2, 2]; what refines the lattice is the 1 / N of the
aggregate alone, 8 bits per visit of a column.  Finito / LFinito: gam[i] in {N/4, N/2}, hat_gamma = N/2, IndBox [-2, 2].  The states (av,
z, w, z_full, the table rows) are handed in on the lattice, zero off the marked columns: svrg_inner, saga_steps, finito_steps and
lfinito_iterate take their state from the caller, and the reference below is a restatement of the STEP (chain_reg_kernels.h:172-232 is
its plain statement), not of the algorithm's meaning.  A live row's table row starts at 15 tau a_i (never a gradient's value) with av =
tau a_i / 8 and z = -2 tau a_i on its columns: its first visit turns those coordinates of z against the idle drift, so a repeat sees
whether the first visit happened.  Logistic leg (SAGA, SAG, Finito): per-coordinate bounds lo = hi = 0 on the marked columns hold every
margin at 0, the coefficient is exactly -y / 2 (exp(0) = 1, as in tests/rows_exact.py) and enters the table and av.

SAG starts from av = 0 and z = +-1, Finito from av = z = +-1 with EVERY table row at z (its aggregate adds z - table_i on every column):
their iterates then rest inside the box until a row visits a column, and a repeat finds z moved by the first visit.

Cached-dots SVRG ("svrgc", chain_dma_kernel's CA_SVRGC) cannot take a handed-in state: its a_i'z_full come from the full pass of the call
before.  Its chain is a whole svrg_iterate after svrg_init at the lattice point x0 = z_full -- the full pass at a lattice point is a
lattice state again (`full_gradient` records its sums) -- compared after 1, 2, 4, 8, 16, 1024 and 2048 steps, whose tail z_full = z / n
is exact; the rows carry the signs of x0 on their columns, since w starts AT z_full and a row with a_i'x0 = 0 would do nothing.

What the lattice costs (also in `default_prox`): NormL1 is run under SVRG only; a Finito repeat inside ONE batch, and any repeat of the
logistic leg (its iterate is pinned), rewrites the row with the value it has: those steps are held by the stale-row defect of the host
file, not by "every live step matters".

Live steps sit where the kernels' structure turns (`live_steps`): steps 0 .. DEPTH + 1, the last DEPTH + 1 steps of every compared step
count, +- DEPTH around every staging boundary (1024 and 2048: CHAIN_CHUNK; 192, 256 and 512 for chain_ws_kernel's record ring of WS_RR =
256 entries, staged up to WS_RR - 64 ahead).  chain_big_kernel stages nothing (it reads idx[s] in the step, chain_reg_kernels.h:286-287)
and chain_wide_kernel keeps the next two steps' rows in three register sets in rotation (chain_wide_kernels.h:425-430; its mailbox step
number is 32 bits wide and does not wrap below 2^32 steps): their marks are the same as everybody's, and the repeats at distance 1, 2 and 3
are their stale-row cases (fix1 / fix2, chain_wide_kernels.h:378).  For the table algorithms the same row recurs at distances 1 .. DEPTH + 1
and WS_STORE_LAG +- 1 (the ws kernel: also around its ring of 16 slots and its stale window of 25), each once inside a chunk and once
STRADDLING a staging boundary (`place_repeats`), and the "seven" cases take one row seven times in a row across step 1024.

One pass of the restatement gives the exact state after every compared step count (NSTEPS: 1, 2, DEPTH - 1, DEPTH, DEPTH + 1, 1023, 1024,
1025, 2049 and the whole chain), so the device runs every prefix against the same reference.

A plain module: tests/test_chains_exact_host.py holds the restatement against the oracle in bits, asserts the bound and plants the
defects; tests/test_gpu_chains_exact.py runs the cases on the device."""
import re

import numpy as np

from rows_exact import Bounds, quantum, vec_of

F64, F32 = np.float64, np.float32
N, NLIVE = 256, 240
CHUNK = 1024                                            # chain_common.h CHAIN_CHUNK
WS_RR, WS_AHEAD, WS_STORE_LAG, WS_RING, WS_STALE = 256, 256 - 64, 6, 16, 16 + 6 + 3      # chain_ws_kernels.h
SHARED_BELOW = 160                                      # d below which the live rows of a table algorithm's chain cannot have disjoint supports
MARKED = 320                                            # marked columns at most: two for each of 160 live rows with disjoint supports
WIDE_SLICE = 2048                                       # chain_launch.inc: WIDE_NT x E columns per workgroup
ALGS = ("svrg", "saga", "sag", "finito", "lfinito")
TABLE_ALGS = ("saga", "sag", "finito")
ALG_NO = {"svrg": 0, "saga": 1, "sag": 1, "finito": 2, "lfinito": 3, "svrgc": 4}
HG, GL = N / 2.0, 0.5


def reg_depth(E):
    """chain_common.h ChainDepth<E>"""
    return 8 if E <= 4 else 4 if E <= 8 else 2


def dma_depth(cls, table):
    """chain_dma_kernels.h DmaDepth<J NT / 256, TABLE> (unsharded); cls = row bytes / 4096, 0 for the one-wave kernels"""
    return (8 if cls <= 2 else 4 if cls <= 4 else 2) if table else (8 if cls <= 4 else 4)


# ---- the condition ------------------------------------------------------------------------------------------------------------------------
def column_worst(terms):
    """terms (k, n): for every column the sum of its k absolute values in units of the column's own quantum (rows_exact.quantum of that
    column); -> the largest over the columns"""
    t = np.abs(np.asarray(terms, F64))
    if t.ndim == 1:
        t = t[:, None]
    m, e = np.frexp(t)
    M = (m * 2.0 ** 53).astype(np.int64)
    low = M & -M
    lowexp = np.where(low > 0, e - 53 + np.log2(np.maximum(low, 1).astype(F64)), np.inf)
    q = lowexp.min(axis=0)                              # log2 of each column's quantum (inf: an all-zero column)
    live = np.isfinite(q)
    if not live.any():
        return 0.0
    return float((t[:, live].sum(axis=0) * 2.0 ** (-q[live])).max())


class ChainBounds(Bounds):
    """rows_exact.Bounds, with the sums of a chain step: `dot` (one sum of many terms: its own quantum) and `update` (one sum per
    coordinate: every coordinate in ITS quantum -- a coordinate no live row touches stays coarse whatever the others do)"""

    def dot(self, name, terms):
        terms = np.asarray(terms, F64)
        self._rec(name, float(np.abs(terms).sum() / quantum(terms)))
        return terms.sum()

    def update(self, name, *terms):
        self._rec(name, column_worst(np.stack([np.broadcast_to(np.asarray(t, F64), np.shape(terms[0])) for t in terms])))


class _NoBounds:
    def dot(self, name, terms):
        return terms.sum()

    def update(self, name, *terms):
        pass


# ---- the data -----------------------------------------------------------------------------------------------------------------------------
def marked_columns(d, vec):
    """where the live rows' non-zeros go: first and last element, the last valid chunk's first element (the neighbour of a masked row's
    first dead chunk), the ends of every workgroup's 2048 columns (a last workgroup of one column: d - 1), and a spread over every
    wave's share of whatever the kernel's layout is; MARKED columns at most (all of them where d is no more)"""
    c = {0, d - 1, max(d - 2, 0), max(d - vec, 0), (d - 1) // vec * vec, min(1, d - 1)}
    for g in range(-(-d // WIDE_SLICE)):
        c |= {min(g * WIDE_SLICE, d - 1), min(g * WIDE_SLICE + WIDE_SLICE - 1, d - 1)}
    c = sorted(c)
    spread = [int(x) for x in np.linspace(0, d - 1, MARKED - len(c))] if d > MARKED else list(range(d))
    return np.array(sorted(set(c) | set(spread)), np.int64)


def live_steps(nsteps, depth, marks, counts=()):
    s = set(range(depth + 2))
    for n in tuple(counts) + (nsteps,):
        s |= set(range(n - depth - 1, n))
    for m in marks:
        s |= set(range(m - depth, m + depth + 1))
    return sorted(k for k in s if 0 <= k < nsteps)


def place_repeats(idx, live, marks, distances, rows, inside_at, chunks=(CHUNK, WS_RR)):
    """the same (live) row at steps (a, a + k) for every k of `distances`: once with a < m <= a + k for a mark m (the first mark with
    room), once inside a chunk from `inside_at` on (`chunks`: the staging lengths no such pair may straddle).  Marks idx and live in place
    -> {k: [(a, a + k, straddled mark or None), ...]}"""
    used, out, take = set(), {}, rows.pop
    for k in distances:
        out[k] = []
        for m in marks:
            a = next((a for a in range(m - 1, m - k - 1, -1) if a >= 0 and a + k < len(idx) and a not in used and a + k not in used), None)
            if a is not None:
                r = take()
                idx[a] = idx[a + k] = r
                live[a] = live[a + k] = True
                used |= {a, a + k}
                out[k].append((a, a + k, m))
                break
        a = inside_at
        while a in used or a + k in used:
            a += 1
        if a + k < len(idx) and all((a - 1) // c == (a + k) // c for c in chunks):
            r = take()
            idx[a] = idx[a + k] = r
            live[a] = live[a + k] = True
            used |= {a, a + k}
            out[k].append((a, a + k, None))
    return out


def prox_apply(kind, v, gl, lo, hi, B=None, name="prox"):
    """op_prox of the oracle / prox_bf of the chains: the soft threshold's three-way form, or the clamp"""
    if kind == "l1":
        if B is not None:
            B.update(name, v, np.full_like(v, gl))
        return v + np.where(v <= -gl, gl, np.where(v >= gl, -gl, -v))
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


class Spec:
    """One chain case.  alg; d; nsteps; depth: the kernel's look-ahead DEPTH (positions and repeat distances); marks: staging boundaries;
    prox: "l1" (threshold 1/2) | "box" ([-2, 2]) | "boxvec" (per-coordinate, [-2, 2]); r: Finito / LFinito batch; repeats: distances of
    recurring rows (table algorithms); seven: one row seven times in a row across step 1024; limit: 24, or 53 (fp64 only); plus: SVRG++'s
    epoch tail (w kept) for the cached-dots kind "svrgc"."""

    def __init__(self, name, alg, d, nsteps=2100, depth=8, marks=(CHUNK, 2 * CHUNK), prox=None, r=1, repeats=None, seven=False, limit=24,
                 counts=None, vec=2, nnz=2, seed0=0, loss="ls", plus=False):
        self.loss, self.plus = loss, plus
        if alg == "svrgc":
            # a whole svrg_iterate: its tail divides z by the step count, so the compared counts are powers of two (1 .. 2 DEPTH, and 1024
            # and 2048 at the chunk boundaries)
            nsteps = min(nsteps, 2 * CHUNK)
            counts = counts if counts is not None else (1, 2, 4, 8, 16, CHUNK, 2 * CHUNK)
            assert all(n & (n - 1) == 0 for n in counts) and nsteps & (nsteps - 1) == 0
            name += "_plus" if plus else ""
        if loss == "logistic":
            assert alg in TABLE_ALGS                         # (SVRG and LFinito take the difference of two coefficients: at margin 0 they cancel)
            prox, name = "pinned", name + "_logistic"
        if alg in ("saga", "sag") and d < SHARED_BELOW and loss == "ls":
            limit = 53                                       # the live rows share columns: SAGA's and SAG's lattice then leaves fp32, fp64 holds it
        name += "_f64only" if limit == 53 else ""
        self.name, self.alg, self.d, self.nsteps, self.depth, self.r = name, alg, int(d), int(nsteps), int(depth), int(r)
        self.prox = prox or default_prox(alg)
        self.marks = tuple(m for m in marks if m < nsteps)
        self.table = alg in TABLE_ALGS
        self.repeats = tuple(repeats if repeats is not None else (sorted(set(range(1, depth + 2)) | {WS_STORE_LAG - 1, WS_STORE_LAG + 1})
                                                                  if self.table else ()))
        self.seven, self.limit, self.vec, self.nnz, self.seed0 = seven, limit, vec, nnz, seed0
        c = counts if counts is not None else (1, 2, depth - 1, depth, depth + 1, 1023, 1024, 1025, 2049)
        self.counts = tuple(sorted({n for n in c if 1 <= n < self.nsteps} | {self.nsteps}))


class Chain:
    """A Spec's data for one seed: A, b, gam, idx (the sample of every step), the live mask, the start state."""

    def __init__(self, spec, seed):
        rng = np.random.default_rng(seed)
        s, d = spec, spec.d
        self.spec, self.seed, self.d, self.table_alg = s, seed, d, s.alg in TABLE_ALGS
        self.cols = marked_columns(d, s.vec)
        nc = len(self.cols)
        self.A = np.zeros((N, d))
        order = rng.permutation(nc)
        order = np.concatenate([[nc - 1, 0], order[(order != nc - 1) & (order != 0)]])[:nc]      # row 0: the last and the first element (step 1's row)
        for i in range(NLIVE):                               # the marked columns dealt round robin: disjoint supports while they last
            mine = self.cols[[order[(i * s.nnz + q) % nc] for q in range(min(s.nnz, nc))]]
            self.A[i, mine] = rng.choice([-1.0, 1.0], len(mine))
        self.b = np.zeros(N)
        self.b[:NLIVE] = rng.integers(-2, 3, NLIVE)
        self.gam = rng.choice([N / 4.0, N / 2.0], N)
        # SAGA / SAG: gamma = 1 (a step reflects the row's residual; the 1 / N of the aggregate is what refines the lattice: module docstring)
        self.lam, self.gamma = (1.0, 1.0) if s.alg in ("saga", "sag") else (1.0, 0.5)
        self.lam_g = GL / (HG if s.alg in ("finito", "lfinito") else self.gamma)
        self.lo = np.full(d, -2.0)
        self.hi = np.full(d, 2.0)
        if s.prox == "boxvec":                               # per-coordinate bounds that differ from one coordinate to the next
            self.lo, self.hi = rng.choice([-2.0, -1.0], d), rng.choice([1.0, 2.0], d)
        if s.prox == "pinned":                               # the logistic leg: lo = hi = 0 on every marked column holds the margins at 0
            self.lo[self.cols] = self.hi[self.cols] = 0.0
            self.b[:] = rng.choice([-1.0, 1.0], N)           # labels (the idle rows' too: their rows are all zero)

        def on_cols(lo, hi):
            v = np.zeros(d)
            v[self.cols] = rng.integers(lo, hi + 1, nc)
            return v

        self.av0, self.z0 = on_cols(-1, 1) * (0.25 if self.table_alg else 1.0), on_cols(-2, 2)
        self.p0, self.zf0 = np.zeros(d), np.zeros(d)        # non-zero on every marked column: every non-zero of a row counts in step 0's dots
        self.p0[self.cols] = rng.choice([-2.0, -1.0, 1.0, 2.0], nc)
        self.zf0[self.cols] = -self.p0[self.cols]            # (and never the iterate's: a column missing from both of a step's dots shows)
        if s.alg == "svrgc":
            # w starts AT z_full and the l1 prox then takes it to 0: a live step does something only if a_i'z_full is not 0, so the
            # row's signs are those of z_full on its columns (up to one sign for the row)
            for i in range(NLIVE):
                nz = np.nonzero(self.A[i])[0]
                self.A[i, nz] = np.sign(self.zf0[nz]) * rng.choice([-1.0, 1.0])
        self.table0 = np.zeros((N, d))
        for i in reversed(range(NLIVE)):                     # (where columns run out and rows share them, the rows the steps take win)
            nz = np.nonzero(self.A[i])[0]
            # 15 tau a_i: never a gradient's value (|a_i'z - b_i| <= 6 inside the box), and with av = tau a_i / 8 on the same columns the
            # row's first visit turns its coordinates of z to the side the idle drift does not lead to: a later visit sees whether it happened
            tau = rng.choice([-1.0, 1.0])
            self.table0[i, nz] = 15.0 * tau * self.A[i, nz]
            if s.alg == "saga" or s.loss == "logistic":
                self.av0[nz] = 0.125 * tau * self.A[i, nz]
                self.p0[nz] = -2.0 * tau * self.A[i, nz]    # where the idle drift z -= gamma av leads
        if s.alg == "sag" and s.loss == "ls":
            # SAG's iterate moves by gamma av alone: from av = 0 and z = +-1 a column rests inside the box until a row visits it, and
            # drifts by that row's small difference afterwards -- a repeat finds z where the first visit did NOT leave it
            self.av0[:] = 0.0
            self.p0[self.cols] = rng.choice([-1.0, 1.0], nc)
        if s.alg == "finito" and s.loss == "ls":
            # Finito adds z - table_i on EVERY column: with av = z = +-1 and every table row (the idle rows' too) starting at z, nothing
            # moves off the columns a live row has visited, and z stays inside the box there; on its own columns a live row starts 3 off
            self.p0[self.cols] = rng.choice([-1.0, 1.0], nc)
            self.av0 = self.p0.copy()
            for i in range(N):
                nz = np.nonzero(self.A[i])[0]
                own = 3.0 * np.sign(self.table0[i, nz])
                self.table0[i] = self.p0
                self.table0[i, nz] += own
        # the steps
        n = s.nsteps
        live = np.zeros(n, bool)
        live[live_steps(n, s.depth, s.marks, s.counts)] = True
        idx = rng.integers(NLIVE, N, n).astype(np.int64)
        fresh = list(range(NLIVE - 1, 0, -1))                # every live step and every repeat takes a row no other step takes: 1, 2, ...
        self.placed = {}
        if s.repeats and n > 200:
            self.placed = place_repeats(idx, live, [m for m in s.marks if not (s.seven and m == CHUNK)], s.repeats, fresh, inside_at=40)
        if s.seven and n > CHUNK + 4:
            idx[CHUNK - 3:CHUNK + 4] = fresh.pop()
            live[CHUNK - 3:CHUNK + 4] = True
        if n > 1:
            idx[1] = 0
        for k in np.nonzero(live)[0]:
            if idx[k] >= NLIVE:
                idx[k] = fresh.pop()
        if n > CHUNK:                                        # slot 0 of the first chunk and of the second hold different b_i and gamma_i
            other = [r for r in reversed(fresh) if self.b[r] != self.b[idx[CHUNK]] and self.gam[r] != self.gam[idx[CHUNK]]]
            idx[0] = other[0]
            fresh.remove(other[0])
        if s.prox == "pinned":
            self.p0[self.cols] = 0.0
        self.idx, self.live = idx, live
        visits = np.bincount(idx[idx < NLIVE], minlength=NLIVE)
        designed = 2 * sum(len(v) for v in self.placed.values()) + (7 if s.seven and n > CHUNK + 4 else 0)
        assert visits.sum() - np.count_nonzero(visits) == designed - (len([1 for v in self.placed.values() for _ in v]) + (1 if s.seven and n > CHUNK + 4 else 0)), \
            "a live row is taken by two steps that are no designed repeat"

    def batches(self, n):
        """the first n samples as Finito batches of r (a short last one)"""
        r = self.spec.r
        return [self.idx[k:min(k + r, n)] for k in range(0, n, r)]


def check_placements(P):
    """every repeat distance of the case sits once inside a chunk and once across a staging boundary, on one row; the seven-fold row"""
    s = P.spec
    if s.nsteps > 200:
        assert set(P.placed) == set(s.repeats), (s.name, sorted(P.placed))
    for k, places in P.placed.items():
        assert {m is not None for a, b, m in places} == {True, False}, (s.name, k, places)
        for a, b, m in places:
            assert b - a == k and P.idx[a] == P.idx[b] < NLIVE and (m is None or a < m <= b), (s.name, k, a, b, m)
            assert m is not None or all((a - 1) // c == b // c for c in (CHUNK, WS_RR)), (s.name, k, a, b)
    if s.seven:
        assert len(set(P.idx[CHUNK - 3:CHUNK + 4])) == 1 and P.idx[CHUNK] < NLIVE


# ---- the step kinds, restated (float64; exact on the lattice) ---------------------------------------------------------------------------------
def full_gradient(P, x, B):
    """SVRG_basic.jl:87-92 (svrg_init, the epoch tail): -> (the row dots a_i'x the pass caches for the cached-dots chain, av = (1 / N) sum_i
    grad f_i(x))"""
    c = P.cols
    products = P.A[:, c] * x[c]
    B.update("full pass: row dots", *products.T)             # (one sum per row: the rows are the columns of the transposed terms)
    dots = products.sum(axis=1)
    B.update("full pass: residual", dots, -P.b)
    grads = ((dots - P.b)[:, None] * P.A) * P.lam
    B.update("full pass: sum", *(grads[:, c] / N))
    return dots, grads.sum(axis=0) / N


def run(P, B=None, D=None, counts=None, keep=None, resume=None):
    """The chain of P.spec.alg over P.idx from P's start state, in the reference's own operation order (oracle/ciao_oracle_impl.inc
    orc_svrg_inner, orc_saga_steps, orc_finito_steps, orc_lfinito_iterate), element for element what the kernels' steps state.
    -> {n: outputs after n steps} for n in counts (default: the spec's).  B: a ChainBounds that records every sum.  D: planted defects
    (tests/test_chains_exact_host.py): {"skip": k} | {"stale": k} | {"b_from": (k, j)} | {"gam_from": (k, j)} | {"dot": (k, columns,
    factor)} (k None: every step) | {"no_zsum": k} | {"swap_sag": k} (None: every step) | {"no_last_prox": True} | {"recompute": True}
    (cached-dots SVRG with a_i'z_full formed in the step: plain SVRG, the same bits) | {"cache_from": (k, j)} (step k reads row j's
    cached dot).  "svrgc" is a whole svrg_iterate from svrg_init at x0 = P.zf0: the inner cycle on the cached dots, then the epoch tail
    z_full = z / n (w = z_full unless spec.plus), z = 0, av = the full gradient at z_full.  keep: a dict that receives
    the state before every live step, and "moved": the steps whose table row changed; resume = (k, state): go on from there with step k
    SKIPPED (the host file's every-live-step-matters check)"""
    s, d, A, c = P.spec, P.d, P.A, P.cols
    B = B if B is not None else _NoBounds()
    D = D or {}
    counts = set(counts if counts is not None else s.counts)
    alg, kind = s.alg, ("l1" if s.prox == "l1" else "box")
    invN, LAM, GAMMA = 1.0 / N, P.lam, P.gamma
    av, p = P.av0.copy(), P.p0.copy()
    zf, zs, table = P.zf0.copy(), P.z0.copy(), P.table0.copy()
    before = {}                                              # a table row as it was before its latest rewrite (the "stale" defect)
    out = {}
    if alg in ("svrg", "svrgc", "saga", "sag"):
        tau, gl = GAMMA, GAMMA * P.lam_g
    else:
        tau, gl = HG, HG * P.lam_g
    prox = lambda v, name="prox": prox_apply(kind, v, gl, P.lo, P.hi, B, name)

    def dot(k, a, x, name):
        terms = a[c] * x[c]
        if D.get("dot") and D["dot"][0] in (k, None):
            _, cols, factor = D["dot"]
            full = a * x
            full[cols] *= factor
            return full.sum()
        return B.dot(name, terms)

    def coef(k, dd, i, name):
        bi = P.b[P.idx[D["b_from"][1]]] if D.get("b_from", (None,))[0] == k else P.b[i]
        if s.loss == "logistic":                             # -y / (1 + exp(y a'x)) at a'x = 0: exactly -y / 2, provided exp(0) = 1
            assert dd == 0, "the logistic leg is exact at margin 0 only"
            return -bi / 2.0
        B.update(name, np.array([dd]), np.array([-bi]))
        return dd - bi

    cache = None
    if alg == "svrgc":                                       # SVRG_basic.jl:57-68, orc_svrg_init: av at x0, w = z_full = x0, z = 0
        p, zs = zf.copy(), np.zeros(d)
        cache, av = full_gradient(P, zf, B)
    if alg == "lfinito":                                     # Finito_LFinito.jl:83-88, orc_lfinito_iterate: z_full = prox(av); the full pass
        zf = prox(av, "LFinito z_full")
        cc = HG * invN
        g = ((A @ zf - P.b)[:, None] * A) * LAM
        B.update("LFinito full pass", zf[c], *[-cc * g[i, c] for i in range(N)])
        av = zf.copy()
        for i in range(N):
            av = av - cc * g[i]
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
        elif alg in ("svrg", "svrgc"):                       # SVRG_basic.jl:74-81
            if alg == "svrgc" and not D.get("recompute"):    # a_i'z_full as the full pass left it (chain_dma_kernel's CA_SVRGC)
                d2 = cache[P.idx[D["cache_from"][1]]] if D.get("cache_from", (None,))[0] == k else cache[i]
            else:
                d2 = dot(k, a, zf, "a'z_full")
            gz = (a * coef(k, d2, i, "residual (z_full)")) * LAM
            gp = (a * coef(k, dot(k, a, p, "a'w"), i, "residual")) * LAM
            B.update("SVRG update", GAMMA * gz[c], -GAMMA * gp[c], -GAMMA * av[c], p[c])
            t = gz - gp
            t = t - av
            t = t * GAMMA
            t = t + p
            p = prox(t)
            if D.get("no_zsum") != k:
                B.update("SVRG sum", zs[c], p[c])
                zs = zs + p
        elif alg in ("saga", "sag"):                         # SAGA_basic.jl:56-65
            gn = (a * coef(k, dot(k, a, p, "a'z"), i, "residual")) * LAM
            sk = before[i] if D.get("stale") == k else table[i]
            dl = (gn - sk) * invN
            B.update("SAGA update", GAMMA * gn[c], -GAMMA * sk[c], GAMMA * av[c], GAMMA * dl[c], p[c])
            B.update("SAGA av", av[c], gn[c] * invN, -sk[c] * invN)
            if (alg == "sag") != ("swap_sag" in D and D["swap_sag"] in (k, None)):
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
            gi = P.gam[P.idx[D["gam_from"][1]]] if D.get("gam_from", (None,))[0] == k else P.gam[i]
            g = (a * coef(k, dot(k, a, p, "a'z"), i, "residual")) * LAM
            sk = before[i] if D.get("stale") == k else table[i]
            t = p - (gi * invN) * g
            rr = HG / gi
            B.update("Finito update", rr * p[c], -rr * (gi * invN) * g[c], -rr * sk[c], av[c])
            av = av + (t - sk) * rr
            before[i] = table[i].copy()
            table[i] = t
            if last:
                p = prox(av)
        else:                                                # Finito_LFinito.jl:92-98
            if inb == 0:
                p = prox(av)
            gi = P.gam[P.idx[D["gam_from"][1]]] if D.get("gam_from", (None,))[0] == k else P.gam[i]
            cc, rr = HG * invN, HG / gi
            gzf = (a * coef(k, dot(k, a, zf, "a'z_full"), i, "residual (z_full)")) * LAM
            gp = (a * coef(k, dot(k, a, p, "a'z"), i, "residual")) * LAM
            B.update("LFinito update", av[c], cc * gzf[c], -cc * gp[c], rr * p[c], -rr * zf[c])
            av = av + cc * gzf
            av = av - cc * gp
            av = av + rr * (p - zf)
        inb = 0 if last else inb + 1
        if k + 1 in counts:
            if alg == "svrg":
                out[k + 1] = {"z": zs.copy(), "w": p.copy()}
            elif alg == "svrgc":                             # SVRG_basic.jl:84-92, orc_svrg_iterate's tail after n = k + 1 steps
                n = k + 1
                assert n & (n - 1) == 0
                new_zf = zs / n
                B.update("tail: z / n", new_zf[c])
                out[n] = {"av": full_gradient(P, new_zf, B)[1], "z": np.zeros(d), "z_full": new_zf, "w": p.copy() if s.plus else new_zf.copy()}
            elif alg == "lfinito":
                out[k + 1] = {"av": av.copy(), "z": p.copy(), "z_full": zf.copy()}
            else:
                z = p
                if alg == "finito" and not last and not D.get("no_last_prox"):      # a short last batch ends in its prox as well
                    z = prox(av, "prox (short last batch)")
                out[k + 1] = {"z": z.copy(), "av": av.copy(), "table": table.copy()}
    return out


def found(spec, tries=24):
    """the CPU search: the first seed from spec.seed0 on whose chain meets the condition -> (Chain, ChainBounds, reference)"""
    worst = []
    for seed in range(spec.seed0, spec.seed0 + tries):
        P, B = Chain(spec, seed), ChainBounds()
        ref = run(P, B)
        if B.worst() < spec.limit:
            return P, B, ref
        worst.append(round(B.worst(), 1))
    raise AssertionError(f"{spec.name}: no seed in {spec.seed0} .. {spec.seed0 + tries - 1} keeps every sum below 2^{spec.limit} quanta ({worst})")


# ---- the classifier: a launch report -> what ran ----------------------------------------------------------------------------------------------
REPORT = re.compile(r"^chain_(kernel|dma_kernel|ws_kernel|wide_kernel|big_kernel)<(f64|f32)((?:,\w+)*)> grid=(\d+) block=(\d+) steps=(\d+)(?: grid=(\d+))?$")
BATCH = re.compile(r"^chain batch: (\d+) chains in (\d+) launch\(es\); first: (.*)$")


def classify(report):
    """-> dict(kind "reg" | "dma" | "ws" | "wide" | "big", dtype, J, E, alg, masked, threads, waves, issuers, workgroups, steps; chains,
    launches of a chain batch)"""
    out = {"chains": 1, "launches": 1}
    m = BATCH.match(report)
    if m:
        out["chains"], out["launches"], report = int(m.group(1)), int(m.group(2)), m.group(3)
    m = REPORT.match(report)
    assert m, report
    tags = [t for t in m.group(3).split(",") if t]
    num = lambda pre: next((int(t[len(pre):]) for t in tags if re.fullmatch(pre + r"\d+", t)), None)
    out.update(kind={"kernel": "reg", "dma_kernel": "dma", "ws_kernel": "ws", "wide_kernel": "wide", "big_kernel": "big"}[m.group(1)],
               dtype=F64 if m.group(2) == "f64" else F32, J=num("J"), E=num("E"), alg=num("alg"), masked="masked" in tags,
               issuers=num("issuers"), workgroups=int(m.group(7) or m.group(4)), threads=int(m.group(5)), waves=int(m.group(5)) // 64,
               steps=int(m.group(6)))
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def default_prox(alg):
    """SVRG: NormL1 (threshold 1/2).  The table algorithms and LFinito: IndBox [-2, 2] -- with NormL1 alone their iterates are not bounded
    on this data (gamma L is far above 1: the lattice's price) and leave the significand within a few dozen live steps: not made exact.
    Not made exact either: SAGA / SAG at d = 7.  Every visit of a column costs log2 N = 8 bits of its aggregate's lattice, the live rows
    need N >= 240 (every live step takes a fresh row, or a later visit rewrites the table row and the earlier step stops mattering), and
    the 73 live steps the positions ask for meet on seven columns about twenty times each: beyond 2^53 on every seed tried.  Fewer live
    steps would give up the positions, a smaller N_total the fresh rows.  At d = 50 .. 128 SAGA and SAG hold in fp64 only (names ending
    in _f64only); Finito, whose lattice does not refine by 1 / N, runs the one-wave register ring (d = 7, 50) in both types."""
    return "l1" if alg in ("svrg", "svrgc") else "box"


def T2(f64, f32):
    return {F64: f64, F32: f32}


def _of(v, dtype):
    return v[dtype] if isinstance(v, dict) else v


class Form:
    """One kernel form on the device: the shape and options that select it (chain_launch.inc plan_chain; the literal tables are in
    tests/test_gpu_chain_dispatch.py) and what the launcher must report -- kind, threads, J (the row's 4 KiB class) or E, masked, issuers,
    workgroups.  cls: the ring's row class for DmaDepth (0: the one-wave kernels); algs: the chains run on it."""

    def __init__(self, name, d, kind, threads, algs, opts=None, J=None, E=None, masked=False, issuers=None, workgroups=1, cls=None,
                 dtypes=(F64, F32), marks=(CHUNK, 2 * CHUNK), nsteps=2100, r=(1,), extra_repeats=()):
        self.name, self._d, self.kind, self.threads, self.algs, self.opts = name, d, kind, threads, tuple(algs), dict(opts or {})
        self._J, self._E, self.masked, self.issuers, self._wg, self.cls, self.dtypes = J, E, masked, issuers, workgroups, cls, dtypes
        self.marks, self.nsteps, self.r, self.extra_repeats = marks, nsteps, r, tuple(extra_repeats)

    def d(self, dtype):
        return _of(self._d, dtype)

    def depth(self, alg, dtype):
        if self.kind == "reg":
            return reg_depth(_of(self._E, dtype))
        if self.kind == "dma":
            return dma_depth(self.cls, alg in TABLE_ALGS)
        return 8                                             # ws: its windows are `extra_repeats`; wide, big: no ring (module docstring)

    def expect(self, alg, dtype, steps):
        return dict(kind=self.kind, dtype=dtype, J=_of(self._J, dtype), E=_of(self._E, dtype), alg=ALG_NO[alg], masked=self.masked,
                    issuers=self.issuers, workgroups=_of(self._wg, dtype), threads=self.threads, waves=self.threads // 64, steps=steps,
                    chains=1, launches=1)

    def spec(self, alg, dtype, r=1, seven=False, prox=None, loss="ls"):
        dep = self.depth(alg, dtype)
        rep = sorted(set(range(1, dep + 2)) | {WS_STORE_LAG - 1, WS_STORE_LAG + 1} | set(self.extra_repeats)) if alg in TABLE_ALGS else ()
        if seven:                                            # (the seven-fold row takes the boundary at 1024 for itself)
            rep = ()
        return Spec(f"{self.name}_{alg}{'_r%d' % r if r > 1 else ''}{'_seven' if seven else ''}", alg, self.d(dtype), nsteps=self.nsteps, depth=dep,
                    marks=self.marks, prox=prox or default_prox(alg), r=r, repeats=rep, seven=seven, vec=vec_of(dtype), loss=loss)


_WS_MARKS = (WS_AHEAD, WS_RR, 2 * WS_RR, CHUNK)
_WS_REP = (WS_RING - 1, WS_RING, WS_RING + 1, WS_STALE - 1, WS_STALE, WS_STALE + 1)
FORMS = [
    # chain_kernel, the register ring: one wave; four waves masked; four waves full; the largest E built (16 in fp64, 32 in fp32)
    Form("reg_1w_d7", 7, "reg", 64, ("svrg", "finito", "lfinito"), E=1, masked=True),     # (SAGA / SAG on 7 columns: not made exact, see default_prox)
    Form("reg_1w_d50", T2(51, 50), "reg", 64, ("svrg", "saga", "sag", "finito"), E=1, masked=True, r=(1, 5)),   # (fp64 rows of 50 are whole 16-byte chunks: the ring's)
    Form("reg_4w_d257", 257, "reg", 256, ALGS, E=4, masked=True, r=(1, 2)),
    Form("reg_4w_full_d1024", 1024, "reg", 256, ("svrg", "saga", "lfinito"), {"chain_no_dma": 1}, E=4),
    Form("reg_e_max", T2(4096, 8192), "reg", 256, ("svrg", "sag", "finito"), {"chain_no_dma": 1}, E=T2(16, 32)),
    # chain_big_kernel: forced, and beyond one workgroup's registers with the several-workgroup chain switched off
    Form("big_d300", 300, "big", 1024, ALGS, {"chain_big": 1}, r=(1, 2)),
    Form("big_beyond", T2(4100, 8196), "big", 1024, ("svrg", "saga"), {"chain_no_wide": 1}),
    # ("svrgc": cached-dots SVRG, the ring's alone -- plan_chain gives every other kernel the algorithm-0 instantiation)
    # chain_dma_kernel, the LDS-DMA ring: one wave (1 and 2 chunks a lane), four waves J = 1, 2, 4, eight waves; exact and masked
    Form("dma_1w_j1", T2(128, 256), "dma", 64, ALGS + ("svrgc",), J=1, cls=0, r=(1, 2, 5)),
    Form("dma_1w_j1_masked", T2(126, 252), "dma", 64, ("svrg", "saga", "finito", "svrgc"), J=1, masked=True, cls=0),
    Form("dma_1w_j2", T2(256, 512), "dma", 64, ("svrg", "sag", "lfinito", "svrgc"), J=1, cls=0),
    Form("dma_4w_short_masked", T2(126, 252), "dma", 256, ("svrg", "saga"), {"chain_four_waves": 1, "chain_no_ws": 1}, J=1, masked=True, cls=1),
    Form("dma_4w_j1", T2(512, 1024), "dma", 256, ALGS + ("svrgc",), {"chain_no_ws": 1}, J=1, cls=1, r=(1, 2)),
    Form("dma_4w_j1_masked", T2(500, 1000), "dma", 256, ("svrg", "saga", "finito"), {"chain_no_ws": 1}, J=1, masked=True, cls=1),
    Form("dma_4w_j2", T2(1024, 2048), "dma", 256, ("svrg", "saga", "finito", "lfinito", "svrgc"), J=2, cls=2),
    Form("dma_4w_j2_masked", T2(1022, 2044), "dma", 256, ("svrg", "sag"), J=2, masked=True, cls=2),
    Form("dma_4w_j4", T2(2048, 4096), "dma", 256, ("svrg", "saga", "finito"), J=4, cls=4),
    Form("dma_4w_j4_masked", T2(2046, 4092), "dma", 256, ("svrg", "saga", "lfinito", "svrgc"), J=4, masked=True, cls=4),
    Form("dma_8w", T2(4096, 8192), "dma", 512, ("svrg", "saga", "sag", "finito", "lfinito", "svrgc"), J=8, cls=8),
    # chain_ws_kernel: SAGA and SAG on rows of 2 .. 4 KiB, one and two issuer waves; 1100 steps: the record ring of 256 wraps four times
    Form("ws_issuers2", T2(512, 1024), "ws", 448, ("saga", "sag"), J=1, issuers=2, marks=_WS_MARKS, nsteps=1100, extra_repeats=_WS_REP),
    Form("ws_issuers2_masked", T2(500, 1000), "ws", 448, ("saga", "sag"), J=1, masked=True, issuers=2, marks=_WS_MARKS, nsteps=1100,
         extra_repeats=_WS_REP),
    Form("ws_issuers1", T2(512, 1024), "ws", 384, ("saga", "sag"), {"chain_ws_issuers": 1}, J=1, issuers=1, marks=_WS_MARKS, nsteps=1100,
         extra_repeats=_WS_REP),
    Form("ws_issuers1_masked", T2(500, 1000), "ws", 384, ("saga",), {"chain_ws_issuers": 1}, J=1, masked=True, issuers=1, marks=_WS_MARKS,
         nsteps=1100, extra_repeats=_WS_REP),
    # chain_wide_kernel: three workgroups, the last with ONE column (fp64); five, the last with one column
    Form("wide_3", 4097, "wide", 256, ("svrg", "saga", "finito", "lfinito"), E=8, workgroups=3, dtypes=(F64,), r=(1, 2)),
    Form("wide_5", 8193, "wide", 256, ("svrg", "saga", "sag", "finito", "lfinito"), E=8, workgroups=5, r=(1, 2)),
]
FORM_BY_NAME = {f.name: f for f in FORMS}
OPTION_DEFAULTS = {"chain_no_dma": 0, "chain_big": 0, "chain_no_wide": 0, "chain_four_waves": 0, "chain_no_ws": 0, "chain_ws_issuers": 0,
                   "chain_max_batch": -1}

# the logistic leg on the device: (form, algorithms)
LOGISTIC = [("reg_4w_d257", ("saga", "finito")), ("dma_1w_j2", ("sag",)), ("dma_4w_j1", ("saga", "finito")), ("dma_8w", ("saga",)),
            ("ws_issuers2", ("saga", "sag")), ("ws_issuers1_masked", ("saga",)), ("wide_5", ("saga", "finito")), ("big_d300", ("sag", "finito"))]

# the host file's cases: the same machinery on small d (d = 50: no 16-byte structure, every column marked; d = 300: marked columns only)
HOST_SPECS = [Spec(f"host_{alg}_d{d}{'_r%d' % r if r > 1 else ''}", alg, d, depth=8, prox=default_prox(alg), r=r)
              for alg in ALGS for d, r in ((50, 1), (300, 2 if alg in ("finito", "lfinito") else 1))]
HOST_SPECS += [Spec(f"host_{alg}_d300", alg, 300, loss="logistic") for alg in TABLE_ALGS]
HOST_SPECS += [Spec("host_svrgc_d50", "svrgc", 50), Spec("host_svrgc_d300", "svrgc", 300, plus=True)]
HOST_SPECS += [Spec("host_svrg_box_d50", "svrg", 50, prox="box"), Spec("host_saga_boxvec_d300", "saga", 300, prox="boxvec"),
               Spec("host_finito_r5_d300", "finito", 300, r=5), Spec("host_saga_seven_d300", "saga", 300, seven=True, repeats=()),
               Spec("host_saga_ws_d400", "saga", 400, nsteps=1100, marks=_WS_MARKS, repeats=sorted(set(range(1, 10)) | set(_WS_REP)))]

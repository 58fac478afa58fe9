"""Exact lattice problems for the rows kernels (csrc/rows_kernels.h, rowsw_, rowsm_, rowsl_kernels.h) and finalize_kernel behind them.

On the data below every sum a rows launch forms -- a row's dot product, a coordinate's partial sum in a wave, a workgroup, a partial
d-vector or finalize, the extra scalar -- is a sum of multiples of one power of two (its quantum) whose ABSOLUTE values add up to less
than 2^24 quanta.  Every partial sum in every order is then representable in fp32 (and fp64), every addition is exact, and the result
does not depend on how rows are dealt to waves, tiles, clusters and partials: it is compared in bits.  A row, chunk, tile or partial
that is dropped, doubled or stale changes the bits.  `Bounds` computes the condition from the data; it is asserted for every case
(tests/test_rows_exact_host.py) -- a condition, not a tolerance.

The data.  Least squares; A in {-1, 0, 1} dense; x0, z, av and b in {-2 .. 2}; lam in {1, 1/2}; N_total a power of two (PackedF(...,
N_total=): the entry points of csrc/api_*.hip accept any N_total >= N on a context with no communicator -- check_problem, api_core.hip -- so every N is
reachable with 1 / N_total a power of two); gam[i] in {N_total / 4, N_total / 2}; hat_gamma = N_total / 2 passed in (the entry points
take it as a number; Finito's own 1 / sum(1 / gam) is a power of two only for uniform gam); prox thresholds 1/2.  Every scalar that
multiplies a sum is then a power of two, so no expected value depends on whether the compiler contracts a multiply-add (the library is
built with -ffp-contract=off; with contraction on, every intermediate below is representable as well, so both forms round nowhere).

The batch modes take ONE batch per call (one rows launch, one finalize), from a state given on the lattice: after a batch z is a finer
lattice and a second batch's dots would round in fp32.  GRAD2 is reached through ciao_lfinito_iterate only, which runs a full GRAD pass
over all rows first and takes z = prox(av) from ITS result; for that z to stay small the problem of the LFinito calls has
b = A z_full - e with e in {-2 .. 2} on every eighth row and 0 elsewhere (b is then a half-integer of the size of a row dot, not in
{-2 .. 2}: the one departure from the plain lattice, and the bound check covers it like everything else).

Logistic leg: x = 0, labels in {-1, 1}: margin 0, coefficient -y / (1 + exp(0)) = -y / 2 exactly, provided exp(0) = 1.  It covers
GRAD (no objective: log 2 is not on a lattice; the row dots are exactly 0), SAGA_INIT, FINITO_INIT and FINITO_BATCH.  Not GRAD2: its
z comes out of the full pass and is not 0.

A plain module: tests/test_gpu_rows_exact.py runs it on the device, tests/test_rows_exact_host.py holds the restatement against the
oracle, asserts the bound for every case and plants the defects bit comparison is there to notice."""
import re

import numpy as np

F64, F32 = np.float64, np.float32
LIMIT_BITS = 24                                         # fp32's significand; asserted for both types (the data are the same)
SWEEPS = ("grad", "saga_init", "finito_init")
BATCHES = ("finito_lists", "finito_blocks", "lfinito_lists", "lfinito_blocks")
MODES = SWEEPS + BATCHES
ROW0 = 4                                                # first row of a row block: off row 0, 16-byte aligned for every d and type


def vec_of(dtype):
    return 16 // np.dtype(dtype).itemsize


# ---- the condition ------------------------------------------------------------------------------------------------------------------------
def quantum(a):
    """the largest power of two that every element of `a` is a multiple of (1 for all zeros)"""
    a = np.abs(np.asarray(a, F64)).ravel()
    a = a[a != 0]
    if a.size == 0:
        return 1.0
    m, e = np.frexp(a)                                  # a = m 2^e, 1/2 <= m < 1: m 2^53 is an integer
    M = (m * 2.0 ** 53).astype(np.int64)
    low = (M & -M).astype(F64)                          # its lowest set bit
    return float(2.0 ** (e - 53 + np.log2(low)).min())


class Bounds:
    """bits[name] = log2 of the largest sum of absolute values, in quanta, over the sums recorded under `name`"""

    def __init__(self):
        self.bits = {}

    def _rec(self, name, worst):
        self.bits[name] = max(self.bits.get(name, 0.0), float(np.log2(max(worst, 1.0))))

    def total(self, name, terms, axis):
        """the sum of `terms` along `axis`, any order: exact when the recorded figure is below the significand's width"""
        terms = np.asarray(terms, F64)
        q = quantum(terms)
        worst = float((np.abs(terms).sum(axis=axis) / q).max()) if terms.size else 0.0
        assert worst < 2.0 ** 53, name                  # (numpy's own float64 sums below are then exact too)
        self._rec(name, worst)
        return terms.sum(axis=axis)

    def value(self, name, v):
        """an elementwise intermediate: representable when |v| / quantum is below the significand's width"""
        v = np.asarray(v, F64)
        self._rec(name, float(np.abs(v).max() / quantum(v)) if v.size else 0.0)
        return v

    def worst(self):
        return max(self.bits.values()) if self.bits else 0.0


def lossless(v, dtype):
    """v (float64) in `dtype`; the cast must not round"""
    v = np.asarray(v, F64)
    c = v.astype(dtype)
    assert np.array_equal(c.astype(F64), v), "an expected value is not representable in the type"
    return c


# ---- the data -----------------------------------------------------------------------------------------------------------------------------
class Problem:
    """Np rows of d lattice elements and everything the five modes take.  loss "logistic": labels, and x0 = z = 0."""

    def __init__(self, Np, d, seed, loss="ls"):
        rng = np.random.default_rng(seed)
        self.Np, self.d, self.loss = int(Np), int(d), loss
        self.Nt = max(64, 1 << int(np.ceil(np.log2(self.Np))))
        self.lam = (1.0, 0.5)[seed % 2] if loss == "ls" else 1.0
        self.A = rng.integers(-1, 2, (Np, d)).astype(F64)
        self.x0 = rng.integers(-2, 3, d).astype(F64)             # the sweeps' and inits' iterate
        self.z = rng.integers(-2, 3, d).astype(F64)              # the Finito batch's z
        self.av = rng.integers(-2, 3, d).astype(F64)             # the batches' incoming av
        self.gam = rng.choice([self.Nt / 4.0, self.Nt / 2.0], Np)
        self.hg = self.Nt / 2.0
        self.gl = 0.5                                            # every prox threshold: tau lam_g
        self.lam_g = self.gl / self.hg                           # Finito's g: tau = hat_gamma
        self.saga_gamma, self.saga_lam_g = 0.5, 1.0              # SAGA's z = prox_{gamma g}((1 - gamma) x0): threshold 1/2
        if loss == "ls":
            self.b = rng.integers(-2, 3, Np).astype(F64)
        else:
            self.b = rng.choice([-1.0, 1.0], Np)
            self.x0[:] = 0
            self.z[:] = 0
        # LFinito: z_full = prox(av), b2 = A z_full - e (the module's docstring)
        self.zf = prox_l1(self.av, self.gl)
        e = rng.integers(-2, 3, Np).astype(F64) * (np.arange(Np) % 8 == 0)
        self.b2 = self.A @ self.zf - e
        self.pass_sum = None
        self.table0 = None                                       # the Finito table the batches start from: finito_init's at x0 (set lazily)

    def start_table(self):
        if self.table0 is None:
            self.table0 = finito_init(self, self.Np, Bounds())["table"]
        return self.table0


def prox_l1(v, gl):
    """prox_elem of csrc/ciao_common.h: v + (v <= -gl ? gl : (v >= gl ? -gl : -v))"""
    return v + np.where(v <= -gl, gl, np.where(v >= gl, -gl, -v))


# ---- the five modes, restated (float64; exact on the lattice) ------------------------------------------------------------------------------
def _s1(P, B, dots, b):
    """GradCoef::s1 (grad f_i = (a s1) s2, s2 = lam): the residual, or -y / (1 + exp(y a'x)) at a'x = 0"""
    if P.loss == "ls":
        return B.value("residual", dots - b)
    assert not dots.any(), "the logistic leg is exact at margin 0 only"
    return -b / 2.0


def grad(P, n, B, x=None):
    """SVRG_basic.jl:87-92 over rows [0, n): av = (1 / N) sum_i grad f_i(x), with the row dots the sweep caches for the SVRG chain and
    the objective that rides on it, obj = (1 / N) sum_i (lam / 2) (a_i'x - b_i)^2 (a double: (double)extra * (1.0 / N_total))"""
    x = P.x0 if x is None else x
    A, b = P.A[:n], P.b[:n]
    dots = B.total("row dots", A * x, 1)
    s1 = _s1(P, B, dots, b)
    S = B.total("GRAD sum", (s1 * P.lam)[:, None] * A, 0)
    out = {"dots": dots, "sum": S, "av": B.value("GRAD av", S / P.Nt)}
    if P.loss == "ls":
        f = B.total("objective", B.value("objective term", (P.lam / 2.0) * s1) * s1, 0)
        out["extra"], out["obj"] = f, f * (1.0 / P.Nt)
    return out


def saga_init(P, n, B):
    """SAGA_basic.jl:42-47: table_i = grad f_i(x0); av = (1 / N) sum_i table_i; z = prox_{gamma g}((1 - gamma) x0) (api_solvers.hip saga_init_t)"""
    A, b = P.A[:n], P.b[:n]
    s1 = _s1(P, B, B.total("row dots", A * P.x0, 1), b)
    table = (A * s1[:, None]) * P.lam
    S = B.total("SAGA_INIT sum", table, 0)
    z = prox_l1((1.0 - P.saga_gamma) * P.x0, P.saga_gamma * P.saga_lam_g)
    return {"table": table, "av": B.value("SAGA_INIT av", S / P.Nt), "z": z}


def finito_init(P, n, B):
    """Finito_basic.jl:77-83: table_i = x0 - (gam_i / N) grad f_i(x0); av = hat_gamma sum_i table_i / gam_i; z = prox_{hat_gamma g}(av)"""
    A, b, gam = P.A[:n], P.b[:n], P.gam[:n]
    s1 = _s1(P, B, B.total("row dots", A * P.x0, 1), b)
    table = B.value("FINITO_INIT table", P.x0 - (gam / P.Nt)[:, None] * ((A * s1[:, None]) * P.lam))
    S = B.total("FINITO_INIT sum", table * (1.0 / gam)[:, None], 0)
    av = B.value("FINITO_INIT av", P.hg * S)
    return {"table": table, "av": av, "z": prox_l1(av, P.hg * P.lam_g)}


def finito_batch(P, rows, B):
    """Finito_basic.jl:109-118 for one batch: t_i = z - (gam_i / N) grad f_i(z); av += sum_i (t_i - table_i) hat_gamma / gam_i;
    table_i = t_i; z = prox_{hat_gamma g}(av) -- from the table of finito_init at x0, P.z and P.av"""
    rows = np.asarray(rows, np.int64)
    A, b, gam = P.A[rows], P.b[rows], P.gam[rows]
    table = P.start_table().copy()
    s1 = _s1(P, B, B.total("row dots", A * P.z, 1), b)
    t = B.value("FINITO_BATCH table", P.z - (gam / P.Nt)[:, None] * ((A * s1[:, None]) * P.lam))
    S = B.total("FINITO_BATCH sum", B.value("FINITO_BATCH difference", t - table[rows]) * (P.hg / gam)[:, None], 0)
    av = B.value("FINITO_BATCH av", S + P.av)
    table[rows] = t
    return {"table": table, "av": av, "z": prox_l1(av, P.hg * P.lam_g), "extra": 0.0}


def lfinito_batch(P, rows, B):
    """Finito_LFinito.jl:83-98 with one batch (api_finito.hip lfinito_iterate_t): z_full = prox(av); the full pass av = z_full - (hat_gamma / N)
    sum_i grad f_i(z_full); z = prox(av); the batch av += (hat_gamma / N) sum_i (grad f_i(z_full) - grad f_i(z)) + (sum_i hat_gamma /
    gam_i) (z - z_full) -- on the problem with targets b2.  z stays the z the batch worked with (the reference's `solution`)."""
    rows = np.asarray(rows, np.int64)
    assert P.loss == "ls"
    zf = P.zf
    if P.pass_sum is None:                               # (the full pass is the same for every batch of the problem)
        d_full = B.total("row dots", P.A * zf, 1)
        P.pass_sum = B.total("GRAD sum", (B.value("residual", d_full - P.b2) * P.lam)[:, None] * P.A, 0)
    av1 = B.value("LFinito pass av", -(P.hg / P.Nt) * P.pass_sum + zf)
    z = prox_l1(av1, P.hg * P.lam_g)
    A, b, gam = P.A[rows], P.b2[rows], P.gam[rows]
    d1, d2 = B.total("row dots", A * zf, 1), B.total("row dots (z)", A * z, 1)
    c = B.value("GRAD2 coefficient", P.lam * B.value("residual", d1 - b) - P.lam * B.value("residual (z)", d2 - b))
    S2 = B.total("GRAD2 sum", c[:, None] * A, 0)
    extra = B.total("GRAD2 extra", P.hg / gam, 0)
    a = B.value("GRAD2 av", (P.hg / P.Nt) * S2)
    a = B.value("GRAD2 av", a + av1)
    a = B.value("GRAD2 av", a + B.value("GRAD2 av", extra * z))
    a = B.value("GRAD2 av", a + B.value("GRAD2 av", -extra * zf))
    return {"av": a, "z": z, "zf": zf, "extra": extra}


def batch_rows(P, n, lists, seed=0):
    """the n rows of a batch: a row block off row 0, or an index list -- distinct, unsorted, from all Np rows"""
    if not lists:
        return np.arange(ROW0, ROW0 + n, dtype=np.int64)
    return np.random.default_rng(1000 + seed + n).permutation(P.Np)[:n].astype(np.int64)


def reference(P, mode, n, B):
    if mode == "grad":
        return grad(P, n, B)
    if mode == "saga_init":
        return saga_init(P, n, B)
    if mode == "finito_init":
        return finito_init(P, n, B)
    rows = batch_rows(P, n, mode.endswith("lists"))
    return finito_batch(P, rows, B) if mode.startswith("finito") else lfinito_batch(P, rows, B)


# ---- the classifier: a launch report -> its workers' trip counts and its partial count ---------------------------------------------------------
# One line per kernel, read from its row loop:
#   rows_split_kernel    workgroup b takes rows b, b + grid, ...                          (for q = blockIdx.x; q < nrows; q += gridDim.x)
#   rows_fast_kernel     wave w = 4 block + wave-in-block takes rows w, w + 4 grid, ...   (both flavours: q += nwaves)
#   rows_generic_kernel  the same with NW waves a workgroup; ,global_acc: a partial per WAVE
#   rows_wrow_kernel     the same with block / 64 waves a workgroup, two rows in flight
#   rows_multi_kernel    wave w takes the groups of R consecutive rows w, w + 4 grid, ... (R = 4 at K2, 2 at K4)
#   rows_small_kernel, rows_smallb_kernel   wave w takes the groups of G = min(64, 64 I / d) consecutive rows w, w + 4 grid, ...
#   rows_smallm_kernel   wave w takes the tiles of 16 rows w, w + 4 grid, ...
#   rows_long_kernel     cluster c takes rows c, c + C, ...: one partial per cluster
FAMILY = re.compile(r"^rows_(fast|multi|split|small|smallm|smallb|wrow|generic|long)_kernel<")


def classify(report, n, d):
    """-> dict(family, grid, workers, unit (rows a trip takes), trips (sorted per-worker trip counts), parts, short (rows of a short
    last unit, 0: none))"""
    m = FAMILY.match(report)
    assert m, report
    fam = m.group(1)
    grid = int(re.search(r"grid=(\d+)", report).group(1))
    block = int(re.search(r"block=(\d+)", report).group(1))
    unit, per_block, parts = 1, block // 64, grid
    if fam == "split":
        per_block = 1
    elif fam == "multi":
        unit = {2: 4, 4: 2}[int(re.search(r",K(\d+),", report).group(1))]
    elif fam in ("small", "smallb"):
        unit = min(64, 64 * int(re.search(r",I(\d+)", report).group(1)) // d)
    elif fam == "smallm":
        unit = 16
    elif fam == "generic":
        per_block = int(re.search(r",NW(\d),", report).group(1))
        assert per_block == block // 64
        if ",global_acc" in report:
            parts = grid * per_block
    workers = grid * per_block
    if fam == "long":
        workers = parts = int(re.search(r"clusters=(\d+)", report).group(1))
        assert grid == workers * int(re.search(r"segments=(\d+)", report).group(1))
    units = -(-n // unit)
    trips = sorted(max(0, -(-(units - w) // workers)) for w in range(workers))
    return {"family": fam, "grid": grid, "workers": workers, "unit": unit, "trips": trips, "parts": parts, "short": n % unit}


def classes(c):
    """the trip classes one launch reaches"""
    t, out = set(c["trips"]), set()
    if 0 in t:
        out.add("an idle worker")
    for k in (1, 2, 3):
        if k in t:
            out.add(f"{k} trip{'s' if k > 1 else ''}")
    if max(t) >= 5:
        out.add(">= 5 trips")
    if len(t - {0}) >= 2:
        out.add("two trip counts in one launch")
    if c["short"]:
        out.add("a short last unit")
    return out


def required(c):
    """what a family's launches must reach together.  rows_split_kernel, the one-wave generic kernel and rows_long_kernel have no idle
    worker: their plans give min(rows, ...) workgroups or clusters of one worker each"""
    need = {"1 trip", "2 trips", "3 trips", ">= 5 trips", "two trip counts in one launch"}
    if c["workers"] > c["grid"] and c["family"] != "long":
        need.add("an idle worker")
    if c["unit"] > 1:
        need.add("a short last unit")
    return need


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
# family regular expressions of tests/test_gpu_layouts.py
FAST = r"^rows_fast_kernel<"
MULTI = r"^rows_multi_kernel<"
EXACT = r"^rows_split_kernel<\w+,J\d+,mode\d> "
MASKED = r"^rows_split_kernel<\w+,J\d+,mode\d,masked> "
SCALAR = r"^rows_split_kernel<\w+,J\d+,mode\d,scalar> "
SMALL = r"^rows_small_kernel<"
SMALLM = r"^rows_smallm_kernel<"
DENSE = r"^rows_smallb_kernel<\w+,mode\d,I8,dense> "
GATHER = r"^rows_smallb_kernel<\w+,mode\d,I8,gather> "
WCH = r"^rows_wrow_kernel<\w+,chunks,K1,"
WEL = r"^rows_wrow_kernel<\w+,elements,K\d,"
LONG8 = r"^rows_long_kernel<\w+,J8,"
LONG4 = r"^rows_long_kernel<\w+,J4,"
GEN4 = r"^rows_generic_kernel<\w+,NW4,mode\d> "
GEN1 = r"^rows_generic_kernel<\w+,NW1,mode\d> "
GENG = r"^rows_generic_kernel<\w+,NW4,mode\d,global_acc> "

OPTION_DEFAULTS = {"sweep_grid": 0, "sweep_blocks_per_cu": 0, "wrow_rows_per_wave": 0, "sweep_multi": 1, "small_mfma": -1, "small_wrow": -1,
                   "force_generic": 0, "split_max_rows": -1, "split_blocks_per_cu": 0, "long_j": 0, "chain_max_batch": -1}


def T2(f64, f32):
    return {F64: f64, F32: f32}


def every(f, modes=MODES):
    return {m: f for m in modes}


class Case:
    """name; d as a function of VEC; library options; {mode: family regular expression} (a dict by type where the two differ); `pad`:
    the family takes rows at a padded stride (and {mode: family} there, where the plan differs); `kind`: how its workers are counted
    (classify); wpb: waves of a workgroup by type (host side; the device test reads block= from the report and asserts it is this)"""

    def __init__(self, name, d, modes, kind, opts=None, pad=True, pad_modes=None, wpb=4, logistic=False):
        self.name, self._d, self.modes, self.kind, self.opts, self.pad = name, d, modes, kind, dict(opts or {}), pad
        self.pad_modes, self._wpb, self.logistic = pad_modes, wpb, logistic

    def d(self, dtype):
        return self._d(vec_of(dtype)) if callable(self._d) else self._d[dtype] if isinstance(self._d, dict) else self._d

    def family(self, mode, dtype, padded=False):
        f = (self.pad_modes if padded and self.pad_modes else self.modes)[mode]
        return f[dtype] if isinstance(f, dict) else f

    def wpb(self, dtype):
        return self._wpb[dtype] if isinstance(self._wpb, dict) else self._wpb

    def long_clusters(self, dtype, num_cu):
        """rowsl_launch.inc long_plan with split_blocks_per_cu = 1: num_cu / S clusters at most"""
        J = self.opts["long_j"]
        S = -(-(self.d(dtype) // vec_of(dtype)) // (J * 256))
        return num_cu // S

    def launches(self, dtype, num_cu):
        """[(rows n, sweep_grid)]: sweep_grid 0 is the plan's own grid.  With sweep_grid g the plan gives min(its own grid, g), and its
        own grid is at least g for the n below on any chip of three CUs and more -- so these launches' trip counts do not depend on the
        CU count; rows_long_kernel takes no sweep_grid and its n are sized from the CU count."""
        if self.kind == "long":
            C = self.long_clusters(dtype, num_cu)
            return [(4, 0), (C + 1, 0), (2 * C + 2, 0), (5 * C + 1, 0)]        # (batches of up to 3 such rows run as a chain: api_finito.hip)
        W1, U = (1 if self.kind == "split" else self.wpb(dtype)), self.unit(dtype)
        rows = lambda units: units * U - (U - 1 if U > 1 else 0)           # a last unit of ONE row where units hold several
        out = []
        if W1 > 1:
            out.append(((W1 - 1) * U, 1))                                      # an idle worker beside workers of one trip
        out += [(rows(5 * W1 + 1), 1),                                         # 6 and 5 trips
                (rows(4 * W1 + max(1, W1 // 2)), 2),                           # 3 and 2
                (rows(3 * W1 + 1), 3),                                         # 2 and 1
                (rows(6 * W1 + 1), 0)]                                         # the plan's own grid
        return out

    def report(self, dtype, n, grid, num_cu):
        """the launch report the host expects of (n, grid), in rows_kernel_name's form: what classify() reads, so that the row-to-worker
        maps are stated there alone"""
        d, v = self.d(dtype), vec_of(dtype)
        if self.kind == "long":
            S = -(-(d // v) // (self.opts["long_j"] * 256))
            C = min(n, self.long_clusters(dtype, num_cu))
            return f"rows_long_kernel<t,J{self.opts['long_j']},mode0> segments={S} clusters={C} grid={S * C} block=256"
        if self.kind == "split":
            return f"rows_split_kernel<t,J1,mode0> grid={grid} block=256"
        wpb = self.wpb(dtype)
        what = {"multi": f"K{d // v // 64},mode0", "small": f"mode0,I{8 if dtype == F32 or d <= 8 else 16}", "smallb": "mode0,I8,dense",
                "generic": f"NW{wpb},mode0"}.get(self.kind, "mode0")
        return f"rows_{self.kind}_kernel<t,{what}> grid={grid} block={64 * wpb}"

    def unit(self, dtype):
        """rows a trip takes (the device test holds every report's to it)"""
        return classify(self.report(dtype, 1, 1, 256), 1, self.d(dtype))["unit"]

    def forced(self, dtype, num_cu):
        """(n, classification) of the launches whose grid the host knows"""
        return [(n, classify(self.report(dtype, n, g, num_cu), n, self.d(dtype))) for n, g in self.launches(dtype, num_cu)
                if g or self.kind == "long"]

    def rows_needed(self, dtype, num_cu):
        return max(n for n, _ in self.launches(dtype, num_cu)) + ROW0

    def problem(self, dtype, num_cu, loss="ls"):
        return Problem(self.rows_needed(dtype, num_cu), self.d(dtype), seed=len(self.name) + self.d(dtype) + (loss != "ls"), loss=loss)


def wrow_waves(dtype, by_chunks):
    """rowsw_kernels.h WrowWaves<sizeof(T), VEC, 1>::block_waves"""
    es = np.dtype(dtype).itemsize
    budget = 6 * ((vec_of(dtype) if by_chunks else 1) * es // 4) + (56 if es == 8 else 40)
    return 2 * max(1, min(8, 512 // ((budget + 7) // 8 * 8)))


_B4 = ("finito_lists", "finito_blocks", "lfinito_lists", "lfinito_blocks")
_G2 = ("grad", "lfinito_lists", "lfinito_blocks")
_LISTS = {"finito_lists": GATHER, "lfinito_lists": GATHER}
CASES = [
    Case("fast_k1", lambda v: 64 * v, every(FAST), "fast", logistic=True),
    Case("fast_k8", lambda v: 512 * v, every(FAST, SWEEPS), "fast"),
    Case("fast_k16", lambda v: 1024 * v, every(FAST, SWEEPS), "fast"),
    Case("fast_k2_prefetch", lambda v: 128 * v, every(FAST), "fast", opts={"sweep_multi": 0}),
    Case("multi_k2", lambda v: 128 * v, every(MULTI, _G2), "multi", logistic=True),
    Case("multi_k4", lambda v: 256 * v, every(MULTI, _G2), "multi", opts={"split_max_rows": 0}),
    Case("split_exact_j1", lambda v: 256 * v, every(EXACT, _B4), "split", logistic=True),
    Case("split_masked_150", lambda v: 150 * v, every(MASKED), "split", logistic=True),
    Case("split_masked_987", lambda v: (4 * 256 - 37) * v, every(MASKED), "split"),
    Case("split_scalar_257", 257, every(SCALAR), "split", logistic=True),
    Case("small_d5", 5, every(SMALL, SWEEPS), "small", logistic=True),
    Case("small_d50", 50, every(SMALL, SWEEPS), "small", opts={"small_mfma": 0}),
    Case("smallm_d50", 50, every(SMALLM, SWEEPS + ("finito_blocks", "lfinito_blocks")), "smallm", opts={"small_wrow": 0}, pad=False, logistic=True),
    Case("smallb_d50", 50, {**_LISTS, "finito_blocks": DENSE, "lfinito_blocks": DENSE}, "smallb", opts={"small_wrow": 0, "small_mfma": 0},
         pad_modes=every(GATHER, _B4), logistic=True),
    Case("wrow_d52", 52, every(WCH, _B4), "wrow", wpb=T2(wrow_waves(F64, True), wrow_waves(F32, True)), logistic=True),
    Case("wrow_d50", 50, every(T2(WCH, WEL), _B4), "wrow", wpb=T2(wrow_waves(F64, True), wrow_waves(F32, False))),
    Case("wrow_d50_one_row_per_wave", 50, every(T2(WCH, WEL), _B4), "wrow", opts={"wrow_rows_per_wave": 1},
         wpb=T2(wrow_waves(F64, True), wrow_waves(F32, False))),
    Case("generic_nw4_257", 257, every(GEN4), "generic", opts={"force_generic": 1}, logistic=True),
    # one wave a workgroup: five d-vectors do not fit 144 KiB of LDS, two (three in GRAD2) do
    Case("generic_nw1", lambda v: 2049 * v + 1, every(GEN1, SWEEPS + ("lfinito_lists",)), "generic", opts={"force_generic": 1}, wpb=1),
    # accumulators in global memory: the smallest d whose two d-vectors exceed 144 KiB (nothing else takes an odd d beyond 4096)
    Case("generic_global_acc", T2(9217, 18433), every(GENG, SWEEPS), "generic"),
    Case("long_j8", lambda v: (16 * 256 + 8) * v, every(LONG8), "long", opts={"long_j": 8, "split_blocks_per_cu": 1}, logistic=True),
    Case("long_j4", lambda v: (16 * 256 + 8) * v, every(LONG4), "long", opts={"long_j": 4, "split_blocks_per_cu": 1}, logistic=True),
]
CASE_BY_NAME = {c.name: c for c in CASES}

# ---- finalize_kernel alone ----------------------------------------------------------------------------------------------------------------
# the two widths (256 threads up to 256 partials, 1024 beyond), rounds of 256 / 1024 partials (8 loads x 32 / 128 slices), the slices
# themselves, the 64-lane sum of the extra scalar
PARTIAL_COUNTS = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
FINALIZE_ROWS = 16400                                   # 1025 x 16: one row per wave on 1025 workgroups of rows_fast_kernel; beyond 16 384, where rows_split_kernel takes several workgroups per CU
FINALIZE_SHAPES = (("fast_k1", lambda v: 64 * v, FAST, {"sweep_blocks_per_cu": 8}), ("split_scalar_257", lambda v: 257, SCALAR, {}))


def finalize_problem(d):
    return Problem(FINALIZE_ROWS, d, seed=7 + d)

"""Rows beyond 2^31 and 2^32 elements: a zero matrix with a few marked rows.

A far row does not need a full matrix, it needs a mostly zero one.  In a device matrix that is zero except for K <= 16 marked rows, with
b = 0 on the zero rows, every zero row adds exactly +0 to a LeastSquares gradient, to a table row, to a square, a moment or a Gram term,
and (-y/2) 0 = 0 to a logistic gradient.  The exact reference of a pass over 4 10^9 elements is then the oracle, or an int64 / float64
numpy restatement, on the K gathered rows with N_total = N (oracle.Problem(..., N_total=)): microseconds on the host.  A kernel that
forms row * ld, b[row], out[row] or an in-tile offset in 32 bits reads a low row instead of the far one: the far row's share goes
missing, a low marked row (other values) is counted twice, row-wise outputs land in the wrong place -- each an O(1) change.

This module is plain (no test, no conftest): the views, the boundaries and marked rows of a view, the integer fill, `gathered`, the
references of every operation tests/test_gpu_far_rows.py runs (tests/test_far_rows_host.py holds them to the oracle on small dense
problems and shows that each notices a dropped or an aliased row), and the device-side checks for outputs too large to copy."""
import numpy as np

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
# one zeroed 1-D device buffer per type, 17.4 GB each: fp32 crosses byte 2^31, byte 2^32, element 2^31 and element 2^32; fp64 crosses
# byte 2^31 .. 2^34 and element 2^31.  fp64 past element 2^32 would take 34 GB and a table of the same size: left out
ELEMS = {F32: 2 ** 32 + 2 ** 26, F64: 2 ** 31 + 2 ** 25}
MAX_MARKED = 16
CHUNK = 2 ** 24                       # elements per device-side check step (the framework's count makes an int64 per element: 0.13 GB)
EPS = {F64: float(np.finfo(np.float64).eps), F32: float(np.finfo(np.float32).eps)}


def tname(dtype):
    return "f64" if np.dtype(dtype) == F64 else "f32"


# ---- views ----------------------------------------------------------------------------------------------------------------------------
class View:
    """N rows of d elements at stride ld inside the buffer of `dtype`; complex: the rows are d / 2 (re, im) pairs"""

    def __init__(self, name, dtype, N, d, ld, complex=False):
        self.name, self.dtype, self.N, self.d, self.ld, self.complex = name, np.dtype(dtype), int(N), int(d), int(ld), complex
        self.es = self.dtype.itemsize
        assert self.ld >= self.d and self.N >= 3 and self.span <= ELEMS[self.dtype], (name, self.span)

    @property
    def span(self):
        return (self.N - 1) * self.ld + self.d

    @property
    def id(self):
        return f"{tname(self.dtype)}-{self.name}"

    def __repr__(self):
        return f"View({self.id}: N={self.N}, d={self.d}, ld={self.ld})"


def dense(dtype, d, complex=False):
    return View(("c" if complex else "d") + str(d), dtype, ELEMS[np.dtype(dtype)] // d, d, d, complex)


def strided(dtype, N, d, odd=False):
    """few rows, huge stride: ld = floor(E / N) rounded down to a 16-byte multiple (odd: to an odd number of elements)"""
    es = np.dtype(dtype).itemsize
    ld = ELEMS[np.dtype(dtype)] // N
    ld -= ld % (16 // es)
    if odd:
        ld -= 1
    return View(f"s{N}x{d}" + ("odd" if odd else ""), dtype, N, d, ld)


def guard_rows(dtype):
    """the rows of the ld < 2^24 guard: N = 200, as many of them as the buffer of the type holds at ld = 2^24 (fp64: 131)"""
    return min(200, (ELEMS[np.dtype(dtype)] - 50) // 2 ** 24 + 1)


def guard(dtype, at):
    """d = 50 on either side of the bound that keeps rows_small_kernel's in-group offsets in 32 bits"""
    return View("guard-at" if at else "guard-below", dtype, guard_rows(dtype), 50, 2 ** 24 if at else 2 ** 24 - 4)


LONG_D = {F32: 16388, F64: 8194}


def views(dtype):
    """every view of tests/test_gpu_far_rows.py for one type, by name"""
    dtype = np.dtype(dtype)
    vs = [dense(dtype, 2)] if dtype == F32 else []     # N > 2^31 rows: the row index itself (first: before the second buffer exists)
    vs += [dense(dtype, 1024), dense(dtype, 1000), dense(dtype, 50), dense(dtype, LONG_D[dtype]), dense(dtype, 8193),
           dense(dtype, 1024, complex=True)]
    vs += [strided(dtype, N, d) for N in (5, 65) for d in (50, 1000, 1024)]
    vs += [strided(dtype, 65, 1000, odd=True), guard(dtype, False), guard(dtype, True)]
    return {v.name: v for v in vs}


ALL_VIEWS = [v for dt in (F32, F64) for v in views(dt).values()]


# ---- boundaries and marked rows ---------------------------------------------------------------------------------------------------------
def boundaries(view):
    """[(name, B in elements)] of the boundaries the view reaches: some row starts at or after B"""
    cand = [("byte 2^31", 2 ** 31 // view.es), ("byte 2^32", 2 ** 32 // view.es), ("element 2^31", 2 ** 31), ("element 2^32", 2 ** 32)]
    return [(n, B) for n, B in cand if -(-B // view.ld) <= view.N - 1]


def rows_at(view, B):
    """(last row ending at or below B, the row straddling B or None, first row starting at or after B)"""
    below = (B - view.d) // view.ld
    r = B // view.ld
    straddle = r if (B % view.ld != 0 and B % view.ld < view.d) else None
    after = -(-B // view.ld)
    assert 0 <= below < after <= view.N - 1 and below * view.ld + view.d <= B <= after * view.ld
    assert straddle is None or (below < straddle < after and straddle * view.ld < B < straddle * view.ld + view.d)
    return below, straddle, after


def marked_rows(view):
    """sorted int64: rows 0, 1, N - 1 and three rows around every reached boundary"""
    rows = {0, 1, view.N - 1}
    for _, B in boundaries(view):
        rows |= {r for r in rows_at(view, B) if r is not None}
    rows = np.array(sorted(rows), dtype=np.int64)
    assert len(rows) <= MAX_MARKED and rows[0] == 0 and rows[-1] == view.N - 1
    return rows


def peak_row(view):
    """the marked row with the largest values (the argmax of the row norms): the first row at or after the highest boundary reached"""
    bs = boundaries(view)
    return rows_at(view, bs[-1][1])[2] if bs else view.N - 1


# ---- the integer fill ---------------------------------------------------------------------------------------------------------------------
def columns(view):
    d = view.d
    return sorted({0, d - 1} | {(m * d) // 5 for m in range(1, 5)} | {d // 2, (2 * d) // 3})


def x_vector(d, dtype, k=0):
    """small nonzero integers (k: another one per model)"""
    v = np.array([1, -2, 3, -1, 2, -3, 4, -4])
    return v[(np.arange(d) * (2 * k + 1) + 3 * k) % 8].astype(dtype)


class Data:
    """the gathered rows of a view: rows (K) int64 ascending, A (K, d), b (K) targets, y (K) labels, all small integers in `dtype`;
    zero[k]: row k is not marked (a zero row some batch visits)"""

    def __init__(self, view, rows, A, b, y, zero):
        self.view, self.rows, self.A, self.b, self.y, self.zero = view, rows, A, b, y, zero
        self.index = {int(r): k for k, r in enumerate(rows)}

    @property
    def K(self):
        return len(self.rows)

    def targets(self, loss):
        return self.y if loss == "logistic" else self.b

    def astype(self, dtype):
        return Data(self.view, self.rows, self.A.astype(dtype), self.b.astype(dtype), self.y.astype(dtype), self.zero)

    def copy(self):
        return Data(self.view, self.rows.copy(), self.A.copy(), self.b.copy(), self.y.copy(), self.zero.copy())

    def local(self, rows):
        return np.array([self.index[int(r)] for r in np.asarray(rows).ravel()], dtype=np.int64).reshape(np.shape(rows))


_FILL = {}


def fill(view, extra=(), marked=None):
    """Data of the marked rows (and of the zero rows `extra`): |a| <= 3, on the peak row 4, nonzero in column 0, column d - 1 and a few
    columns between, distinct per row; b a nonzero integer, y = +-1 in turn.  Drawn again until every row's dot with x and its residual
    are nonzero and no two rows agree (a seeded search, the same data every run)."""
    key = (view.id, view.N, view.ld, tuple(int(e) for e in extra), None if marked is None else tuple(int(m) for m in marked))
    if key in _FILL:
        return _FILL[key].copy()
    marked = marked_rows(view) if marked is None else np.array(sorted(marked), np.int64)
    cols, x = columns(view), x_vector(view.d, np.int64)
    rng = np.random.default_rng(view.N % 1000003 + view.d)
    peak = peak_row(view) if view.N - 1 in marked else int(marked[-1])
    vals = np.array([-3, -2, -1, 1, 2, 3])
    for _ in range(1000):
        A = np.zeros((len(marked), view.d), np.int64)
        for k, r in enumerate(marked):
            A[k, cols] = 4 * rng.choice([-1, 1], len(cols)) if r == peak else rng.choice(vals, len(cols))
        b = rng.choice(vals, len(marked))
        dots = A @ x
        if len({a.tobytes() for a in A}) == len(marked) and np.all(dots != 0) and np.all(dots != b) and len(set(dots.tolist())) == len(marked):
            break
    else:
        raise AssertionError(f"no fill for {view}")
    if view.complex:
        b = np.concatenate([b[:, None], rng.choice(vals, (len(marked), 1))], axis=1)     # (re, im) of every target
    y = np.where(np.arange(len(marked)) % 2 == 0, 1, -1)
    rows = np.array(sorted(set(marked.tolist()) | {int(e) for e in extra}), dtype=np.int64)
    assert rows[-1] <= view.N - 1
    pos = np.searchsorted(rows, marked)
    fA = np.zeros((len(rows), view.d), np.int64)
    fb = np.zeros((len(rows),) + b.shape[1:], np.int64)
    fy = np.ones(len(rows), np.int64)
    zero = np.ones(len(rows), bool)
    fA[pos], fb[pos], fy[pos], zero[pos] = A, b, y, False
    _FILL[key] = Data(view, rows, fA, fb, fy, zero).astype(view.dtype)
    return _FILL[key].copy()


def gathered(view, loss="ls", lam=1.0, data=None):
    """(oracle Problem on the gathered rows with N_total = N, {row: its index among them})"""
    from oracle import twin as O
    data = fill(view) if data is None else data
    t = data.targets(loss)
    return O.Problem("ls_complex" if view.complex else loss, data.A, t.reshape(-1), lam, N_total=view.N), data.index


def window(view, data, off):
    """the d elements of the flat buffer from element `off` on: what a kernel reads that starts a row there"""
    out = np.zeros(view.d, data.A.dtype)
    for k, r in enumerate(data.rows):
        lo = int(r) * view.ld - off                    # where row r's first element falls in the window
        if -view.d < lo < view.d:
            s0, s1 = max(0, -lo), min(view.d, view.d - lo)
            out[lo + s0:lo + s1] = data.A[k, s0:s1]
    return out


def mutants(view, data):
    """[(what, Data)]: each marked row dropped (read as zeros); each far marked row replaced by what its offset reaches modulo 2^32
    bytes, 2^31 and 2^32 elements (the row's data, its target and label through the row index modulo 2^31 and 2^32)"""
    out = []
    full = {int(r): k for k, r in enumerate(data.rows)}
    for k, r in enumerate(data.rows):
        if data.zero[k]:
            continue
        m = data.copy()
        m.A[k], m.b[k], m.y[k] = 0, 0, 1
        out.append((f"row {r} dropped", m))
        off = int(r) * view.ld
        for what, M in (("2^32 bytes", 2 ** 32 // view.es), ("2^31 elements", 2 ** 31), ("2^32 elements", 2 ** 32)):
            if off < M:
                continue
            m = data.copy()
            m.A[k] = window(view, data, off % M)
            if r >= 2 ** 31:                           # the row index itself: b[row], y[row] wrap with it
                j = full.get(int(r) % (2 ** 31 if M == 2 ** 31 else 2 ** 32))
                m.b[k], m.y[k] = (data.b[j], data.y[j]) if j is not None else (0, 1)
            out.append((f"row {r} read modulo {what}", m))
    return out


# ---- references: the oracle on the gathered rows, or a numpy restatement of it ------------------------------------------------------------
# Every function takes the Data (of the run's type, or its float64 copy for close()'s Float64 form) and returns {name: array}.
def _O():
    from oracle import twin as O
    return O


def _problem(data, loss, lam):
    return gathered(data.view, loss, lam, data)[0]


def _grad(op, data, loss, lam, k, x):
    O = _O()
    t = data.targets(loss)
    return O.gradient(op.loss, data.A[k], t[k], lam, x)[0]


def prox_of(kind, dtype, lam=2.0 ** -6):
    O = _O()
    return O.Prox("zero") if kind == "zero" else O.Prox("l1", lam=lam)


def ref_sweep(data, loss, lam=1.0):
    """full_gradient (shard_pass: the rows held, divided by N_total), the row dots, the LeastSquares objective"""
    O = _O()
    T, N = data.A.dtype.type, data.view.N
    op = _problem(data, loss, lam)
    x = x_vector(data.view.d, T)
    out = {"av": O.shard_pass(op, x, np.zeros(data.view.d, T))}
    if not data.view.complex:
        dots = data.A.astype(np.float64) @ x.astype(np.float64)
        out["dots"] = dots.astype(T)
        if loss == "ls":
            out["objective"] = np.array([0.5 * lam * float(np.sum((dots - data.b.astype(np.float64)) ** 2)) / N])
    return out


def chain_steps(data, n=40):
    """about 40 visits of marked rows only, in a fixed shuffled order, a sample repeated inside the prefetch window"""
    marked = data.rows[~data.zero]
    rng = np.random.default_rng(len(marked))
    idx = np.concatenate([rng.permutation(marked) for _ in range(-(-n // len(marked)))])[:n].astype(np.int64)
    idx[5:8] = idx[5]
    idx[10] = idx[8]
    idx[-1] = marked[-1]
    return idx


def chain_state(d, T):
    """(z_full, w, av): small integers and dyadic fractions, w apart from z_full so that a step depends on its row by O(1)"""
    zf = x_vector(d, T)
    w = (zf + x_vector(d, T, 1) / T(4)).astype(T)
    av = (x_vector(d, T, 2) / T(16)).astype(T)
    return zf, w, av


def chain_gamma(loss):
    return 2.0 ** -7 if loss == "ls" else 0.25


def ref_svrg(data, loss, lam=1.0):
    O = _O()
    T, d = data.A.dtype.type, data.view.d
    op, g = _problem(data, loss, lam), prox_of("l1", T)
    zf, w, av = chain_state(d, T)
    z = np.zeros(d, T)
    O.svrg_inner(op, g, T(chain_gamma(loss)), data.local(chain_steps(data)), av, z, zf, w)
    return {"w": w, "z": z}


def ref_svrg_epoch(data, loss, lam=1.0):
    """svrg_init then ONE svrg_iterate over marked rows (SVRG_basic.jl:57-96): the full pass at x, the inner cycle from w = z_full = x, the
    tail z_full = z / m, w = z_full, and the full pass at the new z_full -- each pass the rows held, divided by N_total.  The device runs
    it with reuse_rowdots: the inner cycle then takes a_i'z_full from the N-vector the first pass left, read at the far rows"""
    O = _O()
    T, d = data.A.dtype.type, data.view.d
    op, g = _problem(data, loss, lam), prox_of("l1", T)
    x = x_vector(d, T)
    av = O.shard_pass(op, x, np.zeros(d, T))
    z, zf, w = np.zeros(d, T), x.copy(), x.copy()
    idx = data.local(chain_steps(data))
    O.svrg_inner(op, g, T(chain_gamma(loss)), idx, av, z, zf, w)
    zf = (z / T(len(idx))).astype(T)
    return {"epoch z_full": zf, "epoch w": zf.copy(), "epoch av": O.shard_pass(op, zf, np.zeros(d, T))}


def saga_init_restated(data, loss, lam, g, gamma, x0):
    """SAGA_basic.jl:41-48 on the gathered rows: the other rows of the table are exactly zero and add nothing to av"""
    O = _O()
    T, N = data.A.dtype.type, data.view.N
    op = _problem(data, loss, lam)
    table = np.stack([_grad(op, data, loss, lam, k, x0) for k in range(data.K)])
    av = (table.sum(axis=0, dtype=T) / T(N)).astype(T)
    z = O.prox(g, ((T(1) - T(gamma)) * x0).astype(T), T(gamma))
    return op, table, av, z


def ref_saga(data, loss, lam=1.0):
    """saga_init, then the chain with SAG off and on, each from the init state"""
    O = _O()
    T, d = data.A.dtype.type, data.view.d
    g, gamma, x0 = prox_of("l1", T), chain_gamma(loss), x_vector(d, T)
    op, table, av, z = saga_init_restated(data, loss, lam, g, gamma, x0)
    out = {"init table": table.copy(), "init av": av.copy(), "init z": z.copy()}
    idx = data.local(chain_steps(data))
    for sag in (False, True):
        t, a, zz = table.copy(), av.copy(), z.copy()
        O.saga_steps(op, g, T(gamma), sag, idx, t, a, zz)
        out.update({f"sag{int(sag)} table": t, f"sag{int(sag)} av": a, f"sag{int(sag)} z": zz})
    return out


FINITO_PROX = "zero"                  # hat_gamma is of the size of N: an l1 threshold lam * hat_gamma would clip every iterate to zero


def finito_gam(view):
    """one stepsize for every sample, gamma / N = 2^-7; hat_gamma = gamma / 16 is what the CALLER says (the kernels take both as given): a
    step then depends on its row by O(1) in the table, in av and in z, and the weights hat_gamma / gamma_i of the K <= 15 samples
    visited stay below 1 in sum, so the iterates do not grow"""
    gam = view.N * 2.0 ** -7
    return gam, gam / 16


def finito_init_restated(data, loss, lam, g, x0, params=None):
    """Finito_basic.jl:76-84 on the gathered rows; the other rows of the table are exactly x0, and av = hat_gamma sum_i s_i / gamma_i counts
    them (in float64: the N - K equal terms as one product)"""
    O = _O()
    T, N = data.A.dtype.type, data.view.N
    gam, hg = (T(v) for v in (finito_gam(data.view) if params is None else params))
    op = _problem(data, loss, lam)
    c = T(gam / T(N))
    table = np.stack([(x0 - c * _grad(op, data, loss, lam, k, x0)).astype(T) for k in range(data.K)])
    s = (table.astype(np.float64).sum(axis=0) + float(N - data.K) * x0.astype(np.float64)) / float(gam)
    av = (float(hg) * s).astype(T)
    return op, table, av, O.prox(g, av, hg)


def finito_batches(data, r):
    """batches of r marked rows each (index lists), every marked row met, the second batch again as the last"""
    marked = data.rows[~data.zero]
    rng = np.random.default_rng(r)
    order = np.concatenate([rng.permutation(marked), rng.permutation(marked)])
    bs = [order[i:i + r] for i in range(0, len(order) - r + 1, r)]
    return bs + [bs[1].copy()]


def block_rows(view, length=3):
    """(first, length) of row blocks that start at far marked rows (and at row 0), inside the matrix"""
    first = [int(r) for r in marked_rows(view) if r + length <= view.N and (r == 0 or r * view.ld >= 2 ** 31 // view.es)]
    first = [f for i, f in enumerate(first) if i == 0 or f >= first[i - 1] + length]      # disjoint
    return np.array(first, np.int64), np.full(len(first), length, np.int64)


def block_extra(view):
    f, n = block_rows(view)
    return sorted({int(a) + j for a, m in zip(f, n) for j in range(int(m))})


def finito_state(data, T):
    """a Finito state of small integers and dyadic fractions for the step tests: (table rows of the gathered rows, av, z)"""
    d = data.view.d
    table = np.stack([(x_vector(d, T, 3 + k) / T(2)) * (~data.zero[k]) for k in range(data.K)]).astype(T)
    return table, (x_vector(d, T, 1) / T(4)).astype(T), x_vector(d, T)


def ref_finito(data, loss, lam=1.0):
    """finito_init; finito_steps over index lists of marked rows (r = 1, 3) and over row blocks that start at far rows, from a state of
    small numbers whose other table rows are zero"""
    O = _O()
    T, d = data.A.dtype.type, data.view.d
    g, x0 = prox_of(FINITO_PROX, T), x_vector(d, T)
    op, table, av, z = finito_init_restated(data, loss, lam, g, x0)
    out = {"init table": table, "init av": av, "init z": z}
    gam, hg = (T(v) for v in finito_gam(data.view))
    gv = np.full(data.K, gam, T)
    runs = [(f"lists r={r}", [data.local(b) for b in finito_batches(data, r)]) for r in (1, 3)]
    f, n = block_rows(data.view)
    if set(block_extra(data.view)) <= set(data.index):
        runs.append(("blocks", [data.local(np.arange(a, a + m)) for a, m in zip(f, n)]))
    for name, batches in runs:
        t, a, zz = finito_state(data, T)
        O.finito_steps(op, g, gv, hg, batches, t, a, zz)
        out.update({f"{name} table": t, f"{name} av": a, f"{name} z": zz})
    return out


def lfinito_params(view):
    """hat_gamma / N = 2^-7 and hat_gamma / gamma_i = 1 / 16: as finito_gam, what the caller says"""
    hg = view.N * 2.0 ** -7
    return hg * 16, hg


def ref_lfinito(data, loss, lam=1.0, params=None, blocks=None):
    """Finito_LFinito.jl:66-72 and one :82-100 restated on the gathered rows (the oracle's own full pass runs over all N rows): a zero row
    adds c * 0 to the pass, and r (z - z_full) where a batch visits it"""
    O = _O()
    T, d, N = data.A.dtype.type, data.view.d, data.view.N
    g, x0 = prox_of(FINITO_PROX, T), x_vector(d, T)
    gam, hg = (T(v) for v in (lfinito_params(data.view) if params is None else params))
    op = _problem(data, loss, lam)
    c = T(hg / T(N))
    av = x0.copy()
    for k in range(data.K):
        av -= _grad(op, data, loss, lam, k, x0) * c
    out = {"init av": av.copy()}
    f, n = block_rows(data.view) if blocks is None else blocks
    batches = [data.local(np.arange(a, a + m)) for a, m in zip(f, n)]
    zf = O.prox(g, av, hg)
    av = zf.copy()
    for k in range(data.K):
        av -= c * _grad(op, data, loss, lam, k, zf)
    r = T(hg / gam)
    z = zf
    for bt in batches:
        z = O.prox(g, av, hg)
        for k in bt:
            av += c * _grad(op, data, loss, lam, k, zf)
            av -= c * _grad(op, data, loss, lam, k, z)
            av += r * (z - zf)
    out.update({"z_full": zf, "z": z, "av": av})
    return out


def afinito_params(view):
    """(alpha, tol_b, gamma_i, hat_gamma): the library wants 0 < alpha < 1, so alpha = 0.999 as everywhere in the suite; gamma_i = N / 256 makes
    the model's quadratic coefficient N alpha / (2 gamma_i) = 127.9, twice the largest ||a_i||^2 / 2 = 64 of the fill: no step backtracks,
    so device and oracle cannot part over a decision that sits on a rounding.  hat_gamma = gamma_i / 16 (what the caller says, as for
    Finito): a step moves av by hat_gamma / N = 2^-12 of its row's gradient, some hundred times the tolerance"""
    gam = view.N * 2.0 ** -8
    return 0.999, 1e-9, gam, gam / 16


def afinito_state(data, T, lam=1.0):
    """the adaptive Finito state of the gathered rows, consistent as afinito_init leaves it: points x_i of small half-integers, and per
    sample {c_i, f_i(x_i), gamma_i, a_i'x_i} with grad f_i(x_i) = c_i a_i (LeastSquares: c_i = lam (a_i'x_i - b_i)); av and z"""
    d = data.view.d
    table = np.stack([(x_vector(d, T, 3 + k) / T(2)) * (~data.zero[k]) for k in range(data.K)]).astype(T)
    dots = np.array([np.dot(data.A[k].astype(np.float64), table[k].astype(np.float64)) for k in range(data.K)])
    res = dots - data.b.astype(np.float64)
    c, f = (lam * res).astype(T), (0.5 * lam * res * res).astype(T)
    assert np.array_equal(c.astype(np.float64), lam * res) and np.array_equal(f.astype(np.float64), 0.5 * lam * res * res)
    gam = np.full(data.K, T(afinito_params(data.view)[2]), T)
    return table, c, f, gam, dots.astype(T), (x_vector(d, T, 1) / T(4)).astype(T), x_vector(d, T)


def ref_afinito(data, loss="ls", lam=1.0):
    """afinito_steps over marked rows from afinito_state (LeastSquares rows, as the suite's adaptive Finito tests)"""
    O = _O()
    T, d = data.A.dtype.type, data.view.d
    alpha, tol_b, _, hg = afinito_params(data.view)
    op, g = _problem(data, "ls", lam), prox_of(FINITO_PROX, T)
    table, c, f, gam, dots, av, z = afinito_state(data, T, lam)
    gtable = (c[:, None] * data.A).astype(T)
    done, hg, trials = O.afinito_steps(op, g, T(alpha), T(tol_b), data.local(chain_steps(data)), table, gtable, gam, f, T(hg), av, z)
    return {"table": table, "gradient table": gtable, "gam": gam, "f": f, "av": av, "z": z, "hat_gamma": np.array([hg], T),
            "counts": np.array([done, trials], np.int64)}


def proshi_params(view):
    """(gamma_i, hat_gamma, eta, lo, hi, g's upper bound): gamma_i / N = 2^-7 makes an agent's step depend on its rows of Q and q by O(1);
    hat_gamma = 4 N (what the caller says) keeps gamma_i z = gamma_i (prox(av) - av) / hat_gamma of the size of av"""
    return view.N * 2.0 ** -7, view.N * 4.0, 8.0, -2.0, 2.0, 0.5


def proshi_batches(data):
    """batches of two agents at marked rows; every one met, the second batch again at the end"""
    bs = finito_batches(data, 2)
    return bs


def ref_proshi(data, loss="ls", lam=1.0):
    """proshi_steps with Q = q = the matrix (one buffer serves both), agents at far rows, from a table that is zero off the marked rows"""
    O = _O()
    T, d, N = data.A.dtype.type, data.view.d, data.view.N
    gam, hg, eta, lo, hi, ghi = proshi_params(data.view)
    f = O.SepQuad(data.A, data.A.copy(), eta, lo, hi)
    for o in (f, O.twin_of(f)):
        if o is not None:
            o.N = N                                    # c = gamma_i / N: the agents held are a subset of N
    g = O.Prox("box", lo=-np.inf, hi=ghi, dtype=T)
    table, av, _ = finito_state(data, T)
    z = (x_vector(d, T, 2) / T(gam)).astype(T)
    O.proshi_steps(f, g, np.full(data.K, T(gam), T), T(hg), [data.local(b) for b in proshi_batches(data)], table, av, z)
    return {"table": table, "av": av, "z": z}


def models(d, T, K):
    return [x_vector(d, T, k) for k in range(K)]


def ref_stats(data, lam=1.0, Ks=(3, 17), Kg=(2, 17)):
    """the statistics passes on integer rows, in int64 (exact whatever the order of addition); the zero rows' shares are added as products"""
    v, T = data.view, data.A.dtype.type
    N, K = v.N, data.K
    A = np.rint(data.A).astype(np.int64)
    b = np.rint(data.b).astype(np.int64)
    x = np.rint(x_vector(v.d, T)).astype(np.int64)
    sq = (A * A).sum(axis=1)
    k0 = int(np.argmax(sq))
    out = {"row_sqnorms": sq.astype(np.float64),
           "row_sqnorm_stats": np.array([sq[k0], data.rows[k0], 0 if N > K else sq.min(), sq.sum()], np.float64),
           "col_sqnorms": (A * A).sum(axis=0).astype(np.float64)}
    c = A[0]                                           # col_moments(shift=None): the first row is the shift; a zero row gives -c, c^2
    out["col_moments s1"] = ((A - c).sum(axis=0) - (N - K) * c).astype(np.float64)
    out["col_moments s2"] = (((A - c) ** 2).sum(axis=0) + (N - K) * c * c).astype(np.float64)
    scale = np.rint(x_vector(v.d, np.float64, 5)).astype(np.int64)
    out["scaled"] = (A * scale).astype(T)
    if v.d <= 1024:
        out.update({"gram G": (A.T @ A).astype(np.float64), "gram u": (A.T @ b).astype(np.float64), "gram colsum": A.sum(axis=0).astype(np.float64),
                    "gram bsum": np.array([b.sum(), (b * b).sum()], np.float64)})
    dots = A @ x

    def ls_stats(dt):
        r = dt - b
        return np.array([(r * r).sum(), b.sum(), (b * b).sum(), np.abs(r).max()], np.float64)

    out["margin_stats ls"] = ls_stats(dots)
    y = np.rint(data.y).astype(np.int64)
    t = y * dots                                        # logistic: a zero row has margin 0 (an error, loss log 2)
    out["margin_stats logistic"] = np.array([float(np.sum(np.maximum(-t, 0) + np.log1p(np.exp(-np.abs(t.astype(np.float64)))))) + (N - K) * np.log(2.0),
                                             np.count_nonzero(t <= 0) + (N - K), min(int(t.min()), 0) if N > K else t.min()], np.float64)
    for Km in Ks:
        X = np.stack([np.rint(m).astype(np.int64) for m in models(v.d, T, Km)])
        out[f"margin_stats_multi K={Km}"] = np.stack([ls_stats(A @ xk) for xk in X])
    for Km in Kg:
        X = np.stack([np.rint(m).astype(np.int64) for m in models(v.d, T, Km)])
        out[f"full_gradient_multi K={Km}"] = (A.T @ (A @ X.T - b[:, None])).T.copy()          # S, int64: lam and 1 / N not applied
    return out


def multi_expected(S, lam, N, dtype):
    """T(lam S) * (T(1) / T(N)): the exact recipe of tests/test_multi_rhs_host.py (every partial sum an integer below 2^24)"""
    assert int(np.abs(S).max()) < 2 ** 24
    s = (S * lam).astype(dtype)
    return s * (np.dtype(dtype).type(1) / np.dtype(dtype).type(N))


# what the GPU test allows, in eps of the run's type at the size of the reference (test_gpu_parity.close); each the smallest `scale`
# written at a call site of the same operation in test_gpu_parity.py, test_gpu_long_rows.py or test_gpu_wide_chain.py.  Those were set
# for sums of hundreds of terms; here K <= 16 terms are nonzero.  (scale, scale64): the oracle of the run's type, the Float64 oracle
SCALES = {
    ("sweep", "av"): ({64: 81, 32: 100}, 15),                                              # test_gpu_parity.test_full_gradient
    ("svrg", "w"): ({64: 28, 32: 23}, 460), ("svrg", "z"): ({64: 20, 32: 23}, 270),        # test_chains_on_rows_of_any_length (150 steps)
    ("svrg", "z_full"): ({64: 28, 32: 23}, 460), ("svrg", "av"): ({64: 81, 32: 100}, 15),  # the epoch: w's scale (below test_svrg_epochs' 610 / 410), the sweep's
    ("saga", "init table"): ({64: 28, 32: 32}, 9.3), ("saga", "init av"): ({64: 29, 32: 28}, 13), ("saga", "init z"): (8, 11),   # test_saga_steps
    ("saga", "table"): ({64: 180, 32: 120}, 210), ("saga", "z"): ({64: 26, 32: 24}, 500),  # test_chains_on_rows_of_any_length
    ("saga", "av"): ({64: 130, 32: 140}, 110),                                             # test_saga_steps
    ("finito", "init table"): ({64: 9.4, 32: 11}, 12),                                     # test_finito_steps (init av, z: sum_scale)
    ("finito", "table"): ({64: 86, 32: 100}, 73), ("finito", "z"): ({64: 90, 32: 100}, 73), ("finito", "av"): ({64: 90, 32: 100}, 73),   # any length
    ("afinito", "z"): ({64: 910, 32: 300}, None), ("afinito", "av"): ({64: 910, 32: 300}, None),                              # test_adaptive_finito_steps
    ("afinito", "hat_gamma"): ({64: 58, 32: 48}, None), ("afinito", "gam"): (8, None),   # (no step backtracks: unchanged)
    ("afinito", "table"): ({64: 870, 32: 290}, None), ("afinito", "gradient table"): ({64: 250, 32: 190}, None), ("afinito", "f"): ({64: 130, 32: 450}, None),
    ("proshi", "table"): ({64: 170, 32: 530}, 41), ("proshi", "av"): ({64: 140, 32: 190}, 36), ("proshi", "z"): ({64: 11, 32: 30}, 29),   # test_proshi_steps
    ("lfinito", "init av"): (130, 8),                                                      # test_lfinito_iterations
    ("lfinito", "z"): ({64: 120, 32: 160}, 130), ("lfinito", "av"): ({64: 120, 32: 160}, 130), ("lfinito", "z_full"): ({64: 120, 32: 160}, 130),
}


def sum_scale(N, report):
    """the scale (eps of the run's type at the size of the sum) of a sum of N terms of one sign that a rows launch makes: a wave adds the
    rows it owns one after another, ceil(N / waves) additions at the most; the partials of the `grid` workgroups are added in a chain
    of at most `grid`; 64 more for the reductions inside a wave and a workgroup.  Every addition rounds by eps / 2 of the running sum,
    which never exceeds the result.  grid and block: as the launch report (ctx.last_kernel()) names them."""
    import re
    grid, block = (int(re.search(rf"{w}=(\d+)", report).group(1)) for w in ("grid", "block"))
    waves = grid * max(1, block // 64)
    return (-(-N // waves) + grid + 64) / 2


def scale_of(op, name):
    """(scale, scale64) of output `name` of operation `op`: 'sag0 table' and 'lists r=3 table' are 'table'"""
    if (op, name) in SCALES:
        return SCALES[(op, name)]
    return SCALES[(op, name.split()[-1])]


def tolerance(scales, ref, dtype):
    """the absolute error close() allows for `ref` under scales = (scale, scale64), in the run's type"""
    s = scales[0]
    s = float(s[64 if np.dtype(dtype) == F64 else 32]) if isinstance(s, dict) else float(s)
    return s * EPS[np.dtype(dtype)] * max(float(np.abs(np.asarray(ref, np.float64)).max(initial=0.0)), 1e-30)


# ---- the device side ------------------------------------------------------------------------------------------------------------------
GB = 2 ** 30


def need(nbytes, what):
    """skip only where the device has less free memory than the case needs plus 4 GB; the skip states both figures"""
    import pytest
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + 4 * GB:
        pytest.skip(f"{what}: needs {nbytes / GB:.1f} GB plus 4 GB, the device has {free / GB:.1f} GB free")


class Buffers:
    """the zeroed flat buffer of one type at a time (the other type's are freed first), handed out as views, and ONE second buffer of the
    same size that is not kept zero: the table, the scaled matrix, or b and the row dots at d = 2.  Allocated once per type: 35 GB"""

    def __init__(self):
        self.dtype, self.buf, self.extra = None, None, None

    def release(self):
        import torch
        self.dtype, self.buf, self.extra = None, None, None
        torch.cuda.empty_cache()

    def drop_second(self):
        """free the second buffer (the next second() allocates it again): for the one case that needs the room for something else"""
        import torch
        self.extra = None
        torch.cuda.empty_cache()

    def second(self, dtype, shape=None):
        """the second buffer of the type (contents unspecified), or its leading elements in `shape`"""
        import torch
        flat = self.flat(dtype)
        if self.extra is None:
            need(flat.numel() * flat.element_size(), f"the second {tname(dtype)} buffer")
            self.extra = torch.empty_like(flat)
        if shape is None:
            return self.extra
        n = int(np.prod(shape))
        assert n <= self.extra.numel()
        return self.extra[:n].view(*shape)

    def flat(self, dtype):
        import torch
        dtype = np.dtype(dtype)
        if self.dtype != dtype:
            self.release()
            need(ELEMS[dtype] * dtype.itemsize, f"the {tname(dtype)} buffer")
            self.buf = torch.zeros(ELEMS[dtype], dtype=torch.float64 if dtype == F64 else torch.float32, device="cuda")
            self.dtype = dtype
        return self.buf


class Placed:
    """`with Placed(buffers, view, data) as A:` -- the marked rows written into the zero buffer, A the (N, d) view at stride ld; the
    rows are zeroed again on the way out"""

    def __init__(self, buffers, view, data=None):
        self.flat, self.view, self.data = buffers.flat(view.dtype), view, fill(view) if data is None else data

    def __enter__(self):
        import torch
        v = self.view
        for r, a, z in zip(self.data.rows, self.data.A, self.data.zero):
            if not z:
                self.flat[int(r) * v.ld:int(r) * v.ld + v.d] = torch.from_numpy(a).cuda()
        return self.flat.as_strided((v.N, v.d), (v.ld, 1))

    def __exit__(self, *exc):
        v = self.view
        for r in self.data.rows:
            self.flat[int(r) * v.ld:int(r) * v.ld + v.d].zero_()
        return False


def sparse_vector(N, data, values, fillv, tdtype):
    """a device N-vector of `fillv` with values[k] at the gathered rows"""
    import torch
    t = torch.full((N,), fillv, dtype=tdtype, device="cuda") if fillv else torch.zeros(N, dtype=tdtype, device="cuda")
    for r, v in zip(data.rows, values):
        t[int(r)] = float(v)
    return t


def count_nonzero(t):
    """nonzero elements of a contiguous device tensor of any size, in steps of CHUNK elements"""
    import torch
    flat = t.reshape(-1)
    total = torch.zeros((), dtype=torch.int64, device=t.device)
    for o in range(0, flat.numel(), CHUNK):
        total += torch.count_nonzero(flat[o:o + CHUNK])
    return int(total)


def count_rows_not(t, row):
    """rows of the contiguous (N, d) device matrix t that differ from the d-vector `row` anywhere, in steps of about CHUNK elements"""
    import torch
    step = max(1, CHUNK // t.shape[1])
    total = torch.zeros((), dtype=torch.int64, device=t.device)
    for o in range(0, t.shape[0], step):
        total += (t[o:o + step] != row).any(dim=1).sum()
    return int(total)


def gather_rows(t, rows):
    """the rows `rows` of a device (N, d) matrix or N-vector, as numpy, by plain slices (no index arithmetic of the framework's)"""
    return np.stack([t[int(r)].cpu().numpy() for r in rows])


# ---- which operations run on which view -----------------------------------------------------------------------------------------------
def ops_of(view):
    """the operations tests/test_gpu_far_rows.py runs on a view: the smallest set that reaches each family's address expressions"""
    n = view.name
    if view.complex:
        return ["sweep"]
    if n == "d2":
        return ["rowindex"]
    if n == f"d{LONG_D[view.dtype]}" or n.startswith(("s5x", "guard")):
        return ["sweep"]
    if n == "s65x50":
        return ["sweep", "svrg", "afinito"]            # (the per-sample scalars of 8.7e7 dense rows of 50 would be 5.6 GB more: the strided rows)
    if n == "d8193" or n == "s65x1024":
        return ["sweep", "svrg"]
    if n == "d1024":
        return ["sweep", "svrg", "saga", "finito", "lfinito", "afinito", "proshi", "stats"]
    if n == "d50":
        return ["sweep", "svrg", "saga", "finito", "lfinito", "stats"]
    if n == "d1000":
        return ["sweep", "svrg", "saga", "stats"]
    return ["sweep", "stats"]                          # s65x1000, s65x1000odd


def data_of(view, op):
    """the gathered rows an operation's reference needs: Finito's and LFinito's row blocks visit zero rows next to the marked ones"""
    return fill(view, extra=block_extra(view) if op in ("finito", "lfinito") else ())


def reference(op, data):
    """{name: (expected array, scale or None)} of every output the GPU test compares for `op`; None: compared in bits"""
    out = {}
    if op == "sweep":
        for loss in (("ls",) if data.view.complex else ("ls", "logistic")):
            for k, v in ref_sweep(data, loss).items():
                out[f"{loss} {k}"] = (v, scale_of("sweep", "av") if k == "av" else None)
    elif op == "rowindex":
        for k, v in ref_sweep(data, "ls").items():
            out[k] = (v, scale_of("sweep", "av") if k == "av" else None)
        st = ref_stats(data, Ks=(), Kg=())
        for k in ("row_sqnorm_stats", "col_sqnorms", "margin_stats ls"):
            out[k] = (st[k], None)
    elif op == "stats":
        out = {k: (v, None) for k, v in ref_stats(data).items()}
    else:
        fn = {"svrg": ref_svrg, "saga": ref_saga, "finito": ref_finito, "lfinito": ref_lfinito, "afinito": ref_afinito, "proshi": ref_proshi}[op]
        for loss in (("ls",) if op in ("afinito", "proshi") else ("ls", "logistic")):
            outs = fn(data, loss)
            if op == "svrg" and data.view.name == "d1024":
                outs.update(ref_svrg_epoch(data, loss))
            for k, v in outs.items():
                if op == "finito" and k in ("init av", "init z"):
                    continue                           # sums over all N rows, judged under sum_scale: they do not tell one row from another
                if (op, k) == ("proshi", "z"):
                    continue                           # judged at the size of av / hat_gamma (close(size=)): table and av tell the rows apart
                if (op, k) == ("afinito", "counts"):
                    out[f"{loss} {k}"] = (v, None)
                    continue
                out[f"{loss} {k}"] = (v, scale_of(op, k))
    return out

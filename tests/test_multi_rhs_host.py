"""The K-iterate full pass (csrc/mrhs_kernels.h, csrc/mrhs_launch.inc) without a GPU: launch_mrhs's plan restated, the (N, K) list of
tests/test_gpu_multi_rhs_paths.py held to the plan classes it is there for, the exact integer reference of that file, and -- on the
reference side only -- the proof that the exact comparison can fail: what a dropped row, an unmasked short tile, a shifted b, two swapped
solves or a padded solve written over a real one would compute differs IN BITS from the expected result on every (N, K) of the list.

The plan (mrhs_launch.inc): nkb = ceil(K / 16) column blocks of 16 solves; P = max(1, num_cu / nkb) row partitions, rounded down to a
multiple of 8 from 8 on (the column blocks of a partition then share an XCD), never more than ceil(N / 16); the kernel gives every
partition per = ceil(ceil(N / P) / 16) * 16 rows, whole 16-row tiles, the last non-empty one what is left.  A tile step is STEADY
(tile_step(std::true_type): nothing conditional, pinned instruction groups) while the tile after next is whole: a partition of r rows
makes max(0, floor(r / 16) - 2) steady steps and the rest through the guarded form.

The integer data (test_gpu_multi_rhs_paths.py part 1): a in {-1, 0, 1}, x in {-2 .. 2}, b in {-2 .. 2}, lam in {1, 1/2}, seeded and not
periodic.  With r = A x - b every intermediate of the pass is an integer (lam = 1/2: a half-integer) bounded by max_i sum_j |a_ij x_jk|
<= 2 d and max_j sum_i |a_ij| |r_ik| <= N (2 d + 2) <= 1281 * 2050 < 2^24, so fp32 and fp64 hold every partial sum exactly in ANY order and
the device must give T(lam S) * (T(1) / T(N)) to the bit, S = A'(A X - b) in int64.  The int64 products are torch's on the CPU (numpy's
integer product walks the same operands some twenty times slower); int_reference holds every one of them, at every size, to numpy's
int64 `@` through products with random integer vectors, and test_reference_is_numpy_int64 entry by entry at d = 128."""
import numpy as np
import pytest

TILE = KB = 16
LIMIT = 2 ** 24

# (dtype, d): the nine instantiations mrhs_kernel<T, SL = d / 16>
VARIANTS = [(np.float64, d) for d in (128, 256, 512, 768, 1024)] + [(np.float32, d) for d in (256, 512, 768, 1024)]

# (N, K) of part 1.  At 256 CUs (rows per partition):
#   (1, 2) [1]   (15, 2) [15]   (16, 3) [16]   (17, 2) [16, 1]   (33, 16) [16, 16, 1]   (129, 17) 8 x 16 + [1], plain map, 2 column blocks
#   K = 256, P = 16 (XCD map, 16 blocks): 512 -> 32 each   768 -> 48 each   1280 -> 80 each   1277 -> 15 x 80 + [77]
#                                         1281 -> 13 x 96 + [33, 0, 0]
#   (513, 257) P = 8, 17 blocks: 6 x 80 + [33, 0]      (637, 512) P = 8, 32 blocks: 7 x 80 + [77]      (641, 512): 6 x 96 + [65, 0]
#   K = 528, P = 7 (plain map, 33 blocks): 320 -> 6 x 48 + [32]      560 -> 80 each (five tiles under the plain map and beyond K = 512)
CASES = [(1, 2), (15, 2), (16, 3), (17, 2), (33, 16), (129, 17), (512, 256), (768, 256), (1280, 256), (1277, 256), (1281, 256), (513, 257),
         (637, 512), (641, 512), (320, 528), (560, 528)]
NMAX, KMAX = max(n for n, _ in CASES), max(k for _, k in CASES)


def lam_of(case):
    """lam of a case of the list: 1 and 1/2 in turn (never N: N = 1281 would carry the sums past 2^24)"""
    return (1.0, 0.5)[CASES.index(case) % 2]


def plan(N, K, num_cu):
    """launch_mrhs restated -> (nkb, P, per, [rows of every partition])"""
    nkb = -(-K // KB)
    P = max(1, num_cu // nkb)
    if P >= 8:
        P -= P % 8
    P = min(P, -(-N // TILE))
    per = -(-(-(-N // P)) // TILE) * TILE
    return nkb, P, per, [max(0, min(N, (p + 1) * per) - p * per) for p in range(P)]


def block_map(b, nkb, P):
    """blockIdx.x -> (row partition, column block), as mrhs_kernel computes it"""
    xcd, slot = b & 7, b >> 3
    if (P & 7) == 0:
        return xcd + 8 * (slot // nkb), slot % nkb
    return b // nkb, b % nkb


def steady_steps(rows):
    """the steps of a partition of `rows` rows that run tile_step(std::true_type): t0 = 0, 16, .. while t0 + 48 <= rows"""
    return max(0, rows // TILE - 2)


def report(dtype, d, N, K, num_cu):
    """what ctx.last_kernel() says after the pass"""
    nkb, P, _, _ = plan(N, K, num_cu)
    return f"mrhs_kernel<{'f64' if dtype == np.float64 else 'f32'},SL{d // 16}> grid={nkb * P} block=256 K={K} partitions={P}"


REQUIRED = {"1 whole tile", "2 whole tiles", "3 whole tiles", ">= 5 whole tiles", "1-row tile alone", "13-15-row tile alone",
            "1-row tile after steady steps", "13-15-row tile after steady steps", "empty trailing partition", "N = 1", "xcd map, nkb > 1",
            "plain map, nkb > 1", "K = 2", "K = 16", "K = 17", "K >= 256", "K >= 513", ">= 3 steady steps", ">= 3 steady steps, xcd map, nkb > 1",
            ">= 3 steady steps, plain map, nkb > 1", ">= 3 steady steps, K >= 513"}


def classes(cases, num_cu):
    """the plan classes a list of (N, K) reaches on a device of num_cu compute units"""
    got = set()
    for N, K in cases:
        nkb, P, per, rows = plan(N, K, num_cu)
        xcd = P % 8 == 0
        for r in rows:
            q, rem = divmod(r, TILE)
            if rem == 0 and q in (1, 2, 3):
                got.add(f"{q} whole tile" + ("s" if q > 1 else ""))
            if rem == 0 and q >= 5:
                got.add(">= 5 whole tiles")
            for name, hit in (("1-row", rem == 1), ("13-15-row", 13 <= rem <= 15)):
                if hit and q == 0:
                    got.add(f"{name} tile alone")
                if hit and steady_steps(r) >= 1:
                    got.add(f"{name} tile after steady steps")
            if steady_steps(r) >= 3:
                got.add(">= 3 steady steps")
                if nkb > 1:
                    got.add(f">= 3 steady steps, {'xcd' if xcd else 'plain'} map, nkb > 1")
                if K >= 513:
                    got.add(">= 3 steady steps, K >= 513")
        if rows[-1] == 0:
            got.add("empty trailing partition")
        if N == 1:
            got.add("N = 1")
        if nkb > 1:
            got.add(f"{'xcd' if xcd else 'plain'} map, nkb > 1")
        got |= {f"K = {K}"} & {"K = 2", "K = 16", "K = 17"}
        if K >= 256:
            got.add("K >= 256")
        if K >= 513:
            got.add("K >= 513")
    return got


def call_order(cases):
    """large and small K in turn: a later call then reuses the workspace and the pointer table a larger one left"""
    by_k = sorted(cases, key=lambda c: (c[1], c[0]))
    out = []
    while by_k:
        out.append(by_k.pop())
        if by_k:
            out.append(by_k.pop(0))
    return out


# ---- the integer data and its exact reference ----------------------------------------------------------------------------------------------
_DATA, _REF = {}, {}


def int_data(d):
    """(A (NMAX x d), X (KMAX x d), b (NMAX + 1)) int64, seeded per d, read-only; a case takes the leading N rows and K iterates (b has
    one entry more than A has rows: `b shifted by one row` is then defined at N = NMAX too)"""
    if d not in _DATA:
        rng = np.random.default_rng(7000 + d)
        A, X, b = rng.integers(-1, 2, (NMAX, d)), rng.integers(-2, 3, (KMAX, d)), rng.integers(-2, 3, NMAX + 1)
        assert len({x.tobytes() for x in X}) == KMAX, "two solves share an iterate"
        for v in (A, X, b):
            v.setflags(write=False)
        _DATA[d] = (A, X, b)
    return _DATA[d]


def int_reference(d, N, K):
    """(S (K x d), R (N x K)) int64: R = A X' - b, S = (A' R)' -- row k of S is sum_i (a_i'x_k - b_i) a_i, lam and 1 / N not applied.
    Asserts the condition that makes any order of addition exact.  Computed once per (d, N, K), shared by both types, read-only."""
    if (d, N, K) not in _REF:
        import torch
        A, X, b = int_data(d)
        tA, tX = torch.from_numpy(A[:N].copy()), torch.from_numpy(X[:K].copy())
        R = tA @ tX.T - torch.from_numpy(b[:N].copy())[:, None]
        S = (tA.T.contiguous() @ R).T.contiguous().numpy()
        R = R.numpy()
        assert S.dtype == np.int64 and R.dtype == np.int64
        # held to numpy's int64 `@` at EVERY size, by products with two random integer vectors v in [0, 2^20) (numpy matrix-vector
        # products: O(N d + N K + K d)):  R v = A (X' v) - b sum(v)  and  S' v = A' (R v).  A wrong entry of R or S survives one v with
        # probability at most 2^-20; every term stays below 2^24 * 2^20 * K < 2^63.  Entry by entry: test_reference_is_numpy_int64.
        vs = np.random.default_rng(N * 1000 + K).integers(0, 2 ** 20, (2, K))
        for v in vs:
            Rv = A[:N] @ (X[:K].T @ v) - b[:N] * int(v.sum())
            assert Rv.dtype == np.int64 and np.array_equal(R @ v, Rv) and np.array_equal(S.T @ v, A[:N].T @ Rv), (d, N, K)
        # |a| <= 1: sum_j |a_ij x_jk| <= 2 sum_j |a_ij| and sum_i |a_ij| |r_ik| <= sum_i |r_ik| (upper bounds of the two conditions)
        assert 2 * int(np.abs(A[:N]).sum(axis=1).max()) < LIMIT and int(np.abs(R).sum(axis=0).max()) < LIMIT
        for v in (S, R):
            v.setflags(write=False)
        _REF[(d, N, K)] = (S, R)
    return _REF[(d, N, K)]


def expected(S, lam, N, dtype):
    """T(lam S) * (T(1) / T(N)): one IEEE multiply in the run's type, as mrhs_finalize_kernel's s * invN"""
    s = (S * lam).astype(dtype)
    assert np.array_equal(s.astype(np.float64), S * lam)
    return s * (dtype(1) / dtype(N))


def bits(v):
    return np.ascontiguousarray(v).view(np.int64 if v.dtype == np.float64 else np.int32)


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------
def test_plan_properties():
    """every row in exactly one partition, whole tiles but for the last non-empty partition, grid = nkb P, both block maps bijections"""
    maps = set()
    for num_cu in (64, 256, 304):
        for K in (2, 16, 17, 100, 256, 257, 528, 4096):
            for N in range(1, 701):
                nkb, P, per, rows = plan(N, K, num_cu)
                assert nkb * KB >= K > (nkb - 1) * KB and 1 <= P <= max(1, num_cu // nkb) and P <= -(-N // TILE)
                assert per % TILE == 0 and per >= TILE and len(rows) == P
                # the kernel's own range arithmetic: r_lo = part * per, r_hi = min(r_lo + per, N), nothing to do where r_lo >= r_hi
                seen = 0
                for part in range(P):
                    r_lo = part * per
                    r_hi = r_lo + per if r_lo + per < N else N
                    assert max(0, r_hi - r_lo) == rows[part]
                    if r_lo < r_hi:
                        assert r_lo == seen                                   # contiguous, in order, no row twice
                        seen = r_hi
                assert seen == N
                nonempty = [r for r in rows if r]
                assert all(r == per for r in nonempty[:-1]) and rows == nonempty + [0] * (P - len(nonempty))
                maps.add((nkb, P))
    assert any(P % 8 == 0 and nkb > 1 for nkb, P in maps) and any(P % 8 and nkb > 1 for nkb, P in maps)
    for nkb, P in maps:
        grid = nkb * P
        assert sorted(block_map(b, nkb, P) for b in range(grid)) == [(p, k) for p in range(P) for k in range(nkb)], (nkb, P)
        if P % 8 == 0:   # what the map is for: the column blocks of a partition are slots of one XCD (workgroups go round-robin by blockIdx)
            assert all(block_map(b, nkb, P)[0] % 8 == b % 8 for b in range(grid))


def test_the_list_reaches_every_class_at_256_compute_units():
    got = classes(CASES, 256)
    assert REQUIRED <= got, sorted(REQUIRED - got)
    rows = {c: plan(*c, 256)[3] for c in CASES}
    assert rows[(17, 2)] == [16, 1] and rows[(1277, 256)] == [80] * 15 + [77] and rows[(1281, 256)] == [96] * 13 + [33, 0, 0]
    assert rows[(641, 512)] == [96] * 6 + [65, 0] and rows[(320, 528)] == [48] * 6 + [32] and rows[(560, 528)] == [80] * 7
    assert [plan(*c, 256)[:2] for c in ((129, 17), (512, 256), (513, 257), (637, 512), (560, 528))] == [(2, 9), (16, 16), (17, 8), (32, 8), (33, 7)]
    assert sorted(call_order(CASES)) == sorted(CASES) and [k for _, k in call_order(CASES)][:4] == [528, 2, 528, 2]
    # the eight shapes of tests/test_gpu_multi_rhs.py, for that file's header: tiles per partition
    old = [(256, 2, 37), (256, 16, 1000), (512, 21, 3001), (1024, 48, 2050), (1024, 5, 16), (1024, 33, 40000), (768, 19, 5000), (128, 17, 3000)]
    assert [(plan(N, K, 256)[1], plan(N, K, 256)[2] // TILE) for _, K, N in old] == [(3, 1), (63, 1), (128, 2), (80, 2), (1, 1), (80, 32), (128, 3), (128, 2)]


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------
def test_the_sums_stay_exact_for_every_variant():
    """the two 2^24 conditions from the value ranges alone, for every d and N of the list; and measured, at d = 128, where the matrices
    are small: the largest sums are far below the a-priori bound"""
    import torch
    for d in sorted({d for _, d in VARIANTS}):
        A, X, b = int_data(d)
        assert np.abs(A).max() == 1 and np.abs(X).max() == 2 and np.abs(b).max() == 2
        assert 2 * d < LIMIT and NMAX * (2 * d + 2) < LIMIT
    A, X, b = int_data(128)
    worst = [0, 0]
    for N, K in CASES:
        S, R = int_reference(128, N, K)
        absA, absX, absR = (torch.from_numpy(np.abs(v)) for v in (A[:N], X[:K], R))
        dots, sums = int((absA @ absX.T).max()), int((absA.T.contiguous() @ absR).max())
        assert dots <= 2 * int(np.abs(A[:N]).sum(axis=1).max()) and sums <= int(np.abs(R).sum(axis=0).max()) < LIMIT
        assert int(np.abs(S).max()) <= sums
        worst = [max(worst[0], dots), max(worst[1], sums)]
    print(f"d = 128: max_i sum_j |a_ij x_jk| = {worst[0]}, max_j sum_i |a_ij| |r_ik| = {worst[1]}")


def test_reference_is_numpy_int64():
    A, X, b = int_data(128)
    for N, K in CASES:
        S, R = int_reference(128, N, K)
        Rn = A[:N] @ X[:K].T - b[:N, None]
        assert Rn.dtype == np.int64 and np.array_equal(R, Rn) and np.array_equal(S, (A[:N].T @ Rn).T)
    # expected(): lam S is formed exactly, then ONE multiply by the rounded 1 / N in the run's type
    got = expected(np.array([[3, -7]]), 0.5, 3, np.float32)
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(np.array([[1.5, -3.5]], np.float32) * (np.float32(1) / np.float32(3))))


def mutants(d, N, K, num_cu=256):
    """(name, S') for what the kernel would add up if it were wrong in one place; names of mutations that do not apply to the shape (no
    short tile: N a multiple of 16; no padded solve: K a multiple of 16) are left out"""
    A, X, b = int_data(d)
    S, R = int_reference(d, N, K)
    _, P, per, rows = plan(N, K, num_cu)
    A = A[:N]
    rank1 = lambda i: np.outer(R[i], A[i])                                      # row i's share of every solve
    yield "the last row dropped", S - rank1(N - 1)
    first = per * max(p for p in range(P) if rows[p])
    yield "a partition's first row dropped", S - rank1(first)
    if N % TILE:
        yield "the short tile's copies of the last row not masked", S + (TILE - N % TILE) * rank1(N - 1)
    yield "b shifted by one row", S + (A.T @ (b[:N] - b[1:N + 1]))[None, :]
    sw = S.copy()
    sw[[0, K - 1]] = sw[[K - 1, 0]]
    yield "two solves' iterates swapped", sw
    if K % KB:
        over = S.copy()
        over[K - 1] = over[K - 2]
        yield "a padded solve written over solve K - 1", over


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_mutation_changes_the_expected_bits(dtype):
    """d = 128 (the mutations are statements about rows and solves, not about columns): on every (N, K) of the list every mutation that
    applies to the shape changes the bits of at least one solve's expected result"""
    seen = {}
    for N, K in CASES:
        S, _ = int_reference(128, N, K)
        want = bits(expected(S, lam_of((N, K)), N, dtype))
        names = []
        for name, Sm in mutants(128, N, K):
            assert int(np.abs(Sm).max()) < LIMIT
            changed = (bits(expected(Sm, lam_of((N, K)), N, dtype)) != want).any(axis=1)
            assert changed.any(), (name, N, K)
            names.append(name)
            seen[name] = seen.get(name, 0) + 1
        assert len(names) == 4 + (N % TILE != 0) + (K % KB != 0), (N, K, names)
    assert len(seen) == 6 and min(seen.values()) >= 4, seen

// gram_kernels.h -- the second-order statistics of a packed matrix in ONE pass over its rows (ciao_gram):
//      G = A'A (d x d)      u = A'b      colsum = A'1      bsum = {sum b, sum b^2}
// all in double whatever the rows' type is.  The first pass of this family that is compute-bound: N d^2 flops (upper triangle) on N d
// elements, so it runs on the matrix cores (v_mfma_f64_16x16x4_f64) and the rows reach them through LDS.
//
// Structure.  The d columns are cut into nb = ceil(d / 128) column blocks; only the nb (nb + 1) / 2 tiles (ib, jb) with jb >= ib exist.
// grid = tiles x P row partitions (gram_plan, a pure function of (N, d)).  A workgroup = 4 waves owns one 128 x 128 tile of G over one
// contiguous range of rows and walks it in chunks of 16 rows:
//     1. the chunk's two panels (16 rows x 128 columns of block ib and of block jb; one panel where ib == jb) come from global memory a
//        chunk ahead, coalesced (consecutive threads read consecutive 16-byte pieces of a row), are converted to double where the rows are
//        fp32, and are parked row-major in LDS (two buffers in turn, one barrier per chunk);
//     2. wave (wi, wj) of a 2 x 2 arrangement owns the 64 x 64 quarter: 4 x 4 MFMA tiles, 16 accumulators = 64 doubles per lane.  With the
//        SAMPLE index as the MFMA's k, both operands have the same shape -- lane (l & 15 -> column, l >> 4 -> row of a 4-row group) -- so
//        sixteen consecutive columns of four consecutive rows are read from the row-major LDS copy straight into operand layout: no
//        transpose anywhere.  Per group of 4 rows: 8 LDS reads of one double per lane, 16 MFMAs.
//     3. on a diagonal tile the quarter (1, 0) is the mirror of (0, 1) and is not needed.  Its wave computes the AUGMENTED columns instead:
//        the B operand [b_n, 1, 0, ... 0] against the 8 sixteen-column pieces of the panel gives u (accumulator column 0) and colsum (column 1)
//        for the tile's 128 columns, and against itself sum b^2, sum b (and the row count): the Gram matrix of the row [a_n, b_n, 1] without a
//        column block of its own.  9 MFMAs per 4 rows against the other waves' 16.
//   At the end every workgroup writes one record (the 128 x 128 partial tile; on diagonal tiles also u, colsum, bsum) into the workspace.
//   gram_final_kernel adds a tile's P records in partition order, one thread per element, and writes G[i][j] and its mirror G[j][i] FROM
//   THE SAME SUM for i <= j (elements below the diagonal of a diagonal tile are never read): both triangles hold the same bits.
//   No atomics, no flags, no scratch: the hand-off is the kernel boundary.
//
// What is never read: columns [d, ld) of a row, rows outside the partition.  Chunks of 16 bytes that lie wholly in [0, d) of an existing
// row are vector loads where the base of A and ld allow; everything else is read element by element under its own predicate and what does
// not exist is 0 IN BOTH OPERANDS (the ones of the augmented column included), so padding that holds NaN never meets a multiply.
//
// Order of addition.  An element of a record: the rows of the partition in groups of four, each group by one MFMA onto the running sum;
// then the P records in partition order.  A function of (N, d) alone: not of ld, of the base, of the rows' type (fp32 values are exact in
// double and so is every product of two of them), of the NULL outputs, or of the run.
//
// With a weight per row (ciao_gram_weighted): gram_partial_kernel<Weighted<T>> and gram_final_kernel<Weighted<T>>,
// the same kernel text instantiated on a tag type -- see Weighted<T> below.  G = A' diag(w) A, u = A'(w b), colsum = A'w,
// bsum = {sum w b, sum w b^2, sum w}; plan, tile map, workspace and order of addition are the ones above.
#pragma once

#include "ciao_common.h"

namespace ciao {

constexpr int GRAM_T = 128;                 // columns per block: the tile is GRAM_T x GRAM_T
constexpr int GRAM_KC = 16;                 // rows per staged chunk
constexpr int GRAM_BLOCK = 256;             // four waves, 2 x 2 quarters of 64 x 64
constexpr int GRAM_PITCH = GRAM_T + 16;     // LDS row in doubles: consecutive rows start 128 bytes apart modulo the 256 bytes of banks
constexpr int GRAM_OFF_U = GRAM_T * GRAM_T;          // a record: the tile, then u, colsum (128 each), then {sum b, sum b^2}
constexpr int GRAM_OFF_CS = GRAM_OFF_U + GRAM_T;
constexpr int GRAM_OFF_B = GRAM_OFF_CS + GRAM_T;
constexpr int GRAM_REC = GRAM_OFF_B + 8;             // doubles per (tile, partition) record (weighted: a third sum, sum w, at GRAM_OFF_B + 2)
constexpr int GRAM_WG_TARGET = 2048;        // workgroups asked for (8 per CU, as colsq / rowsq / mscore)
constexpr size_t GRAM_WS_BYTES = (size_t)256 << 20;
constexpr int GRAM_MAX_D = 4096;
constexpr int GRAM_FINAL_BLOCKS = GRAM_T * GRAM_T / GRAM_BLOCK;   // final-kernel workgroups per tile

struct GramPlan {
    int nb;          // column blocks
    int ntiles;      // nb (nb + 1) / 2
    int P;           // row partitions
    int xcd;         // 1: the tiles of a partition share an XCD (P a multiple of 8)
    int grid;        // ntiles * P
    int64_t per;     // rows per partition: whole chunks
    size_t ws_bytes;
};

// a pure function of (N, d); N >= 1, 1 <= d <= GRAM_MAX_D
__host__ __device__ inline GramPlan gram_plan(int64_t N, int64_t d)
{
    GramPlan pl;
    pl.nb = (int)((d + GRAM_T - 1) / GRAM_T);
    pl.ntiles = pl.nb * (pl.nb + 1) / 2;
    const int64_t cap = (int64_t)(GRAM_WS_BYTES / ((size_t)pl.ntiles * GRAM_REC * sizeof(double)));   // >= 3 at d = 4096
    int64_t want = ((GRAM_WG_TARGET + pl.ntiles - 1) / pl.ntiles + 7) / 8 * 8;
    if (want > cap) want = cap;
    if (want >= 8) want = want / 8 * 8;
    int64_t per = ((N + want - 1) / want + GRAM_KC - 1) / GRAM_KC * GRAM_KC;
    if (per < GRAM_KC) per = GRAM_KC;
    pl.per = per;
    pl.P = (int)((N + per - 1) / per);
    pl.xcd = pl.P % 8 == 0;
#ifdef CIAO_GRAM_PLAIN_MAP   // experiment builds only (Makefile EXP=): the A/B of the two blockIdx maps on one shape (CHANGELOG)
    pl.xcd = 0;
#endif
    pl.grid = pl.ntiles * pl.P;
    pl.ws_bytes = (size_t)pl.grid * GRAM_REC * sizeof(double);
    return pl;
}

// tile t -> (ib, jb), jb >= ib, row-major over the upper triangle of blocks
__host__ __device__ inline void gram_tile(int t, int nb, int &ib, int &jb)
{
    int i = 0;
    while (t >= nb - i) {
        t -= nb - i;
        ++i;
    }
    ib = i;
    jb = i + t;
}

template <typename T>
struct GramArgs {
    const T *A;
    const T *b;
    int64_t ld, N, d;
    int64_t per;     // rows per partition
    int P, nb, ntiles, xcd;
    int vec16;       // the base of A and ld are multiples of 16 bytes
    double *rec;     // [tile][partition][GRAM_REC]
};

constexpr size_t gram_lds_bytes() { return (size_t)2 * 2 * GRAM_KC * GRAM_PITCH * sizeof(double); }

// The weighted instantiation (ciao_gram_weighted): gram_partial_kernel<Weighted<T>> is the same kernel text with
// a weight per row, a.w = N doubles; gram_partial_kernel<T> compiles to what it was without it.  Exactly ONE operand of every MFMA
// carries the weight, multiplied in double with one rounding where the operand is made; the other operand is the raw element:
//     - panel J is parked in LDS already weighted (w_n a_nj); on a diagonal tile panel I is parked twice, raw into its own slot and weighted
//       into the J slot a diagonal tile otherwise leaves unused, so every wave reads raw I against weighted J and the MFMA loop is the
//       unweighted one;
//     - the augmented wave keeps a raw [b, 1] and a weighted [w b, w] operand: u, colsum from the panel against the weighted one, and raw
//       against weighted gives sum w b^2 (0, 0), sum w b (0, 1) and sum w (1, 1).
// The thread that parks a chunk of a row fetches that row's weight with the chunk (NLD rows a thread and chunk), at a row index CLAMPED
// into the partition (min(row, r_hi - 1)): nothing beyond w[N - 1] is read, the load has no branch of its own, and its value is first
// used at the parking, after the MFMA loop.  A row that does not exist therefore carries the weight of the partition's last row against
// elements that are 0 in both operands: the products are the zeros a weight of 0 would give, for every finite weight (and a non-finite
// weight of an existing row makes every output NaN whichever way).  With w = 1 every operand is the unweighted one (1 a is exact) and the
// order of addition is the same: the same bits.
template <typename T>
struct Weighted {};
// The row-list instantiations (ciao_gram_rows): gram_partial_kernel<Indexed<TT>>, TT = T or Weighted<T>, is the same
// kernel text over a LIST of rows, a.idx = M int64 row numbers.  List position m plays the part of the row number everywhere: a.N = M, the
// plan is gram_plan(M, d), partitions are ranges of positions, and the weight (Weighted) is read at the position.  Only two addresses
// change: the panel row of position m is row idx[m] of A, and b is read at idx[m].  Records, final kernels and the order of addition are
// the ones above, so the outputs are the bits of the unindexed kernel on the gathered copy A[idx], b[idx].
//   The rows a WAVE parks in one chunk are wave-uniform (fp64: chunk q = 256 i + tid is row 4 i + wave; fp32: rows 8 i + 2 wave and + 1,
// by lane half), so their indices are scalar LOADS into SGPRs -- NLD * RPW of them a wave and chunk, held as the row's offset idx * ld --
// fetched TWO chunks ahead, after the MFMA loop of the chunk before the one whose panel loads use them: the loads' wait is the one in
// front of the barrier, and no wave meets an index before its MFMAs.  The augmented wave, which needs b at the chunk's 16 rows, loads
// ONE entry a lane at the same point and passes it between lanes where it is used (see arow below): two VGPRs that stay put through the
// MFMA loop, and with weights one more of validity bits.  Positions are clamped into the partition (nothing beyond idx[M - 1] is read).
//   An entry outside [0, rows) is a row that does not exist: no load is issued for it and it is 0 in both operands, the ones of the
// augmented column included.  Context.gram(rows=) refuses such a list before any launch; the predicate is here so that the raw entry
// point cannot read out of bounds.
template <typename TT>
struct Indexed {};
template <typename TT>
struct GramElem {
    using type = TT;
    using base = TT;
    static constexpr bool weighted = false;
    static constexpr bool indexed = false;
};
template <typename T>
struct GramElem<Weighted<T>> {
    using type = T;
    using base = Weighted<T>;
    static constexpr bool weighted = true;
    static constexpr bool indexed = false;
};
template <typename TT>
struct GramElem<Indexed<TT>> {
    using type = typename GramElem<TT>::type;
    using base = TT;   // whose final kernel adds the records
    static constexpr bool weighted = GramElem<TT>::weighted;
    static constexpr bool indexed = true;
};
template <typename T>
struct GramArgs<Weighted<T>> : GramArgs<T> {
    const double *w;   // N doubles, 8-byte aligned
};
template <typename TT>
struct GramArgs<Indexed<TT>> : GramArgs<TT> {   // N = M, the length of the list; w (Weighted): M doubles, by position
    const int64_t *idx;   // M row numbers, 8-byte aligned
    int64_t rows;         // the rows A has: an entry outside [0, rows) is a row that does not exist
};

template <typename TT>
__global__ void __launch_bounds__(GRAM_BLOCK) gram_partial_kernel(GramArgs<TT> a)
{
    using T = typename GramElem<TT>::type;
    constexpr bool WEIGHTED = GramElem<TT>::weighted;
    constexpr bool INDEXED = GramElem<TT>::indexed;
    using M = MfmaOf<double>;
    using Acc = typename M::acc;
    constexpr int VEC = 16 / (int)sizeof(T);
    typedef T Vld __attribute__((ext_vector_type(VEC)));
    typedef double D2 __attribute__((ext_vector_type(2)));
    constexpr int CPR = GRAM_T / VEC;                     // 16-byte chunks of a panel row
    constexpr int NLD = GRAM_KC * CPR / GRAM_BLOCK;       // chunks per thread and panel
    constexpr int PANEL = GRAM_KC * GRAM_PITCH;           // doubles of one parked panel
    static_assert(NLD >= 1 && NLD * GRAM_BLOCK == GRAM_KC * CPR, "panel layout");
    constexpr int RPW = WAVE / CPR;                       // (INDEXED) rows of which one wave holds chunks in one load: 1 (fp64) or 2 (fp32)
    static_assert(RPW >= 1 && RPW <= 2 && RPW * CPR == WAVE, "a wave's chunks of one load lie in one or two rows");
    extern __shared__ __attribute__((aligned(16))) unsigned char gram_raw[];
    double *lds = reinterpret_cast<double *>(gram_raw);   // [2 buffers][panel I, panel J][KC][PITCH]
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, h = lane >> 4;
    const int wi = w >> 1, wj = w & 1;

    // blockIdx -> (row partition, tile): with P a multiple of 8 the tiles of one partition are consecutive slots of ONE XCD (workgroups
    // go to XCDs round-robin by blockIdx), so the nb panels of a chunk come from HBM once and from that XCD's L2 for the other tiles
    // (mrhs_kernels.h).  Which workgroup takes which pair changes no result.
    int part, t;
    if (a.xcd) {
        part = (blockIdx.x & 7) + 8 * (int)((blockIdx.x >> 3) / a.ntiles);
        t = (int)((blockIdx.x >> 3) % a.ntiles);
    } else {
        part = (int)(blockIdx.x / a.ntiles);
        t = (int)(blockIdx.x % a.ntiles);
    }
    int ib, jb;
    gram_tile(t, a.nb, ib, jb);
    const bool diag = ib == jb;
    const bool augwave = diag && w == 2;   // quarter (1, 0) of a diagonal tile: the augmented columns instead
    const int64_t r_lo = (int64_t)part * a.per;
    const int64_t r_hi = r_lo + a.per < a.N ? r_lo + a.per : a.N;
    const int64_t ci0 = (int64_t)ib * GRAM_T, cj0 = (int64_t)jb * GRAM_T;

    // (INDEXED) the rows of one chunk.  ri[i][s], wave-uniform, for the rows this wave parks: the row's offset idx[m] * ld in elements, or
    // -1 where the position lies beyond the partition or the entry names no row -- scalar loads at positions clamped into the partition.
    // arow: the augmented wave's, lane (c, h) holding the raw entry at position 4 (c & 3) + h (clamped) -- ONE vector load a lane and chunk,
    // issued after the MFMA loop and first used at the top of the next iteration, where the lane that needs position 4 ks + h takes it
    // from lane (ks, h).  It stays in its two registers through the loop: a register that the MFMA loop reused while the load may be in
    // flight would cost every wave a wait for its loads in front of its MFMAs.
    int64_t ri[NLD][RPW] = {}, arow = 0;
    auto row_at = [&](int64_t pos) -> int64_t {
        int64_t r = -1;
        if constexpr (INDEXED) {
            const int64_t v = a.idx[pos < r_hi ? pos : r_hi - 1];
            r = (pos < r_hi && (uint64_t)v < (uint64_t)a.rows) ? v * a.ld : -1;
        }
        return r;
    };
    auto exists = [&](int64_t r) -> bool {   // of an entry: 0 <= r < rows, one compare
        if constexpr (INDEXED)
            return (uint64_t)r < (uint64_t)a.rows;
        else
            return true;
    };
    auto fetch_rows = [&](int64_t t0) {
#pragma unroll
        for (int i = 0; i < NLD; ++i)
#pragma unroll
            for (int s = 0; s < RPW; ++s) ri[i][s] = row_at(t0 + i * (GRAM_BLOCK / CPR) + w * RPW + s);
        if (augwave) {
            const int64_t pos = t0 + 4 * (c & 3) + h;
            if constexpr (INDEXED) arow = a.idx[pos < r_hi ? pos : r_hi - 1];
        }
    };
    // one panel of the chunk at t0, staged in registers: chunk q = 256 i + tid is chunk q % CPR of row q / CPR
    Vld stI[NLD], stJ[NLD];
    auto load_panel = [&](Vld(&st)[NLD], int64_t c0, int64_t t0) {
        if constexpr (INDEXED) {   // the rows are ri[][] (fetched for this t0); `whole` is uniform in the WAVE here
            bool whole = a.vec16 && c0 + GRAM_T <= a.d;
#pragma unroll
            for (int i = 0; i < NLD; ++i)
#pragma unroll
                for (int s = 0; s < RPW; ++s) whole = whole && ri[i][s] >= 0;
            if (whole) {
#pragma unroll
                for (int i = 0; i < NLD; ++i) {
                    const int64_t off0 = ri[i][0], off1 = ri[i][RPW - 1];
                    const int64_t off = (RPW == 2 && (lane & CPR)) ? off1 : off0;
                    st[i] = *reinterpret_cast<const Vld *>(a.A + off + (c0 + (lane % CPR) * VEC));
                }
            } else {
#pragma unroll
                for (int i = 0; i < NLD; ++i) {
                    const int64_t off0 = ri[i][0], off1 = ri[i][RPW - 1];
                    const int64_t off = (RPW == 2 && (lane & CPR)) ? off1 : off0;
                    const bool have = off >= 0;
                    const int64_t col = c0 + (lane % CPR) * VEC;
                    const T *src = a.A + off + col;
                    if (a.vec16 && have && col + VEC <= a.d) {
                        st[i] = *reinterpret_cast<const Vld *>(src);
                    } else {
#pragma unroll
                        for (int e = 0; e < VEC; ++e) st[i][e] = (have && col + e < a.d) ? src[e] : T(0);
                    }
                }
            }
            return;
        }
        const bool whole = a.vec16 && t0 + GRAM_KC <= r_hi && c0 + GRAM_T <= a.d;   // (uniform in the workgroup)
        if (whole) {
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int q = i * GRAM_BLOCK + tid;
                st[i] = *reinterpret_cast<const Vld *>(a.A + (t0 + q / CPR) * a.ld + (c0 + (q % CPR) * VEC));
            }
        } else {
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int q = i * GRAM_BLOCK + tid;
                const int64_t row = t0 + q / CPR;
                const int64_t col = c0 + (q % CPR) * VEC;
                const T *src = a.A + row * a.ld + col;
                if (a.vec16 && row < r_hi && col + VEC <= a.d) {
                    st[i] = *reinterpret_cast<const Vld *>(src);
                } else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) st[i][e] = (row < r_hi && col + e < a.d) ? src[e] : T(0);
                }
            }
        }
    };
    auto park_panel = [&](const Vld(&st)[NLD], double *dst) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int q = i * GRAM_BLOCK + tid;
            double *o = dst + (q / CPR) * GRAM_PITCH + (q % CPR) * VEC;
#pragma unroll
            for (int e = 0; e < VEC; e += 2) {
                D2 v;
                v[0] = (double)st[i][e];
                v[1] = (double)st[i][e + 1];
                *reinterpret_cast<D2 *>(o + e) = v;
            }
        }
    };
    // (WEIGHTED) the weights of the rows this thread parks, staged with the panels, and the weighted parking: w_n a, one rounding
    double wst[NLD] = {};
    auto load_weights = [&](int64_t t0) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            // (no branch around the load and no use of its value before the parking: either would make the wave wait for the chunk's
            // loads BEFORE its MFMA loop.  The index is clamped into the partition, so nothing beyond w[N - 1] is read; a row that does not
            // exist meets elements that are 0 in both operands, and 0 times a finite weight is the 0 a weight of 0 gives.)
            const int64_t row = t0 + (i * GRAM_BLOCK + tid) / CPR;
            if constexpr (WEIGHTED) wst[i] = a.w[row < r_hi ? row : r_hi - 1];
        }
    };
    auto park_weighted = [&](const Vld(&st)[NLD], double *dst) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int q = i * GRAM_BLOCK + tid;
            double *o = dst + (q / CPR) * GRAM_PITCH + (q % CPR) * VEC;
#pragma unroll
            for (int e = 0; e < VEC; e += 2) {
                D2 v;
                v[0] = wst[i] * (double)st[i][e];
                v[1] = wst[i] * (double)st[i][e + 1];
                *reinterpret_cast<D2 *>(o + e) = v;
            }
        }
    };
    // the augmented B operand of a chunk, lane (column c, slot h), step ks: row t0 + 4 ks + h of [b, 1, 0 ... 0]; 0 where the row does not exist
    // (WEIGHTED: and its weighted twin [w b, w, 0 ... 0])
    double augn[GRAM_KC / 4] = {}, aug[GRAM_KC / 4];
    double augwn[GRAM_KC / 4] = {}, augw[GRAM_KC / 4] = {};
    // (INDEXED, WEIGHTED) which of this lane's 4 positions of the chunk load_aug last loaded name an existing row: bit ks for position
    // 4 ks + h.  (The operands of a chunk are made before load_aug runs for the next one.)
    uint32_t amask = 0;
    auto load_aug = [&](int64_t t0) {
        if constexpr (INDEXED) {   // the rows are in arow (fetched for this t0); b at the row, the weight at the position
            if constexpr (WEIGHTED) amask = 0;
#pragma unroll
            for (int ks = 0; ks < GRAM_KC / 4; ++ks) {
                const int64_t pos = t0 + 4 * ks + h;
                const int src = (16 * h + ks) * 4;   // lane (ks, h)
                const int64_t row = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)((uint64_t)arow >> 32)) << 32) |
                                              (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)arow));
                const bool have = pos < r_hi && exists(row);
                if constexpr (WEIGHTED) amask |= have ? 1u << ks : 0u;
                if constexpr (WEIGHTED) {   // loads without branches: b at row 0 where the row does not exist (its value is not used)
                    augn[ks] = (double)a.b[have ? row : 0];
                    augwn[ks] = a.w[pos < r_hi ? pos : r_hi - 1];
                } else {
                    double v = 0.0;
                    if (have) {
                        if (c == 0) v = (double)a.b[row];
                        if (c == 1) v = 1.0;
                    }
                    augn[ks] = v;
                }
            }
            return;
        }
#pragma unroll
        for (int ks = 0; ks < GRAM_KC / 4; ++ks) {
            const int64_t row = t0 + 4 * ks + h;
            if constexpr (WEIGHTED) {   // the raw b_n and w_n by loads without branches (clamped index); the operands are made where they are used
                const int64_t rc = row < r_hi ? row : r_hi - 1;
                augn[ks] = (double)a.b[rc];
                augwn[ks] = a.w[rc];
                continue;
            }
            double v = 0.0;
            if (row < r_hi) {
                if (c == 0) v = (double)a.b[row];
                if (c == 1) v = 1.0;
            }
            augn[ks] = v;
        }
    };

    Acc acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = Acc(0.0);

    if (r_lo < r_hi) {
        if constexpr (INDEXED) fetch_rows(r_lo);
        if constexpr (WEIGHTED) load_weights(r_lo);
        load_panel(stI, ci0, r_lo);
        if (!diag) load_panel(stJ, cj0, r_lo);
        if (augwave) load_aug(r_lo);
        if constexpr (INDEXED) fetch_rows(r_lo + GRAM_KC);
        park_panel(stI, lds);
        if constexpr (WEIGHTED) {
            if (diag)
                park_weighted(stI, lds + PANEL);
            else
                park_weighted(stJ, lds + PANEL);
        } else {
            if (!diag) park_panel(stJ, lds + PANEL);
        }
    }
    __syncthreads();
    int buf = 0;
    for (int64_t t0 = r_lo; t0 < r_hi; t0 += GRAM_KC) {   // (uniform in the workgroup)
        const bool next = t0 + GRAM_KC < r_hi;
#pragma unroll
        for (int ks = 0; ks < GRAM_KC / 4; ++ks) {
            if constexpr (WEIGHTED) {   // [b, 1, 0 ... 0] and [w b, w, 0 ... 0] of row t0 + 4 ks + h from the raw loads of a chunk ago; 0 where the row does not exist
                const bool have = augwave && (INDEXED ? (amask >> ks & 1u) != 0 : t0 + 4 * ks + h < r_hi);
                aug[ks] = have ? (c == 0 ? augn[ks] : c == 1 ? 1.0 : 0.0) : 0.0;
                augw[ks] = have && c < 2 ? augwn[ks] * aug[ks] : 0.0;
            } else {
                aug[ks] = augn[ks];
            }
        }
        if (next) {
            if constexpr (WEIGHTED) load_weights(t0 + GRAM_KC);
            load_panel(stI, ci0, t0 + GRAM_KC);
            if (!diag) load_panel(stJ, cj0, t0 + GRAM_KC);
            if (augwave) load_aug(t0 + GRAM_KC);
        }
        const double *sI = lds + (size_t)buf * 2 * PANEL;
        const double *sJ = (!WEIGHTED && diag) ? sI : sI + PANEL;
        if (!augwave) {
            const double *pI = sI + h * GRAM_PITCH + wi * 64 + c;
            const double *pJ = sJ + h * GRAM_PITCH + wj * 64 + c;
#pragma unroll
            for (int ks = 0; ks < GRAM_KC / 4; ++ks) {
                double av[4], bv[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    av[s] = pI[ks * 4 * GRAM_PITCH + s * 16];
                    bv[s] = pJ[ks * 4 * GRAM_PITCH + s * 16];
                }
#pragma unroll
                for (int si = 0; si < 4; ++si)
#pragma unroll
                    for (int sj = 0; sj < 4; ++sj) acc[si * 4 + sj] = M::mma(av[si], bv[sj], acc[si * 4 + sj]);
            }
        } else {
            const double *pI = sI + h * GRAM_PITCH + c;
#pragma unroll
            for (int ks = 0; ks < GRAM_KC / 4; ++ks) {
                double av[8];
#pragma unroll
                for (int s = 0; s < 8; ++s) av[s] = pI[ks * 4 * GRAM_PITCH + s * 16];
#pragma unroll
                for (int s = 0; s < 8; ++s) acc[s] = M::mma(av[s], WEIGHTED ? augw[ks] : aug[ks], acc[s]);
                acc[8] = M::mma(aug[ks], WEIGHTED ? augw[ks] : aug[ks], acc[8]);
            }
        }
        // the rows of the chunk after the next: used by the next iteration's loads, waited for at the barrier
        if constexpr (INDEXED) fetch_rows(t0 + 2 * GRAM_KC);
        if (next) {
            double *dst = lds + (size_t)(buf ^ 1) * 2 * PANEL;
            park_panel(stI, dst);
            if constexpr (WEIGHTED) {
                if (diag)
                    park_weighted(stI, dst + PANEL);
                else
                    park_weighted(stJ, dst + PANEL);
            } else {
                if (!diag) park_panel(stJ, dst + PANEL);
            }
        }
        __syncthreads();
        buf ^= 1;
    }

    // ---- the workgroup's record.  Accumulator lane (c, h), register q: row M::row(h, q), column c of its 16 x 16 piece.
    double *rec = a.rec + ((size_t)t * a.P + part) * GRAM_REC;
    if (!augwave) {
#pragma unroll
        for (int si = 0; si < 4; ++si)
#pragma unroll
            for (int sj = 0; sj < 4; ++sj)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    rec[(wi * 64 + si * 16 + M::row(h, q)) * GRAM_T + wj * 64 + sj * 16 + c] = acc[si * 4 + sj][q];
    } else {
        if (c < 2) {
            double *o = rec + (c == 0 ? GRAM_OFF_U : GRAM_OFF_CS);
#pragma unroll
            for (int s = 0; s < 8; ++s)
#pragma unroll
                for (int q = 0; q < 4; ++q) o[s * 16 + M::row(h, q)] = acc[s][q];
            // [b, 1]'[b, 1]: row 0 (h = 0, q = 0), column 0: sum b^2; column 1: sum b
            if (h == 0) rec[GRAM_OFF_B + (c == 0 ? 1 : 0)] = acc[8][0];
            // (WEIGHTED) [b, 1]'[w b, w]: row 1 (h = 1, q = 0), column 1: sum w
            if (WEIGHTED && h == 1 && c == 1) rec[GRAM_OFF_B + 2] = acc[8][0];
        }
    }
}

// Workgroups [0, 64 ntiles): 256 elements of a tile each, thread = element (i, j): the P records in partition order, then G[i][j] and
// its mirror from the same sum.  Workgroups [64 ntiles, 64 ntiles + nb): u (threads 0 .. 127) and colsum (128 .. 255) of a column block, from
// the records of its diagonal tile.  The last workgroup: bsum, from the records of tile 0 (Weighted<T>: three sums).  NULL outputs are skipped.
// (T only keeps the two units' copies apart.)
template <typename TT>
__global__ void __launch_bounds__(GRAM_BLOCK) gram_final_kernel(int64_t d, int nb, int ntiles, int P, const double *rec, double *G, int64_t ldg,
                                                                 double *u, double *colsum, double *bsum)
{
    constexpr int NBSUM = GramElem<TT>::weighted ? 3 : 2;   // the weighted statistics: a third slot, sum w
    const int blk = blockIdx.x, tid = threadIdx.x;
    if (blk < ntiles * GRAM_FINAL_BLOCKS) {
        const int t = blk / GRAM_FINAL_BLOCKS, e = (blk % GRAM_FINAL_BLOCKS) * GRAM_BLOCK + tid;
        int ib, jb;
        gram_tile(t, nb, ib, jb);
        const int64_t gi = (int64_t)ib * GRAM_T + e / GRAM_T, gj = (int64_t)jb * GRAM_T + e % GRAM_T;
        if (gi >= d || gj >= d || gi > gj) return;
        const double *q = rec + (size_t)t * P * GRAM_REC + e;
        double s = 0.0;
        for (int p = 0; p < P; ++p) s += q[(size_t)p * GRAM_REC];
        G[gi * ldg + gj] = s;
        if (gi != gj) G[gj * ldg + gi] = s;
    } else if (blk < ntiles * GRAM_FINAL_BLOCKS + nb) {
        const int ib = blk - ntiles * GRAM_FINAL_BLOCKS;
        double *out = tid < GRAM_T ? u : colsum;
        const int64_t col = (int64_t)ib * GRAM_T + (tid & (GRAM_T - 1));
        if (!out || col >= d) return;
        const int t = ib * nb - ib * (ib - 1) / 2;   // the diagonal tile (ib, ib)
        const double *q = rec + (size_t)t * P * GRAM_REC + GRAM_OFF_U + tid;
        double s = 0.0;
        for (int p = 0; p < P; ++p) s += q[(size_t)p * GRAM_REC];
        out[col] = s;
    } else if (bsum && tid < NBSUM) {
        const double *q = rec + GRAM_OFF_B + tid;
        double s = 0.0;
        for (int p = 0; p < P; ++p) s += q[(size_t)p * GRAM_REC];
        bsum[tid] = s;
    }
}

}  // namespace ciao

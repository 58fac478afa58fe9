// mscore_kernels.h -- the per-sample statistics of K models in ONE pass over A (ciao_margin_stats_multi): for every
// iterate x_k, k < K, the four doubles ciao_margin_stats leaves for the row dots a_i'x_k at s = s_k -- without the N x K dots ever
// existing in memory.  Model selection over a regularisation path, folds or restarts: the K-wide form of section 8.7.
//
// Structure: GEMM 1 of mrhs_kernel (mrhs_kernels.h) with mstat_elem (mstat_kernels.h) as its epilogue.
//   grid = (ceil(K / 16) model blocks) x (P row partitions).  A workgroup = 4 waves owns 16 models and a contiguous range of rows and walks
//   it in tiles of 16 rows.  The padded row length DP = 16 SL is split four ways over the waves: wave w owns the columns [w DW, (w+1) DW),
//   DW = 4 SL.  Per tile and wave:
//     1. its 16 x DW piece of the tile comes from global memory a tile ahead, coalesced (consecutive lanes read consecutive 16-byte chunks
//        of a row), and is parked row-major in the wave's own LDS area once the tile before has been read out of that area;
//     2. D_w(16 rows x 16 models) += a[j] (x) z[j], j < SL, on v_mfma_*_16x16x4: lane (row r = l & 15, slot h = l >> 4) reads
//        a[j] = tile[r][h SL + j] from LDS; z[j] = x_model[that column] sits in REGISTERS for the whole kernel;
//     3. the four partial D_w meet in LDS (one barrier per tile, two slots in turn); thread (wave w, model c = l & 15, slot h) takes ONE
//        of the tile's 256 (row, model) pairs -- row(h, w), model c --, adds the four partials in wave order and keeps the dot;
//     4. that dot goes through mstat_elem<T, LOSS> into the thread's MstatAcc while the NEXT tile multiplies: the call stands behind the
//        next tile's MFMAs in program order and depends on none of them, so the double exp / log / log1p run beside the matrix pipe and
//        the row stream instead of after them.
//   At the end the 16 threads of a model are combined in a fixed order (slots by the butterfly 16, 32; then the waves in wave order) and
//   the workgroup writes one record of four doubles per model.  mscore_final_kernel, one workgroup per model, adds the model's P records
//   as mstat_final_kernel adds its own.  No atomics, no scratch, no flags: the hand-off is the kernel boundary.
//
// What is never read: columns [d, ld) of a row, rows outside the partition, x_k beyond d.  Chunks that lie wholly in [0, d) of an existing
// row are 16-byte loads where the base of A and ld allow; everything else is read element by element under its own predicate and what does
// not exist is 0 IN BOTH OPERANDS, so padding that holds NaN never meets a multiply.  The rows a partial last tile lacks are zero and
// their (row, model) pairs are skipped by the epilogue.
//
// Order of addition.  A dot: column w DW + h SL + j in the order of j inside the MFMA's slot h, the four slots by the MFMA, the four waves
// as (0 + 1) + (2 + 3).  A model's sums: thread (w, h) adds the rows row(h, w), 16 + row(h, w), ... of the partition in order; slots,
// waves, partitions as above.  All of it is a function of (N, d, T) alone: not of K, of the model's place in the list (a column of an
// MFMA is computed from its own column of B only), of the other iterates, of the device or of any alignment.
//
// The row-list instantiations (ciao_margin_stats_multi_rows): mscore_partial_kernel<MscoreRows<T>, SL, LOSS> is the
// same kernel text over a LIST of rows, a.idx = M int64 row numbers (or NULL: position = row), written the way
// gram_partial_kernel<Indexed<...>> was.  List position m plays the part of the row number everywhere: a.N = M, the plan is mscore_parts(M) /
// mscore_part_rows(M), partitions are ranges of positions.  Two addresses change: the tile row of position m is row idx[m] of A, and b is
// read at idx[m].  Records, mscore_final_kernel and the order of addition are the ones above, so the outputs are the bits of the call
// without a list on the gathered copy A[idx], b[idx].
//   A tile's 16 entries live in ONE register pair of the wave: lane l holds the entry of position t0 + (l & 15), or -1 where the position
// lies beyond the partition or the entry names no row of A.  The lane that loads chunk q takes the entry of tile row q / CPR from a lane
// that holds it (a scalar read where a wave's 64 chunks lie in one row).  The entries of a tile are requested one whole tile ahead of the
// row loads that use them -- those of the tile after next when the next tile's row loads are issued -- so the two-halves staging never
// waits on an index.  Positions are clamped into the partition (nothing beyond idx[M - 1] is read); row offsets are formed in int64.
//   An entry outside [0, rows) issues no load, its row is zero in the tile and its (row, model) pairs are SKIPPED by the epilogue, as a
// partial tile's missing rows are; the 16-byte fast path of a tile needs all 16 entries valid.
//   a.off (K doubles, or NULL): model k's per-sample terms see (double)dot + off[k] -- one double addition, the intercept of a fitted
// model.  With off = NULL no addition is made at all: the bits of the kernel above, signed zeros included.
#pragma once

#include <type_traits>

#include "mstat_kernels.h"

namespace ciao {

constexpr int MSCORE_TILE = 16;           // rows per tile = MFMA rows
constexpr int MSCORE_KB = 16;             // models per workgroup = MFMA columns
constexpr int MSCORE_BLOCK = 256;         // four waves
constexpr int MSCORE_PART_TARGET = 2048;  // row partitions at most (8 per CU, as colsq / rowsq): one model block alone fills the machine
constexpr int MSCORE_MAX_D = 1024;        // 16 models' iterates in the registers of one workgroup
constexpr int MSCORE_MAX_K = 256;
constexpr int MSCORE_REC = 4;             // doubles per (workgroup, model) record

// rows of one partition: whole tiles, a pure function of N
__host__ __device__ inline int64_t mscore_part_rows(int64_t N)
{
    const int64_t per = (N + MSCORE_PART_TARGET - 1) / MSCORE_PART_TARGET;
    const int64_t t = (per + MSCORE_TILE - 1) / MSCORE_TILE * MSCORE_TILE;
    return t < MSCORE_TILE ? MSCORE_TILE : t;
}
__host__ __device__ inline int mscore_parts(int64_t N)
{
    const int64_t per = mscore_part_rows(N);
    return (int)((N + per - 1) / per);
}
// MFMA steps per wave and slot: the padded row length is 16 SL
__host__ __device__ inline int mscore_sl(int64_t d) { return d <= 64 ? 4 : d <= 256 ? 16 : d <= 512 ? 32 : 64; }

// the tag of the row-list instantiations, and what a kernel's first template argument says
template <typename T>
struct MscoreRows {};
template <typename TT>
struct MscoreElem {
    using type = TT;
    static constexpr bool rows = false;
};
template <typename T>
struct MscoreElem<MscoreRows<T>> {
    using type = T;
    static constexpr bool rows = true;
};

template <typename T>
struct MscoreArgs {
    const T *A;
    const T *b;
    int64_t ld, N, d;
    int64_t per;             // rows per partition
    int P;                   // row partitions
    int nkb;                 // model blocks = ceil(K / 16); the grid is 8 nkb ceil(P / 8)
    int K;                   // models (the last block's missing ones multiply zeros and are never reported)
    int vec16;               // the base of A and ld are multiples of 16 bytes
    const T *const *x;       // K device pointers, 16-byte aligned
    const double *s;         // K dual scalings
    double *rec;             // [model blocks][P][16][MSCORE_REC]
};

template <typename T>
struct MscoreArgs<MscoreRows<T>> : MscoreArgs<T> {   // N = M, the length of the list
    const int64_t *idx;   // M row numbers, 8-byte aligned, or NULL: position = row
    int64_t rows;         // the rows A has: an entry outside [0, rows) is a row that does not exist
    const double *off;    // K offsets, or NULL: none is added
};

template <typename T, int SL>
constexpr size_t mscore_lds_bytes()
{
    // per wave: its 16 x (4 SL) piece of a tile with padded rows; then the exchange area: 2 slots x 4 waves x 4 values x 64 lanes
    return (size_t)4 * MSCORE_TILE * (4 * SL + 16 / sizeof(T)) * sizeof(T) + (size_t)2 * 4 * 4 * WAVE * sizeof(T);
}

template <typename TT, int SL, int LOSS>
__global__ void __launch_bounds__(MSCORE_BLOCK) mscore_partial_kernel(MscoreArgs<TT> a)
{
    using T = typename MscoreElem<TT>::type;
    constexpr bool ROWS = MscoreElem<TT>::rows;
    using M = MfmaOf<T>;
    using Acc = typename M::acc;
    constexpr int VEC = 16 / (int)sizeof(T);
    typedef T Vld __attribute__((ext_vector_type(VEC)));
    constexpr int DW = 4 * SL;                      // columns per wave
    constexpr int PITCH = DW + VEC;                 // padded LDS row (elements)
    constexpr int CPR = DW / VEC;                   // 16-byte chunks of a row of the wave's piece
    constexpr int NLD = MSCORE_TILE * CPR / WAVE;   // chunks per lane and tile
    static_assert(SL % VEC == 0 && NLD >= 1 && NLD * WAVE == MSCORE_TILE * CPR, "tile layout");
    static_assert(4 * MSCORE_KB * MSCORE_REC * sizeof(double) <= (size_t)2 * 4 * 4 * WAVE * sizeof(T), "the final combine reuses the exchange area");
    extern __shared__ __attribute__((aligned(16))) unsigned char mscore_raw[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r = lane & 15, h = lane >> 4;
    T *tile = reinterpret_cast<T *>(mscore_raw) + (size_t)w * MSCORE_TILE * PITCH;
    T *xch = reinterpret_cast<T *>(mscore_raw) + (size_t)4 * MSCORE_TILE * PITCH;   // [2][4 waves][4 regs][64 lanes]

    // blockIdx -> (row partition, model block): the model blocks of one partition are consecutive slots of ONE XCD (workgroups go to XCDs
    // round-robin by blockIdx), so they read the same tiles at about the same time through one L2 -- spread over the XCDs, a tile came
    // from HBM once per XCD (K = 256, fp64, d = 1024: 203 ms; with this map: CHANGELOG).  Which workgroup takes which pair changes no result.
    const int nkb = a.nkb;
    const int part = (blockIdx.x & 7) + 8 * (int)((blockIdx.x >> 3) / nkb), kb = (int)((blockIdx.x >> 3) % nkb);
    if (part >= a.P) return;   // (the grid covers the partitions rounded up to a multiple of 8; uniform in the workgroup)
    const int64_t r_lo = (int64_t)part * a.per;
    const int64_t r_hi = r_lo + a.per < a.N ? r_lo + a.per : a.N;
    const int model = kb * MSCORE_KB + r;

    // the iterates of this block's 16 models, as the B operand: lane (model c = r, slot h), step j: x_c[w DW + h SL + j]; 0 beyond d and
    // for a model that does not exist
    T z[SL];
    {
        const int col0 = w * DW + h * SL;
        const T *xc = nullptr;
        if (model < a.K) {
            xc = a.x[model];
            xc = (const T *)(const __attribute__((address_space(1))) T *)(uintptr_t)xc;   // global memory, not generic (mrhs_kernels.h)
        }
#pragma unroll
        for (int j = 0; j < SL; j += VEC) {
            if (xc && col0 + j + VEC <= a.d) {
                const Vld v = *reinterpret_cast<const Vld *>(xc + col0 + j);
#pragma unroll
                for (int e = 0; e < VEC; ++e) z[j + e] = v[e];
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) z[j + e] = (xc && col0 + j + e < a.d) ? xc[col0 + j + e] : T(0);
            }
        }
    }
    const double s = model < a.K ? a.s[model] : 1.0;
    // (ROWS) the model's offset; has_off is uniform in the grid
    double off = 0.0;
    bool has_off = false;
    if constexpr (ROWS) {
        has_off = a.off != nullptr;
        if (has_off && model < a.K) off = a.off[model];
    }
    // (ROWS) the 16 entries of the tile at t0 (t0 < r_hi): lane l holds the row of position t0 + (l & 15), -1 where there is none
    auto entries = [&](int64_t t0) -> int64_t {
        int64_t v = -1;
        if constexpr (ROWS) {
            const int64_t pos = t0 + r;
            const int64_t pc = pos < r_hi ? pos : r_hi - 1;
            const int64_t e = a.idx ? a.idx[pc] : pc;
            v = (pos < r_hi && (uint64_t)e < (uint64_t)a.rows) ? e : -1;
        }
        return v;
    };
    auto entry_of = [&](int64_t ent, int row) -> int64_t {   // the entry of tile row `row`, from a lane that holds it
        return (int64_t)__shfl((long long)ent, row, WAVE);
    };

    // The wave's 16 x DW piece of the tile at t0, staged in registers: chunk q = 64 i + lane is chunk q % CPR of row q / CPR.  It travels in
    // two halves (i below / from NLD / 2: the upper and the lower rows), so that the loads of the tile after next for the first half are in
    // flight while the second half of the next tile is awaited: the memory queue of the CU never runs empty.
    Vld st[NLD];
    auto load_half = [&](auto half_tag, int64_t t0, int64_t ent) {   // ent (ROWS): entries(t0)
        constexpr int I0 = decltype(half_tag)::value == 0 ? 0 : NLD / 2, I1 = decltype(half_tag)::value == 0 ? NLD / 2 : NLD;
        if constexpr (ROWS) {
            const bool whole = a.vec16 && (int64_t)(w + 1) * DW <= a.d && __all(ent >= 0);   // (uniform in the wave)
#pragma unroll
            for (int i = I0; i < I1; ++i) {
                const int q = i * WAVE + lane;
                int64_t row;
                if constexpr (CPR >= WAVE) {   // the wave's 64 chunks of one load lie in one row: a scalar read
                    constexpr int CPW = CPR / WAVE;
                    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)ent, i / CPW);
                    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)ent >> 32), i / CPW);
                    row = (int64_t)(((uint64_t)hi << 32) | lo);
                } else {
                    row = entry_of(ent, q / CPR);
                }
                const int64_t col = w * DW + (q % CPR) * VEC;
                const T *src = a.A + row * a.ld + col;   // (not formed into an access where row is -1)
                if (whole || (a.vec16 && row >= 0 && col + VEC <= a.d)) {
                    st[i] = __builtin_nontemporal_load(reinterpret_cast<const Vld *>(src));
                } else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) st[i][e] = (row >= 0 && col + e < a.d) ? __builtin_nontemporal_load(src + e) : T(0);
                }
            }
            return;
        }
        const bool whole = a.vec16 && t0 + MSCORE_TILE <= r_hi && (int64_t)(w + 1) * DW <= a.d;   // (uniform in the wave)
        if (whole) {
#pragma unroll
            for (int i = I0; i < I1; ++i) {
                const int q = i * WAVE + lane;
                st[i] = __builtin_nontemporal_load(reinterpret_cast<const Vld *>(a.A + (t0 + q / CPR) * a.ld + (w * DW + (q % CPR) * VEC)));
            }
        } else {
#pragma unroll
            for (int i = I0; i < I1; ++i) {
                const int q = i * WAVE + lane;
                const int64_t row = t0 + q / CPR;
                const int64_t col = w * DW + (q % CPR) * VEC;
                const T *src = a.A + row * a.ld + col;
                if (a.vec16 && row < r_hi && col + VEC <= a.d) {
                    st[i] = __builtin_nontemporal_load(reinterpret_cast<const Vld *>(src));
                } else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) st[i][e] = (row < r_hi && col + e < a.d) ? __builtin_nontemporal_load(src + e) : T(0);
                }
            }
        }
    };
    auto park_half = [&](auto half_tag) {
        constexpr int I0 = decltype(half_tag)::value == 0 ? 0 : NLD / 2, I1 = decltype(half_tag)::value == 0 ? NLD / 2 : NLD;
#pragma unroll
        for (int i = I0; i < I1; ++i) {
            const int q = i * WAVE + lane;
            *reinterpret_cast<Vld *>(tile + (q / CPR) * PITCH + (q % CPR) * VEC) = st[i];
        }
    };
    constexpr std::integral_constant<int, 0> H0{};
    constexpr std::integral_constant<int, 1> H1{};

    // this thread's (row, model) pair of a tile: row(h, w) -- register w of the accumulator layout -- and model c = r
    const int myrow = M::row(h, w);
    MstatAcc acc;
    acc.m = LOSS == CIAO_LOSS_LOGISTIC ? -__builtin_inf() : 0.0;
    T pend = T(0), bpend = T(0), bq = T(0);
    bool pvalid = false;
    int par = 0;
    // (ROWS) e1, e2: the entries of the next tile and of the tile after next, -1 in every lane where there is no such tile; vq: this
    // thread's pair of the tile whose label is in bq exists
    int64_t e1 = -1, e2 = -1;
    bool vq = false;

    if (r_lo < r_hi) {
        const int64_t e0 = entries(r_lo);
        if constexpr (ROWS) {
            if (r_lo + MSCORE_TILE < r_hi) e1 = entries(r_lo + MSCORE_TILE);
            if (r_lo + 2 * MSCORE_TILE < r_hi) e2 = entries(r_lo + 2 * MSCORE_TILE);
        }
        load_half(H0, r_lo, e0);
        load_half(H1, r_lo, e0);
        if constexpr (ROWS) {
            const int64_t eb = entry_of(e0, myrow);
            vq = eb >= 0;
            if (vq) bq = a.b[eb];
        } else {
            if (r_lo + myrow < r_hi) bq = a.b[r_lo + myrow];
        }
        park_half(H0);
        park_half(H1);
        if (r_lo + MSCORE_TILE < r_hi) {
            load_half(H0, r_lo + MSCORE_TILE, e1);
            load_half(H1, r_lo + MSCORE_TILE, e1);
        }
    }
    for (int64_t t0 = r_lo; t0 < r_hi; t0 += MSCORE_TILE) {   // (uniform in the workgroup)
        const bool next1 = t0 + MSCORE_TILE < r_hi, next2 = t0 + 2 * MSCORE_TILE < r_hi;
        T bn = T(0);
        bool vn = false;
        if constexpr (ROWS) {
            const int64_t eb = entry_of(e1, myrow);
            vn = eb >= 0;
            if (vn) bn = a.b[eb];
        } else {
            if (t0 + MSCORE_TILE + myrow < r_hi) bn = a.b[t0 + MSCORE_TILE + myrow];
        }
        // ---- GEMM 1: this wave's share of the 16 x 16 row dots, sixteen bytes per LDS read: lane (row r, slot h), step j: tile[r][h SL + j]
        Acc D = Acc(T(0));
        {
            const T *trow = tile + r * PITCH + h * SL;
#pragma unroll
            for (int j = 0; j < SL; j += VEC) {
                const Vld av = *reinterpret_cast<const Vld *>(trow + j);
#pragma unroll
                for (int e = 0; e < VEC; ++e) D = M::mma(av[e], z[j + e], D);
            }
        }
        // ---- behind those reads (a wave's LDS operations execute in order: no barrier) the next tile takes this one's place in the wave's
        // own LDS area, half by half, and each half of the tile after next is requested as soon as its registers are free
        if (next1) {
            park_half(H0);
            if (next2) load_half(H0, t0 + 2 * MSCORE_TILE, e2);
            park_half(H1);
            if (next2) load_half(H1, t0 + 2 * MSCORE_TILE, e2);
        }
        if constexpr (ROWS) {   // the entries of the tile after the one whose row loads were just issued: first used one iteration from here
            e1 = e2;
            e2 = t0 + 3 * MSCORE_TILE < r_hi ? entries(t0 + 3 * MSCORE_TILE) : -1;
        }
        // ---- the tile before: its dot through the per-sample terms, beside the MFMAs above
        if (pvalid) {
            if constexpr (ROWS)
                mstat_elem_d<LOSS>(acc, s, (double)bpend, has_off ? (double)pend + off : (double)pend);
            else
                mstat_elem<T, LOSS>(acc, s, pend, bpend);
        }
        // ---- the four partial D through LDS; every thread adds the partials of its own pair in wave order
        T *slot = xch + (size_t)par * 4 * 4 * WAVE;
#pragma unroll
        for (int q = 0; q < 4; ++q) slot[(w * 4 + q) * WAVE + lane] = D[q];
        __syncthreads();
        pend = (slot[(0 * 4 + w) * WAVE + lane] + slot[(1 * 4 + w) * WAVE + lane]) + (slot[(2 * 4 + w) * WAVE + lane] + slot[(3 * 4 + w) * WAVE + lane]);
        par ^= 1;
        pvalid = ROWS ? vq : t0 + myrow < r_hi;
        bpend = bq;
        bq = bn;
        vq = vn;
    }
    if (pvalid) {
        if constexpr (ROWS)
            mstat_elem_d<LOSS>(acc, s, (double)bpend, has_off ? (double)pend + off : (double)pend);
        else
            mstat_elem<T, LOSS>(acc, s, pend, bpend);
    }

    // ---- the workgroup's record: the four slots of a model inside a wave (distances 16, 32: every lane ends with the same bits), then
    // the four waves in wave order through LDS
#pragma unroll
    for (int dist = 16; dist <= 32; dist <<= 1) {
        acc.a0 += __shfl_xor(acc.a0, dist, WAVE);
        acc.a1 += __shfl_xor(acc.a1, dist, WAVE);
        acc.a2 += __shfl_xor(acc.a2, dist, WAVE);
        acc.m = fmax2(acc.m, __shfl_xor(acc.m, dist, WAVE));
    }
    __syncthreads();   // the last tile's exchange has been read by everyone
    double *comb = reinterpret_cast<double *>(xch);   // [4 waves][16 models][4]
    if (h == 0) {
        double *o = comb + (w * MSCORE_KB + r) * MSCORE_REC;
        o[0] = acc.a0;
        o[1] = acc.a1;
        o[2] = acc.a2;
        o[3] = acc.m;
    }
    __syncthreads();
    if (threadIdx.x < MSCORE_KB) {
        const double *o = comb + r * MSCORE_REC;
        double a0 = o[0], a1 = o[1], a2 = o[2], m = o[3];
        for (int ww = 1; ww < 4; ++ww) {
            const double *q = comb + (ww * MSCORE_KB + r) * MSCORE_REC;
            a0 += q[0];
            a1 += q[1];
            a2 += q[2];
            m = fmax2(m, q[3]);
        }
        double *out = a.rec + (((size_t)kb * a.P + part) * MSCORE_KB + r) * MSCORE_REC;
        out[0] = a0;
        out[1] = a1;
        out[2] = a2;
        out[3] = m;
    }
}

// workgroup k: model k's P records in partition order -- thread t adds the records t, t + 256, ... in index order, then the fixed-order
// combine of mstat_final_kernel; out[4k .. 4k + 4)
template <typename T, int LOSS>
__global__ void __launch_bounds__(CERT_BLOCK) mscore_final_kernel(int P, const double *rec, double *out)
{
    __shared__ double lds[CERT_BLOCK / WAVE][4];
    const int k = blockIdx.x, kb = k / MSCORE_KB, c = k % MSCORE_KB;
    MstatAcc acc;
    acc.m = LOSS == CIAO_LOSS_LOGISTIC ? -__builtin_inf() : 0.0;
    for (int i = threadIdx.x; i < P; i += CERT_BLOCK) {
        const double *q = rec + (((size_t)kb * P + i) * MSCORE_KB + c) * MSCORE_REC;
        acc.a0 += q[0];
        acc.a1 += q[1];
        acc.a2 += q[2];
        acc.m = fmax2(acc.m, q[3]);
    }
    mstat_block_combine(acc, lds);
    if (threadIdx.x == 0) {
        double *o = out + (size_t)k * 4;
        o[0] = acc.a0;
        o[1] = acc.a1;
        o[2] = acc.a2;
        o[3] = LOSS == CIAO_LOSS_LOGISTIC ? -acc.m : acc.m;
    }
}

}  // namespace ciao

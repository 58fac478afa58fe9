// rowsq_kernels.h -- row sums of squares and their summary (ciao_row_sqnorms): the per-sample smoothness
// constants L_i = lam ||a_i||^2 (LeastSquares) / ||a_i||^2 / 4 (logistic) of a packed matrix, from which every step size is derived.
//
// out[i] = sum_j A[i,j]^2 for the N resident rows: ONE pass over A, every element read once, 16-byte non-temporal loads, squares formed
// and added in double ((double)a * (double)a: exact for fp32 input).  Beside the N-vector (which may be absent) rowsq_partial_kernel
// leaves one record per workgroup -- max, the smallest row index attaining it, min, sum over the workgroup's rows -- and
// rowsq_final_kernel, one workgroup, combines the records in workgroup order.  No atomics, no scratch, no flags: the hand-off is the
// kernel boundary (ciao_common.h: the per-XCD L2s are not coherent with each other).
//
// The ORDER OF ADDITION of a row is a function of d alone, that of the summary a function of (N, d) alone (rowsq_plan):
//   * a row is cut into 16-byte chunks (VEC = 16 / sizeof(T) columns, the last one possibly partial); the squares of a chunk are added
//     in column order;
//   * a row belongs to a group of G lanes of one wave, G = the power of two that covers the row's chunks, 64 at most, so that a wave
//     holds 64 / G rows side by side; lane g of the group takes the chunks g, g + G, g + 2G, ...;
//   * a lane adds its chunks into ROWSQ_U slots, chunk number k (counted per lane) into slot k mod ROWSQ_U, each slot in the order of
//     k; then the slots in the order 0, 1, ... (a row of up to 64 ROWSQ_U chunks: simply the lane's chunks in order).  ROWSQ_U chunks
//     are in flight per lane; rows of few chunks per lane fill the slots with several rows (mode 0..2: 8, 4, 2 rows per group);
//   * the G lanes are combined by a butterfly of the fixed distances G/2, ..., 2, 1;
//   * a row beyond ROWSQ_SPLIT_CHUNKS chunks (64 KiB) is taken by the four waves of the workgroup as four contiguous quarters (whole
//     multiples of 64 chunks), each as above, the four results added in wave order through LDS.
// Where the base of A or ld is not a multiple of 16 bytes (and in the partial last chunk) the same lane reads the same columns element
// by element: which lane adds which element in which order -- and with it every bit of the result -- is the same for every layout of
// the same matrix.  A chunk or a row that does not exist contributes +0.0, which changes no bit of a sum of squares.
//
// A workgroup takes a contiguous block of rows_per_wg rows, so the records are in row order.  The summary treats NaN as the largest
// and the smallest value: a NaN in any row makes max, min and sum NaN and argmax the first such row.
#pragma once

#include "cert_ws.h"   // ROWSQ_WG_TARGET, ROWSQ_REC
#include "ciao_common.h"

namespace ciao {

constexpr int ROWSQ_BLOCK = 256;                 // threads of both kernels: four waves
constexpr int ROWSQ_WAVES = ROWSQ_BLOCK / WAVE;
constexpr int ROWSQ_U = 8;                       // 16-byte chunks in flight per lane = slots of a lane's sum
constexpr int64_t ROWSQ_SPLIT_CHUNKS = 4096;     // rows beyond this many chunks (64 KiB): the four waves share a row
constexpr int ROWSQ_MODE_SPLIT = 4;

struct RowsqPlan {
    int g_log2;            // lanes of a row's group = 1 << g_log2
    int mode;              // 0..2: (1, 2, 4) chunks per lane and row, (8, 4, 2) rows per group at once; 3: a wave per row, any length;
                           // ROWSQ_MODE_SPLIT: a workgroup per row
    int64_t quarter;       // split mode: chunks of a wave's quarter (a whole multiple of 64)
    int64_t rows_per_wg;   // contiguous rows of a workgroup: a whole multiple of the rows it takes per iteration
    int64_t grid;          // workgroups = records
};

// vec = elements of a 16-byte chunk (4 fp32, 2 fp64)
__host__ __device__ inline RowsqPlan rowsq_plan(int64_t N, int64_t d, int vec)
{
    RowsqPlan pl;
    const int64_t chunks = (d + vec - 1) / vec;
    int64_t step;
    pl.quarter = 0;
    if (chunks > ROWSQ_SPLIT_CHUNKS) {
        pl.g_log2 = 6;
        pl.mode = ROWSQ_MODE_SPLIT;
        pl.quarter = ((chunks + ROWSQ_WAVES - 1) / ROWSQ_WAVES + WAVE - 1) / WAVE * WAVE;
        step = 1;
    } else {
        pl.g_log2 = 0;
        while (pl.g_log2 < 6 && ((int64_t)1 << pl.g_log2) < chunks) ++pl.g_log2;
        const int64_t trips = (chunks + ((int64_t)1 << pl.g_log2) - 1) >> pl.g_log2;   // chunks per lane: 1 unless the group is a whole wave
        pl.mode = trips <= 1 ? 0 : trips <= 2 ? 1 : trips <= 4 ? 2 : 3;
        step = (int64_t)ROWSQ_WAVES * (ROWSQ_U >> pl.mode) * (WAVE >> pl.g_log2);
    }
    int64_t per = (N + ROWSQ_WG_TARGET - 1) / ROWSQ_WG_TARGET;
    per = (per + step - 1) / step * step;
    if (per < step) per = step;
    pl.rows_per_wg = per;
    pl.grid = (N + per - 1) / per;
    if (pl.grid < 1) pl.grid = 1;
    return pl;
}

// ---- the summary: (max, argmax, min, sum) ---------------------------------------------------------------------------------------------
struct RowsqStat {
    double mx, arg, mn, sum;   // arg: a row index, exact as a double
};
__device__ __forceinline__ RowsqStat rowsq_stat_none()
{
    RowsqStat s;
    s.mx = -__builtin_huge_val();
    s.arg = __builtin_huge_val();
    s.mn = __builtin_huge_val();
    s.sum = 0.0;
    return s;
}
// a (+) b: b's sum is added to a's; the larger maximum wins, a NaN beats every number, equal maxima (two NaNs too) keep the smaller index
__device__ __forceinline__ void rowsq_stat_merge(RowsqStat &a, const RowsqStat &b)
{
    const bool an = a.mx != a.mx, bn = b.mx != b.mx;
    const bool take = an ? (bn && b.arg < a.arg) : (bn || b.mx > a.mx || (b.mx == a.mx && b.arg < a.arg));
    a.mx = take ? b.mx : a.mx;
    a.arg = take ? b.arg : a.arg;
    a.mn = (a.mn != a.mn) ? a.mn : ((b.mn != b.mn || b.mn < a.mn) ? b.mn : a.mn);
    a.sum += b.sum;
}
__device__ __forceinline__ void rowsq_stat_add(RowsqStat &a, double v, int64_t row)
{
    RowsqStat b;
    b.mx = v;
    b.arg = (double)row;
    b.mn = v;
    b.sum = v;
    rowsq_stat_merge(a, b);
}
// the 256 threads' summaries -> one, valid in thread 0: a butterfly of the distances 32 ... 1 inside a wave (every lane ends with the
// same bits: the merge is symmetric), then the four waves in wave order through LDS.  All 256 threads call it.
__device__ __forceinline__ void rowsq_stat_block(RowsqStat &s, double (*lds)[4])
{
#pragma unroll
    for (int dist = WAVE / 2; dist > 0; dist >>= 1) {
        RowsqStat o;
        o.mx = __shfl_xor(s.mx, dist, WAVE);
        o.arg = __shfl_xor(s.arg, dist, WAVE);
        o.mn = __shfl_xor(s.mn, dist, WAVE);
        o.sum = __shfl_xor(s.sum, dist, WAVE);
        rowsq_stat_merge(s, o);
    }
    const int wave = (int)threadIdx.x >> 6;
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        lds[wave][0] = s.mx;
        lds[wave][1] = s.arg;
        lds[wave][2] = s.mn;
        lds[wave][3] = s.sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < ROWSQ_WAVES; ++w) {
            RowsqStat o;
            o.mx = lds[w][0];
            o.arg = lds[w][1];
            o.mn = lds[w][2];
            o.sum = lds[w][3];
            rowsq_stat_merge(s, o);
        }
    }
}

// ---- a chunk ---------------------------------------------------------------------------------------------------------------------------
// v = the VEC columns of chunk c of the row at rowp; live: the row and the chunk exist.  One 16-byte load where the layout allows it and
// the chunk is whole (c < full = d / VEC); otherwise the columns below d one by one; what does not exist is 0.
template <typename T, bool VEC16>
__device__ __forceinline__ void rowsq_load(const T *rowp, int64_t c, int64_t full, int64_t d, bool live, T (&v)[16 / sizeof(T)])
{
    constexpr int VEC = 16 / (int)sizeof(T);
    typedef T VecT __attribute__((ext_vector_type(VEC)));
    const int64_t col = c * VEC;
    if (VEC16 && live && c < full) {
        const VecT t = __builtin_nontemporal_load(reinterpret_cast<const VecT *>(rowp + col));
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = t[j];
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = (live && col + j < d) ? __builtin_nontemporal_load(rowp + col + j) : T(0);
    }
}
// the squares of a chunk, added in column order
template <typename T>
__device__ __forceinline__ double rowsq_chunk(const T (&v)[16 / sizeof(T)])
{
    constexpr int VEC = 16 / (int)sizeof(T);
    double q = (double)v[0] * (double)v[0];
#pragma unroll
    for (int j = 1; j < VEC; ++j) q += (double)v[j] * (double)v[j];
    return q;
}
// the butterfly over a group of 1 << g_log2 lanes: distances G/2 ... 1 (all 64 lanes active; every lane of a group ends with the same bits)
__device__ __forceinline__ double rowsq_group_sum(double s, int g_log2)
{
    for (int dist = (1 << g_log2) >> 1; dist > 0; dist >>= 1) s += __shfl_xor(s, dist, WAVE);
    return s;
}

// modes 0..2: rows of at most TP = 1 << TPL chunks per lane, RB = ROWSQ_U / TP rows per group at once.  Wave w of the workgroup takes the
// rows lo + (4 it + w) RB R + r R + group, R = 64 / G groups per wave, r < RB.
template <typename T, bool VEC16, int TPL>
__device__ __forceinline__ void rowsq_short_rows(const T *A, int64_t d, int64_t ld, int64_t lo, int64_t hi, int g_log2, double *out, RowsqStat &st)
{
    constexpr int VEC = 16 / (int)sizeof(T), U = ROWSQ_U, TP = 1 << TPL, RB = U / TP;
    const int lane = (int)threadIdx.x & (WAVE - 1), wave = (int)threadIdx.x >> 6;
    const int R = WAVE >> g_log2;
    const int g = lane & ((1 << g_log2) - 1), grp = lane >> g_log2;
    const int64_t chunks = (d + VEC - 1) / VEC, full = d / VEC;
    const int64_t per_wave = (int64_t)RB * R;
    for (int64_t base = lo + wave * per_wave; base < hi; base += ROWSQ_WAVES * per_wave) {   // (uniform in the wave)
        T v[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = base + (int64_t)(u / TP) * R + grp;
            const int64_t c = g + ((int64_t)(u % TP) << g_log2);
            rowsq_load<T, VEC16>(A + row * ld, c, full, d, row < hi && c < chunks, v[u]);
        }
        double s[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            s[r] = rowsq_chunk<T>(v[r * TP]);
#pragma unroll
            for (int k = 1; k < TP; ++k) s[r] += rowsq_chunk<T>(v[r * TP + k]);
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) s[r] = rowsq_group_sum(s[r], g_log2);
        if (g == 0) {
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int64_t row = base + (int64_t)r * R + grp;
                if (row < hi) {
                    if (out) out[row] = s[r];
                    rowsq_stat_add(st, s[r], row);
                }
            }
        }
    }
}

// the chunks c0 + lane, c0 + lane + 64, ... below c1 of one row, by one wave: slots, then the butterfly over the 64 lanes
template <typename T, bool VEC16>
__device__ __forceinline__ double rowsq_wave_span(const T *rowp, int64_t c0, int64_t c1, int64_t full, int64_t d)
{
    constexpr int VEC = 16 / (int)sizeof(T), U = ROWSQ_U;
    const int lane = (int)threadIdx.x & (WAVE - 1);
    double slot[U];
#pragma unroll
    for (int u = 0; u < U; ++u) slot[u] = 0.0;
    for (int64_t cb = c0; cb < c1; cb += (int64_t)U * WAVE) {   // (uniform in the wave)
        T v[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t c = cb + (int64_t)u * WAVE + lane;
            rowsq_load<T, VEC16>(rowp, c, full, d, c < c1, v[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) slot[u] += rowsq_chunk<T>(v[u]);
    }
    double s = slot[0];
#pragma unroll
    for (int u = 1; u < U; ++u) s += slot[u];
    return rowsq_group_sum(s, 6);
}

// out[i] for the rows [blockIdx.x * rows_per_wg, ...) and the workgroup's record.  VEC16: the base of A and ld are multiples of 16 bytes.
template <typename T, bool VEC16>
__global__ void __launch_bounds__(ROWSQ_BLOCK)
    rowsq_partial_kernel(const T *A, int64_t N, int64_t d, int64_t ld, int64_t rows_per_wg, int g_log2, int mode, int64_t quarter, double *out,
                         double *rec)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    __shared__ double lds[ROWSQ_WAVES][4];
    __shared__ double quarters[ROWSQ_WAVES];
    const int64_t lo = (int64_t)blockIdx.x * rows_per_wg;
    const int64_t hi = lo + rows_per_wg < N ? lo + rows_per_wg : N;
    const int lane = (int)threadIdx.x & (WAVE - 1), wave = (int)threadIdx.x >> 6;
    const int64_t chunks = (d + VEC - 1) / VEC, full = d / VEC;
    RowsqStat st = rowsq_stat_none();
    if (mode == 0) {
        rowsq_short_rows<T, VEC16, 0>(A, d, ld, lo, hi, g_log2, out, st);
    } else if (mode == 1) {
        rowsq_short_rows<T, VEC16, 1>(A, d, ld, lo, hi, g_log2, out, st);
    } else if (mode == 2) {
        rowsq_short_rows<T, VEC16, 2>(A, d, ld, lo, hi, g_log2, out, st);
    } else if (mode == 3) {
        for (int64_t row = lo + wave; row < hi; row += ROWSQ_WAVES) {
            const double s = rowsq_wave_span<T, VEC16>(A + row * ld, 0, chunks, full, d);
            if (lane == 0) {
                if (out) out[row] = s;
                rowsq_stat_add(st, s, row);
            }
        }
    } else {
        const int64_t c0 = wave * quarter;
        const int64_t c1 = c0 + quarter < chunks ? c0 + quarter : chunks;
        for (int64_t row = lo; row < hi; ++row) {   // (uniform in the workgroup)
            const double s = rowsq_wave_span<T, VEC16>(A + row * ld, c0, c1, full, d);
            if (lane == 0) quarters[wave] = s;
            __syncthreads();
            if (threadIdx.x == 0) {
                double t = quarters[0];
                for (int w = 1; w < ROWSQ_WAVES; ++w) t += quarters[w];
                if (out) out[row] = t;
                rowsq_stat_add(st, t, row);
            }
            __syncthreads();
        }
    }
    rowsq_stat_block(st, lds);
    if (threadIdx.x == 0) {
        double *r = rec + (int64_t)blockIdx.x * ROWSQ_REC;
        r[0] = st.mx;
        r[1] = st.arg;
        r[2] = st.mn;
        r[3] = st.sum;
    }
}

// one workgroup: thread t merges the records t, t + 256, ... in index order, then the same fixed-order combine; res[0..4) = max, argmax,
// min, sum.  (A template on T although it reads doubles only, as colsq_final_kernel and screen_count_kernel are: this header is compiled
// into one unit per element type, and a plain __global__ function would be defined in both.)
template <typename T>
__global__ void __launch_bounds__(ROWSQ_BLOCK) rowsq_final_kernel(int nrec, const double *rec, double *res)
{
    __shared__ double lds[ROWSQ_WAVES][4];
    RowsqStat st = rowsq_stat_none();
    for (int i = threadIdx.x; i < nrec; i += ROWSQ_BLOCK) {
        const double *r = rec + (int64_t)i * ROWSQ_REC;
        RowsqStat o;
        o.mx = r[0];
        o.arg = r[1];
        o.mn = r[2];
        o.sum = r[3];
        rowsq_stat_merge(st, o);
    }
    rowsq_stat_block(st, lds);
    if (threadIdx.x == 0) {
        res[0] = st.mx;
        res[1] = st.arg;
        res[2] = st.mn;
        res[3] = st.sum;
    }
}

}  // namespace ciao

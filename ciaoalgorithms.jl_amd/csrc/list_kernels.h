// list_kernels.h -- a matrix-vector product and its adjoint over a LIST of rows (ciao_list_dots, ciao_list_combine; DESIGN.md
// section 8.16): the first-order passes of a problem on a row subset (a training fold, a bootstrap resample, held-out rows) at the
// cost of the rows touched, without a gathered copy.
//
//   listdot_kernel          out[m] = sum_j (double)A[idx[m], j] * (double)x[j]      m = 0 .. M-1
//   listcomb_partial_kernel
//   + listcomb_final_kernel out[j] = sum_m c[m] * (double)A[idx[m], j]              j = 0 .. d-1
//
// idx = M int64 row numbers (INDEXED), or none: position = row.  List position m plays the part of the row number everywhere; the only
// change is that the row of position m is row idx[m] of A.  So the call over idx gives BIT FOR BIT what the unindexed call gives on the
// gathered copy A[idx] (c unchanged), for every ld, base and alignment.  Both are one pass over the M rows named: every element read
// once, 16-byte non-temporal loads of A, element loads where the base of A or ld is not a multiple of 16 bytes (and in a partial last
// chunk) by the same lane / thread.  Products and sums in double: (double)a * (double)x is exact for fp32 rows.  No atomics, no scratch.
//
// listdot: the decomposition of rowsq_kernels.h (rowsq_plan(M, d); d <= 4096, so never its split mode): a group of G <= 64 lanes per
// row, a lane's chunks into slots in chunk order, the butterfly of the fixed distances.  The order of addition of a row is a function of
// d alone: a row's result has the same bits at every list position, for every M and every neighbour.  x lives in LDS in the rows' own
// type (16 KiB at d = 4096 fp32, 32 KiB fp64), converted where it is used, and is zero beyond d up to the last chunk a lane can name: a
// chunk that does not exist contributes (+0.0) * (+0.0).  out[m] is written by lane 0 of the row's group, and by nobody else.
//
// listcomb: the decomposition of col_walk.h (col_plan(M, d, VEC, 1)) with list positions in the place of rows: thread (c, r) owns one
// 16-byte chunk of columns and the positions lo + r, lo + r + tr, ... of its slab, in order, COLSQ_U rows in flight; idx and c of a trip
// are loaded ahead of its row loads (those of the NEXT trip while this one's rows are on their way).  The term of a position is
//     c * (double)a
// rounded once, then added to the thread's sum (two operations: no fma, explicit or contracted -- the units are built with
// -ffp-contract=off); the indexed and the unindexed instantiation share the one line that spells it.  col_combine and col_final as they
// are: one partial d-vector per slab, added in slab order.  The order of addition is a function of (M, d) alone.
//
// An entry of idx outside [0, N) issues no load: out[m] = +0.0 in the dots, no term in the combine.  Nothing is read in columns
// [d, ld), in rows the list does not name, or beyond idx[M - 1] / c[M - 1].  Row offsets are formed in int64.
#pragma once

#include "col_walk.h"
#include "rowsq_kernels.h"

namespace ciao {

constexpr int LIST_MAX_D = 4096;   // x in one workgroup's LDS; the Gram route's bound

// the chunks of x a lane of listdot_kernel can name: a whole multiple of what the lanes of a group (modes 0..2) / of a wave (mode 3)
// take per trip; x is zero from d up to there
__host__ __device__ inline int64_t listdot_cover(int64_t chunks, int g_log2, int mode)
{
    return mode < 3 ? ((int64_t)1 << mode) << g_log2 : (chunks + ROWSQ_U * WAVE - 1) / (ROWSQ_U * WAVE) * (ROWSQ_U * WAVE);
}

// the row of list position m (m < M), and whether it exists
template <bool INDEXED>
__device__ __forceinline__ int64_t list_row(const int64_t *idx, int64_t m)
{
    if constexpr (INDEXED)
        return idx[m];
    else
        return m;
}
__device__ __forceinline__ bool list_row_ok(int64_t row, int64_t N) { return (uint64_t)row < (uint64_t)N; }

// the products of chunk c of a row with chunk c of x, added in column order.  x comes from LDS (xs, zero from d on); an experiment build
// with -DCIAO_LISTDOT_X_CACHE reads it from global memory through the cache instead, element by element below d (tools/list_passes_time.py
// times the two side by side; DESIGN.md section 8.16 has the figures) -- the same values, the same products, the same bits
template <typename T>
__device__ __forceinline__ double listdot_chunk(const T (&v)[16 / sizeof(T)], const T *xs, const T *xg, int64_t c, int64_t d)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    typedef T VecT __attribute__((ext_vector_type(VEC)));
#ifdef CIAO_LISTDOT_X_CACHE
    VecT xv;
#pragma unroll
    for (int j = 0; j < VEC; ++j) xv[j] = c * VEC + j < d ? xg[c * VEC + j] : T(0);
#else
    const VecT xv = *reinterpret_cast<const VecT *>(xs + c * VEC);
#endif
    double q = (double)v[0] * (double)xv[0];
#pragma unroll
    for (int j = 1; j < VEC; ++j) q += (double)v[j] * (double)xv[j];
    return q;
}

// modes 0..2 (rowsq_short_rows with list positions): wave w takes the positions lo + (4 it + w) RB R + r R + group
template <typename T, bool VEC16, bool INDEXED, int TPL>
__device__ __forceinline__ void listdot_short_rows(const T *A, int64_t N, int64_t d, int64_t ld, const int64_t *idx, int64_t lo, int64_t hi,
                                                   int g_log2, const T *xs, const T *xg, double *out)
{
    constexpr int VEC = 16 / (int)sizeof(T), U = ROWSQ_U, TP = 1 << TPL, RB = U / TP;
    const int lane = (int)threadIdx.x & (WAVE - 1), wave = (int)threadIdx.x >> 6;
    const int R = WAVE >> g_log2;
    const int g = lane & ((1 << g_log2) - 1), grp = lane >> g_log2;
    const int64_t chunks = (d + VEC - 1) / VEC, full = d / VEC;
    const int64_t per_wave = (int64_t)RB * R;
    int64_t base = lo + wave * per_wave;
    int64_t row[RB], nxt[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        const int64_t m = base + (int64_t)r * R + grp;
        row[r] = m < hi ? list_row<INDEXED>(idx, m) : -1;
    }
    for (; base < hi; base += ROWSQ_WAVES * per_wave) {   // (uniform in the wave)
#pragma unroll
        for (int r = 0; r < RB; ++r) {   // the next trip's rows, ahead of this trip's loads
            const int64_t m = base + ROWSQ_WAVES * per_wave + (int64_t)r * R + grp;
            nxt[r] = m < hi ? list_row<INDEXED>(idx, m) : -1;
        }
        T v[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t c = g + ((int64_t)(u % TP) << g_log2);
            rowsq_load<T, VEC16>(A + row[u / TP] * ld, c, full, d, list_row_ok(row[u / TP], N) && c < chunks, v[u]);
        }
        double s[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            s[r] = listdot_chunk<T>(v[r * TP], xs, xg, g, d);
#pragma unroll
            for (int k = 1; k < TP; ++k) s[r] += listdot_chunk<T>(v[r * TP + k], xs, xg, g + ((int64_t)k << g_log2), d);
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) s[r] = rowsq_group_sum(s[r], g_log2);
        if (g == 0) {
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int64_t m = base + (int64_t)r * R + grp;
                if (m < hi) out[m] = list_row_ok(row[r], N) ? s[r] : 0.0;
            }
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) row[r] = nxt[r];
    }
}

// mode 3 (rowsq_wave_span over the whole row): the chunks lane, lane + 64, ... of one row by one wave
template <typename T, bool VEC16>
__device__ __forceinline__ double listdot_wave_row(const T *rowp, bool ok, int64_t chunks, int64_t full, int64_t d, const T *xs, const T *xg)
{
    constexpr int VEC = 16 / (int)sizeof(T), U = ROWSQ_U;
    const int lane = (int)threadIdx.x & (WAVE - 1);
    double slot[U];
#pragma unroll
    for (int u = 0; u < U; ++u) slot[u] = 0.0;
    for (int64_t cb = 0; cb < chunks; cb += (int64_t)U * WAVE) {   // (uniform in the wave)
        T v[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t c = cb + (int64_t)u * WAVE + lane;
            rowsq_load<T, VEC16>(rowp, c, full, d, ok && c < chunks, v[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) slot[u] += listdot_chunk<T>(v[u], xs, xg, cb + (int64_t)u * WAVE + lane, d);
    }
    double s = slot[0];
#pragma unroll
    for (int u = 1; u < U; ++u) s += slot[u];
    return rowsq_group_sum(s, 6);
}

// out[m] for the positions [blockIdx.x * rows_per_wg, ...).  VEC16: the base of A and ld are multiples of 16 bytes.  x: d elements of T
// at any element alignment.
template <typename T, bool VEC16, bool INDEXED>
__global__ void __launch_bounds__(ROWSQ_BLOCK)
    listdot_kernel(const T *A, int64_t N, int64_t d, int64_t ld, const int64_t *idx, int64_t M, const T *x, int64_t rows_per_wg, int g_log2,
                   int mode, double *out)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    __shared__ __attribute__((aligned(16))) T xs[LIST_MAX_D];
    const int64_t lo = (int64_t)blockIdx.x * rows_per_wg;
    const int64_t hi = lo + rows_per_wg < M ? lo + rows_per_wg : M;
    const int lane = (int)threadIdx.x & (WAVE - 1), wave = (int)threadIdx.x >> 6;
    const int64_t chunks = (d + VEC - 1) / VEC, full = d / VEC;
#ifndef CIAO_LISTDOT_X_CACHE
    const int64_t xlen = listdot_cover(chunks, g_log2, mode) * VEC;   // <= LIST_MAX_D for d <= LIST_MAX_D
    for (int64_t i = threadIdx.x; i < xlen; i += ROWSQ_BLOCK) xs[i] = i < d ? x[i] : T(0);
    __syncthreads();
#endif
    if (mode == 0) {
        listdot_short_rows<T, VEC16, INDEXED, 0>(A, N, d, ld, idx, lo, hi, g_log2, xs, x, out);
    } else if (mode == 1) {
        listdot_short_rows<T, VEC16, INDEXED, 1>(A, N, d, ld, idx, lo, hi, g_log2, xs, x, out);
    } else if (mode == 2) {
        listdot_short_rows<T, VEC16, INDEXED, 2>(A, N, d, ld, idx, lo, hi, g_log2, xs, x, out);
    } else {
        int64_t m = lo + wave;
        int64_t row = m < hi ? list_row<INDEXED>(idx, m) : -1;
        for (; m < hi; m += ROWSQ_WAVES) {   // (uniform in the wave)
            const int64_t nxt = m + ROWSQ_WAVES < hi ? list_row<INDEXED>(idx, m + ROWSQ_WAVES) : -1;
            const bool ok = list_row_ok(row, N);
            const double s = listdot_wave_row<T, VEC16>(A + row * ld, ok, chunks, full, d, xs, x);
            if (lane == 0) out[m] = ok ? s : 0.0;
            row = nxt;
        }
    }
}

// ---- the adjoint -----------------------------------------------------------------------------------------------------------------------
// one term: acc[j] += c * (double)a for the columns of the thread's chunk (the ONE spelling of the product, both instantiations)
template <int VEC, typename V>
__device__ __forceinline__ void listcomb_add(double (&acc)[VEC], double c, const V &v, bool ok)
{
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const double t = c * (double)v[j];
        acc[j] = ok ? acc[j] + t : acc[j];
    }
}

// the VEC columns from col of row `row` of A (ok: the row exists; else zeros, no load)
template <typename T, bool WHOLE>
__device__ __forceinline__ void listcomb_load(const T *A, int64_t ld, int64_t row, bool ok, int64_t col, const bool (&colok)[16 / sizeof(T)],
                                              T (&v)[16 / sizeof(T)])
{
    constexpr int VEC = 16 / (int)sizeof(T);
    typedef T VecT __attribute__((ext_vector_type(VEC)));
    const T *p = A + row * ld + col;
    if (WHOLE) {
        VecT t;
#pragma unroll
        for (int j = 0; j < VEC; ++j) t[j] = T(0);
        if (ok) t = __builtin_nontemporal_load(reinterpret_cast<const VecT *>(p));
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = t[j];
    } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = (ok && colok[j]) ? __builtin_nontemporal_load(p + j) : T(0);
    }
}

// the positions pos, pos + tr, ... < hi of one chunk of columns: col_walk's loop over a list
template <typename T, bool WHOLE, bool INDEXED>
__device__ __forceinline__ void listcomb_walk(const T *A, int64_t N, int64_t ld, const int64_t *idx, const double *cv, int64_t pos, int64_t hi,
                                              int tr, int64_t col, int64_t d, double (&acc)[16 / sizeof(T)])
{
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr int U = COLSQ_U;
    bool colok[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) colok[j] = col + j < d;
    int64_t row[U], nrow[U];
    double cc[U], ncc[U];
    bool have = pos + (int64_t)(U - 1) * tr < hi;
    if (have) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            row[u] = list_row<INDEXED>(idx, pos + (int64_t)u * tr);
            cc[u] = cv[pos + (int64_t)u * tr];
        }
    }
    while (have) {
        const int64_t np = pos + (int64_t)U * tr;
        const bool more = np + (int64_t)(U - 1) * tr < hi;
        if (more) {   // idx and c of the next trip, ahead of this trip's row loads
#pragma unroll
            for (int u = 0; u < U; ++u) {
                nrow[u] = list_row<INDEXED>(idx, np + (int64_t)u * tr);
                ncc[u] = cv[np + (int64_t)u * tr];
            }
        }
        T v[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) listcomb_load<T, WHOLE>(A, ld, row[u], list_row_ok(row[u], N), col, colok, v[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) listcomb_add<VEC>(acc, cc[u], v[u], list_row_ok(row[u], N));
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                row[u] = nrow[u];
                cc[u] = ncc[u];
            }
        }
        pos = np;
        have = more;
    }
    for (; pos < hi; pos += tr) {
        const int64_t rw = list_row<INDEXED>(idx, pos);
        const double c1 = cv[pos];
        const bool ok = list_row_ok(rw, N);
        T v[VEC];
        listcomb_load<T, WHOLE>(A, ld, rw, ok, col, colok, v);
        listcomb_add<VEC>(acc, c1, v, ok);
    }
}

// partial[y * d + j] = sum over the positions of slab y of c[m] * A[idx[m], j].  VEC16: the base of A and ld are multiples of 16 bytes.
template <typename T, bool VEC16, bool INDEXED>
__global__ void __launch_bounds__(COLSQ_BLOCK)
    listcomb_partial_kernel(const T *A, int64_t N, int64_t d, int64_t ld, const int64_t *idx, int64_t M, const double *cv, int64_t slab,
                            int tc_log2, double *partial)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    const int tc = 1 << tc_log2, tr = COLSQ_BLOCK >> tc_log2;
    const int c = (int)threadIdx.x & (tc - 1), r = (int)threadIdx.x >> tc_log2;
    const int64_t col = ((int64_t)blockIdx.x * tc + c) * VEC;
    const int64_t lo = (int64_t)blockIdx.y * slab;
    const int64_t hi = lo + slab < M ? lo + slab : M;
    double acc[1][VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[0][j] = 0.0;
    if (col < d) {
        if (VEC16 && col + VEC <= d)
            listcomb_walk<T, true, INDEXED>(A, N, ld, idx, cv, lo + r, hi, tr, col, d, acc[0]);
        else
            listcomb_walk<T, false, INDEXED>(A, N, ld, idx, cv, lo + r, hi, tr, col, d, acc[0]);
    }
    col_combine(acc, tc, tr, c, r, col, d, partial);
}

// out[j] = the nslab partials of column j in slab order (col_final)
template <typename T>
__global__ void __launch_bounds__(COLSQ_BLOCK) listcomb_final_kernel(int64_t d, int nslab, const double *partial, double *out)
{
    col_final(d, nslab, partial, out);
}

}  // namespace ciao

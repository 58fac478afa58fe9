// col_walk.h -- what the column passes share: ciao_col_sqnorms (colsq_kernels.h), ciao_col_moments and ciao_scale_columns
// (colmom_kernels.h).  Each promises results that do not depend on the layout of A, bit for bit; the decomposition that makes this
// true is written once, here.
//
// A is cut into row slabs x column panels.  A workgroup is 256 threads arranged as tc columns x tr rows (tc * tr = 256): thread (c, r)
// owns ONE 16-byte chunk of columns (VEC = 16 / sizeof(T) of them) of the panel and the rows lo + r, lo + r + tr, ... of the slab, taken
// in row order, COLSQ_U rows in flight per thread (256 threads x 8 rows x 16 bytes = 32 KiB per workgroup, up to eight workgroups per
// CU).  tc = the power of two that covers the row's chunks, 256 at most: a row narrower than 256 chunks puts tr = 256 / tc rows in the
// workgroup, a wider one takes several panels (blockIdx.x).
//
// col_plan -- chunks, tc, panels, slab length, slab count -- is a pure function of (N, d): not of the device, the occupancy, ld or the
// alignment of A.  col_walk is the loop over a thread's rows: where the base of A or ld is not a multiple of 16 bytes (and in the last
// chunk of a d that is no multiple of VEC) the same thread reads the same columns element by element, so which thread meets which
// element in which order is the same for every layout of the same matrix.  What is done with a row's chunk is the caller's functor.
//
// The passes that add (squares, shifted moments) use no row reduction and no floating-point atomics: col_combine adds the tr row
// groups of a workgroup in the order r = 0, 1, ... through LDS and leaves NS partial d-vectors of doubles per slab in the context's
// workspace, col_final adds the partials of each column in slab order; the hand-off is the kernel boundary (ciao_common.h: the per-XCD
// L2s are not coherent with each other).
#pragma once

#include <stdio.h>

#include <string>

#include "ciao_common.h"

namespace ciao {

constexpr int COLSQ_BLOCK = 256;                     // threads of every column kernel
constexpr int COLSQ_U = 8;                           // rows in flight per thread
constexpr int COLSQ_WG_TARGET = 2048;                // workgroups of the pass (panels x slabs) where N allows: 8 per CU
constexpr int64_t COLSQ_WS_BYTES = (int64_t)32 << 20;   // the partials take min(32 MiB, ...) -- or 8 nsum d bytes (one slab) where that is more
constexpr int COLSQ_FC = 64, COLSQ_FR = 4;           // col_final: columns x slab groups of a workgroup

struct ColsqPlan {
    int tc_log2;      // column threads of a workgroup = 1 << tc_log2; row groups tr = COLSQ_BLOCK >> tc_log2
    int64_t panels;   // column panels of tc chunks (grid x)
    int64_t slab;     // rows of one slab: a whole multiple of tr * COLSQ_U
    int64_t nslab;    // slabs (grid y) = partial d-vectors of each sum
};

// vec = elements of a 16-byte chunk (4 fp32, 2 fp64); nsum = partial d-vectors of doubles a slab leaves in the workspace
__host__ __device__ inline ColsqPlan col_plan(int64_t N, int64_t d, int vec, int nsum)
{
    ColsqPlan pl;
    const int64_t chunks = (d + vec - 1) / vec;
    int tc = 1;
    pl.tc_log2 = 0;
    while (tc < COLSQ_BLOCK && tc < chunks) {
        tc *= 2;
        ++pl.tc_log2;
    }
    pl.panels = (chunks + tc - 1) / tc;
    const int64_t step = (int64_t)(COLSQ_BLOCK / tc) * COLSQ_U;   // rows a workgroup takes per unrolled iteration
    int64_t want = COLSQ_WG_TARGET / pl.panels;
    const int64_t cap = COLSQ_WS_BYTES / (8 * nsum * d);           // fewer slabs as d grows: the workspace bound
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    int64_t slab = (N + want - 1) / want;
    slab = (slab + step - 1) / step * step;
    if (slab < 4 * step) slab = 4 * step;
    pl.slab = slab;
    pl.nslab = (N + slab - 1) / slab;
    if (pl.nslab < 1) pl.nslab = 1;
    return pl;
}

// The rows row, row + tr, ... < hi of the chunk at base = A + col (col < d): f(row, chunk) for each of them in that order, non-temporal
// loads, the U loads of an unrolled trip before its first call.  chunk[j] is the element of column col + j: one 16-byte vector where
// VEC16 (base and ld are multiples of 16 bytes) and the chunk lies within d, a T[VEC] loaded element by element otherwise, with T(0)
// where the column is past d.  The whole-chunk test and the validity flags are formed from col and d as they stand (col + VEC <= d,
// col + j < d), not from one difference d - col: with that hipcc ties the two together, the 16-byte kernels take fewer registers, one
// more wave per SIMD fits, and the fp64 squares at d = 50 measured 4 % slower (profiles/col_walk_ab.txt).
template <typename T, bool VEC16, typename F>
__device__ __forceinline__ void col_walk(const T *base, int64_t ld, int64_t row, int64_t hi, int tr, int64_t col, int64_t d, F f)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr int U = COLSQ_U;
    typedef T VecT __attribute__((ext_vector_type(VEC)));
    if (VEC16 && col + VEC <= d) {
        for (; row + (int64_t)(U - 1) * tr < hi; row += (int64_t)U * tr) {
            VecT v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(reinterpret_cast<const VecT *>(base + (row + (int64_t)u * tr) * ld));
#pragma unroll
            for (int u = 0; u < U; ++u) f(row + (int64_t)u * tr, v[u]);
        }
        for (; row < hi; row += tr) f(row, __builtin_nontemporal_load(reinterpret_cast<const VecT *>(base + row * ld)));
    } else {
        bool ok[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) ok[j] = col + j < d;
        for (; row + (int64_t)(U - 1) * tr < hi; row += (int64_t)U * tr) {
            T v[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < VEC; ++j) v[u][j] = ok[j] ? __builtin_nontemporal_load(base + (row + (int64_t)u * tr) * ld + j) : T(0);
#pragma unroll
            for (int u = 0; u < U; ++u) f(row + (int64_t)u * tr, v[u]);
        }
        for (; row < hi; row += tr) {
            T v[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = ok[j] ? __builtin_nontemporal_load(base + row * ld + j) : T(0);
            f(row, v);
        }
    }
}

// The tr row groups of a workgroup -> one, for NS sums, in the order r = 0, 1, ..., by the thread of row group 0 that owns the chunk:
// partial[(s * gridDim.y + y) * d + col + j] = sum s of slab y = blockIdx.y.  Every thread of the workgroup calls it, with the
// coordinates (tc, tr, c, r) its kernel walked with.
template <int NS, int VEC>
__device__ __forceinline__ void col_combine(const double (&acc)[NS][VEC], int tc, int tr, int c, int r, int64_t col, int64_t d, double *partial)
{
    __shared__ double lds[NS][COLSQ_BLOCK * VEC];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int j = 0; j < VEC; ++j) lds[s][(int)threadIdx.x * VEC + j] = acc[s][j];
    __syncthreads();
    if (r == 0 && col < d) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            if (col + j < d) {
                double t[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) t[s] = lds[s][c * VEC + j];
                for (int rr = 1; rr < tr; ++rr)
#pragma unroll
                    for (int s = 0; s < NS; ++s) t[s] += lds[s][(rr * tc + c) * VEC + j];
#pragma unroll
                for (int s = 0; s < NS; ++s) partial[((int64_t)s * gridDim.y + blockIdx.y) * d + col + j] = t[s];
            }
        }
    }
}

// out[j] = the nslab partials of column j (partial[y * d + j]) in slab order: thread (c, g) adds the g-th quarter of the slabs
// (contiguous, in order), the four quarters are added in order through LDS.  Workgroup blockIdx.x owns COLSQ_FC columns.
__device__ __forceinline__ void col_final(int64_t d, int nslab, const double *partial, double *out)
{
    __shared__ double lds[COLSQ_FR][COLSQ_FC];
    const int c = (int)threadIdx.x & (COLSQ_FC - 1), g = (int)threadIdx.x / COLSQ_FC;
    const int64_t col = (int64_t)blockIdx.x * COLSQ_FC + c;
    const int per = (nslab + COLSQ_FR - 1) / COLSQ_FR;
    const int y0 = g * per;
    const int y1 = y0 + per < nslab ? y0 + per : nslab;
    double s = 0.0;
    if (col < d) {
        const double *p = partial + col;
        int y = y0;
        for (; y + 8 <= y1; y += 8) {
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = p[(int64_t)(y + k) * d];
#pragma unroll
            for (int k = 0; k < 8; ++k) s += v[k];
        }
        for (; y < y1; ++y) s += p[(int64_t)y * d];
    }
    lds[g][c] = s;
    __syncthreads();
    if (g == 0 && col < d) {
        double t = lds[0][c];
        for (int k = 1; k < COLSQ_FR; ++k) t += lds[k][c];
        out[col] = t;
    }
}

// host side: a matrix of T at base with row stride ld (elements) can be walked with 16-byte accesses
template <typename T>
inline bool col_vec16(const void *base, int64_t ld)
{
    return (reinterpret_cast<uintptr_t>(base) & 15u) == 0 && ((size_t)ld * sizeof(T)) % 16 == 0;
}

// host side: what every column pass reports of its launch, "kernel<f64,vec16> grid=PxS block=256 tc=.. slab=.."
template <typename T>
inline std::string col_report(const char *kernel, bool vec16, const ColsqPlan &pl)
{
    char buf[160];
    snprintf(buf, sizeof buf, "%s<%s,%s> grid=%lldx%lld block=%d tc=%d slab=%lld", kernel, sizeof(T) == 8 ? "f64" : "f32",
             vec16 ? "vec16" : "elem", (long long)pl.panels, (long long)pl.nslab, COLSQ_BLOCK, 1 << pl.tc_log2, (long long)pl.slab);
    return buf;
}

}  // namespace ciao

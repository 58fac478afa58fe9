// colsq_kernels.h -- gap-safe feature screening (ciao_col_sqnorms, ciao_screen).
//
// Column sums of squares, out[j] = sum_i A[i,j]^2 over the N resident rows: ONE pass over A, every element read once, 16-byte
// non-temporal loads, squares formed and added in double ((double)a * (double)a: exact for fp32 input).  No row reduction and no
// floating-point atomics: A is cut into row slabs x column panels, colsq_partial_kernel leaves one partial d-panel of doubles per
// workgroup in the context's workspace, colsq_final_kernel adds the partials of each column in slab order; the hand-off is the kernel
// boundary (ciao_common.h: the per-XCD L2s are not coherent with each other).
//
// A workgroup is 256 threads arranged as tc columns x tr rows (tc * tr = 256): thread (c, r) owns ONE 16-byte chunk of columns
// (VEC = 16 / sizeof(T) of them) of the panel and the rows lo + r, lo + r + tr, ... of the slab, added in row order, COLSQ_U rows in
// flight per thread (256 threads x 8 rows x 16 bytes = 32 KiB per workgroup, up to eight workgroups per CU).  tc = the power of two
// that covers the row's chunks, 256 at most: a row narrower than 256 chunks puts tr = 256 / tc rows in the workgroup (their sums are
// combined in the order r = 0, 1, ... through LDS), a wider one takes several panels (blockIdx.x).
//
// colsq_plan -- chunks, tc, panels, slab length, slab count -- is a pure function of (N, d): not of the device, the occupancy, ld or
// the alignment of A.  Where the base of A or ld is not a multiple of 16 bytes (and in the last chunk of a d that is no multiple of
// VEC) the same thread reads the same columns element by element, so which thread adds which element in which order -- and with it
// every bit of the result -- is the same for every layout of the same matrix.
//
// The screening rule, keep[j] = !(s |grad_j| + kappa sqrt(colsq_j) < mu) in double (a NaN anywhere keeps the coordinate), and the
// count of the kept: screen_kernel + screen_count_kernel, built as cert_kernels.h's reduction is (cert_slice / cert_grid / CERT_REC,
// the four waves in order through LDS, one record per workgroup, one workgroup combines them).  The count is exact as a double.
#pragma once

#include "cert_kernels.h"

namespace ciao {

constexpr int COLSQ_BLOCK = 256;                     // threads of both column kernels
constexpr int COLSQ_U = 8;                           // rows in flight per thread
constexpr int COLSQ_WG_TARGET = 2048;                // workgroups of the pass (panels x slabs) where N allows: 8 per CU
constexpr int64_t COLSQ_WS_BYTES = (int64_t)32 << 20;   // the partials take min(32 MiB, ...) -- or 8 d bytes (one slab) where d > 4 Mi
constexpr int COLSQ_FC = 64, COLSQ_FR = 4;           // colsq_final_kernel: columns x slab groups of a workgroup

struct ColsqPlan {
    int tc_log2;      // column threads of a workgroup = 1 << tc_log2; row groups tr = COLSQ_BLOCK >> tc_log2
    int64_t panels;   // column panels of tc chunks (grid x)
    int64_t slab;     // rows of one slab: a whole multiple of tr * COLSQ_U
    int64_t nslab;    // slabs (grid y) = partial d-vectors
};

// vec = elements of a 16-byte chunk (4 fp32, 2 fp64)
__host__ __device__ inline ColsqPlan colsq_plan(int64_t N, int64_t d, int vec)
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
    const int64_t cap = COLSQ_WS_BYTES / (8 * d);                  // fewer slabs as d grows: the workspace bound
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

// partial[y * d + j] = sum over the rows of slab y of A[i, j]^2.  VEC16: the base of A and ld are multiples of 16 bytes.
template <typename T, bool VEC16>
__global__ void __launch_bounds__(COLSQ_BLOCK)
    colsq_partial_kernel(const T *A, int64_t N, int64_t d, int64_t ld, int64_t slab, int tc_log2, double *partial)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr int U = COLSQ_U;
    typedef T VecT __attribute__((ext_vector_type(VEC)));
    __shared__ double lds[COLSQ_BLOCK * VEC];
    const int tc = 1 << tc_log2, tr = COLSQ_BLOCK >> tc_log2;
    const int c = (int)threadIdx.x & (tc - 1), r = (int)threadIdx.x >> tc_log2;
    const int64_t col = ((int64_t)blockIdx.x * tc + c) * VEC;
    const int64_t lo = (int64_t)blockIdx.y * slab;
    const int64_t hi = lo + slab < N ? lo + slab : N;
    double acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.0;
    if (col < d) {
        const T *base = A + col;
        int64_t row = lo + r;
        if (VEC16 && col + VEC <= d) {
            for (; row + (int64_t)(U - 1) * tr < hi; row += (int64_t)U * tr) {
                VecT v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(reinterpret_cast<const VecT *>(base + (row + (int64_t)u * tr) * ld));
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int j = 0; j < VEC; ++j) acc[j] += (double)v[u][j] * (double)v[u][j];
            }
            for (; row < hi; row += tr) {
                const VecT v = __builtin_nontemporal_load(reinterpret_cast<const VecT *>(base + row * ld));
#pragma unroll
                for (int j = 0; j < VEC; ++j) acc[j] += (double)v[j] * (double)v[j];
            }
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
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int j = 0; j < VEC; ++j) acc[j] += (double)v[u][j] * (double)v[u][j];
            }
            for (; row < hi; row += tr) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const T v = ok[j] ? __builtin_nontemporal_load(base + row * ld + j) : T(0);
                    acc[j] += (double)v * (double)v;
                }
            }
        }
    }
    // the tr row groups -> one, in the order r = 0, 1, ..., by the thread of row group 0 that owns the chunk
#pragma unroll
    for (int j = 0; j < VEC; ++j) lds[(int)threadIdx.x * VEC + j] = acc[j];
    __syncthreads();
    if (r == 0 && col < d) {
        double *out = partial + (int64_t)blockIdx.y * d + col;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            if (col + j < d) {
                double s = lds[c * VEC + j];
                for (int rr = 1; rr < tr; ++rr) s += lds[(rr * tc + c) * VEC + j];
                out[j] = s;
            }
        }
    }
}

// out[j] = the nslab partials of column j in slab order: thread (c, g) adds the g-th quarter of the slabs (contiguous, in order),
// the four quarters are added in order through LDS
template <typename T>
__global__ void __launch_bounds__(COLSQ_BLOCK) colsq_final_kernel(int64_t d, int nslab, const double *partial, double *out)
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

// keep[k] = !(s |grad_k| + kappa sqrt(colsq_k) < mu), one byte per coordinate; rec[blockIdx.x * CERT_REC] = the slice's kept count.
// Workgroup b owns the coordinates [b*slice, min((b+1)*slice, d)), thread t the coordinates t, t + 256, ... of the slice.
template <typename T>
__global__ void __launch_bounds__(CERT_BLOCK)
    screen_kernel(int64_t d, int64_t slice, const T *grad, const double *colsq, double s, double kappa, double mu, uint8_t *keep, double *rec)
{
    __shared__ double lds[CERT_BLOCK / WAVE];
    const int64_t lo = (int64_t)blockIdx.x * slice;
    const int64_t hi = lo + slice < d ? lo + slice : d;
    double cnt = 0.0;
    for (int64_t k = lo + threadIdx.x; k < hi; k += CERT_BLOCK) {
        const double lhs = s * fabs((double)grad[k]) + kappa * sqrt(colsq[k]);
        const bool kept = !(lhs < mu);
        keep[k] = kept ? 1 : 0;
        cnt += kept ? 1.0 : 0.0;
    }
    cnt = wave_allsum(cnt);
    if ((threadIdx.x & (WAVE - 1)) == 0) lds[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CERT_BLOCK / WAVE; ++w) cnt += lds[w];
        rec[(int64_t)blockIdx.x * CERT_REC] = cnt;
    }
}

// one workgroup: thread t adds the records t, t + 256, ... in index order, then the same fixed-order combine; out[0] = kept coordinates
template <typename T>
__global__ void __launch_bounds__(CERT_BLOCK) screen_count_kernel(int nrec, const double *rec, double *out)
{
    __shared__ double lds[CERT_BLOCK / WAVE];
    double cnt = 0.0;
    for (int i = threadIdx.x; i < nrec; i += CERT_BLOCK) cnt += rec[(int64_t)i * CERT_REC];
    cnt = wave_allsum(cnt);
    if ((threadIdx.x & (WAVE - 1)) == 0) lds[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CERT_BLOCK / WAVE; ++w) cnt += lds[w];
        out[0] = cnt;
    }
}

}  // namespace ciao

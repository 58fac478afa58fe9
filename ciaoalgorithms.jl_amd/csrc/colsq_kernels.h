// colsq_kernels.h -- gap-safe feature screening (ciao_col_sqnorms, ciao_screen).
//
// Column sums of squares, out[j] = sum_i A[i,j]^2 over the N resident rows: ONE pass over A, every element read once, 16-byte
// non-temporal loads, squares formed and added in double ((double)a * (double)a: exact for fp32 input).  The decomposition -- row slabs
// x column panels, which thread adds which element in which order, the combine through LDS, the partials and their final sum -- is
// col_walk.h's, so every bit of the result is the same for every layout of the same matrix: colsq_partial_kernel leaves one partial
// d-panel of doubles per workgroup in the context's workspace, colsq_final_kernel adds the partials of each column in slab order.
//
// The screening rule, keep[j] = !(s |grad_j| + kappa sqrt(colsq_j) < mu) in double (a NaN anywhere keeps the coordinate), and the
// count of the kept: screen_kernel + screen_count_kernel, built as cert_kernels.h's reduction is (cert_slice / cert_grid / CERT_REC,
// the four waves in order through LDS, one record per workgroup, one workgroup combines them).  The count is exact as a double.
#pragma once

#include "cert_kernels.h"
#include "col_walk.h"

namespace ciao {

// one partial d-vector per slab
__host__ __device__ inline ColsqPlan colsq_plan(int64_t N, int64_t d, int vec) { return col_plan(N, d, vec, 1); }

// partial[y * d + j] = sum over the rows of slab y of A[i, j]^2.  VEC16: the base of A and ld are multiples of 16 bytes.
template <typename T, bool VEC16>
__global__ void __launch_bounds__(COLSQ_BLOCK)
    colsq_partial_kernel(const T *A, int64_t N, int64_t d, int64_t ld, int64_t slab, int tc_log2, double *partial)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    const int tc = 1 << tc_log2, tr = COLSQ_BLOCK >> tc_log2;
    const int c = (int)threadIdx.x & (tc - 1), r = (int)threadIdx.x >> tc_log2;
    const int64_t col = ((int64_t)blockIdx.x * tc + c) * VEC;
    const int64_t lo = (int64_t)blockIdx.y * slab;
    const int64_t hi = lo + slab < N ? lo + slab : N;
    double acc[1][VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[0][j] = 0.0;
    if (col < d)
        col_walk<T, VEC16>(A + col, ld, lo + r, hi, tr, col, d, [&](int64_t, const auto &v) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[0][j] += (double)v[j] * (double)v[j];
        });
    col_combine(acc, tc, tr, c, r, col, d, partial);
}

// out[j] = the nslab partials of column j in slab order (col_final)
template <typename T>
__global__ void __launch_bounds__(COLSQ_BLOCK) colsq_final_kernel(int64_t d, int nslab, const double *partial, double *out)
{
    col_final(d, nslab, partial, out);
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

// mstat_kernels.h -- the per-sample reduction (ciao_margin_stats, ciao_certificate_samples): one pass over the row dots a_i'x and the
// targets / labels b_i of the N samples that leaves four doubles,
//   logistic rows, t_i = b_i dots_i:   [0] sum_i softplus(-t_i)   [1] E(s) = sum_i h(s sigma(-t_i))   [2] #{i: t_i <= 0}   [3] min_i t_i
//   LeastSquares rows, r_i = dots_i - b_i:   [0] sum_i r_i^2      [1] sum_i b_i                        [2] sum_i b_i^2      [3] max_i |r_i|
// with h(u) = u log u + (1 - u) log(1 - u), the entropy term of the logistic dual.  All arithmetic in double
// from the T-typed dot and label.
//
// Built as cert_kernels.h is, over the N samples instead of the d coordinates: mstat_partial_kernel leaves one record per workgroup
// (cert_slice / cert_grid / CERT_REC: the same pure functions of the length), mstat_final_kernel combines the records, the hand-off is
// the kernel boundary.  Which thread adds which sample in which order depends on N alone -- not on the device, the occupancy or the
// alignment of the pointers -- so the four numbers are bitwise reproducible between runs, contexts and pointer alignments.
#pragma once

#include "cert_kernels.h"

namespace ciao {

// sums a0 a1 a2 and one maximum: max_i |r_i|, or max_i (-t_i) = -min_i t_i (negated once, by mstat_final_kernel)
struct MstatAcc {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, m;
};

__device__ __forceinline__ double mstat_xlogx(double u) { return u > 0.0 ? u * log(u) : 0.0; }

// Stable on either side of t = 0: e = exp(-|t|) <= 1, sigma(-t) and sigma(t) are e / (1 + e) and 1 / (1 + e) in the order the sign of t
// gives.  v = s sigma(-t); w = 1 - v is formed as (1 - s) + s sigma(t), two non-negative terms: no cancellation where v is close to 1.
// The double form is what the T-typed one below evaluates after its two conversions; mscore_partial_kernel's row-list instantiations
// call it with an offset already added to the dot.
template <int LOSS>
__device__ __forceinline__ void mstat_elem_d(MstatAcc &c, double s, double bd, double dot)
{
    if (LOSS == CIAO_LOSS_LOGISTIC) {
        const double t = bd * dot;
        const double e = exp(-fabs(t));
        const double big = 1.0 / (1.0 + e), small = e / (1.0 + e);
        const double sneg = t >= 0.0 ? small : big, spos = t >= 0.0 ? big : small;
        const double v = s * sneg, w = (1.0 - s) + s * spos;
        c.a0 += fmax2(-t, 0.0) + log1p(e);
        c.a1 += mstat_xlogx(v) + mstat_xlogx(w);
        c.a2 += t <= 0.0 ? 1.0 : 0.0;
        c.m = fmax2(c.m, -t);
    } else {
        const double b = bd, r = dot - b;
        c.a0 += r * r;
        c.a1 += b;
        c.a2 += b * b;
        c.m = fmax2(c.m, fabs(r));
    }
}
template <typename T, int LOSS>
__device__ __forceinline__ void mstat_elem(MstatAcc &c, double s, T dot, T bi)
{
    mstat_elem_d<LOSS>(c, s, (double)bi, (double)dot);
}

// the four waves' values -> one, in wave order, through LDS; valid in thread 0
__device__ __forceinline__ void mstat_block_combine(MstatAcc &c, double (*lds)[4])
{
    c.a0 = wave_allsum(c.a0);
    c.a1 = wave_allsum(c.a1);
    c.a2 = wave_allsum(c.a2);
    c.m = wave_allmax(c.m);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        lds[wave][0] = c.a0;
        lds[wave][1] = c.a1;
        lds[wave][2] = c.a2;
        lds[wave][3] = c.m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CERT_BLOCK / WAVE; ++w) {
            c.a0 += lds[w][0];
            c.a1 += lds[w][1];
            c.a2 += lds[w][2];
            c.m = fmax2(c.m, lds[w][3]);
        }
    }
}

// Workgroup b owns the samples [b*slice, min((b+1)*slice, N)); thread t owns the 16-byte chunks t, t + 256, ... of the slice and adds
// their samples in index order.  vec16: dots and b are 16-byte aligned; otherwise, and in the last chunk of an N that is no multiple
// of the chunk, element loads by the same thread.  s: the literal s_lit, or (M_dev non-null) formed here from M = *M_dev = the
// infinity norm of grad f that cert_final_kernel left, and mu: the dual point's scaling without a host round trip.
template <typename T, int LOSS>
__global__ void __launch_bounds__(CERT_BLOCK)
    mstat_partial_kernel(int64_t N, int64_t slice, const T *dots, const T *b, double s_lit, const double *M_dev, double mu, int vec16, double *rec)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    typedef T VecT __attribute__((ext_vector_type(VEC)));
    __shared__ double lds[CERT_BLOCK / WAVE][4];
    double s = s_lit;
    if (M_dev) {
        const double M = *M_dev;
        s = M == 0.0 ? 1.0 : fmin2(1.0, mu / M);
    }
    const int64_t lo = (int64_t)blockIdx.x * slice;
    const int64_t hi = lo + slice < N ? lo + slice : N;
    MstatAcc c;
    c.m = LOSS == CIAO_LOSS_LOGISTIC ? -__builtin_inf() : 0.0;
    for (int64_t k = lo + (int64_t)threadIdx.x * VEC; k < hi; k += (int64_t)CERT_BLOCK * VEC) {
        if (vec16 && k + VEC <= hi) {
            const VecT dv = *reinterpret_cast<const VecT *>(dots + k), bv = *reinterpret_cast<const VecT *>(b + k);
#pragma unroll
            for (int j = 0; j < VEC; ++j) mstat_elem<T, LOSS>(c, s, dv[j], bv[j]);
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                if (k + j < hi) mstat_elem<T, LOSS>(c, s, dots[k + j], b[k + j]);
        }
    }
    mstat_block_combine(c, lds);
    if (threadIdx.x == 0) {
        double *r = rec + (int64_t)blockIdx.x * CERT_REC;
        r[0] = c.a0;
        r[1] = c.a1;
        r[2] = c.a2;
        r[3] = c.m;
    }
}

// one workgroup: thread t adds the records t, t + 256, ... in index order, then the same fixed-order combine; out[0..4)
template <typename T, int LOSS>
__global__ void __launch_bounds__(CERT_BLOCK) mstat_final_kernel(int nrec, const double *rec, double *out)
{
    __shared__ double lds[CERT_BLOCK / WAVE][4];
    MstatAcc c;
    c.m = LOSS == CIAO_LOSS_LOGISTIC ? -__builtin_inf() : 0.0;
    for (int i = threadIdx.x; i < nrec; i += CERT_BLOCK) {
        const double *r = rec + (int64_t)i * CERT_REC;
        c.a0 += r[0];
        c.a1 += r[1];
        c.a2 += r[2];
        c.m = fmax2(c.m, r[3]);
    }
    mstat_block_combine(c, lds);
    if (threadIdx.x == 0) {
        out[0] = c.a0;
        out[1] = c.a1;
        out[2] = c.a2;
        out[3] = LOSS == CIAO_LOSS_LOGISTIC ? -c.m : c.m;
    }
}

}  // namespace ciao

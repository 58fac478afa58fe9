// cert_kernels.h -- the optimality certificate's reduction over the d coordinates (ciao_certificate): one pass over x and
// av = grad f(x) that leaves five doubles,
//     S0 = sum_k (x_k - prox_{gamma g}(x_k - gamma av_k)_k)^2      S1 = sum_k x_k av_k      S2 = sum_k g_k(x_k)  (NormL1's value)
//     M  = max_k |av_k|                                             V  = max_k Box violation of x_k  (0 for the other proxes)
// Per-coordinate work in T (prox_elem / prox_value_elem, as the fused epilogue has them), accumulation in double.
//
// Two kernels: cert_partial_kernel leaves one record per workgroup, cert_final_kernel combines the records.  The hand-off is the
// kernel boundary (ciao_common.h: the per-XCD L2s are not coherent with each other; no in-kernel flags).  Which thread adds which
// coordinate in which order depends on d alone -- not on the device, the occupancy or the alignment of the pointers (an unaligned
// vector is read element by element by the thread that would have read the 16-byte chunk) -- so the five numbers are bitwise
// reproducible from run to run, context to context, and between a caller's av and the library's own.
#pragma once

#include "cert_ws.h"   // CERT_GRID_CAP, CERT_REC
#include "ciao_common.h"

namespace ciao {

constexpr int CERT_BLOCK = 256;       // threads of both kernels
constexpr int CERT_SLICE = 1024;      // coordinates of one workgroup's slice up to CERT_GRID_CAP slices; whole multiples of it beyond

// the slice of a d-vector: a pure function of d
__host__ __device__ inline int64_t cert_slice(int64_t d)
{
    const int64_t per = (d + CERT_GRID_CAP - 1) / CERT_GRID_CAP;
    return per <= CERT_SLICE ? CERT_SLICE : (per + CERT_SLICE - 1) / CERT_SLICE * CERT_SLICE;
}
__host__ __device__ inline int cert_grid(int64_t d)
{
    const int64_t s = cert_slice(d);
    return (int)((d + s - 1) / s);
}

// max over the 64 lanes of a wave, identical in every lane (the butterfly of wave_allsum; all 64 lanes active)
__device__ __forceinline__ double wave_allmax(double v)
{
    v = fmax2(v, dpp_mov<0xB1>(v));
    v = fmax2(v, dpp_mov<0x4E>(v));
    v = fmax2(v, dpp_mov<0x141>(v));
    v = fmax2(v, dpp_mov<0x140>(v));
    const double r0 = readlane(v, 0), r1 = readlane(v, 16), r2 = readlane(v, 32), r3 = readlane(v, 48);
    return fmax2(fmax2(r0, r1), fmax2(r2, r3));
}

struct CertAcc {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, m = 0.0, v = 0.0;
};

template <typename T>
__device__ __forceinline__ void cert_elem(CertAcc &c, const ProxD<T> &g, T gamma, int64_t k, T xk, T ak)
{
    const T r = xk - prox_elem(g, xk - gamma * ak, gamma, k);
    c.s0 += (double)r * (double)r;
    c.s1 += (double)xk * (double)ak;
    c.s2 += (double)prox_value_elem(g, xk);
    c.m = fmax2(c.m, (double)fabs2(ak));
    if (g.kind == CIAO_PROX_BOX) {
        const double l = (double)(g.lo_vec ? g.lo_vec[k] : g.lo), h = (double)(g.hi_vec ? g.hi_vec[k] : g.hi);
        c.v = fmax2(c.v, fmax2(l - (double)xk, (double)xk - h));
    }
}

// the four waves' values -> one, in wave order, through LDS; valid in thread 0
__device__ __forceinline__ void cert_block_combine(CertAcc &c, double (*lds)[5])
{
    c.s0 = wave_allsum(c.s0);
    c.s1 = wave_allsum(c.s1);
    c.s2 = wave_allsum(c.s2);
    c.m = wave_allmax(c.m);
    c.v = wave_allmax(c.v);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        lds[wave][0] = c.s0;
        lds[wave][1] = c.s1;
        lds[wave][2] = c.s2;
        lds[wave][3] = c.m;
        lds[wave][4] = c.v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CERT_BLOCK / WAVE; ++w) {
            c.s0 += lds[w][0];
            c.s1 += lds[w][1];
            c.s2 += lds[w][2];
            c.m = fmax2(c.m, lds[w][3]);
            c.v = fmax2(c.v, lds[w][4]);
        }
    }
}

// Workgroup b owns the coordinates [b*slice, min((b+1)*slice, d)); thread t owns the 16-byte chunks t, t + 256, ... of the slice and
// adds their elements in index order.  vec16: x and av are 16-byte aligned (a slice starts at a multiple of 1024 elements, so every
// whole chunk is then one 16-byte load); otherwise, and in the last chunk of a d that is no multiple of the chunk, element loads.
template <typename T>
__global__ void __launch_bounds__(CERT_BLOCK)
    cert_partial_kernel(int64_t d, int64_t slice, ProxD<T> g, const T *x, const T *av, T gamma, int vec16, double *rec)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    typedef T VecT __attribute__((ext_vector_type(VEC)));
    __shared__ double lds[CERT_BLOCK / WAVE][5];
    const int64_t lo = (int64_t)blockIdx.x * slice;
    const int64_t hi = lo + slice < d ? lo + slice : d;
    CertAcc c;
    for (int64_t k = lo + (int64_t)threadIdx.x * VEC; k < hi; k += (int64_t)CERT_BLOCK * VEC) {
        if (vec16 && k + VEC <= hi) {
            const VecT xv = *reinterpret_cast<const VecT *>(x + k), avv = *reinterpret_cast<const VecT *>(av + k);
#pragma unroll
            for (int j = 0; j < VEC; ++j) cert_elem(c, g, gamma, k + j, xv[j], avv[j]);
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                if (k + j < hi) cert_elem(c, g, gamma, k + j, x[k + j], av[k + j]);
        }
    }
    cert_block_combine(c, lds);
    if (threadIdx.x == 0) {
        double *r = rec + (int64_t)blockIdx.x * CERT_REC;
        r[0] = c.s0;
        r[1] = c.s1;
        r[2] = c.s2;
        r[3] = c.m;
        r[4] = c.v;
    }
}

// one workgroup: thread t adds the records t, t + 256, ... in index order, then the same fixed-order combine; out[0..5) = S0 S1 S2 M V
template <typename T>
__global__ void __launch_bounds__(CERT_BLOCK) cert_final_kernel(int nrec, const double *rec, double *out)
{
    __shared__ double lds[CERT_BLOCK / WAVE][5];
    CertAcc c;
    for (int i = threadIdx.x; i < nrec; i += CERT_BLOCK) {
        const double *r = rec + (int64_t)i * CERT_REC;
        c.s0 += r[0];
        c.s1 += r[1];
        c.s2 += r[2];
        c.m = fmax2(c.m, r[3]);
        c.v = fmax2(c.v, r[4]);
    }
    cert_block_combine(c, lds);
    if (threadIdx.x == 0) {
        out[0] = c.s0;
        out[1] = c.s1;
        out[2] = c.s2;
        out[3] = c.m;
        out[4] = c.v;
    }
}

}  // namespace ciao

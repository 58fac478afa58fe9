// colmom_kernels.h -- column standardisation (ciao_col_moments, ciao_scale_columns).
//
// Shifted column moments, s1[j] = sum_i (A[i,j] - c_j) and s2[j] = sum_i (A[i,j] - c_j)^2 over the N resident rows, c = a device d-vector
// of doubles or (NULL) the first resident row: ONE pass over A, every element read once, 16-byte non-temporal loads; the difference
// (double)a - c_j, its square and every addition in double.  The decomposition is colsq_kernels.h's: row slabs x column panels, thread
// (c, r) of a workgroup owns one 16-byte chunk of columns and the rows lo + r, lo + r + tr, ... of the slab in row order, COLSQ_U rows in
// flight; the tr row groups are combined in the order r = 0, 1, ... through LDS; colmom_partial_kernel leaves TWO partial d-panels per
// workgroup in the context's workspace (all s1 panels, then all s2 panels), colmom_final_kernel adds the partials of each column in slab
// order (blockIdx.y: which of the two sums).  No atomics, no scratch; the hand-off is the kernel boundary.
//
// colmom_plan is colsq_plan with the workspace bound taken for two panels: a pure function of (N, d).  Where the base of A or ld is not a
// multiple of 16 bytes (and in the last chunk of a d that is no multiple of VEC) the same thread reads the same columns element by
// element, so every bit of both sums is the same for every layout of the same matrix.
//
// Scaling, out[i,j] = (T)(((double)a_ij - center_j) * scale_j): one subtraction and one multiplication in double (no contraction: the units
// are built with -ffp-contract=off), one rounding to T.  colscale_kernel walks the same slabs and panels; a thread keeps its chunk of
// center / scale in registers, loads COLSQ_U rows, then stores them: every element is read and written by the SAME thread and a row is
// loaded before it is stored, so out may be A itself.  16-byte loads and stores where both bases and both strides allow, element by
// element otherwise; the columns [d, ld_out) of a row are never written.
#pragma once

#include "colsq_kernels.h"

namespace ciao {

// colsq_plan with cap = COLSQ_WS_BYTES / (16 d): two partial d-vectors of doubles per slab
__host__ __device__ inline ColsqPlan colmom_plan(int64_t N, int64_t d, int vec)
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
    const int64_t step = (int64_t)(COLSQ_BLOCK / tc) * COLSQ_U;
    int64_t want = COLSQ_WG_TARGET / pl.panels;
    const int64_t cap = COLSQ_WS_BYTES / (16 * d);
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

// partial[y * d + j] = sum over the rows of slab y of (A[i,j] - c_j), partial[(gridDim.y + y) * d + j] = the same of its square;
// c_j = shift[j], or A[0,j] where shift is NULL.  VEC16: the base of A and ld are multiples of 16 bytes.
template <typename T, bool VEC16>
__global__ void __launch_bounds__(COLSQ_BLOCK)
    colmom_partial_kernel(const T *A, int64_t N, int64_t d, int64_t ld, int64_t slab, int tc_log2, const double *shift, double *partial)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr int U = COLSQ_U;
    typedef T VecT __attribute__((ext_vector_type(VEC)));
    __shared__ double lds[2][COLSQ_BLOCK * VEC];
    const int tc = 1 << tc_log2, tr = COLSQ_BLOCK >> tc_log2;
    const int c = (int)threadIdx.x & (tc - 1), r = (int)threadIdx.x >> tc_log2;
    const int64_t col = ((int64_t)blockIdx.x * tc + c) * VEC;
    const int64_t lo = (int64_t)blockIdx.y * slab;
    const int64_t hi = lo + slab < N ? lo + slab : N;
    double a1[VEC], a2[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) a1[j] = a2[j] = 0.0;
    if (col < d) {
        const T *base = A + col;
        bool ok[VEC];
        double cj[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            ok[j] = col + j < d;
            cj[j] = !ok[j] ? 0.0 : shift ? shift[col + j] : (double)base[j];
        }
        int64_t row = lo + r;
        if (VEC16 && col + VEC <= d) {
            for (; row + (int64_t)(U - 1) * tr < hi; row += (int64_t)U * tr) {
                VecT v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(reinterpret_cast<const VecT *>(base + (row + (int64_t)u * tr) * ld));
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        const double t = (double)v[u][j] - cj[j];
                        a1[j] += t;
                        a2[j] += t * t;
                    }
            }
            for (; row < hi; row += tr) {
                const VecT v = __builtin_nontemporal_load(reinterpret_cast<const VecT *>(base + row * ld));
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const double t = (double)v[j] - cj[j];
                    a1[j] += t;
                    a2[j] += t * t;
                }
            }
        } else {
            for (; row + (int64_t)(U - 1) * tr < hi; row += (int64_t)U * tr) {
                T v[U][VEC];
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int j = 0; j < VEC; ++j) v[u][j] = ok[j] ? __builtin_nontemporal_load(base + (row + (int64_t)u * tr) * ld + j) : T(0);
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        const double t = (double)v[u][j] - cj[j];
                        a1[j] += t;
                        a2[j] += t * t;
                    }
            }
            for (; row < hi; row += tr) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const T v = ok[j] ? __builtin_nontemporal_load(base + row * ld + j) : T(0);
                    const double t = (double)v - cj[j];
                    a1[j] += t;
                    a2[j] += t * t;
                }
            }
        }
    }
    // the tr row groups -> one, in the order r = 0, 1, ..., by the thread of row group 0 that owns the chunk
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        lds[0][(int)threadIdx.x * VEC + j] = a1[j];
        lds[1][(int)threadIdx.x * VEC + j] = a2[j];
    }
    __syncthreads();
    if (r == 0 && col < d) {
        double *out1 = partial + (int64_t)blockIdx.y * d + col;
        double *out2 = partial + ((int64_t)gridDim.y + blockIdx.y) * d + col;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            if (col + j < d) {
                double s = lds[0][c * VEC + j], q = lds[1][c * VEC + j];
                for (int rr = 1; rr < tr; ++rr) {
                    s += lds[0][(rr * tc + c) * VEC + j];
                    q += lds[1][(rr * tc + c) * VEC + j];
                }
                out1[j] = s;
                out2[j] = q;
            }
        }
    }
}

// s1[j] (blockIdx.y = 0) / s2[j] (1) = the nslab partials of column j in slab order: thread (c, g) adds the g-th quarter of the slabs
// (contiguous, in order), the four quarters are added in order through LDS -- colsq_final_kernel's order
template <typename T>
__global__ void __launch_bounds__(COLSQ_BLOCK) colmom_final_kernel(int64_t d, int nslab, const double *partial, double *s1, double *s2)
{
    __shared__ double lds[COLSQ_FR][COLSQ_FC];
    const int c = (int)threadIdx.x & (COLSQ_FC - 1), g = (int)threadIdx.x / COLSQ_FC;
    const int64_t col = (int64_t)blockIdx.x * COLSQ_FC + c;
    const int per = (nslab + COLSQ_FR - 1) / COLSQ_FR;
    const int y0 = g * per;
    const int y1 = y0 + per < nslab ? y0 + per : nslab;
    double s = 0.0;
    if (col < d) {
        const double *p = partial + (int64_t)blockIdx.y * nslab * d + col;
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
        (blockIdx.y ? s2 : s1)[col] = t;
    }
}

// out[i,j] = (T)(((double)A[i,j] - center_j) * scale_j); NULL center = 0, NULL scale = 1.  out may be A (with ldo == ld): no __restrict__.
// VEC16: both bases and both strides are multiples of 16 bytes.
template <typename T, bool VEC16>
__global__ void __launch_bounds__(COLSQ_BLOCK)
    colscale_kernel(const T *A, int64_t N, int64_t d, int64_t ld, int64_t slab, int tc_log2, const double *center, const double *scale, T *out,
                    int64_t ldo)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr int U = COLSQ_U;
    typedef T VecT __attribute__((ext_vector_type(VEC)));
    const int tc = 1 << tc_log2, tr = COLSQ_BLOCK >> tc_log2;
    const int c = (int)threadIdx.x & (tc - 1), r = (int)threadIdx.x >> tc_log2;
    const int64_t col = ((int64_t)blockIdx.x * tc + c) * VEC;
    if (col >= d) return;
    const int64_t lo = (int64_t)blockIdx.y * slab;
    const int64_t hi = lo + slab < N ? lo + slab : N;
    const T *base = A + col;
    T *obase = out + col;
    bool ok[VEC];
    double cj[VEC], sj[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        ok[j] = col + j < d;
        cj[j] = ok[j] && center ? center[col + j] : 0.0;
        sj[j] = ok[j] && scale ? scale[col + j] : 1.0;
    }
    int64_t row = lo + r;
    if (VEC16 && col + VEC <= d) {
        for (; row + (int64_t)(U - 1) * tr < hi; row += (int64_t)U * tr) {
            VecT v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(reinterpret_cast<const VecT *>(base + (row + (int64_t)u * tr) * ld));
#pragma unroll
            for (int u = 0; u < U; ++u) {
                VecT w;
#pragma unroll
                for (int j = 0; j < VEC; ++j) w[j] = (T)(((double)v[u][j] - cj[j]) * sj[j]);
                __builtin_nontemporal_store(w, reinterpret_cast<VecT *>(obase + (row + (int64_t)u * tr) * ldo));
            }
        }
        for (; row < hi; row += tr) {
            const VecT v = __builtin_nontemporal_load(reinterpret_cast<const VecT *>(base + row * ld));
            VecT w;
#pragma unroll
            for (int j = 0; j < VEC; ++j) w[j] = (T)(((double)v[j] - cj[j]) * sj[j]);
            __builtin_nontemporal_store(w, reinterpret_cast<VecT *>(obase + row * ldo));
        }
    } else {
        for (; row + (int64_t)(U - 1) * tr < hi; row += (int64_t)U * tr) {
            T v[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < VEC; ++j) v[u][j] = ok[j] ? __builtin_nontemporal_load(base + (row + (int64_t)u * tr) * ld + j) : T(0);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < VEC; ++j)
                    if (ok[j]) __builtin_nontemporal_store((T)(((double)v[u][j] - cj[j]) * sj[j]), obase + (row + (int64_t)u * tr) * ldo + j);
        }
        for (; row < hi; row += tr) {
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                if (ok[j]) {
                    const T v = __builtin_nontemporal_load(base + row * ld + j);
                    __builtin_nontemporal_store((T)(((double)v - cj[j]) * sj[j]), obase + row * ldo + j);
                }
        }
    }
}

}  // namespace ciao

// colmom_kernels.h -- column standardisation (ciao_col_moments, ciao_scale_columns).
//
// Shifted column moments, s1[j] = sum_i (A[i,j] - c_j) and s2[j] = sum_i (A[i,j] - c_j)^2 over the N resident rows, c = a device d-vector
// of doubles or (NULL) the first resident row: ONE pass over A, every element read once, 16-byte non-temporal loads; the difference
// (double)a - c_j, its square and every addition in double.  The decomposition is col_walk.h's, shared with colsq_kernels.h: the same
// plan, walk, combine and final sum, so every bit of both sums is the same for every layout of the same matrix.  colmom_partial_kernel
// leaves TWO partial d-panels per workgroup in the context's workspace (all s1 panels, then all s2 panels), colmom_final_kernel adds the
// partials of each column in slab order (blockIdx.y: which of the two sums).  No atomics, no scratch.
//
// Scaling, out[i,j] = (T)(((double)a_ij - center_j) * scale_j): one subtraction and one multiplication in double (no contraction: the units
// are built with -ffp-contract=off), one rounding to T.  colscale_kernel walks the same slabs and panels; a thread keeps its chunk of
// center / scale in registers, loads COLSQ_U rows, then stores them: every element is read and written by the SAME thread and a row is
// loaded before it is stored, so out may be A itself.  16-byte loads and stores where both bases and both strides allow, element by
// element otherwise; the columns [d, ld_out) of a row are never written.
#pragma once

#include <type_traits>

#include "colsq_kernels.h"

namespace ciao {

// two partial d-vectors per slab.  ciao_scale_columns leaves none, and walks the slabs of the moments all the same.
__host__ __device__ inline ColsqPlan colmom_plan(int64_t N, int64_t d, int vec) { return col_plan(N, d, vec, 2); }

// partial[y * d + j] = sum over the rows of slab y of (A[i,j] - c_j), partial[(gridDim.y + y) * d + j] = the same of its square;
// c_j = shift[j], or A[0,j] where shift is NULL.  VEC16: the base of A and ld are multiples of 16 bytes.
template <typename T, bool VEC16>
__global__ void __launch_bounds__(COLSQ_BLOCK)
    colmom_partial_kernel(const T *A, int64_t N, int64_t d, int64_t ld, int64_t slab, int tc_log2, const double *shift, double *partial)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    const int tc = 1 << tc_log2, tr = COLSQ_BLOCK >> tc_log2;
    const int c = (int)threadIdx.x & (tc - 1), r = (int)threadIdx.x >> tc_log2;
    const int64_t col = ((int64_t)blockIdx.x * tc + c) * VEC;
    const int64_t lo = (int64_t)blockIdx.y * slab;
    const int64_t hi = lo + slab < N ? lo + slab : N;
    double acc[2][VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[0][j] = acc[1][j] = 0.0;
    if (col < d) {
        const T *base = A + col;
        double cj[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) cj[j] = col + j >= d ? 0.0 : shift ? shift[col + j] : (double)base[j];
        col_walk<T, VEC16>(base, ld, lo + r, hi, tr, col, d, [&](int64_t, const auto &v) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const double t = (double)v[j] - cj[j];
                acc[0][j] += t;
                acc[1][j] += t * t;
            }
        });
    }
    col_combine(acc, tc, tr, c, r, col, d, partial);
}

// s1[j] (blockIdx.y = 0) / s2[j] (1) = the nslab partials of column j in slab order (col_final)
template <typename T>
__global__ void __launch_bounds__(COLSQ_BLOCK) colmom_final_kernel(int64_t d, int nslab, const double *partial, double *s1, double *s2)
{
    col_final(d, nslab, partial + (int64_t)blockIdx.y * nslab * d, blockIdx.y ? s2 : s1);
}

// out[i,j] = (T)(((double)A[i,j] - center_j) * scale_j); NULL center = 0, NULL scale = 1.  out may be A (with ldo == ld): no __restrict__.
// VEC16: both bases and both strides are multiples of 16 bytes.
template <typename T, bool VEC16>
__global__ void __launch_bounds__(COLSQ_BLOCK)
    colscale_kernel(const T *A, int64_t N, int64_t d, int64_t ld, int64_t slab, int tc_log2, const double *center, const double *scale, T *out,
                    int64_t ldo)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    typedef T VecT __attribute__((ext_vector_type(VEC)));
    const int tc = 1 << tc_log2, tr = COLSQ_BLOCK >> tc_log2;
    const int c = (int)threadIdx.x & (tc - 1), r = (int)threadIdx.x >> tc_log2;
    const int64_t col = ((int64_t)blockIdx.x * tc + c) * VEC;
    if (col >= d) return;
    const int64_t lo = (int64_t)blockIdx.y * slab;
    const int64_t hi = lo + slab < N ? lo + slab : N;
    T *obase = out + col;
    bool ok[VEC];
    double cj[VEC], sj[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        ok[j] = col + j < d;
        cj[j] = ok[j] && center ? center[col + j] : 0.0;
        sj[j] = ok[j] && scale ? scale[col + j] : 1.0;
    }
    col_walk<T, VEC16>(A + col, ld, lo + r, hi, tr, col, d, [&](int64_t row, const auto &v) {
        if constexpr (std::is_same_v<decltype(v), const VecT &>) {   // a whole chunk: one 16-byte store
            VecT w;
#pragma unroll
            for (int j = 0; j < VEC; ++j) w[j] = (T)(((double)v[j] - cj[j]) * sj[j]);
            __builtin_nontemporal_store(w, reinterpret_cast<VecT *>(obase + row * ldo));
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                if (ok[j]) __builtin_nontemporal_store((T)(((double)v[j] - cj[j]) * sj[j]), obase + row * ldo + j);
        }
    });
}

}  // namespace ciao

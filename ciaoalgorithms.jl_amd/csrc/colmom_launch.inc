// colmom_launch.inc -- host side of the standardisation kernels (colmom_kernels.h); included once per element type with CIAO_T defined
#include "colmom_kernels.h"
#include "launch.h"

namespace ciao {

// s1[j] = sum_i (A[i,j] - c_j), s2[j] = sum_i (A[i,j] - c_j)^2 (device, d doubles each); c = shift, or the first row where shift is NULL.
// The partials live in ctx->partial: 2 * nslab * d doubles, at most COLSQ_WS_BYTES (or two d-vectors where that alone is more).  Slabs,
// panels and grid come from colmom_plan(N, d); only the KIND of load depends on the layout.
template <>
int32_t launch_colmom<CIAO_T>(ciao_ctx *ctx, const ciao_problem *p, const double *shift, double *s1, double *s2)
{
    using T = CIAO_T;
    constexpr int VEC = 16 / (int)sizeof(T);
    const ColsqPlan pl = colmom_plan(p->N, p->d, VEC);
    CIAO_TRY(ensure(ctx, &ctx->partial, &ctx->partial_bytes, 2 * (size_t)pl.nslab * (size_t)p->d * sizeof(double)));
    double *partial = (double *)ctx->partial;
    const bool vec16 = col_vec16<T>(p->A, p->ld);
    const dim3 grid((unsigned)pl.panels, (unsigned)pl.nslab);
    if (vec16)
        hipLaunchKernelGGL((colmom_partial_kernel<T, true>), grid, dim3(COLSQ_BLOCK), 0, ctx->stream, (const T *)p->A, p->N, p->d, p->ld, pl.slab,
                           pl.tc_log2, shift, partial);
    else
        hipLaunchKernelGGL((colmom_partial_kernel<T, false>), grid, dim3(COLSQ_BLOCK), 0, ctx->stream, (const T *)p->A, p->N, p->d, p->ld, pl.slab,
                           pl.tc_log2, shift, partial);
    CIAO_HIP(hipGetLastError());
    hipLaunchKernelGGL((colmom_final_kernel<T>), dim3((unsigned)((p->d + COLSQ_FC - 1) / COLSQ_FC), 2), dim3(COLSQ_BLOCK), 0, ctx->stream, p->d,
                       (int)pl.nslab, (const double *)partial, s1, s2);
    CIAO_HIP(hipGetLastError());
    ctx->last_kernel = col_report<T>("colmom_partial_kernel", vec16, pl) + (shift ? " shift=given" : " shift=row0");
    return CIAO_OK;
}

// out[i,j] = (T)(((double)A[i,j] - center_j) * scale_j) over the same slabs and panels; no workspace
template <>
int32_t launch_colscale<CIAO_T>(ciao_ctx *ctx, const ciao_problem *p, const double *center, const double *scale, void *out, int64_t ld_out)
{
    using T = CIAO_T;
    constexpr int VEC = 16 / (int)sizeof(T);
    const ColsqPlan pl = colmom_plan(p->N, p->d, VEC);
    const bool vec16 = col_vec16<T>(p->A, p->ld) && col_vec16<T>(out, ld_out);
    const dim3 grid((unsigned)pl.panels, (unsigned)pl.nslab);
    if (vec16)
        hipLaunchKernelGGL((colscale_kernel<T, true>), grid, dim3(COLSQ_BLOCK), 0, ctx->stream, (const T *)p->A, p->N, p->d, p->ld, pl.slab,
                           pl.tc_log2, center, scale, (T *)out, ld_out);
    else
        hipLaunchKernelGGL((colscale_kernel<T, false>), grid, dim3(COLSQ_BLOCK), 0, ctx->stream, (const T *)p->A, p->N, p->d, p->ld, pl.slab,
                           pl.tc_log2, center, scale, (T *)out, ld_out);
    CIAO_HIP(hipGetLastError());
    ctx->last_kernel = col_report<T>("colscale_kernel", vec16, pl) + (out == p->A ? " in place" : "");
    return CIAO_OK;
}

}  // namespace ciao

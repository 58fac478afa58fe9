// colsq_launch.inc -- host side of the screening kernels (colsq_kernels.h); included once per element type with CIAO_T defined
#include "colsq_kernels.h"
#include "launch.h"

namespace ciao {


// out[j] = sum_i A[i,j]^2 (device, d doubles).  The partials live in ctx->partial: nslab * d doubles, at most COLSQ_WS_BYTES (or one
// d-vector where that alone is more).  Slabs, panels and grid come from colsq_plan(N, d); only the KIND of load depends on the layout.
template <>
int32_t launch_colsq<CIAO_T>(ciao_ctx *ctx, const ciao_problem *p, double *out)
{
    using T = CIAO_T;
    constexpr int VEC = 16 / (int)sizeof(T);
    const ColsqPlan pl = colsq_plan(p->N, p->d, VEC);
    CIAO_TRY(ensure(ctx, &ctx->partial, &ctx->partial_bytes, (size_t)pl.nslab * (size_t)p->d * sizeof(double)));
    double *partial = (double *)ctx->partial;
    const bool vec16 = col_vec16<T>(p->A, p->ld);
    const dim3 grid((unsigned)pl.panels, (unsigned)pl.nslab);
    if (vec16)
        hipLaunchKernelGGL((colsq_partial_kernel<T, true>), grid, dim3(COLSQ_BLOCK), 0, ctx->stream, (const T *)p->A, p->N, p->d, p->ld, pl.slab,
                           pl.tc_log2, partial);
    else
        hipLaunchKernelGGL((colsq_partial_kernel<T, false>), grid, dim3(COLSQ_BLOCK), 0, ctx->stream, (const T *)p->A, p->N, p->d, p->ld, pl.slab,
                           pl.tc_log2, partial);
    CIAO_HIP(hipGetLastError());
    hipLaunchKernelGGL((colsq_final_kernel<T>), dim3((unsigned)((p->d + COLSQ_FC - 1) / COLSQ_FC)), dim3(COLSQ_BLOCK), 0, ctx->stream, p->d,
                       (int)pl.nslab, (const double *)partial, out);
    CIAO_HIP(hipGetLastError());
    ctx->last_kernel = col_report<T>("colsq_partial_kernel", vec16, pl);
    return CIAO_OK;
}

// keep[k] and the kept count (cnt, one device double): rec = cert_grid(d) * CERT_REC doubles of workspace
template <>
int32_t launch_screen<CIAO_T>(ciao_ctx *ctx, int64_t d, const void *grad, const double *colsq, double s, double kappa, double mu,
                              uint8_t *keep, double *rec, double *cnt)
{
    using T = CIAO_T;
    const int64_t slice = cert_slice(d);
    const int grid = cert_grid(d);
    hipLaunchKernelGGL((screen_kernel<T>), dim3(grid), dim3(CERT_BLOCK), 0, ctx->stream, d, slice, (const T *)grad, colsq, s, kappa, mu, keep, rec);
    CIAO_HIP(hipGetLastError());
    hipLaunchKernelGGL((screen_count_kernel<T>), dim3(1), dim3(CERT_BLOCK), 0, ctx->stream, grid, (const double *)rec, cnt);
    CIAO_HIP(hipGetLastError());
    char buf[96];
    snprintf(buf, sizeof buf, "colsq_screen_kernel<%s> grid=%d block=%d", sizeof(T) == 8 ? "f64" : "f32", grid, CERT_BLOCK);
    ctx->last_kernel = buf;
    return CIAO_OK;
}

}  // namespace ciao

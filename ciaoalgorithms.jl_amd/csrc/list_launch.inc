// list_launch.inc -- host side of the row-list passes (list_kernels.h); included once per element type with CIAO_T defined
#include "list_kernels.h"
#include "launch.h"

namespace ciao {

// out[m] = a_{idx[m]}' x (device, M >= 1 doubles); idx = M device int64 row numbers or NULL (position = row, M = N).  Groups, mode,
// rows per workgroup and grid come from rowsq_plan(M, d); only the KIND of load depends on the layout of A.
template <>
int32_t launch_listdot<CIAO_T>(ciao_ctx *ctx, const ciao_problem *p, const int64_t *idx, int64_t M, const void *x, double *out)
{
    using T = CIAO_T;
    constexpr int VEC = 16 / (int)sizeof(T);
    static_assert(LIST_MAX_D * (int)sizeof(T) <= 32768, "x of listdot_kernel lives in LDS");
    const RowsqPlan pl = rowsq_plan(M, p->d, VEC);
    const bool vec16 = col_vec16<T>(p->A, p->ld);
    const dim3 grid((unsigned)pl.grid);
#define CIAO_LISTDOT(V, I)                                                                                                                  \
    hipLaunchKernelGGL((listdot_kernel<T, V, I>), grid, dim3(ROWSQ_BLOCK), 0, ctx->stream, (const T *)p->A, p->N, p->d, p->ld, idx, M,      \
                       (const T *)x, pl.rows_per_wg, pl.g_log2, pl.mode, out)
    if (vec16) {
        if (idx)
            CIAO_LISTDOT(true, true);
        else
            CIAO_LISTDOT(true, false);
    } else {
        if (idx)
            CIAO_LISTDOT(false, true);
        else
            CIAO_LISTDOT(false, false);
    }
#undef CIAO_LISTDOT
    CIAO_HIP(hipGetLastError());
    char buf[160];
    snprintf(buf, sizeof buf, "listdot_kernel<%s,%s%s> grid=%lld block=%d G=%d mode=%d rows_per_wg=%lld", sizeof(T) == 8 ? "f64" : "f32",
             vec16 ? "vec16" : "elem", idx ? ",rows" : "", (long long)pl.grid, ROWSQ_BLOCK, 1 << pl.g_log2, pl.mode, (long long)pl.rows_per_wg);
    ctx->last_kernel = buf;
    return CIAO_OK;
}

// out[j] = sum_m c[m] A[idx[m], j] (device, d doubles), M >= 1.  The partials live in ctx->partial: nslab * d doubles.  Slabs, panels
// and grid come from col_plan(M, d, VEC, 1).
template <>
int32_t launch_listcomb<CIAO_T>(ciao_ctx *ctx, const ciao_problem *p, const int64_t *idx, int64_t M, const double *c, double *out)
{
    using T = CIAO_T;
    constexpr int VEC = 16 / (int)sizeof(T);
    const ColsqPlan pl = col_plan(M, p->d, VEC, 1);
    CIAO_TRY(ensure(ctx, &ctx->partial, &ctx->partial_bytes, (size_t)pl.nslab * (size_t)p->d * sizeof(double)));
    double *partial = (double *)ctx->partial;
    const bool vec16 = col_vec16<T>(p->A, p->ld);
    const dim3 grid((unsigned)pl.panels, (unsigned)pl.nslab);
#define CIAO_LISTCOMB(V, I)                                                                                                                 \
    hipLaunchKernelGGL((listcomb_partial_kernel<T, V, I>), grid, dim3(COLSQ_BLOCK), 0, ctx->stream, (const T *)p->A, p->N, p->d, p->ld, idx, \
                       M, c, pl.slab, pl.tc_log2, partial)
    if (vec16) {
        if (idx)
            CIAO_LISTCOMB(true, true);
        else
            CIAO_LISTCOMB(true, false);
    } else {
        if (idx)
            CIAO_LISTCOMB(false, true);
        else
            CIAO_LISTCOMB(false, false);
    }
#undef CIAO_LISTCOMB
    CIAO_HIP(hipGetLastError());
    hipLaunchKernelGGL((listcomb_final_kernel<T>), dim3((unsigned)((p->d + COLSQ_FC - 1) / COLSQ_FC)), dim3(COLSQ_BLOCK), 0, ctx->stream, p->d,
                       (int)pl.nslab, (const double *)partial, out);
    CIAO_HIP(hipGetLastError());
    ctx->last_kernel = col_report<T>("listcomb_partial_kernel", vec16, pl) + (idx ? ",rows" : "");
    return CIAO_OK;
}

}  // namespace ciao

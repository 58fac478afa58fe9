// rowsq_launch.inc -- host side of the row sums of squares (rowsq_kernels.h); included once per element type with CIAO_T defined
#include "rowsq_kernels.h"
#include "launch.h"

namespace ciao {


// out[i] = sum_j A[i,j]^2 (device, N doubles, or NULL) and one record per workgroup in rec; res non-NULL: rowsq_final_kernel leaves
// {max, argmax, min, sum} there.  Groups, mode, rows per workgroup and grid come from rowsq_plan(N, d); only the KIND of load depends
// on the layout.
template <>
int32_t launch_rowsq<CIAO_T>(ciao_ctx *ctx, const ciao_problem *p, double *out, double *rec, double *res)
{
    using T = CIAO_T;
    constexpr int VEC = 16 / (int)sizeof(T);
    const RowsqPlan pl = rowsq_plan(p->N, p->d, VEC);
    if (pl.grid > ROWSQ_WG_TARGET) {
        set_error("ciao_row_sqnorms: the plan asks for %lld records, the workspace holds %d", (long long)pl.grid, ROWSQ_WG_TARGET);
        return CIAO_ERR_UNSUPPORTED;
    }
    const bool vec16 = (reinterpret_cast<uintptr_t>(p->A) & 15u) == 0 && ((size_t)p->ld * sizeof(T)) % 16 == 0;
    const dim3 grid((unsigned)pl.grid);
    if (vec16)
        hipLaunchKernelGGL((rowsq_partial_kernel<T, true>), grid, dim3(ROWSQ_BLOCK), 0, ctx->stream, (const T *)p->A, p->N, p->d, p->ld,
                           pl.rows_per_wg, pl.g_log2, pl.mode, pl.quarter, out, rec);
    else
        hipLaunchKernelGGL((rowsq_partial_kernel<T, false>), grid, dim3(ROWSQ_BLOCK), 0, ctx->stream, (const T *)p->A, p->N, p->d, p->ld,
                           pl.rows_per_wg, pl.g_log2, pl.mode, pl.quarter, out, rec);
    CIAO_HIP(hipGetLastError());
    if (res) {
        hipLaunchKernelGGL((rowsq_final_kernel<T>), dim3(1), dim3(ROWSQ_BLOCK), 0, ctx->stream, (int)pl.grid, (const double *)rec, res);
        CIAO_HIP(hipGetLastError());
    }
    char buf[160];
    snprintf(buf, sizeof buf, "rowsq_partial_kernel<%s,%s> grid=%lld block=%d G=%d mode=%d rows_per_wg=%lld%s", sizeof(T) == 8 ? "f64" : "f32",
             vec16 ? "vec16" : "elem", (long long)pl.grid, ROWSQ_BLOCK, 1 << pl.g_log2, pl.mode, (long long)pl.rows_per_wg,
             res ? " +final" : "");
    ctx->last_kernel = buf;
    return CIAO_OK;
}

}  // namespace ciao

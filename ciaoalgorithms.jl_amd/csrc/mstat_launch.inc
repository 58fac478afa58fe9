// mstat_launch.inc -- host side of the per-sample reduction (mstat_kernels.h); included once per element type with CIAO_T defined
#include "mstat_kernels.h"
#include "launch.h"

namespace ciao {


// rec: cert_grid(N) * CERT_REC doubles of workspace; out: the four results (both device memory).  M_dev non-null: s is formed on the
// device from *M_dev and mu (mu <= 0: s = 1 is passed as the literal instead).
template <>
int32_t launch_mstat<CIAO_T>(ciao_ctx *ctx, int loss, int64_t N, const void *dots, const void *b, double s, const double *M_dev, double mu,
                             double *rec, double *out)
{
    using T = CIAO_T;
    const int64_t slice = cert_slice(N);
    const int grid = cert_grid(N);
    const int vec16 = ((reinterpret_cast<uintptr_t>(dots) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0;
    if (loss == CIAO_LOSS_LOGISTIC) {
        hipLaunchKernelGGL((mstat_partial_kernel<T, CIAO_LOSS_LOGISTIC>), dim3(grid), dim3(CERT_BLOCK), 0, ctx->stream, N, slice, (const T *)dots,
                           (const T *)b, s, M_dev, mu, vec16, rec);
        CIAO_HIP(hipGetLastError());
        hipLaunchKernelGGL((mstat_final_kernel<T, CIAO_LOSS_LOGISTIC>), dim3(1), dim3(CERT_BLOCK), 0, ctx->stream, grid, (const double *)rec, out);
    } else {
        hipLaunchKernelGGL((mstat_partial_kernel<T, CIAO_LOSS_LS>), dim3(grid), dim3(CERT_BLOCK), 0, ctx->stream, N, slice, (const T *)dots,
                           (const T *)b, s, M_dev, mu, vec16, rec);
        CIAO_HIP(hipGetLastError());
        hipLaunchKernelGGL((mstat_final_kernel<T, CIAO_LOSS_LS>), dim3(1), dim3(CERT_BLOCK), 0, ctx->stream, grid, (const double *)rec, out);
    }
    CIAO_HIP(hipGetLastError());
    char buf[96];
    snprintf(buf, sizeof buf, "mstat_partial_kernel<%s,%s> grid=%d block=%d", sizeof(T) == 8 ? "f64" : "f32",
             loss == CIAO_LOSS_LOGISTIC ? "logistic" : "ls", grid, CERT_BLOCK);
    ctx->last_kernel = buf;
    return CIAO_OK;
}

}  // namespace ciao

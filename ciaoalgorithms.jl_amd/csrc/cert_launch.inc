// cert_launch.inc -- host side of the certificate's reduction (cert_kernels.h); included once per element type with CIAO_T defined
#include "cert_kernels.h"
#include "launch.h"

namespace ciao {


// rec: cert_grid(d) * CERT_REC doubles of workspace; out: the five results (both device memory)
template <>
int32_t launch_cert<CIAO_T>(ciao_ctx *ctx, int64_t d, const ciao_prox_desc *g, const void *x, const void *av, double gamma, double *rec,
                            double *out)
{
    using T = CIAO_T;
    const int64_t slice = cert_slice(d);
    const int grid = cert_grid(d);
    const int vec16 = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(av)) & 15u) == 0;
    hipLaunchKernelGGL((cert_partial_kernel<T>), dim3(grid), dim3(CERT_BLOCK), 0, ctx->stream, d, slice, make_prox<T>(g), (const T *)x,
                       (const T *)av, (T)gamma, vec16, rec);
    CIAO_HIP(hipGetLastError());
    hipLaunchKernelGGL((cert_final_kernel<T>), dim3(1), dim3(CERT_BLOCK), 0, ctx->stream, grid, (const double *)rec, out);
    CIAO_HIP(hipGetLastError());
    char buf[96];
    snprintf(buf, sizeof buf, "cert_partial_kernel<%s> grid=%d block=%d", sizeof(T) == 8 ? "f64" : "f32", grid, CERT_BLOCK);
    ctx->last_kernel = buf;
    return CIAO_OK;
}

}  // namespace ciao

// chain_cdma_launch.inc -- host dispatch of chain_cdma_kernel (complex chains on the LDS-DMA ring) for one real type (CIAO_T);
// units of their own (chain_cdma_f32/f64.hip) so that the build spreads over the cores.

#include "chain_dma_kernels.h"
#include "ciao_ctx.h"
#include "launch.h"

namespace ciao {

namespace {
template <typename T, int ALG, int J, bool MASKED>
int32_t launch_cdma_jm(ciao_ctx *ctx, ChainArgs<T> &a)
{
    constexpr size_t lds = chain_cdma_lds_bytes<T, J, ALG>();
    static_assert(lds <= 160 * 1024, "LDS budget");
    auto kern = &chain_cdma_kernel<T, J, ALG, MASKED>;
    if (lds > 60 * 1024)
        CIAO_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(1), dim3(CHAIN_NT), lds, ctx->stream, a);
    return CIAO_OK;
}
template <typename T, int ALG>
int32_t launch_cdma_a(ciao_ctx *ctx, int J, bool masked, ChainArgs<T> &a)
{
    switch (J) {
        case 1: return masked ? launch_cdma_jm<T, ALG, 1, true>(ctx, a) : launch_cdma_jm<T, ALG, 1, false>(ctx, a);
        case 2: return masked ? launch_cdma_jm<T, ALG, 2, true>(ctx, a) : launch_cdma_jm<T, ALG, 2, false>(ctx, a);
        case 4: return masked ? launch_cdma_jm<T, ALG, 4, true>(ctx, a) : launch_cdma_jm<T, ALG, 4, false>(ctx, a);
        default: set_error("internal: bad J %d for the complex LDS-DMA chain", J); return CIAO_ERR_UNSUPPORTED;
    }
}
}  // namespace

template <>
int32_t launch_cdma<CIAO_T>(ciao_ctx *ctx, int alg, int J, bool masked, ChainArgs<CIAO_T> &a)
{
    switch (alg) {
        case CA_SVRG: return launch_cdma_a<CIAO_T, CA_SVRG>(ctx, J, masked, a);
        case CA_SAGA: return launch_cdma_a<CIAO_T, CA_SAGA>(ctx, J, masked, a);
        case CA_FINITO: return launch_cdma_a<CIAO_T, CA_FINITO>(ctx, J, masked, a);
        case CA_LFINITO: return launch_cdma_a<CIAO_T, CA_LFINITO>(ctx, J, masked, a);
        default: set_error("internal: bad chain alg %d", alg); return CIAO_ERR_ARG;
    }
}

}  // namespace ciao

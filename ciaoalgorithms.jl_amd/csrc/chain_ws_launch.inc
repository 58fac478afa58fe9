// chain_ws_launch.inc -- host dispatch of chain_ws_kernel (the wave-specialised chain) for one real type (CIAO_T) and one
// algorithm (CIAO_WS_ALG): the instantiations are what takes the compile time, so they are spread over translation units.

#include "chain_ws_kernels.h"
#include "ciao_ctx.h"
#include "launch.h"

namespace ciao {

namespace {
template <typename T, int ALG, int LOSS, int J, bool MASKED, int NISS>
int32_t launch_ws_jmn(ciao_ctx *ctx, ChainArgs<T> &a)
{
    constexpr size_t lds = WsLayout<T, J, ALG>::total;
    static_assert(lds <= 160 * 1024, "LDS budget");
    auto kern = &chain_ws_kernel<T, J, ALG, LOSS, MASKED, NISS>;
    if (lds > 60 * 1024)
        CIAO_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(1), dim3((WS_NCW + 1 + NISS) * WAVE), lds, ctx->stream, a);
    return CIAO_OK;
}

}  // namespace

// rows of up to 4 KiB (J = 1; beyond, chain_dma_kernel is faster); the issuer count, 1 or 2, is plan_chain's decision (chain_launch.inc)
template <typename T, int ALG, int LOSS>
int32_t launch_ws(ciao_ctx *ctx, int issuers, bool masked, ChainArgs<T> &a)
{
    if (issuers == 1)
        return masked ? launch_ws_jmn<T, ALG, LOSS, 1, true, 1>(ctx, a) : launch_ws_jmn<T, ALG, LOSS, 1, false, 1>(ctx, a);
    return masked ? launch_ws_jmn<T, ALG, LOSS, 1, true, 2>(ctx, a) : launch_ws_jmn<T, ALG, LOSS, 1, false, 2>(ctx, a);
}

template int32_t launch_ws<CIAO_T, CIAO_WS_ALG, CIAO_LOSS_LS>(ciao_ctx *, int, bool, ChainArgs<CIAO_T> &);
template int32_t launch_ws<CIAO_T, CIAO_WS_ALG, CIAO_LOSS_LOGISTIC>(ciao_ctx *, int, bool, ChainArgs<CIAO_T> &);

}  // namespace ciao

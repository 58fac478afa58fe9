// gramcdg_launch.inc -- host side of the general coordinate-descent kernels (gramcdg_kernels.h); a unit of its own (gramcdg.hip) beside
// gramcd.hip, so that gramcd_kernel's four instantiations are compiled from the text they always were
#include "gramcdg_kernels.h"
#include "launch.h"

namespace ciao {

template <int BLOCK, bool VEC>
static int32_t gramcdg_go(ciao_ctx *ctx, const GramCdgPlan &pl, const GramCdgArgs &a)
{
    auto kern = &gramcdg_kernel<BLOCK, VEC>;
    if (pl.lds > 60 * 1024)
        CIAO_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, pl.lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)pl.grid), dim3(BLOCK), (size_t)pl.lds, ctx->stream, a);
    CIAO_HIP(hipGetLastError());
    return CIAO_OK;
}

// K models of d coordinates over nsets Gram matrices; the arguments have been checked (api_analysis.hip: ciao_gram_cd_general).  Block, load kind,
// grid and LDS come from gramcdg_plan(d, ldg, sg, alignment of G, K); with one set the set stride plays no part.
int32_t launch_gram_cd_general(ciao_ctx *ctx, const GramCdgArgs &args, int64_t K)
{
    GramCdgArgs a = args;
    if (a.nsets == 1)
        a.sg = 0;
    const GramCdgPlan pl = gramcdg_plan(a.d, a.ldg, a.sg, (reinterpret_cast<uintptr_t>(a.G) & 15u) == 0, K);
    if (pl.block == GRAMCD_SMALL_BLOCK)
        CIAO_TRY(pl.vec16 ? (gramcdg_go<GRAMCD_SMALL_BLOCK, true>(ctx, pl, a)) : (gramcdg_go<GRAMCD_SMALL_BLOCK, false>(ctx, pl, a)));
    else
        CIAO_TRY(pl.vec16 ? (gramcdg_go<GRAMCD_LARGE_BLOCK, true>(ctx, pl, a)) : (gramcdg_go<GRAMCD_LARGE_BLOCK, false>(ctx, pl, a)));
    char buf[192];
    snprintf(buf, sizeof buf, "gramcdg_kernel<%d,%s> grid=%d block=%d lds=%d sets=%d", pl.block, pl.vec16 ? "vec16" : "elem", pl.grid, pl.block, pl.lds,
             a.nsets);
    ctx->last_kernel = buf;
    return CIAO_OK;
}

}  // namespace ciao

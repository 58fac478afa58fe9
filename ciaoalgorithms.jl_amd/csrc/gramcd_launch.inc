// gramcd_launch.inc -- host side of the coordinate-descent kernels (gramcd_kernels.h); state and arithmetic are double whatever the rows
// the Gram matrix came from were, so there is one unit (gramcd.hip)
#include "gramcd_kernels.h"
#include "launch.h"

namespace ciao {

template <int BLOCK, bool VEC>
static int32_t gramcd_go(ciao_ctx *ctx, const GramCdPlan &pl, const GramCdArgs &a)
{
    auto kern = &gramcd_kernel<BLOCK, VEC>;
    if (pl.lds > 60 * 1024)
        CIAO_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, pl.lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)pl.grid), dim3(BLOCK), (size_t)pl.lds, ctx->stream, a);
    CIAO_HIP(hipGetLastError());
    return CIAO_OK;
}

// K models of d coordinates; the arguments have been checked (api_analysis.hip: ciao_gram_cd).  Block, load kind, grid and LDS come from
// gramcd_plan(d, ldg, alignment of G, K).
int32_t launch_gram_cd(ciao_ctx *ctx, int64_t d, int64_t K, const double *G, int64_t ldg, const double *u, const double *inv, const double *tau,
                       double *X, int64_t ldx, double tol, int32_t max_sweeps, double *R, int64_t ldr, double *stat)
{
    const GramCdPlan pl = gramcd_plan(d, ldg, (reinterpret_cast<uintptr_t>(G) & 15u) == 0, K);
    GramCdArgs a{};
    a.G = G;
    a.u = u;
    a.inv = inv;
    a.tau = tau;
    a.X = X;
    a.R = R;
    a.stat = stat;
    a.ldg = ldg;
    a.ldx = ldx;
    a.ldr = ldr;
    a.tol = tol;
    a.d = (int)d;
    a.max_sweeps = max_sweeps;
    if (pl.block == GRAMCD_SMALL_BLOCK)
        CIAO_TRY(pl.vec16 ? (gramcd_go<GRAMCD_SMALL_BLOCK, true>(ctx, pl, a)) : (gramcd_go<GRAMCD_SMALL_BLOCK, false>(ctx, pl, a)));
    else
        CIAO_TRY(pl.vec16 ? (gramcd_go<GRAMCD_LARGE_BLOCK, true>(ctx, pl, a)) : (gramcd_go<GRAMCD_LARGE_BLOCK, false>(ctx, pl, a)));
    char buf[160];
    snprintf(buf, sizeof buf, "gramcd_kernel<%d,%s> grid=%d block=%d lds=%d", pl.block, pl.vec16 ? "vec16" : "elem", pl.grid, pl.block, pl.lds);
    ctx->last_kernel = buf;
    return CIAO_OK;
}

}  // namespace ciao

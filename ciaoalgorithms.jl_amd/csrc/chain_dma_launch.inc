// chain_dma_launch.inc -- host dispatch of chain_dma_kernel (the LDS-DMA fast chain) for one real type (CIAO_T) and one PART
// of the algorithms (CIAO_DMA_PART: 0 = SVRG, 1 = SAGA / SAG, 2 = Finito, 3 = SVRG with cached row dots, 4 = LFinito): the
// instantiations are what takes the compile time, so they are spread over translation units.

#include "chain_dma_kernels.h"
#include "ciao_ctx.h"
#include "launch.h"

namespace ciao {

namespace {
// An open chain batch (ciao_ctx_chain_batch_begin): the launch of a chain kernel is RECORDED -- kernel, block, LDS, argument block,
// the byte ranges of its state and which of them it writes -- and made by ciao_ctx_chain_batch_end, one launch per kernel with one
// workgroup per chain.  Only the chains without a Finito batch structure are taken (SVRG inner cycles, SAGA / SAG steps).
template <typename T, int ALG>
inline int32_t chain_batch_record(ciao_ctx *ctx, const void *kern, unsigned block, size_t lds, const ChainArgs<T> &a)
{
    constexpr bool svrg = (ALG == CA_SVRG || ALG == CA_SVRGC);
    if (!(svrg || ALG == CA_SAGA || ALG == CA_FINITO) || a.nshards > 0) {
        set_error("a chain batch takes SVRG inner cycles, SAGA / SAG steps and small-batch Finito steps of unsharded problems only");
        return CIAO_ERR_UNSUPPORTED;
    }
    ciao_chain_rec r;
    r.kern = kern;
    r.block = block;
    r.lds = lds;
    r.args.assign(reinterpret_cast<const unsigned char *>(&a), reinterpret_cast<const unsigned char *>(&a) + sizeof a);
    const size_t vb = (size_t)a.d * sizeof(T);
    auto range = [&](int k, const void *p, size_t bytes, bool w) {
        r.lo[k] = static_cast<const unsigned char *>(p);
        r.hi[k] = p ? r.lo[k] + bytes : r.lo[k];
        r.wr[k] = w;
    };
    range(0, a.av, vb, !svrg);
    range(1, a.z, vb, true);
    range(2, a.zf, vb, false);
    range(3, a.w, vb, svrg);
    range(4, svrg ? nullptr : a.table, (size_t)a.N * vb, true);
    ctx->batch.push_back(std::move(r));
    return CIAO_OK;
}

// LDS-DMA fast chain: d*sizeof(T) == J * 256 * 16 bytes, 16-byte aligned rows / vectors / table
template <typename T, int ALG, int LOSS, int J, bool MASKED, int NT, bool SHARDED>
int32_t launch_dma_jms(ciao_ctx *ctx, ChainArgs<T> &a)
{
    constexpr size_t lds = chain_dma_lds_bytes<T, J, ALG, NT, SHARDED>();
    static_assert(lds <= 160 * 1024, "LDS budget");
    auto kern = &chain_dma_kernel<T, J, ALG, LOSS, MASKED, NT, SHARDED>;
    if (lds > 60 * 1024)
        CIAO_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (ctx->batch_open) return chain_batch_record<T, ALG>(ctx, reinterpret_cast<const void *>(kern), NT, lds, a);
    hipLaunchKernelGGL(kern, dim3(1), dim3(NT), lds, ctx->stream, a);
    return CIAO_OK;
}

template <typename T, int ALG, int LOSS, int J, bool MASKED, int NT>
int32_t launch_dma_jm(ciao_ctx *ctx, ChainArgs<T> &a)
{
    // the two chains that may run over a shard table (ciao_ctx_set_shards); never the single-wave kernels: plan_chain keeps a
    // sharded problem on four waves (a problem that needs several GPUs does not have 2 KiB rows, and the variants cost build time)
    if constexpr ((ALG == CA_SVRG || ALG == CA_SAGA) && NT != 64) {
        if (a.nshards > 0) return launch_dma_jms<T, ALG, LOSS, J, MASKED, NT, true>(ctx, a);
    }
    if (a.nshards > 0) {
        set_error("internal: chain algorithm %d cannot run over a shard table", ALG);
        return CIAO_ERR_UNSUPPORTED;
    }
    return launch_dma_jms<T, ALG, LOSS, J, MASKED, NT, false>(ctx, a);
}

template <typename T, int ALG, int LOSS, int J, int NT>
int32_t launch_dma_j(ciao_ctx *ctx, bool masked, ChainArgs<T> &a)
{
    return masked ? launch_dma_jm<T, ALG, LOSS, J, true, NT>(ctx, a) : launch_dma_jm<T, ALG, LOSS, J, false, NT>(ctx, a);
}

}  // namespace

// the kernel class (J chunks per thread, NT threads, MASKED) is plan_chain's decision (chain_launch.inc); the six that exist:
template <typename T, int ALG, int LOSS>
int32_t launch_dma(ciao_ctx *ctx, int J, int NT, bool masked, ChainArgs<T> &a)
{
    switch (J * 1000 + NT) {
        case 1064: return launch_dma_j<T, ALG, LOSS, 1, 64>(ctx, masked, a);    // one wave: rows of up to 1 KiB ...
        case 2064: return launch_dma_j<T, ALG, LOSS, 2, 64>(ctx, masked, a);    // ... and up to 2 KiB
        case 1256: return launch_dma_j<T, ALG, LOSS, 1, 256>(ctx, masked, a);   // four waves: 4, 8, 16 KiB
        case 2256: return launch_dma_j<T, ALG, LOSS, 2, 256>(ctx, masked, a);
        case 4256: return launch_dma_j<T, ALG, LOSS, 4, 256>(ctx, masked, a);
        case 4512: return launch_dma_j<T, ALG, LOSS, 4, 512>(ctx, masked, a);   // eight waves: 32 KiB
        default: set_error("internal: no chain_dma_kernel class J=%d NT=%d", J, NT); return CIAO_ERR_UNSUPPORTED;
    }
}

#ifndef CIAO_DMA_LOSS   // both losses in this unit
#define CIAO_DMA_INST(AA)                                                                                   \
    template int32_t launch_dma<CIAO_T, AA, CIAO_LOSS_LS>(ciao_ctx *, int, int, bool, ChainArgs<CIAO_T> &);      \
    template int32_t launch_dma<CIAO_T, AA, CIAO_LOSS_LOGISTIC>(ciao_ctx *, int, int, bool, ChainArgs<CIAO_T> &);
#elif CIAO_DMA_LOSS == 0
#define CIAO_DMA_INST(AA) template int32_t launch_dma<CIAO_T, AA, CIAO_LOSS_LS>(ciao_ctx *, int, int, bool, ChainArgs<CIAO_T> &);
#else
#define CIAO_DMA_INST(AA) template int32_t launch_dma<CIAO_T, AA, CIAO_LOSS_LOGISTIC>(ciao_ctx *, int, int, bool, ChainArgs<CIAO_T> &);
#endif
#if CIAO_DMA_PART == 0
CIAO_DMA_INST(CA_SVRG)
#elif CIAO_DMA_PART == 1
CIAO_DMA_INST(CA_SAGA)
#elif CIAO_DMA_PART == 2
CIAO_DMA_INST(CA_FINITO)
#elif CIAO_DMA_PART == 3
CIAO_DMA_INST(CA_SVRGC)
#else
CIAO_DMA_INST(CA_LFINITO)
#endif
#undef CIAO_DMA_INST

}  // namespace ciao

// mscore_launch.inc -- host side of the K-model per-sample statistics (mscore_kernels.h); included once per element type with CIAO_T defined
#include <string.h>

#include "mscore_kernels.h"
#include "launch.h"

namespace ciao {

namespace {
template <typename T, int SL, int LOSS>
int32_t launch_mscore_sl_loss(ciao_ctx *ctx, int grid, int K, const MscoreArgs<T> &a, double *out)
{
    constexpr size_t lds = mscore_lds_bytes<T, SL>();
    static_assert(lds <= 160 * 1024, "LDS budget");
    auto kern = &mscore_partial_kernel<T, SL, LOSS>;
    if (lds > 60 * 1024)
        CIAO_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(MSCORE_BLOCK), lds, ctx->stream, a);
    CIAO_HIP(hipGetLastError());
    hipLaunchKernelGGL((mscore_final_kernel<T, LOSS>), dim3((unsigned)K), dim3(CERT_BLOCK), 0, ctx->stream, a.P, (const double *)a.rec, out);
    CIAO_HIP(hipGetLastError());
    return CIAO_OK;
}
template <typename T, int SL>
int32_t launch_mscore_sl(ciao_ctx *ctx, int loss, int grid, int K, const MscoreArgs<T> &a, double *out)
{
    return loss == CIAO_LOSS_LS ? launch_mscore_sl_loss<T, SL, CIAO_LOSS_LS>(ctx, grid, K, a, out)
                                : launch_mscore_sl_loss<T, SL, CIAO_LOSS_LOGISTIC>(ctx, grid, K, a, out);
}
}  // namespace

// true: the one-pass kernel takes this problem and these vectors (the caller runs K times row dots + launch_mstat otherwise).  Any ld,
// any base of A; the iterates 16-byte aligned, as the header asks.
template <>
bool mscore_supported<CIAO_T>(const ciao_ctx *ctx, const ciao_problem *p, int K, const void *const *x)
{
    if (ctx->mscore_off) return false;
    if (!(p->loss == CIAO_LOSS_LS || p->loss == CIAO_LOSS_LOGISTIC) || p->N < 1 || K < 1 || K > MSCORE_MAX_K) return false;
    if (p->d < 1 || p->d > MSCORE_MAX_D) return false;
    for (int k = 0; k < K; ++k)
        if (!x[k] || (reinterpret_cast<uintptr_t>(x[k]) & 15u) != 0) return false;
    return true;
}

// out_host[4k .. 4k + 4): model k's four numbers.  The partition and the tile walk come from (N, d, T) alone; only the KIND of load
// depends on the layout, and the grid's second factor on K.
template <>
int32_t launch_mscore<CIAO_T>(ciao_ctx *ctx, const ciao_problem *p, int K, const void *const *x, const double *s_host, double *out_host)
{
    using T = CIAO_T;
    const int nkb = (K + MSCORE_KB - 1) / MSCORE_KB;
    const int P = mscore_parts(p->N);
    const int grid = 8 * nkb * ((P + 7) / 8);   // whole groups of 8 partitions: the model blocks of a partition share an XCD
    // workspace (ctx->partial): the K results, then the records; (ctx->mrhs_ptrs): the K pointers, then the K scalings
    const size_t head = (size_t)4 * MSCORE_MAX_K * sizeof(double);
    CIAO_TRY(ensure(ctx, &ctx->partial, &ctx->partial_bytes, head + (size_t)nkb * P * MSCORE_KB * MSCORE_REC * sizeof(double)));
    CIAO_TRY(ensure(ctx, &ctx->mrhs_ptrs, &ctx->mrhs_ptrs_bytes, (size_t)2 * K * sizeof(void *)));
    static_assert(sizeof(void *) == sizeof(double), "pointers and scalings share one staging vector");
    ctx->mrhs_host.resize((size_t)2 * K);
    for (int k = 0; k < K; ++k) {
        ctx->mrhs_host[k] = const_cast<void *>(x[k]);
        const double sk = s_host ? s_host[k] : 1.0;
        memcpy(&ctx->mrhs_host[K + k], &sk, sizeof sk);
    }
    CIAO_HIP(hipMemcpyAsync(ctx->mrhs_ptrs, ctx->mrhs_host.data(), (size_t)2 * K * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
    CIAO_HIP(hipStreamSynchronize(ctx->stream));   // the host vector may be rewritten by the next call
    MscoreArgs<T> a{};
    a.A = (const T *)p->A;
    a.b = (const T *)p->b;
    a.ld = p->ld;
    a.N = p->N;
    a.d = p->d;
    a.per = mscore_part_rows(p->N);
    a.P = P;
    a.nkb = nkb;
    a.K = K;
    a.vec16 = (reinterpret_cast<uintptr_t>(p->A) & 15u) == 0 && ((size_t)p->ld * sizeof(T)) % 16 == 0;
    a.x = reinterpret_cast<const T *const *>(ctx->mrhs_ptrs);
    a.s = reinterpret_cast<const double *>((void **)ctx->mrhs_ptrs + K);
    double *out = (double *)ctx->partial;
    a.rec = out + 4 * MSCORE_MAX_K;
    const int sl = mscore_sl(p->d);
    switch (sl) {
        case 4: CIAO_TRY((launch_mscore_sl<T, 4>(ctx, p->loss, grid, K, a, out))); break;
        case 16: CIAO_TRY((launch_mscore_sl<T, 16>(ctx, p->loss, grid, K, a, out))); break;
        case 32: CIAO_TRY((launch_mscore_sl<T, 32>(ctx, p->loss, grid, K, a, out))); break;
        default: CIAO_TRY((launch_mscore_sl<T, 64>(ctx, p->loss, grid, K, a, out))); break;
    }
    CIAO_HIP(hipMemcpyAsync(out_host, out, (size_t)4 * K * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CIAO_HIP(hipStreamSynchronize(ctx->stream));
    char nm[160];
    snprintf(nm, sizeof nm, "mscore_partial_kernel<%s,SL%d,%s,%s> grid=%d block=%d K=%d partitions=%d", sizeof(T) == 8 ? "f64" : "f32", sl,
             p->loss == CIAO_LOSS_LOGISTIC ? "logistic" : "ls", a.vec16 ? "vec16" : "elem", grid, MSCORE_BLOCK, K, P);
    ctx->last_kernel = nm;
    return CIAO_OK;
}

}  // namespace ciao

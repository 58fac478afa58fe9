// mscore_launch.inc -- host side of the K-model per-sample statistics (mscore_kernels.h); included once per element type with CIAO_T defined
#include <string.h>

#include "mscore_kernels.h"
#include "launch.h"

namespace ciao {

namespace {
// TT = T, or MscoreRows<T>: the row-list instantiations (their records are added by the same final kernel)
template <typename TT, int SL, int LOSS>
int32_t launch_mscore_sl_loss(ciao_ctx *ctx, int grid, int K, const MscoreArgs<TT> &a, double *out)
{
    using T = typename MscoreElem<TT>::type;
    constexpr size_t lds = mscore_lds_bytes<T, SL>();
    static_assert(lds <= 160 * 1024, "LDS budget");
    auto kern = &mscore_partial_kernel<TT, SL, LOSS>;
    if (lds > 60 * 1024)
        CIAO_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(MSCORE_BLOCK), lds, ctx->stream, a);
    CIAO_HIP(hipGetLastError());
    hipLaunchKernelGGL((mscore_final_kernel<T, LOSS>), dim3((unsigned)K), dim3(CERT_BLOCK), 0, ctx->stream, a.P, (const double *)a.rec, out);
    CIAO_HIP(hipGetLastError());
    return CIAO_OK;
}
template <typename TT, int SL>
int32_t launch_mscore_sl(ciao_ctx *ctx, int loss, int grid, int K, const MscoreArgs<TT> &a, double *out)
{
    return loss == CIAO_LOSS_LS ? launch_mscore_sl_loss<TT, SL, CIAO_LOSS_LS>(ctx, grid, K, a, out)
                                : launch_mscore_sl_loss<TT, SL, CIAO_LOSS_LOGISTIC>(ctx, grid, K, a, out);
}
template <typename TT>
int32_t launch_mscore_any(ciao_ctx *ctx, int loss, int sl, int grid, int K, const MscoreArgs<TT> &a, double *out)
{
    switch (sl) {
        case 4: return launch_mscore_sl<TT, 4>(ctx, loss, grid, K, a, out);
        case 16: return launch_mscore_sl<TT, 16>(ctx, loss, grid, K, a, out);
        case 32: return launch_mscore_sl<TT, 32>(ctx, loss, grid, K, a, out);
        default: return launch_mscore_sl<TT, 64>(ctx, loss, grid, K, a, out);
    }
}

// what both launchers stage and fill alike.  Workspace (ctx->partial): the K results, then the records; (ctx->mrhs_ptrs): the K pointers,
// the K scalings and (off_host) the K offsets.  M: the rows, or list positions, of the plan.
template <typename T>
int32_t mscore_stage(ciao_ctx *ctx, const ciao_problem *p, int64_t M, int K, const void *const *x, const double *s_host, const double *off_host,
                     MscoreArgs<T> &a, int *grid)
{
    const int nkb = (K + MSCORE_KB - 1) / MSCORE_KB;
    const int P = mscore_parts(M);
    const int nv = off_host ? 3 : 2;
    *grid = 8 * nkb * ((P + 7) / 8);   // whole groups of 8 partitions: the model blocks of a partition share an XCD
    const size_t head = (size_t)4 * MSCORE_MAX_K * sizeof(double);
    CIAO_TRY(ensure(ctx, &ctx->partial, &ctx->partial_bytes, head + (size_t)nkb * P * MSCORE_KB * MSCORE_REC * sizeof(double)));
    CIAO_TRY(ensure(ctx, &ctx->mrhs_ptrs, &ctx->mrhs_ptrs_bytes, (size_t)nv * K * sizeof(void *)));
    static_assert(sizeof(void *) == sizeof(double), "pointers, scalings and offsets share one staging vector");
    ctx->mrhs_host.resize((size_t)nv * K);
    for (int k = 0; k < K; ++k) {
        ctx->mrhs_host[k] = const_cast<void *>(x[k]);
        const double sk = s_host ? s_host[k] : 1.0;
        memcpy(&ctx->mrhs_host[K + k], &sk, sizeof sk);
        if (off_host) memcpy(&ctx->mrhs_host[2 * K + k], &off_host[k], sizeof(double));
    }
    CIAO_HIP(hipMemcpyAsync(ctx->mrhs_ptrs, ctx->mrhs_host.data(), (size_t)nv * K * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
    CIAO_HIP(hipStreamSynchronize(ctx->stream));   // the host vector may be rewritten by the next call
    a.A = (const T *)p->A;
    a.b = (const T *)p->b;
    a.ld = p->ld;
    a.N = M;
    a.d = p->d;
    a.per = mscore_part_rows(M);
    a.P = P;
    a.nkb = nkb;
    a.K = K;
    a.vec16 = (reinterpret_cast<uintptr_t>(p->A) & 15u) == 0 && ((size_t)p->ld * sizeof(T)) % 16 == 0;
    a.x = reinterpret_cast<const T *const *>(ctx->mrhs_ptrs);
    a.s = reinterpret_cast<const double *>((void **)ctx->mrhs_ptrs + K);
    a.rec = (double *)ctx->partial + 4 * MSCORE_MAX_K;
    return CIAO_OK;
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
    MscoreArgs<T> a{};
    int grid = 0;
    CIAO_TRY(mscore_stage<T>(ctx, p, p->N, K, x, s_host, nullptr, a, &grid));
    double *out = (double *)ctx->partial;
    const int sl = mscore_sl(p->d);
    CIAO_TRY(launch_mscore_any<T>(ctx, p->loss, sl, grid, K, a, out));
    CIAO_HIP(hipMemcpyAsync(out_host, out, (size_t)4 * K * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CIAO_HIP(hipStreamSynchronize(ctx->stream));
    char nm[160];
    snprintf(nm, sizeof nm, "mscore_partial_kernel<%s,SL%d,%s,%s> grid=%d block=%d K=%d partitions=%d", sizeof(T) == 8 ? "f64" : "f32", sl,
             p->loss == CIAO_LOSS_LOGISTIC ? "logistic" : "ls", a.vec16 ? "vec16" : "elem", grid, MSCORE_BLOCK, K, a.P);
    ctx->last_kernel = nm;
    return CIAO_OK;
}

// The same over the list idx[0 .. M), M >= 1, or (idx = NULL, M = N) over every row in order, with an offset per model (off_host: K host
// doubles, or NULL): mscore_partial_kernel<MscoreRows<T>, ...>.  The plan is that of M rows; the caller has checked d, K and the alignment
// of the iterates (there is no fallback here).
template <>
int32_t launch_mscore_rows<CIAO_T>(ciao_ctx *ctx, const ciao_problem *p, const int64_t *idx, int64_t M, int K, const void *const *x,
                                   const double *off_host, const double *s_host, double *out_host)
{
    using T = CIAO_T;
    MscoreArgs<MscoreRows<T>> a{};
    int grid = 0;
    CIAO_TRY(mscore_stage<T>(ctx, p, M, K, x, s_host, off_host, a, &grid));
    a.idx = idx;
    a.rows = p->N;
    a.off = off_host ? reinterpret_cast<const double *>((void **)ctx->mrhs_ptrs + 2 * K) : nullptr;
    double *out = (double *)ctx->partial;
    const int sl = mscore_sl(p->d);
    CIAO_TRY(launch_mscore_any<MscoreRows<T>>(ctx, p->loss, sl, grid, K, a, out));
    CIAO_HIP(hipMemcpyAsync(out_host, out, (size_t)4 * K * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CIAO_HIP(hipStreamSynchronize(ctx->stream));
    char nm[200];
    snprintf(nm, sizeof nm, "mscore_partial_kernel<rows,%s,SL%d,%s,%s,%s,%s> grid=%d block=%d K=%d partitions=%d", sizeof(T) == 8 ? "f64" : "f32",
             sl, p->loss == CIAO_LOSS_LOGISTIC ? "logistic" : "ls", a.vec16 ? "vec16" : "elem", idx ? "list" : "all", off_host ? "offset" : "plain",
             grid, MSCORE_BLOCK, K, a.P);
    ctx->last_kernel = nm;
    return CIAO_OK;
}

}  // namespace ciao

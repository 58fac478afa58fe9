// gram_launch.inc -- host side of the Gram statistics (gram_kernels.h); included once per element type with CIAO_T defined
#include "gram_kernels.h"
#include "launch.h"

namespace ciao {

// G (d x d device doubles at row stride ldg), u, colsum (d device doubles each, or NULL), bsum (2 device doubles, or NULL) over the N >= 1
// local rows.  The records live in ctx->partial: gram_plan(N, d).ws_bytes, at most GRAM_WS_BYTES.  Tiles, partitions and grid come from
// gram_plan(N, d); only the KIND of load depends on the layout.
// TT = T: the unweighted kernels; TT = Weighted<T>: the weighted ones (w = N device doubles; bsum has 3 slots).  Plan, workspace, tile map
// and the order of addition are the same.
template <typename TT>
static int32_t gram_dispatch(ciao_ctx *ctx, const ciao_problem *p, const int64_t *idx, int64_t M, const double *w, double *G, int64_t ldg,
                             double *u, double *colsum, double *bsum)
{
    using T = CIAO_T;
    constexpr bool weighted = GramElem<TT>::weighted;
    constexpr bool indexed = GramElem<TT>::indexed;   // over the list idx[0 .. M): M takes the place of N in the plan and in the kernel
    const int64_t rows = indexed ? M : p->N;
    const GramPlan pl = gram_plan(rows, p->d);
    CIAO_TRY(ensure(ctx, &ctx->partial, &ctx->partial_bytes, pl.ws_bytes));
    GramArgs<TT> a{};
    a.A = (const T *)p->A;
    a.b = (const T *)p->b;
    a.ld = p->ld;
    a.N = rows;
    a.d = p->d;
    a.per = pl.per;
    a.P = pl.P;
    a.nb = pl.nb;
    a.ntiles = pl.ntiles;
    a.xcd = pl.xcd;
    a.vec16 = (reinterpret_cast<uintptr_t>(p->A) & 15u) == 0 && ((size_t)p->ld * sizeof(T)) % 16 == 0;
    a.rec = (double *)ctx->partial;
    if constexpr (weighted) a.w = w;
    if constexpr (indexed) {
        a.idx = idx;
        a.rows = p->N;
    }
    constexpr size_t lds = gram_lds_bytes();
    static_assert(lds <= 80 * 1024, "two workgroups per CU");
    auto kern = &gram_partial_kernel<TT>;
    if (lds > 60 * 1024)
        CIAO_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)pl.grid), dim3(GRAM_BLOCK), lds, ctx->stream, a);
    CIAO_HIP(hipGetLastError());
    const int fgrid = pl.ntiles * GRAM_FINAL_BLOCKS + pl.nb + 1;
    hipLaunchKernelGGL((gram_final_kernel<typename GramElem<TT>::base>), dim3((unsigned)fgrid), dim3(GRAM_BLOCK), 0, ctx->stream, p->d, pl.nb, pl.ntiles, pl.P,
                       (const double *)a.rec, G, ldg, u, colsum, bsum);
    CIAO_HIP(hipGetLastError());
    char buf[200];
    snprintf(buf, sizeof buf, "gram_partial_kernel<%s,%s%s%s> grid=%d block=%d tile=%dx%d chunk=%d tiles=%d partitions=%d rows=%lld map=%s workspace=%zu",
             sizeof(T) == 8 ? "f64" : "f32", a.vec16 ? "vec16" : "elem", weighted ? ",w" : "", indexed ? ",rows" : "", pl.grid, GRAM_BLOCK, GRAM_T, GRAM_T, GRAM_KC,
             pl.ntiles, pl.P, (long long)pl.per, pl.xcd ? "xcd" : "plain", pl.ws_bytes);
    ctx->last_kernel = buf;
    return CIAO_OK;
}

template <>
int32_t launch_gram<CIAO_T>(ciao_ctx *ctx, const ciao_problem *p, double *G, int64_t ldg, double *u, double *colsum, double *bsum)
{
    return gram_dispatch<CIAO_T>(ctx, p, nullptr, 0, nullptr, G, ldg, u, colsum, bsum);
}

// the same over weighted rows: w = N device doubles (non-NULL), bsum = 3 device doubles or NULL
template <>
int32_t launch_gram_weighted<CIAO_T>(ciao_ctx *ctx, const ciao_problem *p, const double *w, double *G, int64_t ldg, double *u, double *colsum,
                                     double *bsum)
{
    return gram_dispatch<Weighted<CIAO_T>>(ctx, p, nullptr, 0, w, G, ldg, u, colsum, bsum);
}

// the same over the list idx[0 .. M), M >= 1 (gram_partial_kernel<Indexed<...>>): w = M device doubles by list position, or NULL
template <>
int32_t launch_gram_rows<CIAO_T>(ciao_ctx *ctx, const ciao_problem *p, const int64_t *idx, int64_t M, const double *w, double *G, int64_t ldg,
                                 double *u, double *colsum, double *bsum)
{
    return w ? gram_dispatch<Indexed<Weighted<CIAO_T>>>(ctx, p, idx, M, w, G, ldg, u, colsum, bsum)
             : gram_dispatch<Indexed<CIAO_T>>(ctx, p, idx, M, nullptr, G, ldg, u, colsum, bsum);
}

}  // namespace ciao

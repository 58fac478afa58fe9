// api_analysis.hip -- the passes that measure a problem or an iterate and change neither: the optimality certificate and its per-sample
// terms, row dots and margin statistics, screening, row and column statistics, column scaling, Gram statistics, the row-list passes
// and coordinate descent on a Gram matrix.  Five of them share the workspace ctx->cert: cert_ws.h has its layouts.

#include <math.h>

#include "api_internal.h"
#include "gramcdg_kernels.h"   // GramCdgArgs

namespace ciao {

// The certificate's own pass (certificate_t below: want_fval, the raw sum of the f_i left in res->obj[1], grad f(x) into `own`), optionally
// with the row dots a_i'x written to `rowdot_out` (ciao_row_dots, ciao_certificate_samples).
template <typename T>
static int32_t samples_pass(ciao_ctx *ctx, const ciao_problem *p, const void *x, T *rowdot_out, CertResults *res, T *own)
{
    RowsArgs<T> a = rows_args<T>(p);
    a.x1 = (const T *)x;
    a.want_fval = 1;
    a.rowdot_out = rowdot_out;
    ctx->rowdot_A = nullptr;   // a full pass: whatever the SVRG chain had cached belongs to an older one
    Epilogue<T> e = epi_zero<T>();
    e.c_sum = a.invN;
    e.av_out = own;
    e.obj_out = res->obj;   // the epilogue writes obj_out[1]
    e.obj_scale = 1.0;
    return launch_rows<T>(ctx, RM_GRAD, a, e);
}

// out_host[1..6) of both certificates from launch_cert's five
static void cert_out(const CertResults &h, double gamma, double *out_host)
{
    out_host[1] = h.S2;
    out_host[2] = sqrt(h.S0) / gamma;
    out_host[3] = h.M;
    out_host[4] = h.S1;
    out_host[5] = h.V;
}

// The certificate at x: (with av == NULL) one full pass that also sums the f_i(x) -- the monitor's extra scalar, armed for this
// pass alone and left RAW in the workspace (obj_scale = 1: the division by N_total is made on the host exactly as objective_t
// makes it, so F is bitwise ciao_objective's) -- then the reduction over the d coordinates, one copy, one synchronisation.
template <typename T>
static int32_t certificate_t(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *x, const void *av, double gamma,
                             double *out_host)
{
    CIAO_TRY(ensure(ctx, &ctx->cert, &ctx->cert_bytes, sizeof(CertWs) + (av ? 0 : (size_t)p->d * sizeof(T))));
    CertWs *ws = (CertWs *)ctx->cert;
    const bool own_pass = !av;
    if (own_pass) {
        T *own = (T *)(ws + 1);
        CIAO_TRY(samples_pass<T>(ctx, p, x, (T *)nullptr, &ws->res, own));
        av = own;
    }
    CIAO_TRY(launch_cert<T>(ctx, p->d, g, x, av, gamma, ws->rec, &ws->res.S0));
    CertResults h;
    CIAO_HIP(hipMemcpyAsync(&h, &ws->res, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    CIAO_HIP(hipStreamSynchronize(ctx->stream));
    if (own_pass) out_host[0] = h.obj[1] / (double)p->N_total;   // (a caller's av: out_host[0] stays what the caller put there)
    cert_out(h, gamma, out_host);
    return CIAO_OK;
}

// out[i] = a_i'x for the N local rows: the certificate's pass with rowdot_out = out; its d-vector stays in the workspace.
template <typename T>
static int32_t row_dots_t(ciao_ctx *ctx, const ciao_problem *p, const void *x, void *out)
{
    CIAO_TRY(ensure(ctx, &ctx->cert, &ctx->cert_bytes, sizeof(MstatWs) + (size_t)p->d * sizeof(T)));
    MstatWs *ws = (MstatWs *)ctx->cert;
    return samples_pass<T>(ctx, p, x, (T *)out, &ws->res, (T *)(ws + 1));
}

// the per-sample reduction alone, over caller's dots: two kernels, one copy, one synchronisation
template <typename T>
static int32_t margin_stats_t(ciao_ctx *ctx, const ciao_problem *p, const void *dots, double s, double *out_host)
{
    CIAO_TRY(ensure(ctx, &ctx->cert, &ctx->cert_bytes, sizeof(MstatWs)));
    MstatWs *ws = (MstatWs *)ctx->cert;
    CIAO_TRY(launch_mstat<T>(ctx, p->loss, p->N, dots, p->b, s, nullptr, 0.0, ws->rec, ws->stat));
    CIAO_HIP(hipMemcpyAsync(out_host, ws->stat, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CIAO_HIP(hipStreamSynchronize(ctx->stream));
    return CIAO_OK;
}

// K models' statistics: the one-pass kernel where it applies (mscore_launch.inc); otherwise, per model, exactly what ciao_row_dots
// followed by ciao_margin_stats launch -- the dots go to ctx->rowdot (the SVRG chain's cache is invalid from here on).
template <typename T>
static int32_t margin_stats_multi_t(ciao_ctx *ctx, const ciao_problem *p, int K, const void *const *x, const double *s_host, double *out_host)
{
    if (mscore_supported<T>(ctx, p, K, x)) return launch_mscore<T>(ctx, p, K, x, s_host, out_host);
    CIAO_TRY(ensure(ctx, &ctx->rowdot, &ctx->rowdot_bytes, (size_t)p->N * sizeof(T)));
    for (int k = 0; k < K; ++k) {
        CIAO_TRY(row_dots_t<T>(ctx, p, x[k], ctx->rowdot));
        CIAO_TRY(margin_stats_t<T>(ctx, p, ctx->rowdot, s_host ? s_host[k] : 1.0, out_host + 4 * (size_t)k));
    }
    return CIAO_OK;
}

// The certificate with its per-sample terms: the certificate's pass with the row dots kept (ctx->rowdot: the SVRG chain's cache is
// invalid from here on), the reduction over the d coordinates, then the reduction over the N samples with s formed on the device from
// the first one's ||grad f||_inf -- no host round trip between the two --, one copy, one synchronisation.
template <typename T>
static int32_t certificate_samples_t(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *x, double gamma,
                                     double *out_host)
{
    CIAO_TRY(ensure(ctx, &ctx->cert, &ctx->cert_bytes, sizeof(MstatWs) + (size_t)p->d * sizeof(T)));
    CIAO_TRY(ensure(ctx, &ctx->rowdot, &ctx->rowdot_bytes, (size_t)p->N * sizeof(T)));
    MstatWs *ws = (MstatWs *)ctx->cert;
    T *own = (T *)(ws + 1);
    CIAO_TRY(samples_pass<T>(ctx, p, x, (T *)ctx->rowdot, &ws->res, own));
    CIAO_TRY(launch_cert<T>(ctx, p->d, g, x, own, gamma, ws->rec, &ws->res.S0));
    const bool scaled = g && g->kind == CIAO_PROX_L1 && g->lam > 0.0;
    CIAO_TRY(launch_mstat<T>(ctx, p->loss, p->N, ctx->rowdot, p->b, 1.0, scaled ? &ws->res.M : nullptr, scaled ? g->lam : 0.0, ws->rec, ws->stat));
    struct {
        CertResults res;
        double stat[4];
    } h;   // the head of MstatWs up to the last of the four statistics
    CIAO_HIP(hipMemcpyAsync(&h, ws, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    CIAO_HIP(hipStreamSynchronize(ctx->stream));
    out_host[0] = h.res.obj[1] / (double)p->N_total;
    cert_out(h.res, gamma, out_host);
    for (int k = 0; k < 4; ++k) out_host[6 + k] = h.stat[k];
    return CIAO_OK;
}

// the screening rule over d coordinates: two kernels, one copy of the count, one synchronisation
template <typename T>
static int32_t screen_t(ciao_ctx *ctx, int64_t d, const void *grad, const double *colsq, double s, double kappa, double mu, uint8_t *keep,
                        int64_t *n_kept_host)
{
    CIAO_TRY(ensure(ctx, &ctx->cert, &ctx->cert_bytes, sizeof(ScreenWs)));
    ScreenWs *ws = (ScreenWs *)ctx->cert;
    CIAO_TRY(launch_screen<T>(ctx, d, grad, colsq, s, kappa, mu, keep, ws->rec, &ws->count));
    double cnt = 0.0;
    CIAO_HIP(hipMemcpyAsync(&cnt, &ws->count, sizeof cnt, hipMemcpyDeviceToHost, ctx->stream));
    CIAO_HIP(hipStreamSynchronize(ctx->stream));
    *n_kept_host = (int64_t)cnt;
    return CIAO_OK;
}

// the row sums of squares: one kernel (two with the summary); with stats_host one copy of four doubles and one synchronisation
template <typename T>
static int32_t row_sqnorms_t(ciao_ctx *ctx, const ciao_problem *p, double *out, double *stats_host)
{
    CIAO_TRY(ensure(ctx, &ctx->cert, &ctx->cert_bytes, sizeof(RowsqWs)));
    RowsqWs *ws = (RowsqWs *)ctx->cert;
    CIAO_TRY(launch_rowsq<T>(ctx, p, out, ws->rec, stats_host ? ws->summary : nullptr));
    if (stats_host) {
        CIAO_HIP(hipMemcpyAsync(stats_host, ws->summary, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        CIAO_HIP(hipStreamSynchronize(ctx->stream));
    }
    return CIAO_OK;
}

// the Gram statistics of no row: every sum is zero (bsum has nb entries)
static int32_t gram_zero(ciao_ctx *ctx, int64_t d, double *G, int64_t ldg, double *u, double *colsum, double *bsum, int nb)
{
    CIAO_HIP(hipMemset2DAsync(G, (size_t)ldg * sizeof(double), 0, (size_t)d * sizeof(double), (size_t)d, ctx->stream));
    if (u) CIAO_HIP(hipMemsetAsync(u, 0, (size_t)d * sizeof(double), ctx->stream));
    if (colsum) CIAO_HIP(hipMemsetAsync(colsum, 0, (size_t)d * sizeof(double), ctx->stream));
    if (bsum) CIAO_HIP(hipMemsetAsync(bsum, 0, nb * sizeof(double), ctx->stream));
    return CIAO_OK;
}

static int32_t check_samples(const ciao_problem *p, const char *who)
{
    CIAO_REQUIRE(p->loss != CIAO_LOSS_LS_COMPLEX, "%s covers real problems only (complex T: no per-sample quantities on the device)", who);
    CIAO_REQUIRE(p->loss != CIAO_LOSS_ZERO, "%s needs data rows (Zero() terms have no a_i'x)", who);
    return CIAO_OK;
}

}  // namespace ciao

using namespace ciao;

extern "C" {

int32_t ciao_certificate(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *x, const void *av, double gamma,
                         double *out_host)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_TRY(check_prox(g));
    CIAO_REQUIRE(p->loss != CIAO_LOSS_LS_COMPLEX && !(g && g->kind == CIAO_PROX_L1_COMPLEX),
                 "the certificate covers real problems only (complex T: no device certificate)");
    CIAO_REQUIRE(x && out_host, "x or out_host is NULL");
    CIAO_REQUIRE(gamma > 0 && gamma <= 1.79769313486231570815e308, "gamma must be > 0 and finite");
    return DISPATCH(p->dtype, certificate_t, ctx, p, g, x, av, gamma, out_host);
}

int32_t ciao_row_dots(ciao_ctx *ctx, const ciao_problem *p, const void *x, void *out)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_TRY(check_samples(p, "ciao_row_dots"));
    CIAO_REQUIRE(x && (out || p->N == 0), "x or out is NULL");
    return DISPATCH(p->dtype, row_dots_t, ctx, p, x, out);
}

int32_t ciao_margin_stats(ciao_ctx *ctx, const ciao_problem *p, const void *dots, double s, double *out_host)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_TRY(check_samples(p, "ciao_margin_stats"));
    CIAO_REQUIRE(p->N >= 1, "ciao_margin_stats needs at least one sample (N = 0)");
    CIAO_REQUIRE(dots && out_host, "dots or out_host is NULL");
    CIAO_REQUIRE(s >= 0.0 && s <= 1.0, "the dual scaling s must lie in [0, 1] (got %g)", s);
    return DISPATCH(p->dtype, margin_stats_t, ctx, p, dots, s, out_host);
}

int32_t ciao_margin_stats_multi(ciao_ctx *ctx, const ciao_problem *p, int32_t K, const void *const *x, const double *s_host, double *out_host)
{
    CIAO_REQUIRE(ctx && p && x && out_host, "ciao_margin_stats_multi: the context, the problem, the pointer table or out_host is NULL");
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_TRY(check_samples(p, "ciao_margin_stats_multi"));
    CIAO_REQUIRE(p->N >= 1, "ciao_margin_stats_multi needs at least one sample (N = 0)");
    CIAO_REQUIRE(K >= 1 && K <= 256, "ciao_margin_stats_multi: K must be in 1..256 (got %d)", K);
    for (int k = 0; k < K; ++k) {
        CIAO_REQUIRE(x[k], "ciao_margin_stats_multi: x[%d] is NULL", k);
        CIAO_REQUIRE(!s_host || (s_host[k] >= 0.0 && s_host[k] <= 1.0), "ciao_margin_stats_multi: the dual scaling s[%d] must lie in [0, 1] (got %g)",
                     k, s_host[k]);
    }
    return DISPATCH(p->dtype, margin_stats_multi_t, ctx, p, K, x, s_host, out_host);
}

int32_t ciao_margin_stats_multi_rows(ciao_ctx *ctx, const ciao_problem *p, const int64_t *idx, int64_t M, int32_t K, const void *const *x,
                                     const double *offset_host, const double *s_host, double *out_host)
{
    CIAO_REQUIRE(ctx && p && x && out_host, "ciao_margin_stats_multi_rows: the context, the problem, the pointer table or out_host is NULL");
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_TRY(check_samples(p, "ciao_margin_stats_multi_rows"));
    CIAO_REQUIRE(p->N >= 1, "ciao_margin_stats_multi_rows needs at least one sample (N = 0)");
    CIAO_REQUIRE(M >= 1, "ciao_margin_stats_multi_rows: the list must name at least one row (got M=%lld)", (long long)M);
    CIAO_REQUIRE(idx || M == p->N, "ciao_margin_stats_multi_rows: without a row list (idx = NULL) M must be the number of rows, N=%lld (got M=%lld)",
                 (long long)p->N, (long long)M);
    CIAO_REQUIRE(aligned8(idx), "ciao_margin_stats_multi_rows: the row list idx is not aligned to 8 bytes");
    CIAO_REQUIRE(K >= 1 && K <= 256, "ciao_margin_stats_multi_rows: K must be in 1..256 (got %d)", K);
    CIAO_REQUIRE(p->d <= 1024, "ciao_margin_stats_multi_rows takes rows of at most 1024 elements (got d=%lld): score the models one by one "
                               "(ciao_list_dots)", (long long)p->d);
    for (int k = 0; k < K; ++k) {
        CIAO_REQUIRE(x[k], "ciao_margin_stats_multi_rows: x[%d] is NULL", k);
        CIAO_REQUIRE((reinterpret_cast<uintptr_t>(x[k]) & 15u) == 0, "ciao_margin_stats_multi_rows: x[%d] is not aligned to 16 bytes (no fallback "
                                                                      "for lists: score that model with ciao_list_dots)", k);
        CIAO_REQUIRE(!s_host || (s_host[k] >= 0.0 && s_host[k] <= 1.0),
                     "ciao_margin_stats_multi_rows: the dual scaling s[%d] must lie in [0, 1] (got %g)", k, s_host[k]);
        CIAO_REQUIRE(!offset_host || (offset_host[k] - offset_host[k] == 0.0), "ciao_margin_stats_multi_rows: the offset of model %d is not finite (got %g)",
                     k, offset_host[k]);
    }
    return DISPATCH(p->dtype, launch_mscore_rows, ctx, p, idx, M, (int)K, x, offset_host, s_host, out_host);
}

int32_t ciao_certificate_samples(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *x, double gamma,
                                 double *out_host)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_TRY(check_prox(g));
    CIAO_TRY(check_samples(p, "ciao_certificate_samples"));
    CIAO_REQUIRE(!(g && g->kind == CIAO_PROX_L1_COMPLEX), "ciao_certificate_samples covers real problems only (complex prox)");
    CIAO_REQUIRE(!ctx->hook && ctx->shards.nshards == 0,
                 "ciao_certificate_samples on a row-sharded context: the per-sample sums would need an all-reduce of their own");
    CIAO_REQUIRE(p->N >= 1, "ciao_certificate_samples needs at least one sample (N = 0)");
    CIAO_REQUIRE(x && out_host, "x or out_host is NULL");
    CIAO_REQUIRE(gamma > 0 && gamma <= 1.79769313486231570815e308, "gamma must be > 0 and finite");
    return DISPATCH(p->dtype, certificate_samples_t, ctx, p, g, x, gamma, out_host);
}

int32_t ciao_col_sqnorms(ciao_ctx *ctx, const ciao_problem *p, double *out)
{
    CIAO_REQUIRE(ctx && p && out, "ciao_col_sqnorms: the context, the problem or the output vector is NULL");
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_REQUIRE(p->loss != CIAO_LOSS_LS_COMPLEX, "ciao_col_sqnorms covers real problems only (complex T: screening is not defined on (re, im) pairs)");
    CIAO_REQUIRE(p->loss != CIAO_LOSS_ZERO, "ciao_col_sqnorms needs data rows (Zero() terms have no matrix A)");
    CIAO_REQUIRE(p->N >= 1, "ciao_col_sqnorms needs at least one resident row (N = 0: there are no columns to sum)");
    return DISPATCH(p->dtype, launch_colsq, ctx, p, out);
}

int32_t ciao_row_sqnorms(ciao_ctx *ctx, const ciao_problem *p, double *out, double *stats_host)
{
    CIAO_REQUIRE(ctx && p, "ciao_row_sqnorms: the context or the problem is NULL");
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_REQUIRE(p->loss != CIAO_LOSS_ZERO, "ciao_row_sqnorms needs data rows (Zero() terms have no matrix A)");
    CIAO_REQUIRE(p->N >= 1, "ciao_row_sqnorms needs at least one resident row (N = 0: there is no row to sum)");
    CIAO_REQUIRE(out || stats_host, "ciao_row_sqnorms: out and stats_host are both NULL (nothing was asked for)");
    return DISPATCH(p->dtype, row_sqnorms_t, ctx, p, out, stats_host);
}

int32_t ciao_col_moments(ciao_ctx *ctx, const ciao_problem *p, const double *shift, double *s1, double *s2)
{
    CIAO_REQUIRE(ctx && p && s1 && s2, "ciao_col_moments: the context, the problem or one of the two output vectors is NULL");
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_REQUIRE(p->loss != CIAO_LOSS_LS_COMPLEX, "ciao_col_moments covers real problems only (complex T: a column of (re, im) pairs has no real mean)");
    CIAO_REQUIRE(p->loss != CIAO_LOSS_ZERO, "ciao_col_moments needs data rows (Zero() terms have no matrix A)");
    if (p->N == 0) {   // a rank that holds no row: both sums are zero, nothing is launched
        CIAO_HIP(hipMemsetAsync(s1, 0, (size_t)p->d * sizeof(double), ctx->stream));
        CIAO_HIP(hipMemsetAsync(s2, 0, (size_t)p->d * sizeof(double), ctx->stream));
        return CIAO_OK;
    }
    return DISPATCH(p->dtype, launch_colmom, ctx, p, shift, s1, s2);
}

int32_t ciao_scale_columns(ciao_ctx *ctx, const ciao_problem *p, const double *center, const double *scale, void *out, int64_t ld_out)
{
    CIAO_REQUIRE(ctx && p && (out || p->N == 0), "ciao_scale_columns: the context, the problem or the output matrix is NULL");
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_REQUIRE(p->loss != CIAO_LOSS_LS_COMPLEX, "ciao_scale_columns covers real problems only (complex T: columns of (re, im) pairs are not scaled)");
    CIAO_REQUIRE(p->loss != CIAO_LOSS_ZERO, "ciao_scale_columns needs data rows (Zero() terms have no matrix A)");
    CIAO_REQUIRE(ld_out >= p->d, "ciao_scale_columns: the row stride of out, ld_out=%lld, is below d=%lld", (long long)ld_out, (long long)p->d);
    if (p->N == 0) return CIAO_OK;
    if (!(out == p->A && ld_out == p->ld)) {
        // the bytes either matrix spans; out may be A itself (same stride: every element is read and written by one thread), nothing else
        const size_t es = p->dtype == CIAO_F64 ? 8 : 4;
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(p->A), a1 = a0 + ((size_t)(p->N - 1) * (size_t)p->ld + (size_t)p->d) * es;
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + ((size_t)(p->N - 1) * (size_t)ld_out + (size_t)p->d) * es;
        CIAO_REQUIRE(o1 <= a0 || a1 <= o0, "ciao_scale_columns: out overlaps A without being A itself with the same row stride "
                                           "(in place means out == A and ld_out == ld)");
    }
    return DISPATCH(p->dtype, launch_colscale, ctx, p, center, scale, out, ld_out);
}

int32_t ciao_gram(ciao_ctx *ctx, const ciao_problem *p, double *G, int64_t ldg, double *u, double *colsum, double *bsum)
{
    CIAO_REQUIRE(ctx && p && G, "ciao_gram: the context, the problem or the output matrix G is NULL");
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_REQUIRE(p->loss != CIAO_LOSS_LS_COMPLEX, "ciao_gram covers real problems only (complex T: A'A of (re, im) pairs is not the Gram matrix of the complex rows)");
    CIAO_REQUIRE(p->loss != CIAO_LOSS_ZERO, "ciao_gram needs data rows (Zero() terms have no matrix A)");
    CIAO_REQUIRE(ldg >= p->d, "ciao_gram: the row stride of G, ldg=%lld, is below d=%lld", (long long)ldg, (long long)p->d);
    CIAO_REQUIRE(p->d <= 4096, "ciao_gram takes rows of at most 4096 elements (got d=%lld: G alone would be %.0f MiB)", (long long)p->d,
                 (double)p->d * (double)p->d * 8.0 / 1048576.0);
    // a rank that holds no row: every sum is zero, nothing is launched
    if (p->N == 0) return gram_zero(ctx, p->d, G, ldg, u, colsum, bsum, 2);
    return DISPATCH(p->dtype, launch_gram, ctx, p, G, ldg, u, colsum, bsum);
}

int32_t ciao_gram_weighted(ciao_ctx *ctx, const ciao_problem *p, const double *w, double *G, int64_t ldg, double *u, double *colsum,
                           double *bsum)
{
    CIAO_REQUIRE(ctx && p && G, "ciao_gram_weighted: the context, the problem or the output matrix G is NULL");
    CIAO_REQUIRE(w || p->N == 0, "ciao_gram_weighted: the weight vector w is NULL (ciao_gram is the unweighted call)");
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_REQUIRE(p->loss != CIAO_LOSS_LS_COMPLEX, "ciao_gram_weighted covers real problems only (complex T: A'A of (re, im) pairs is not the Gram matrix of the complex rows)");
    CIAO_REQUIRE(p->loss != CIAO_LOSS_ZERO, "ciao_gram_weighted needs data rows (Zero() terms have no matrix A)");
    CIAO_REQUIRE(ldg >= p->d, "ciao_gram_weighted: the row stride of G, ldg=%lld, is below d=%lld", (long long)ldg, (long long)p->d);
    CIAO_REQUIRE(p->d <= 4096, "ciao_gram_weighted takes rows of at most 4096 elements (got d=%lld: G alone would be %.0f MiB)", (long long)p->d,
                 (double)p->d * (double)p->d * 8.0 / 1048576.0);
    CIAO_REQUIRE(aligned8(w), "ciao_gram_weighted: the weight vector w is not aligned to 8 bytes");
    // a rank that holds no row: every sum is zero, nothing is launched
    if (p->N == 0) return gram_zero(ctx, p->d, G, ldg, u, colsum, bsum, 3);
    return DISPATCH(p->dtype, launch_gram_weighted, ctx, p, w, G, ldg, u, colsum, bsum);
}

int32_t ciao_gram_rows(ciao_ctx *ctx, const ciao_problem *p, const int64_t *idx, int64_t M, const double *w, double *G, int64_t ldg, double *u,
                       double *colsum, double *bsum)
{
    CIAO_REQUIRE(ctx && p && G, "ciao_gram_rows: the context, the problem or the output matrix G is NULL");
    CIAO_REQUIRE(M >= 0, "ciao_gram_rows: the length of the row list, M=%lld, is negative", (long long)M);
    CIAO_REQUIRE(idx || M == 0, "ciao_gram_rows: the row list idx is NULL");
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_REQUIRE(p->loss != CIAO_LOSS_LS_COMPLEX, "ciao_gram_rows covers real problems only (complex T: A'A of (re, im) pairs is not the Gram matrix of the complex rows)");
    CIAO_REQUIRE(p->loss != CIAO_LOSS_ZERO, "ciao_gram_rows needs data rows (Zero() terms have no matrix A)");
    CIAO_REQUIRE(ldg >= p->d, "ciao_gram_rows: the row stride of G, ldg=%lld, is below d=%lld", (long long)ldg, (long long)p->d);
    CIAO_REQUIRE(p->d <= 4096, "ciao_gram_rows takes rows of at most 4096 elements (got d=%lld: G alone would be %.0f MiB)", (long long)p->d,
                 (double)p->d * (double)p->d * 8.0 / 1048576.0);
    CIAO_REQUIRE(aligned8(idx), "ciao_gram_rows: the row list idx is not aligned to 8 bytes");
    CIAO_REQUIRE(aligned8(w), "ciao_gram_rows: the weight vector w is not aligned to 8 bytes");
    // an empty list (or no row that an entry could name): every sum is zero, nothing is launched
    if (M == 0 || p->N == 0) return gram_zero(ctx, p->d, G, ldg, u, colsum, bsum, w ? 3 : 2);
    return DISPATCH(p->dtype, launch_gram_rows, ctx, p, idx, M, w, G, ldg, u, colsum, bsum);
}

// what ciao_list_dots and ciao_list_combine refuse alike (v = x or c)
static int32_t check_list(ciao_ctx *ctx, const ciao_problem *p, const char *name, const int64_t *idx, int64_t M)
{
    CIAO_REQUIRE(M >= 0, "%s: the length of the row list, M=%lld, is negative", name, (long long)M);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_REQUIRE(p->loss != CIAO_LOSS_LS_COMPLEX, "%s covers real problems only (complex T: rows of (re, im) pairs)", name);
    CIAO_REQUIRE(p->loss != CIAO_LOSS_ZERO, "%s needs data rows (Zero() terms have no matrix A)", name);
    CIAO_REQUIRE(p->d <= 4096, "%s takes rows of at most 4096 elements (got d=%lld)", name, (long long)p->d);
    CIAO_REQUIRE(idx || M == p->N, "%s: without a row list (idx = NULL) M must be the number of rows, N=%lld (got M=%lld)", name,
                 (long long)p->N, (long long)M);
    CIAO_REQUIRE(aligned8(idx), "%s: the row list idx is not aligned to 8 bytes", name);
    return CIAO_OK;
}

int32_t ciao_list_dots(ciao_ctx *ctx, const ciao_problem *p, const int64_t *idx, int64_t M, const void *x, double *out)
{
    CIAO_REQUIRE(ctx && p && x && out, "ciao_list_dots: the context, the problem, x or the output vector is NULL");
    CIAO_ENTER(ctx);
    CIAO_TRY(check_list(ctx, p, "ciao_list_dots", idx, M));
    CIAO_REQUIRE(aligned8(out), "ciao_list_dots: the output vector is not aligned to 8 bytes");
    if (M == 0) return CIAO_OK;   // an empty list: there is nothing to write, nothing is launched
    return DISPATCH(p->dtype, launch_listdot, ctx, p, idx, M, x, out);
}

int32_t ciao_list_combine(ciao_ctx *ctx, const ciao_problem *p, const int64_t *idx, int64_t M, const double *c, double *out)
{
    CIAO_REQUIRE(ctx && p && c && out, "ciao_list_combine: the context, the problem, c or the output vector is NULL");
    CIAO_ENTER(ctx);
    CIAO_TRY(check_list(ctx, p, "ciao_list_combine", idx, M));
    CIAO_REQUIRE(aligned8(c, out), "ciao_list_combine: c or the output vector is not aligned to 8 bytes");
    if (M == 0) {   // an empty list: the sum of no term, nothing is launched
        CIAO_HIP(hipMemsetAsync(out, 0, (size_t)p->d * sizeof(double), ctx->stream));
        return CIAO_OK;
    }
    return DISPATCH(p->dtype, launch_listcomb, ctx, p, idx, M, c, out);
}

int32_t ciao_gram_cd(ciao_ctx *ctx, int64_t d, int64_t K, const double *G, int64_t ldg, const double *u, const double *inv, const double *tau,
                     double *X, int64_t ldx, double tol, int32_t max_sweeps, double *R, int64_t ldr, double *stat)
{
    CIAO_REQUIRE(ctx && G && u && inv && tau && X && stat, "ciao_gram_cd: the context, G, u, inv, tau, X or stat is NULL");
    CIAO_ENTER(ctx);
    CIAO_REQUIRE(d >= 1 && d <= 4096, "ciao_gram_cd takes 1 <= d <= 4096 coordinates (got d=%lld: x, r and the diagonal live in LDS)", (long long)d);
    CIAO_REQUIRE(K >= 1 && K <= 4096, "ciao_gram_cd takes 1 <= K <= 4096 models in one launch (got K=%lld)", (long long)K);
    CIAO_REQUIRE(ldg >= d, "ciao_gram_cd: the row stride of G, ldg=%lld, is below d=%lld", (long long)ldg, (long long)d);
    CIAO_REQUIRE(ldx >= d, "ciao_gram_cd: the stride of X, ldx=%lld, is below d=%lld", (long long)ldx, (long long)d);
    CIAO_REQUIRE(!R || ldr >= d, "ciao_gram_cd: the stride of R, ldr=%lld, is below d=%lld", (long long)ldr, (long long)d);
    CIAO_REQUIRE(aligned8(G, u, inv, tau, X, R, stat), "ciao_gram_cd: a buffer is not aligned to 8 bytes");
    CIAO_REQUIRE(tol >= 0.0, "ciao_gram_cd: tol must be >= 0 (got %g)", tol);
    CIAO_REQUIRE(max_sweeps >= 1 && max_sweeps <= 1024, "ciao_gram_cd takes 1 <= max_sweeps <= 1024 per launch (got %d): relaunch from the returned X", (int)max_sweeps);
    return launch_gram_cd(ctx, d, K, G, ldg, u, inv, tau, X, ldx, tol, max_sweeps, R, ldr, stat);
}

int32_t ciao_gram_cd_general(ciao_ctx *ctx, int64_t d, int64_t K, const double *G, int64_t ldg, int64_t sg, int64_t nsets, const int32_t *gsel,
                             const double *u, int64_t ldu, const double *inv, int64_t ldinv, const double *tau, const double *pf, int64_t ldpf,
                             const double *lo, int64_t ldlo, const double *hi, int64_t ldhi, double *X, int64_t ldx, const double *tol,
                             int32_t max_sweeps, double *R, int64_t ldr, double *stat)
{
    CIAO_REQUIRE(ctx && G && u && inv && tau && X && tol && stat, "ciao_gram_cd_general: the context, G, u, inv, tau, X, tol or stat is NULL");
    CIAO_ENTER(ctx);
    CIAO_REQUIRE(d >= 1 && d <= 4096, "ciao_gram_cd_general takes 1 <= d <= 4096 coordinates (got d=%lld: x, r, the diagonal and t live in LDS)", (long long)d);
    CIAO_REQUIRE(K >= 1 && K <= 4096, "ciao_gram_cd_general takes 1 <= K <= 4096 models in one launch (got K=%lld)", (long long)K);
    CIAO_REQUIRE(ldg >= d, "ciao_gram_cd_general: the row stride of G, ldg=%lld, is below d=%lld", (long long)ldg, (long long)d);
    CIAO_REQUIRE(nsets >= 1 && nsets <= 2147483647, "ciao_gram_cd_general needs at least one Gram matrix (got nsets=%lld)", (long long)nsets);
    CIAO_REQUIRE(nsets == 1 || sg >= (d - 1) * ldg + d, "ciao_gram_cd_general: the set stride sg=%lld is below (d-1) ldg + d = %lld: the Gram matrices overlap",
                 (long long)sg, (long long)((d - 1) * ldg + d));
    CIAO_REQUIRE(ldx >= d, "ciao_gram_cd_general: the stride of X, ldx=%lld, is below d=%lld", (long long)ldx, (long long)d);
    CIAO_REQUIRE(!R || ldr >= d, "ciao_gram_cd_general: the stride of R, ldr=%lld, is below d=%lld", (long long)ldr, (long long)d);
    CIAO_REQUIRE((ldu == 0 || ldu >= d) && (ldinv == 0 || ldinv >= d), "ciao_gram_cd_general: the strides of u and inv must be 0 (shared) or >= d=%lld (got %lld, %lld)",
                 (long long)d, (long long)ldu, (long long)ldinv);
    CIAO_REQUIRE((!pf || ldpf == 0 || ldpf >= d) && (!lo || ldlo == 0 || ldlo >= d) && (!hi || ldhi == 0 || ldhi >= d),
                 "ciao_gram_cd_general: the strides of pf, lo and hi must be 0 (shared) or >= d=%lld (got %lld, %lld, %lld)", (long long)d, (long long)ldpf,
                 (long long)ldlo, (long long)ldhi);
    CIAO_REQUIRE(aligned8(G, u, inv, tau, pf, lo, hi, tol, X, R, stat) && (reinterpret_cast<uintptr_t>(gsel) & 3u) == 0,
                 "ciao_gram_cd_general: a buffer is not aligned to 8 bytes (gsel: 4 bytes)");
    CIAO_REQUIRE(max_sweeps >= 1 && max_sweeps <= 1024, "ciao_gram_cd_general takes 1 <= max_sweeps <= 1024 per launch (got %d): relaunch from the returned X", (int)max_sweeps);
    // the kernel's argument block, in its own order
    const GramCdgArgs a{G,   gsel, u,   inv,   tau,  pf,   lo,   hi,  tol, X,      R,          stat,
                        ldg, sg,   ldu, ldinv, ldpf, ldlo, ldhi, ldx, ldr, (int)d, (int)nsets, max_sweeps};
    return launch_gram_cd_general(ctx, a, K);
}

int32_t ciao_screen(ciao_ctx *ctx, int32_t dtype, int64_t d, const void *grad, const double *colsq, double s, double kappa, double mu,
                    uint8_t *keep, int64_t *n_kept_host)
{
    CIAO_REQUIRE(ctx && grad && colsq && keep && n_kept_host, "ciao_screen: the context, grad, colsq, keep or n_kept_host is NULL");
    CIAO_ENTER(ctx);
    CIAO_REQUIRE(dtype == CIAO_F32 || dtype == CIAO_F64, "ciao_screen: dtype must be CIAO_F32 or CIAO_F64 (got %d)", dtype);
    CIAO_REQUIRE(d >= 1, "ciao_screen needs at least one coordinate (got d = %lld)", (long long)d);
    CIAO_REQUIRE(s >= 0.0 && s <= 1.0, "ciao_screen: the dual scaling s must lie in [0, 1] (got %g)", s);
    CIAO_REQUIRE(kappa >= 0.0, "ciao_screen: the radius kappa must be >= 0 and not NaN (got %g; +inf keeps every coordinate)", kappa);
    CIAO_REQUIRE(mu > 0.0 && mu <= 1.79769313486231570815e308, "ciao_screen: the l1 weight mu must be > 0 and finite (got %g)", mu);
    return DISPATCH(dtype, screen_t, ctx, d, grad, colsq, s, kappa, mu, keep, n_kept_host);
}

}  // extern "C"

// launch.h -- host dispatch entry points shared by the API units (api_*.hip) and the per-type instantiation units.  The launchers are
// declared against the argument types only: a unit includes the kernel header of what it launches itself (its *_launch.inc).
#pragma once

#include "cert_ws.h"
#include "ciao_common.h"
#include "ciao_ctx.h"
#include "peer_args.h"
#include "rows_args.h"

namespace ciao {

template <typename T>
struct ChainArgs;         // chain_common.h
template <typename T>
struct ProshiArgs;        // proshi_args.h
template <typename T>
struct ProshiChainArgs;
template <typename T>
struct AFinitoArgs;       // afinito_args.h

// the next reduction's view of the peer mailboxes (advances the sequence number: every rank makes the same reductions in the
// same order)
inline PeerDev peer_dev(ciao_ctx *ctx)
{
    PeerDev p{};
    p.world = ctx->peer_world;
    p.rank = ctx->peer_rank;
    p.seq = ++ctx->peer_seq;
    p.slot_bytes = ctx->peer_slot_bytes;
    for (int r = 0; r < PEER_MAX; ++r) p.mail[r] = ctx->peer_mail[r];
    p.counter = ctx->peer_counter;
    p.errflag = ctx->errflag;
    // the chain owner's broadcast sets peer_wait_s_once for the one reduction that has to outwait a whole chain kernel
    const int64_t wait_s = ctx->peer_wait_s_once > ctx->peer_timeout_s ? ctx->peer_wait_s_once : ctx->peer_timeout_s;
    p.wait_ticks = (unsigned long long)wait_s * PEER_TICKS_PER_S;
    return p;
}

// the all-reduce hook over `count` elements of `buf` (device memory), in order on the ctx's stream
inline int32_t allreduce_hook(ciao_ctx *ctx, void *buf, int64_t count, int32_t dtype)
{
    const int32_t hs = ctx->hook(ctx->hook_user, buf, count, dtype, (void *)ctx->stream);
    if (hs != 0) {
        set_error("all-reduce hook failed with status %d", hs);
        return CIAO_ERR_HOOK;
    }
    return CIAO_OK;
}

// rows kernel + finalize (+ all-reduce hook) + epilogue.  Specialised in rows_f32.hip / rows_f64.hip.
template <typename T>
int32_t launch_rows(ciao_ctx *ctx, int mode, RowsArgs<T> &a, const Epilogue<T> &ep);
// same, but leaves the reduced sum in ctx->sumbuf[0..d) and the extra scalar in ctx->sumbuf[d]; no epilogue.
template <typename T>
int32_t launch_rows_raw(ciao_ctx *ctx, int mode, RowsArgs<T> &a);
// the sequential chains: plan, launch (inside an open chain batch: record) and name.  Specialised in chain_f32.hip / chain_f64.hip.
template <typename T>
int32_t launch_chain(ciao_ctx *ctx, int alg, ChainArgs<T> &a);

// the LDS-DMA fast chain for one (algorithm, loss) in the kernel class the chain plan chose: J chunks per thread of NT threads, one of
// (1,64) (2,64) (1,256) (2,256) (4,256) (4,512).  Defined in chain_dma_launch.inc, instantiated in chain_dma{0..4}_f32/f64.hip.
template <typename T, int ALG, int LOSS>
int32_t launch_dma(ciao_ctx *ctx, int J, int NT, bool masked, ChainArgs<T> &a);

// the wave-specialised chain (chain_ws_kernels.h: consumer / stager / issuer waves, barrier-free exchange) for SAGA / SAG on rows
// of up to 4 KiB, with the issuer waves the chain plan chose (1 or 2).  Defined in chain_ws_launch.inc, instantiated in chain_ws1_f32/f64.hip.
template <typename T, int ALG, int LOSS>
int32_t launch_ws(ciao_ctx *ctx, int issuers, bool masked, ChainArgs<T> &a);

// complex chains on the LDS-DMA ring (chain_cdma_kernel): rows of whole 16-byte chunks up to 16 KiB.  Specialised in
// chain_cdma_f32.hip / chain_cdma_f64.hip.
template <typename T>
int32_t launch_cdma(ciao_ctx *ctx, int alg, int J, bool masked, ChainArgs<T> &a);

// the full-gradient pass for K iterates in one pass over A (mrhs_kernels.h: MFMA).  Specialised in mrhs_f32.hip / mrhs_f64.hip.
template <typename T>
bool mrhs_supported(const ciao_ctx *ctx, const ciao_problem *p, int K, const void *const *x, void *const *av);
template <typename T>
int32_t launch_mrhs(ciao_ctx *ctx, const ciao_problem *p, int K, const void *const *x, void *const *av);

// full-gradient sweeps over rows of 17 .. 256 elements on the matrix cores (rowsm_kernels.h).  Specialised in rowsm_f32.hip / rowsm_f64.hip.
template <typename T>
size_t smallm_lds(int64_t d, int nb, bool table_in);   // table_in: RM_FINITO_BATCH (a third tile stream: the old table rows)
template <typename T>
int32_t launch_smallm(ciao_ctx *ctx, int mode, int grid, size_t lds, RowsArgs<T> &a);

// Finito batches over an index list (or a row block) of rows of tabular size, one wave per row (rowsw_kernels.h).  Specialised in
// rowsw_f32.hip / rowsw_f64.hip.  wrow_plan: false when the shape / mode is not for this kernel.
template <typename T>
bool wrow_plan(int mode, const RowsArgs<T> &a, int *vec, int *k);
template <typename T>
int32_t launch_wrow(ciao_ctx *ctx, int mode, int vec, int k, int grid, RowsArgs<T> &a);
template <typename T>
int wrow_block_waves(int vec, int k);

// sweeps / batch steps over rows beyond 64 KiB: a cluster of S workgroups per row (rowsl_kernels.h).  Specialised in rowsl_f32.hip /
// rowsl_f64.hip.  long_plan: CIAO_ERR_UNSUPPORTED (no error text) when the shape is not for this kernel.
constexpr int LONG_J_DEFAULT = 8;   // 16-byte chunks per thread: a workgroup's segment is J * 4 KiB of the row (Finito batches: 4)
constexpr int LONG_BPC_J4 = 4, LONG_BPC_J8 = 2;   // workgroups per CU (never more than the occupancy calculator allows)
template <typename T>
int32_t long_plan(ciao_ctx *ctx, int mode, int64_t d, int64_t nrows, int *J, int *S, int *C);
template <typename T>
int32_t launch_long(ciao_ctx *ctx, int mode, int J, int S, int C, RowsArgs<T> &a);

// the certificate's reduction over the d coordinates (cert_kernels.h): five doubles into `out`; rec = workspace of CERT_GRID_CAP records.
// Workspace of ciao_certificate: CertWs (cert_ws.h).  Specialised in cert_f32.hip / cert_f64.hip.
template <typename T>
int32_t launch_cert(ciao_ctx *ctx, int64_t d, const ciao_prox_desc *g, const void *x, const void *av, double gamma, double *rec, double *out);

// the per-sample reduction over the N row dots and targets (mstat_kernels.h): four doubles into `out`; rec = workspace of CERT_GRID_CAP
// records.  s: the literal, or (M_dev non-null) formed on the device as M == 0 ? 1 : min(1, mu / M) with M = *M_dev.  Specialised in
// mstat_f32.hip / mstat_f64.hip.  Workspace of the entry points that use it: MstatWs (cert_ws.h).
template <typename T>
int32_t launch_mstat(ciao_ctx *ctx, int loss, int64_t N, const void *dots, const void *b, double s, const double *M_dev, double mu,
                     double *rec, double *out);

// the same four doubles for K models in one pass over A (mscore_kernels.h: MFMA row dots, mstat_elem as their epilogue): 4 K host
// doubles.  Records and results in ctx->partial, the pointer / scaling table in ctx->mrhs_ptrs (both grown there).  Specialised in
// mscore_f32.hip / mscore_f64.hip.
template <typename T>
bool mscore_supported(const ciao_ctx *ctx, const ciao_problem *p, int K, const void *const *x);
template <typename T>
int32_t launch_mscore(ciao_ctx *ctx, const ciao_problem *p, int K, const void *const *x, const double *s_host, double *out_host);
// ... over a list of rows (ciao_margin_stats_multi_rows): idx = M >= 1 device int64 row numbers, or NULL (position = row, M = N);
// off_host = K host doubles added to model k's dots, or NULL; the plan is that of M rows.  d <= 1024, 16-byte aligned iterates (checked
// by the caller: no fallback).
template <typename T>
int32_t launch_mscore_rows(ciao_ctx *ctx, const ciao_problem *p, const int64_t *idx, int64_t M, int K, const void *const *x,
                           const double *off_host, const double *s_host, double *out_host);

// Gap-safe screening (colsq_kernels.h).  launch_colsq: out[j] = sum_i A[i,j]^2 over the N local rows, d device doubles; the partial
// d-vectors go to ctx->partial (grown here).  launch_screen: keep[k] = !(s |grad_k| + kappa sqrt(colsq_k) < mu) and their count into
// *cnt (device); rec = workspace of CERT_GRID_CAP records.  Workspace of ciao_screen: ScreenWs (cert_ws.h).
// Specialised in colsq_f32.hip / colsq_f64.hip.
template <typename T>
int32_t launch_colsq(ciao_ctx *ctx, const ciao_problem *p, double *out);
template <typename T>
int32_t launch_screen(ciao_ctx *ctx, int64_t d, const void *grad, const double *colsq, double s, double kappa, double mu, uint8_t *keep,
                      double *rec, double *cnt);

// Row sums of squares and their summary (rowsq_kernels.h).  launch_rowsq: out[i] = sum_j A[i,j]^2 for the N local rows (N device doubles,
// or NULL), one record per workgroup into rec (ROWSQ_WG_TARGET records at most) and, where res is non-NULL, {max, argmax, min, sum} into
// res[0..4) (device).  Workspace of ciao_row_sqnorms: RowsqWs (cert_ws.h).  Specialised in rowsq_f32.hip / rowsq_f64.hip.
template <typename T>
int32_t launch_rowsq(ciao_ctx *ctx, const ciao_problem *p, double *out, double *rec, double *res);

// Column standardisation (colmom_kernels.h).  launch_colmom: s1[j] = sum_i (A[i,j] - c_j), s2[j] = sum_i (A[i,j] - c_j)^2 over the N local
// rows, d device doubles each, c = shift (d device doubles) or the first local row (NULL); the partial d-vectors go to ctx->partial (grown
// here).  launch_colscale: out[i,j] = (T)(((double)A[i,j] - center_j) * scale_j), NULL center = 0, NULL scale = 1; out may be p->A with
// ld_out = p->ld.  Specialised in colmom_f32.hip / colmom_f64.hip.
template <typename T>
int32_t launch_colmom(ciao_ctx *ctx, const ciao_problem *p, const double *shift, double *s1, double *s2);
template <typename T>
int32_t launch_colscale(ciao_ctx *ctx, const ciao_problem *p, const double *center, const double *scale, void *out, int64_t ld_out);

// Gram statistics (gram_kernels.h).  launch_gram: G = A'A (d x d device doubles at row stride ldg, both triangles), u = A'b, colsum = A'1
// (d device doubles each, or NULL), bsum = {sum b, sum b^2} (2 device doubles, or NULL) over the N >= 1 local rows; the records of
// gram_plan(N, d) go to ctx->partial (grown here).  Specialised in gram_f32.hip / gram_f64.hip.
template <typename T>
int32_t launch_gram(ciao_ctx *ctx, const ciao_problem *p, double *G, int64_t ldg, double *u, double *colsum, double *bsum);
// ... with a weight per row (w: N device doubles, not NULL): A' diag(w) A and the weighted sums; bsum = {sum w b, sum w b^2, sum w}
template <typename T>
int32_t launch_gram_weighted(ciao_ctx *ctx, const ciao_problem *p, const double *w, double *G, int64_t ldg, double *u, double *colsum,
                             double *bsum);
// ... over a list of rows (ciao_gram_rows): idx = M >= 1 device int64 row numbers, w = M device doubles or NULL; the plan is gram_plan(M, d)
template <typename T>
int32_t launch_gram_rows(ciao_ctx *ctx, const ciao_problem *p, const int64_t *idx, int64_t M, const double *w, double *G, int64_t ldg, double *u,
                         double *colsum, double *bsum);

// A matrix-vector product and its adjoint over a list of rows (list_kernels.h; ciao_list_dots, ciao_list_combine): idx = M >= 1 device
// int64 row numbers, or NULL (position = row, M = N).  launch_listdot: out[m] = a_{idx[m]}'x, M device doubles, x = d elements of the
// rows' type; launch_listcomb: out[j] = sum_m c[m] A[idx[m], j], d device doubles, the partial d-vectors go to ctx->partial (grown
// here).  Specialised in list_f32.hip / list_f64.hip.
template <typename T>
int32_t launch_listdot(ciao_ctx *ctx, const ciao_problem *p, const int64_t *idx, int64_t M, const void *x, double *out);
template <typename T>
int32_t launch_listcomb(ciao_ctx *ctx, const ciao_problem *p, const int64_t *idx, int64_t M, const double *c, double *out);

// Coordinate descent on a Gram matrix (gramcd_kernels.h; ciao_gram_cd): K models, one workgroup each; arguments already checked.
// Defined in gramcd.hip.
int32_t launch_gram_cd(ciao_ctx *ctx, int64_t d, int64_t K, const double *G, int64_t ldg, const double *u, const double *inv, const double *tau,
                       double *X, int64_t ldx, double tol, int32_t max_sweeps, double *R, int64_t ldr, double *stat);
// Its general form (gramcdg_kernels.h; ciao_gram_cd_general): per-model Gram matrix, u, inv, penalty factors, bounds and tol; the
// arguments, already checked, as the kernel's own block.  Defined in gramcdg.hip.
struct GramCdgArgs;
int32_t launch_gram_cd_general(ciao_ctx *ctx, const GramCdgArgs &args, int64_t K);

// ProShI agent rows (init or one batch) + finalize + epilogue.  Specialised in rows_f32.hip / rows_f64.hip.
template <typename T>
int32_t launch_proshi(ciao_ctx *ctx, bool init, ProshiArgs<T> &a, const Epilogue<T> &ep);
// a run of equal-sized small ProShI batches as one coordinate-parallel launch (proshi_chain_kernel).  Specialised there too.
template <typename T>
int32_t launch_proshi_chain(ciao_ctx *ctx, ProshiChainArgs<T> &c);
// adaptive Finito chain (one sample per step, backtracking).  Specialised in chain_f32.hip / chain_f64.hip.
template <typename T>
int32_t launch_afinito(ciao_ctx *ctx, int loss, AFinitoArgs<T> &a);

}  // namespace ciao

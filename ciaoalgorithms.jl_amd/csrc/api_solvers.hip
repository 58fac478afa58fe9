// api_solvers.hip -- the passes over all rows (gradient, prox, full gradient, proximal-gradient step, objective), SVRG and SAGA / SAG,
// and the batch of independent chains; also what api_finito.hip shares with them (the chains' argument block, the owner's broadcast,
// the prox launch, the objective monitor's second half: declared in api_internal.h, instantiated at the end of the namespace here).

#include <string.h>

#include <algorithm>
#include <vector>

#include "api_internal.h"
#include "chain_common.h"
#include "vector_kernels.h"

namespace ciao {

template <typename T>
ChainArgs<T> chain_args(const ciao_problem *p, const ciao_prox_desc *g)
{
    ChainArgs<T> a{};
    a.A = (p->loss == CIAO_LOSS_ZERO) ? nullptr : (const T *)p->A;
    a.b = (p->loss == CIAO_LOSS_ZERO) ? nullptr : (const T *)p->b;
    a.ld = p->ld;
    a.d = p->d;
    a.loss = p->loss;
    a.lam = (T)p->lam;
    a.batch = 1;
    a.invN = T(1) / (T)p->N_total;
    a.gam_uniform = T(1);
    a.g = make_prox<T>(g);
    a.N = p->N;
    a.nshards = 0;
    return a;
}

// Row-sharded chains: after the owner's chain, vectors u and v (d each) are all-reduced with the non-owners contributing
// zeros, so every rank ends with the owner's values (the sum adds exact zeros: bitwise the owner's).
// `nsteps` = the length of the chain the owner runs first: the other ranks enqueue their half of the reduction at once and WAIT in
// it for the owner's whole chain kernel -- seconds at 10^7 steps.  RCCL and a host hook tolerate any skew; the peer mailboxes'
// wait is bounded in wall-clock time, so this one reduction is given the chain's worth of it (2 us per step is several times
// the slowest chain, remote rows included) on top of the ordinary limit.
template <typename T>
int32_t broadcast_from_owner(ciao_ctx *ctx, int64_t d, void *u, void *v, int64_t nsteps)
{
    struct Once {
        ciao_ctx *c;
        ~Once() { c->peer_wait_s_once = 0; }
    } once{ctx};
    ctx->peer_wait_s_once = ctx->peer_timeout_s + 60 + nsteps / 500000;
    const size_t bytes = (size_t)d * sizeof(T);
    CIAO_TRY(ensure(ctx, &ctx->sumbuf, &ctx->sumbuf_bytes, 2 * bytes + sizeof(T)));
    char *buf = (char *)ctx->sumbuf;
    if (ctx->shards.owner) {
        CIAO_HIP(hipMemcpyAsync(buf, u, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        CIAO_HIP(hipMemcpyAsync(buf + bytes, v, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        CIAO_HIP(hipMemsetAsync(buf, 0, 2 * bytes, ctx->stream));
    }
    CIAO_TRY(allreduce_hook(ctx, buf, 2 * d, sizeof(T) == 8 ? CIAO_F64 : CIAO_F32));
    CIAO_HIP(hipMemcpyAsync(u, buf, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    CIAO_HIP(hipMemcpyAsync(v, buf + bytes, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return CIAO_OK;
}

template <typename T>
int32_t prox_launch(ciao_ctx *ctx, int64_t d, const ciao_prox_desc *g, const T *x, T gamma, T scale, T *y)
{
    hipLaunchKernelGGL((prox_kernel<T>), dim3((unsigned)((d + 255) / 256)), dim3(256), 0, ctx->stream, d, make_prox<T>(g), x,
                       gamma, scale, y);
    CIAO_HIP(hipGetLastError());
    return CIAO_OK;
}

// ---- objective monitor (ciao_ctx_set_monitor) ------------------------------------------------------
// While a monitor is set, every FULL pass over the rows (mode GRAD, no index list) also sums the values f_i(x) the
// reference's gradient! returns and discards: they ride on the same sweep as the extra reduced scalar (all-reduced with the
// d-vector on a row-sharded problem), the epilogue leaves (1/N) sum_i f_i(x) in obj[1], and one small launch adds g(x).
template <typename T>
int32_t monitor_end(ciao_ctx *ctx, int64_t d, const void *x)
{
    if (!ctx->monitor) return CIAO_OK;
    hipLaunchKernelGGL((gvalue_kernel<T>), dim3(1), dim3(256), 0, ctx->stream, d, make_prox<T>(ctx->monitor_has_g ? &ctx->monitor_g : nullptr),
                       (const T *)x, ctx->monitor + 2, ctx->monitor);
    CIAO_HIP(hipGetLastError());
    return CIAO_OK;
}

// ---- typed implementations -------------------------------------------------------------------------------------------
template <typename T>
static int32_t full_gradient_t(ciao_ctx *ctx, const ciao_problem *p, const void *x, void *av, bool keep_rowdots = false)
{
    RowsArgs<T> a = rows_args<T>(p);
    a.x1 = (const T *)x;
    ctx->rowdot_A = nullptr;   // whatever was cached belongs to an older pass
    if (keep_rowdots && ctx->svrg_cache_rowdots && !ctx->hook && p->N > 0 && p->loss != CIAO_LOSS_ZERO) {
        CIAO_TRY(ensure(ctx, &ctx->rowdot, &ctx->rowdot_bytes, (size_t)p->N * sizeof(T)));
        a.rowdot_out = (T *)ctx->rowdot;
        ctx->rowdot_A = p->A;
        ctx->rowdot_x = x;
        ctx->rowdot_N = p->N;
    }
    Epilogue<T> e = epi_zero<T>();
    e.c_sum = a.invN;   // av = sum / N
    e.av_out = (T *)av;
    monitor_begin<T>(ctx, p, a, e);
    CIAO_TRY(launch_rows<T>(ctx, RM_GRAD, a, e));
    return monitor_end<T>(ctx, p->d, x);
}

template <typename T>
static int32_t proxgrad_t(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double gamma, const void *x, void *av,
                          void *y)
{
    RowsArgs<T> a = rows_args<T>(p);
    a.x1 = (const T *)x;
    Epilogue<T> e = epi_zero<T>();
    e.c_sum = a.invN;
    e.av_out = (T *)av;
    e.z_out = (T *)y;   // y = prox_{gamma g}(x - gamma*av)
    e.tau = (T)gamma;
    e.p0 = -(T)gamma;
    e.p1 = T(1);
    e.pw = (const T *)x;
    e.g = make_prox<T>(g);
    if (y == x && ctx->monitor) {   // the monitor reads x after the sweep: keep a copy when the step overwrites it
        CIAO_TRY(ensure(ctx, &ctx->monx, &ctx->monx_bytes, (size_t)p->d * sizeof(T)));
        CIAO_HIP(hipMemcpyAsync(ctx->monx, x, (size_t)p->d * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
    }
    monitor_begin<T>(ctx, p, a, e);
    CIAO_TRY(launch_rows<T>(ctx, RM_GRAD, a, e));
    return monitor_end<T>(ctx, p->d, (y == x && ctx->monitor) ? ctx->monx : x);
}

template <typename T>
static int32_t svrg_inner_t(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double gamma, int64_t m,
                            const int64_t *idx, const void *av, void *z, const void *z_full, void *w, bool use_rowdots = false)
{
    ChainArgs<T> a = chain_args<T>(p, g);
    a.nsteps = m;
    a.idx = idx;
    a.gamma = (T)gamma;
    a.av = (T *)av;   // read-only for SVRG
    a.z = (T *)z;
    a.zf = (T *)z_full;
    a.w = (T *)w;
    if (ctx->shards.nshards > 0) {   // row-sharded problem: the owner runs the one chain over every shard's rows
        if (ctx->shards.owner) {
            shard_args<T>(ctx, p, a, false);
            CIAO_TRY(launch_chain<T>(ctx, CA_SVRG, a));
        }
        return ctx->hook ? broadcast_from_owner<T>(ctx, p->d, z, w, m) : CIAO_OK;
    }
    // a_i'z_full for every row is already known if the last full pass on this ctx was the one at this z_full
    if (use_rowdots && ctx->rowdot_A == p->A && ctx->rowdot_x == z_full && ctx->rowdot_N == p->N && ctx->rowdot_A) {
        a.gam = (const T *)ctx->rowdot;
        return launch_chain<T>(ctx, CA_SVRGC, a);
    }
    return launch_chain<T>(ctx, CA_SVRG, a);
}

// SVRG_basic.jl:84-92: z_full = z / m; basic: w = z_full; z = 0; av = (1/N) sum_i grad f_i(z_full)
template <typename T>
static int32_t svrg_epoch_tail_t(ciao_ctx *ctx, const ciao_problem *p, int64_t m, int32_t plus, void *av, void *z, void *z_full, void *w)
{
    ctx->rowdot_A = nullptr;   // z_full is about to change
    hipLaunchKernelGGL((svrg_tail_kernel<T>), dim3((unsigned)((p->d + 255) / 256)), dim3(256), 0, ctx->stream, p->d, (T)m,
                       (int)plus, (T *)z, (T *)z_full, (T *)w);
    CIAO_HIP(hipGetLastError());
    return full_gradient_t<T>(ctx, p, z_full, av, true);
}

// K full passes at K iterates: ONE pass over A on the matrix cores where the shape allows (mrhs_kernels.h), K single sweeps otherwise
template <typename T>
static int32_t full_gradient_multi_t(ciao_ctx *ctx, const ciao_problem *p, int32_t K, const void *const *x, void *const *av)
{
    ctx->rowdot_A = nullptr;   // whatever was cached belongs to an older pass
    if (mrhs_supported<T>(ctx, p, K, x, av)) return launch_mrhs<T>(ctx, p, K, x, av);
    for (int k = 0; k < K; ++k) CIAO_TRY(full_gradient_t<T>(ctx, p, x[k], av[k]));
    return CIAO_OK;
}

// SVRG_basic.jl:84-92 for K solves over the same rows: every solve's tail (z_full = z / m; w = z_full; z = 0), then the K full
// passes at the K new z_full as one multi-right-hand-side pass
template <typename T>
static int32_t svrg_epoch_tail_multi_t(ciao_ctx *ctx, const ciao_problem *p, int32_t K, int64_t m, int32_t plus, void *const *av,
                                       void *const *z, void *const *z_full, void *const *w)
{
    ctx->rowdot_A = nullptr;
    for (int k = 0; k < K; ++k) {
        hipLaunchKernelGGL((svrg_tail_kernel<T>), dim3((unsigned)((p->d + 255) / 256)), dim3(256), 0, ctx->stream, p->d, (T)m, (int)plus,
                           (T *)z[k], (T *)z_full[k], (T *)w[k]);
    }
    CIAO_HIP(hipGetLastError());
    return full_gradient_multi_t<T>(ctx, p, K, const_cast<const void *const *>(z_full), av);
}

template <typename T>
static int32_t svrg_iterate_t(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double gamma, int64_t m,
                              const int64_t *idx, int32_t plus, int32_t reuse_rowdots, void *av, void *z, void *z_full, void *w)
{
    CIAO_TRY(svrg_inner_t<T>(ctx, p, g, gamma, m, idx, av, z, z_full, w, reuse_rowdots != 0));
    return svrg_epoch_tail_t<T>(ctx, p, m, plus, av, z, z_full, w);
}

template <typename T>
static int32_t saga_init_t(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double gamma, const void *x0,
                           void *table, void *av, void *z)
{
    RowsArgs<T> a = rows_args<T>(p);
    a.x1 = (const T *)x0;
    a.table = (T *)table;
    Epilogue<T> e = epi_zero<T>();
    e.c_sum = a.invN;
    e.av_out = (T *)av;
    CIAO_TRY(launch_rows<T>(ctx, RM_SAGA_INIT, a, e));
    // z = prox_{gamma g}((1 - gamma) x0)      SAGA_basic.jl:48
    return prox_launch<T>(ctx, p->d, g, (const T *)x0, (T)gamma, T(1) - (T)gamma, (T *)z);
}

template <typename T>
static int32_t saga_steps_t(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double gamma, int32_t sag,
                            int64_t nsteps, const int64_t *idx, void *table, void *av, void *z)
{
    ChainArgs<T> a = chain_args<T>(p, g);
    a.nsteps = nsteps;
    a.idx = idx;
    a.gamma = (T)gamma;
    a.sag = sag;
    a.table = (T *)table;
    a.av = (T *)av;
    a.z = (T *)z;
    if (ctx->shards.nshards > 0) {   // row-sharded problem: data rows AND table rows of the other shards are peer memory
        if (ctx->shards.owner) {
            shard_args<T>(ctx, p, a, true);
            CIAO_TRY(launch_chain<T>(ctx, CA_SAGA, a));
        }
        return ctx->hook ? broadcast_from_owner<T>(ctx, p->d, z, av, nsteps) : CIAO_OK;
    }
    return launch_chain<T>(ctx, CA_SAGA, a);
}

template <typename T>
static int32_t objective_t(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *x, double *obj)
{
    RowsArgs<T> a = rows_args<T>(p);
    a.x1 = (const T *)x;
    a.want_fval = 1;
    CIAO_TRY(launch_rows_raw<T>(ctx, RM_GRAD, a));
    hipLaunchKernelGGL((gvalue_kernel<T>), dim3(1), dim3(256), 0, ctx->stream, p->d, make_prox<T>(g), (const T *)x, ctx->scal,
                       (double *)nullptr);
    CIAO_HIP(hipGetLastError());
    T fsum;
    double gval;
    CIAO_HIP(hipMemcpyAsync(&fsum, (const T *)ctx->sumbuf + p->d, sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    CIAO_HIP(hipMemcpyAsync(&gval, ctx->scal, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CIAO_HIP(hipStreamSynchronize(ctx->stream));
    *obj = (double)fsum / (double)p->N_total + gval;
    return CIAO_OK;
}

// single-sample gradient!(y, f_i, x) on one wave
template <typename T>
static int32_t gradient_t(ciao_ctx *ctx, const ciao_problem *p, int64_t i, const void *x, void *y, void *fval)
{
    const bool zero = p->loss == CIAO_LOSS_ZERO;
    hipLaunchKernelGGL((gradient_kernel<T>), dim3(1), dim3(WAVE), 0, ctx->stream, zero ? nullptr : (const T *)p->A, zero ? nullptr : (const T *)p->b,
                       p->ld, p->d, p->loss, (T)p->lam, i, (const T *)x, (T *)y, (T *)fval);
    CIAO_HIP(hipGetLastError());
    return CIAO_OK;
}

template <typename T>
static int32_t prox_t(ciao_ctx *ctx, int64_t d, const ciao_prox_desc *g, const void *x, double gamma, void *y)
{
    return prox_launch<T>(ctx, d, g, (const T *)x, (T)gamma, T(1), (T *)y);
}

#define CIAO_SHARED_INST(T)                                                                                  \
    template ChainArgs<T> chain_args<T>(const ciao_problem *, const ciao_prox_desc *);                       \
    template int32_t broadcast_from_owner<T>(ciao_ctx *, int64_t, void *, void *, int64_t);                  \
    template int32_t prox_launch<T>(ciao_ctx *, int64_t, const ciao_prox_desc *, const T *, T, T, T *);      \
    template int32_t monitor_end<T>(ciao_ctx *, int64_t, const void *);
CIAO_SHARED_INST(float)
CIAO_SHARED_INST(double)
#undef CIAO_SHARED_INST

}  // namespace ciao

using namespace ciao;

extern "C" {

// ---- a batch of independent chains in one launch per kernel ---------------------------------------------------------------
int32_t ciao_ctx_chain_batch_begin(ciao_ctx *ctx)
{
    CIAO_ENTER(ctx);   // (refuses a second begin)
    ctx->batch.clear();
    ctx->batch_open = 1;
    return CIAO_OK;
}

int32_t ciao_ctx_chain_batch_end(ciao_ctx *ctx, int32_t launch)
{
    CIAO_ENTER_BATCHABLE(ctx);
    CIAO_REQUIRE(ctx->batch_open, "no chain batch is open on this ctx");
    ctx->batch_open = 0;
    std::vector<ciao_chain_rec> recs;
    recs.swap(ctx->batch);
    if (!launch || recs.empty()) return CIAO_OK;
    const size_t K = recs.size();
    // No chain may write what another one touches: sort the state ranges by their start and compare each with the ones that begin
    // inside it (read-only ranges -- a shared z_full, say -- may overlap)
    {
        struct Rg { const unsigned char *lo, *hi; bool wr; size_t chain; };
        std::vector<Rg> rg;
        rg.reserve(K * 5);
        for (size_t c = 0; c < K; ++c)
            for (int k = 0; k < 5; ++k)
                if (recs[c].hi[k] > recs[c].lo[k]) rg.push_back({recs[c].lo[k], recs[c].hi[k], recs[c].wr[k], c});
        std::sort(rg.begin(), rg.end(), [](const Rg &x, const Rg &y) { return x.lo < y.lo; });
        for (size_t i = 0; i < rg.size(); ++i)
            for (size_t j = i + 1; j < rg.size() && rg[j].lo < rg[i].hi; ++j)
                if (rg[i].chain != rg[j].chain && (rg[i].wr || rg[j].wr)) {
                    set_error("chains %zu and %zu of the batch overlap in a state vector / table that one of them writes: the chains of a "
                              "batch run concurrently and must own their av / z / w (SVRG: w, z; SAGA: z, av, table)", rg[i].chain, rg[j].chain);
                    return CIAO_ERR_ARG;
                }
    }
    // group by kernel (first appearance first); the argument blocks of a group are contiguous in the staging buffer
    std::vector<std::vector<size_t>> groups;
    for (size_t c = 0; c < K; ++c) {
        size_t gi = 0;
        for (; gi < groups.size(); ++gi) {
            const ciao_chain_rec &f = recs[groups[gi][0]];
            if (f.kern == recs[c].kern && f.block == recs[c].block && f.lds == recs[c].lds && f.args.size() == recs[c].args.size()) break;
        }
        if (gi == groups.size()) groups.emplace_back();
        groups[gi].push_back(c);
    }
    size_t total = 0;
    for (const auto &g : groups) total += (g.size() * recs[g[0]].args.size() + 255) & ~(size_t)255;
    CIAO_TRY(ensure(ctx, &ctx->batch_dev, &ctx->batch_dev_bytes, total));
    if (!ctx->batch_ev) CIAO_HIP(hipEventCreateWithFlags(&ctx->batch_ev, hipEventDisableTiming));
    CIAO_HIP(hipEventSynchronize(ctx->batch_ev));   // the previous batch's staging copy has been read (no-op for a fresh event)
    if (ctx->batch_host_bytes < total) {
        if (ctx->batch_host) (void)hipHostFree(ctx->batch_host);
        ctx->batch_host = nullptr;
        ctx->batch_host_bytes = 0;
        CIAO_HIP(hipHostMalloc(&ctx->batch_host, total, hipHostMallocDefault));
        ctx->batch_host_bytes = total;
    }
    std::vector<size_t> off(groups.size());
    size_t at = 0;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        off[gi] = at;
        const size_t ab = recs[groups[gi][0]].args.size();
        for (size_t k = 0; k < groups[gi].size(); ++k)
            memcpy(static_cast<unsigned char *>(ctx->batch_host) + at + k * ab, recs[groups[gi][k]].args.data(), ab);
        at += (groups[gi].size() * ab + 255) & ~(size_t)255;
    }
    CIAO_HIP(hipMemcpyAsync(ctx->batch_dev, ctx->batch_host, total, hipMemcpyHostToDevice, ctx->stream));
    CIAO_HIP(hipEventRecord(ctx->batch_ev, ctx->stream));
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        ciao_chain_rec &f = recs[groups[gi][0]];
        // the by-value argument: the first chain's block with `multi` (its first field, whatever T) -> this group's blocks
        const void *multi = static_cast<unsigned char *>(ctx->batch_dev) + off[gi];
        memcpy(f.args.data(), &multi, sizeof multi);
        void *kargs[1] = {f.args.data()};
        CIAO_HIP(hipLaunchKernel(f.kern, dim3((unsigned)groups[gi].size()), dim3(f.block), kargs, f.lds, ctx->stream));
    }
    char nm[256];
    snprintf(nm, sizeof nm, "chain batch: %zu chains in %zu launch(es); first: %s grid=%zu", K, groups.size(),
             recs[groups[0][0]].name.c_str(), groups[0].size());
    ctx->last_kernel = nm;
    return CIAO_OK;
}

int32_t ciao_gradient(ciao_ctx *ctx, const ciao_problem *p, int64_t i, const void *x, void *y, void *fval)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_REQUIRE(x && y, "x or y is NULL");
    CIAO_REQUIRE(i >= 0 && i < p->N, "sample index %lld outside [0, %lld)", (long long)i, (long long)p->N);
    return DISPATCH(p->dtype, gradient_t, ctx, p, i, x, y, fval);
}

int32_t ciao_prox(ciao_ctx *ctx, int32_t dtype, int64_t d, const ciao_prox_desc *g, const void *x, double gamma, void *y)
{
    CIAO_ENTER(ctx);
    ctx->rowdot_A = nullptr;
    CIAO_REQUIRE(dtype == CIAO_F32 || dtype == CIAO_F64, "bad dtype %d", dtype);
    CIAO_REQUIRE(d >= 0 && (d == 0 || (x && y)), "bad d or NULL vector");
    CIAO_TRY(check_prox(g));
    CIAO_REQUIRE(!(g && g->kind == CIAO_PROX_L1_COMPLEX) || d % 2 == 0, "CIAO_PROX_L1_COMPLEX works on (re, im) pairs: d must be even");
    if (d == 0) return CIAO_OK;
    return DISPATCH(dtype, prox_t, ctx, d, g, x, gamma, y);
}

int32_t ciao_full_gradient(ciao_ctx *ctx, const ciao_problem *p, const void *x, void *av)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_REQUIRE(x && av, "x or av is NULL");
    return DISPATCH(p->dtype, full_gradient_t, ctx, p, x, av);
}

int32_t ciao_full_gradient_multi(ciao_ctx *ctx, const ciao_problem *p, int32_t K, const void *const *x, void *const *av)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_REQUIRE(K >= 1 && K <= 4096 && x && av, "K must be in 1..4096 and the pointer tables non-NULL");
    for (int k = 0; k < K; ++k) CIAO_REQUIRE(x[k] && av[k], "x[%d] or av[%d] is NULL", k, k);
    CIAO_REQUIRE(p->loss != CIAO_LOSS_LS_COMPLEX, "complex problems: one ciao_full_gradient per iterate");
    return DISPATCH(p->dtype, full_gradient_multi_t, ctx, p, K, x, av);
}

int32_t ciao_proxgrad_step(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double gamma, const void *x,
                           void *av, void *y)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_solve(ctx, p, g));
    CIAO_REQUIRE(x && av && y, "x, av or y is NULL");
    CIAO_REQUIRE(gamma > 0, "gamma must be > 0");
    return DISPATCH(p->dtype, proxgrad_t, ctx, p, g, gamma, x, av, y);
}

int32_t ciao_objective(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *x, double *obj_host)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_solve(ctx, p, g));
    CIAO_REQUIRE(x && obj_host, "x or obj_host is NULL");
    return DISPATCH(p->dtype, objective_t, ctx, p, g, x, obj_host);
}

int32_t ciao_svrg_init(ciao_ctx *ctx, const ciao_problem *p, const void *x0, void *av, void *z, void *z_full, void *w)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_REQUIRE(x0 && av && z && z_full && w, "NULL state vector");
    const size_t bytes = (size_t)p->d * (p->dtype == CIAO_F64 ? 8 : 4);
    CIAO_TRY(DISPATCH(p->dtype, full_gradient_t, ctx, p, x0, av, true));
    if (ctx->rowdot_A) ctx->rowdot_x = z_full;   // z_full becomes a copy of x0: the cached a_i'x0 are a_i'z_full
    if (z_full != x0) CIAO_HIP(hipMemcpyAsync(z_full, x0, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    if (w != x0) CIAO_HIP(hipMemcpyAsync(w, x0, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    CIAO_HIP(hipMemsetAsync(z, 0, bytes, ctx->stream));
    return CIAO_OK;
}

int32_t ciao_svrg_inner(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double gamma, int64_t m,
                        const int64_t *idx, const void *av, void *z, const void *z_full, void *w)
{
    CIAO_ENTER_BATCHABLE(ctx);
    CIAO_REQUIRE(!ctx->batch_open || (!ctx->hook && ctx->shards.nshards == 0), "a chain batch cannot run on a row-sharded problem");
    const void *keep = ctx->rowdot_A;
    CIAO_TRY(check_problem(ctx, p));
    ctx->rowdot_A = keep;   // z_full is read-only here: a following ciao_svrg_iterate may still reuse the row dots
    CIAO_TRY(check_prox(g));
    CIAO_TRY(check_pair(p, g));
    CIAO_REQUIRE(m >= 0 && (m == 0 || idx), "m < 0 or idx is NULL");
    CIAO_REQUIRE(m == 0 || p->N > 0 || ctx->shards.nshards > 0, "cannot sample from an empty problem");
    CIAO_REQUIRE(av && z && z_full && w, "NULL state vector");
    CIAO_REQUIRE(gamma > 0, "gamma must be > 0");
    CIAO_REQUIRE(!ctx->hook || ctx->shards.nshards > 0,
                 "the SVRG inner cycle is a sequential chain: on a row-sharded problem it needs a shard table (ciao_ctx_set_shards)");
    CIAO_TRY(check_shards(ctx, p, false));
    return DISPATCH(p->dtype, svrg_inner_t, ctx, p, g, gamma, m, idx, av, z, z_full, w);
}

int32_t ciao_svrg_iterate(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double gamma, int64_t m,
                          const int64_t *idx, int32_t plus, int32_t reuse_rowdots, void *av, void *z, void *z_full, void *w)
{
    CIAO_ENTER(ctx);
    const void *keep = ctx->rowdot_A;
    CIAO_TRY(check_problem(ctx, p));
    // the a_i'z_full of the last full pass are used only when the CALLER vouches that A and z_full still hold what that
    // pass read (reuse_rowdots) AND the previous call on this ctx was svrg_init / svrg_iterate / svrg_inner on these buffers
    ctx->rowdot_A = reuse_rowdots ? keep : nullptr;
    CIAO_TRY(check_prox(g));
    CIAO_TRY(check_pair(p, g));
    CIAO_REQUIRE(m >= 1 && idx, "m < 1 or idx is NULL");
    CIAO_REQUIRE(p->N > 0 || ctx->shards.nshards > 0, "cannot sample from an empty problem");
    CIAO_REQUIRE(av && z && z_full && w, "NULL state vector");
    CIAO_REQUIRE(gamma > 0, "gamma must be > 0");
    CIAO_REQUIRE(!ctx->hook || ctx->shards.nshards > 0,
                 "the SVRG inner cycle is a sequential chain: on a row-sharded problem it needs a shard table (ciao_ctx_set_shards)");
    CIAO_TRY(check_shards(ctx, p, false));
    return DISPATCH(p->dtype, svrg_iterate_t, ctx, p, g, gamma, m, idx, plus, reuse_rowdots, av, z, z_full, w);
}

int32_t ciao_svrg_epoch_tail(ciao_ctx *ctx, const ciao_problem *p, int64_t m, int32_t plus, void *av, void *z, void *z_full, void *w)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_REQUIRE(m >= 1, "m < 1");
    CIAO_REQUIRE(av && z && z_full && w, "NULL state vector");
    return DISPATCH(p->dtype, svrg_epoch_tail_t, ctx, p, m, plus, av, z, z_full, w);
}

int32_t ciao_svrg_epoch_tail_multi(ciao_ctx *ctx, const ciao_problem *p, int32_t K, int64_t m, int32_t plus, void *const *av,
                                   void *const *z, void *const *z_full, void *const *w)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_REQUIRE(m >= 1, "m < 1");
    CIAO_REQUIRE(K >= 1 && K <= 4096 && av && z && z_full && w, "K must be in 1..4096 and the pointer tables non-NULL");
    for (int k = 0; k < K; ++k) CIAO_REQUIRE(av[k] && z[k] && z_full[k] && w[k], "NULL state vector of solve %d", k);
    CIAO_REQUIRE(p->loss != CIAO_LOSS_LS_COMPLEX, "complex problems: one ciao_svrg_epoch_tail per solve");
    return DISPATCH(p->dtype, svrg_epoch_tail_multi_t, ctx, p, K, m, plus, av, z, z_full, w);
}

int32_t ciao_saga_init(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double gamma, const void *x0,
                       void *table, void *av, void *z)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_solve(ctx, p, g));
    CIAO_REQUIRE(x0 && av && z && (table || p->N == 0), "NULL state vector / table");
    CIAO_REQUIRE(gamma > 0, "gamma must be > 0");
    return DISPATCH(p->dtype, saga_init_t, ctx, p, g, gamma, x0, table, av, z);
}

int32_t ciao_saga_steps(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double gamma, int32_t sag,
                        int64_t nsteps, const int64_t *idx, void *table, void *av, void *z)
{
    CIAO_ENTER_BATCHABLE(ctx);
    CIAO_REQUIRE(!ctx->batch_open || (!ctx->hook && ctx->shards.nshards == 0), "a chain batch cannot run on a row-sharded problem");
    CIAO_TRY(check_solve(ctx, p, g));
    CIAO_REQUIRE(nsteps >= 0 && (nsteps == 0 || idx), "nsteps < 0 or idx is NULL");
    CIAO_REQUIRE(nsteps == 0 || p->N > 0 || ctx->shards.nshards > 0, "cannot sample from an empty problem");
    CIAO_REQUIRE((table || ctx->shards.nshards > 0) && av && z, "NULL state vector / table");
    CIAO_REQUIRE(gamma > 0, "gamma must be > 0");
    CIAO_REQUIRE(!ctx->hook || ctx->shards.nshards > 0,
                 "SAGA steps are a sequential chain: on a row-sharded problem they need a shard table (ciao_ctx_set_shards)");
    CIAO_TRY(check_shards(ctx, p, true));
    return DISPATCH(p->dtype, saga_steps_t, ctx, p, g, gamma, sag, nsteps, idx, table, av, z);
}

}  // extern "C"

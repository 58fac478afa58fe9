// api_finito.hip -- the Finito family (Finito, LFinito, adaptive Finito) and ProShI: the solvers whose steps come in batches, each batch
// r dependent steps of a sequential chain or one batch-parallel launch (BatchSrc, batch_as_chain), with the hat_gamma they share.

#include <vector>

#include "afinito_args.h"
#include "api_internal.h"
#include "chain_common.h"
#include "proshi_kernels.h"   // proshi_solution_kernel
#include "vector_kernels.h"

namespace ciao {

template <typename T>
static int32_t finito_init_t(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *gam, double hat_gamma,
                             const void *x0, void *table, void *av, void *z)
{
    RowsArgs<T> a = rows_args<T>(p);
    a.x1 = (const T *)x0;
    a.table = (T *)table;
    a.gam = (const T *)gam;
    a.hat_gamma = (T)hat_gamma;
    Epilogue<T> e = epi_zero<T>();
    e.c_sum = (T)hat_gamma;   // av = hat_gamma * sum_i s_i/gam_i
    e.av_out = (T *)av;
    e.z_out = (T *)z;         // z = prox_{hat_gamma g}(av)
    e.tau = (T)hat_gamma;
    e.g = make_prox<T>(g);
    return launch_rows<T>(ctx, RM_FINITO_INIT, a, e);
}

// Where the batches of a call come from: index lists (bidx[bptr[t] .. bptr[t+1]), device int64) or contiguous row blocks
// (first[t] .. first[t]+len[t]: the static batches of Finito_basic.jl:52-58, no index array at all).
struct BatchSrc {
    const int64_t *bptr = nullptr, *bidx = nullptr;    // index lists
    const int64_t *first = nullptr, *len = nullptr;    // row blocks (host arrays)
    bool blocks() const { return first != nullptr; }
    int64_t size(int64_t t) const { return blocks() ? len[t] : bptr[t + 1] - bptr[t]; }
    const int64_t *idx(int64_t t) const { return blocks() ? nullptr : bidx + bptr[t]; }
    int64_t row0(int64_t t) const { return blocks() ? first[t] : 0; }
};

// the end of the run of consecutive batches that have batch t's size: [t, same_size_run) of the call's n batches
static int64_t same_size_run(const BatchSrc &src, int64_t t, int64_t n)
{
    int64_t t1 = t + 1;
    while (t1 < n && src.size(t1) == src.size(t)) ++t1;
    return t1;
}

// Row blocks that run as a sequential chain need their indices spelled out on the device: first[t] .. first[t]+r-1 for
// t in [t0, t1), r each, into the ctx's index workspace (host-built, one upload per run; pageable memory, so the copy is
// complete when hipMemcpyAsync returns and the host buffer may go).
static int32_t block_indices(ciao_ctx *ctx, const BatchSrc &src, int64_t t0, int64_t t1, int64_t r, const int64_t **out)
{
    const size_t n = (size_t)((t1 - t0) * r);
    CIAO_TRY(ensure(ctx, &ctx->idxbuf, &ctx->idxbuf_bytes, n * sizeof(int64_t)));
    std::vector<int64_t> h;
    try {
        h.resize(n);
    } catch (...) {
        set_error("out of host memory (%zu block indices)", n);
        return CIAO_ERR_ALLOC;
    }
    size_t k = 0;
    for (int64_t t = t0; t < t1; ++t)
        for (int64_t q = 0; q < r; ++q) h[k++] = src.first[t] + q;
    CIAO_HIP(hipMemcpyAsync(ctx->idxbuf, h.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    CIAO_HIP(hipStreamSynchronize(ctx->stream));   // h goes out of scope: be certain the staging copy has consumed it
    *out = (const int64_t *)ctx->idxbuf;
    return CIAO_OK;
}

// chain_args of a Finito / LFinito chain run: the batches [t, t1) of r rows each as (t1 - t) * r dependent steps
template <typename T>
static int32_t chain_run_args(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const BatchSrc &src, int64_t t, int64_t t1, int64_t r,
                              const void *gam, double hat_gamma, void *av, void *z, ChainArgs<T> &a)
{
    a = chain_args<T>(p, g);
    a.nsteps = (t1 - t) * r;
    a.idx = src.idx(t);
    if (src.blocks()) CIAO_TRY(block_indices(ctx, src, t, t1, r, &a.idx));
    a.batch = r;
    a.gam = (const T *)gam;
    a.hat_gamma = (T)hat_gamma;
    a.av = (T *)av;
    a.z = (T *)z;
    return CIAO_OK;
}

// Batches of r samples: r dependent chain steps in one persistent workgroup, or one batch-parallel rows launch?
// "chain_max_batch" >= 0 fixes the crossover; -1 (default) derives it from measurements on MI355X: a batch-parallel step
// costs ~10 us of launches + latency whatever r (tools/finito_batch_time.py), a chain step 0.45-1.5 us growing with the row.
template <typename T>
static bool batch_as_chain(const ciao_ctx *ctx, const ciao_problem *p, int64_t r)
{
    if (ctx->hook) return false;                       // sharded batches need the all-reduce between kernels
    // beyond 8192 elements: tiny batches only -- the several-workgroup chain (chain_wide_kernel, up to 131 072 elements) takes about 3 us
    // per sample, the one-workgroup any-d chain 12 us and more, a batch-parallel step of such rows 10 us and more
    if (p->d > 32 * CHAIN_NT) return r <= ((p->d <= 131072 && !ctx->chain_no_wide) ? 3 : 2);
    if (sizeof(T) == 8 && p->d > 16 * CHAIN_NT && !ctx->chain_no_wide && ctx->chain_max_batch < 0) return r <= 3;   // (fp64 rows of 4097 .. 8192 elements: the same chain)
    int64_t lim = ctx->chain_max_batch;
    if (lim < 0) {
        // measured after the chain work of round 2 (tools/gpu_s34.sh, profiles/r02_batch_chain_crossover.txt; Finito, fp32): a
        // batch-parallel step costs 7.5-9.5 us up to r = 64 whatever r; a chain step 0.39 / 0.50 / 0.82 / 1.6 us per sample at
        // 4 / 8 / 16 / 32 KiB rows, 0.29-0.34 us on the single-wave shapes (rows of up to 2 KiB)
        const int64_t rowb = p->d * (int64_t)sizeof(T);
        if (rowb % 4096 == 0 && rowb <= 32768 && rowb != 12288 && rowb != 20480 && rowb != 24576 && rowb != 28672)
            lim = rowb == 4096 ? 22 : (rowb == 8192 ? 15 : (rowb == 16384 ? 10 : 5));
        else if (rowb < 1024)
            lim = 28;   // rows under 1 KiB: chain steps 0.2-0.5 us against ~14 us per batch on the scalar generic kernel
        else if (rowb <= 2048 && rowb % 16 == 0)
            lim = 22;
        else
            lim = 14;
    }
    return r <= lim;
}

template <typename T>
static int32_t finito_steps_t(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *gam, double hat_gamma,
                              int64_t nit, const BatchSrc &src, void *table, void *av, void *z)
{
    if (ctx->batch_open && nit > 0) {
        // recorded into a chain batch: the whole call must be ONE chain launch -- every iteration's batch of the same small size
        // (a second launch of the same solve would have to wait for the first: not something a batch can express)
        const int64_t r0 = src.size(0);
        bool uniform = !src.blocks() && r0 >= 1;
        for (int64_t tt = 1; uniform && tt < nit; ++tt) uniform = src.size(tt) == r0;
        if (!uniform || !batch_as_chain<T>(ctx, p, r0)) {
            set_error("a chain batch takes Finito steps whose batches all have the same size, small enough to run as a sequential "
                      "chain (index-list form; option chain_max_batch), got %lld iterations starting with a batch of %lld",
                      (long long)nit, (long long)r0);
            return CIAO_ERR_UNSUPPORTED;
        }
    }
    int64_t t = 0;
    while (t < nit) {
        const int64_t r = src.size(t);
        // on a row-sharded problem a batch may have no member on this rank: it still joins the all-reduce with a zero sum
        CIAO_REQUIRE(r >= 1 || (ctx->hook && r == 0), "Finito batch %lld is empty", (long long)t);
        const int64_t t1 = same_size_run(src, t, nit);
        if (batch_as_chain<T>(ctx, p, r)) {
            ChainArgs<T> a;
            CIAO_TRY(chain_run_args<T>(ctx, p, g, src, t, t1, r, gam, hat_gamma, av, z, a));
            a.table = (T *)table;
            CIAO_TRY(launch_chain<T>(ctx, CA_FINITO, a));
        } else {
            for (int64_t tt = t; tt < t1; ++tt) {
                RowsArgs<T> a = rows_args<T>(p);
                a.nrows = r;
                a.idx = src.idx(tt);
                a.row0 = src.row0(tt);
                a.x1 = (const T *)z;
                a.table = (T *)table;
                a.gam = (const T *)gam;
                a.hat_gamma = (T)hat_gamma;
                Epilogue<T> e = epi_zero<T>();
                e.c_acc = T(1);   // av += sum_i (t_i - s_i) hat_gamma/gam_i
                e.acc_in = (const T *)av;
                e.c_sum = T(1);
                e.av_out = (T *)av;
                e.z_out = (T *)z;   // z = prox_{hat_gamma g}(av)
                e.tau = (T)hat_gamma;
                e.g = make_prox<T>(g);
                CIAO_TRY(launch_rows<T>(ctx, RM_FINITO_BATCH, a, e));
            }
        }
        t = t1;
    }
    return CIAO_OK;
}

// LFinito's full pass: av = x - (hg/N) sum_i grad f_i(x)       Finito_LFinito.jl:84-88
template <typename T>
static int32_t lfinito_full_pass(ciao_ctx *ctx, const ciao_problem *p, T hg, const void *x, void *av)
{
    RowsArgs<T> a = rows_args<T>(p);
    a.x1 = (const T *)x;
    Epilogue<T> e = epi_zero<T>();
    e.c_sum = -(hg * a.invN);
    e.c_u = T(1);
    e.u = (const T *)x;
    e.av_out = (T *)av;
    monitor_begin<T>(ctx, p, a, e);
    CIAO_TRY(launch_rows<T>(ctx, RM_GRAD, a, e));
    return monitor_end<T>(ctx, p->d, x);
}

template <typename T>
static int32_t lfinito_init_t(ciao_ctx *ctx, const ciao_problem *p, double hat_gamma, const void *x0, void *av, void *z,
                              void *z_full)
{
    CIAO_TRY(lfinito_full_pass<T>(ctx, p, (T)hat_gamma, x0, av));   // av = x0 - (hat_gamma/N) sum grad f_i(x0)
    const size_t bytes = (size_t)p->d * sizeof(T);
    CIAO_HIP(hipMemcpyAsync(z, av, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    CIAO_HIP(hipMemcpyAsync(z_full, av, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return CIAO_OK;
}

template <typename T>
static int32_t lfinito_iterate_t(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *gam,
                                 double hat_gamma, int64_t nb, const BatchSrc &src, void *av, void *z, void *z_full)
{
    const T hg = (T)hat_gamma;
    // z_full = prox_{hg g}(av)                                   Finito_LFinito.jl:83
    CIAO_TRY(prox_launch<T>(ctx, p->d, g, (const T *)av, hg, T(1), (T *)z_full));
    CIAO_TRY(lfinito_full_pass<T>(ctx, p, hg, z_full, av));   // av = z_full - (hg/N) sum_i grad f_i(z_full)            :84-88
    int64_t t = 0;
    bool z_ready = false;
    while (t < nb) {
        const int64_t r = src.size(t);
        CIAO_REQUIRE(r >= 1 || (ctx->hook && r == 0), "LFinito batch %lld is empty", (long long)t);
        const int64_t t1 = same_size_run(src, t, nb);
        if (batch_as_chain<T>(ctx, p, r)) {
            ChainArgs<T> a;
            CIAO_TRY(chain_run_args<T>(ctx, p, g, src, t, t1, r, gam, hat_gamma, av, z, a));
            a.zf = (T *)z_full;
            CIAO_TRY(launch_chain<T>(ctx, CA_LFINITO, a));
            z_ready = false;
        } else {
            for (int64_t tt = t; tt < t1; ++tt) {
                // z = prox_{hg g}(av), :92 -- already written by the previous batch's epilogue when there was one
                if (!z_ready) CIAO_TRY(prox_launch<T>(ctx, p->d, g, (const T *)av, hg, T(1), (T *)z));
                RowsArgs<T> a = rows_args<T>(p);
                a.nrows = r;
                a.idx = src.idx(tt);
                a.row0 = src.row0(tt);
                a.x1 = (const T *)z_full;   // acc += (coef(z_full) - coef(z)) a_i
                a.x2 = (const T *)z;
                a.gam = (const T *)gam;
                a.hat_gamma = hg;
                Epilogue<T> e = epi_zero<T>();
                e.c_acc = T(1);
                e.acc_in = (const T *)av;
                e.c_sum = hg * a.invN;
                e.uv_extra = 1;   // + (sum_i hg/gam_i) * (z - z_full)
                e.c_u = T(1);
                e.u = (const T *)z;
                e.c_v = T(-1);
                e.v = (const T *)z_full;
                e.av_out = (T *)av;
                // every batch but the last also leaves the NEXT batch's z = prox_{hg g}(av) (one launch less per batch;
                // each thread reads its own z[k] above before it overwrites it).  After the last batch z stays the z that
                // batch worked with: that is the reference's `solution` (Finito_LFinito.jl:105).
                z_ready = (tt + 1 < nb);
                if (z_ready) {
                    e.z_out = (T *)z;
                    e.tau = hg;
                    e.g = make_prox<T>(g);
                }
                CIAO_TRY(launch_rows<T>(ctx, RM_GRAD2, a, e));
            }
        }
        t = t1;
    }
    return CIAO_OK;
}

template <typename T>
static int32_t afinito_init_t(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double alpha, const void *x0,
                              void *table, void *meta, void *av, void *z, void *hat_gamma_dev, const void *gam_override)
{
    RowsArgs<T> a = rows_args<T>(p);
    a.x1 = (const T *)x0;
    a.table = (T *)table;
    a.meta = (T *)meta;
    a.gam = (const T *)gam_override;   // stepsizes the host resolved by re-probing (entries > 0 are used as they are)
    a.alpha = (T)alpha;
    a.Nd = (double)p->N_total;
    Epilogue<T> e = epi_zero<T>();
    e.c_sum = T(1);
    e.inv_extra = 1;              // hat_gamma = 1 / sum_i 1/gamma_i ; av = hat_gamma * sum ; z = prox_{hat_gamma g}(av)
    e.hg_out = (T *)hat_gamma_dev;
    e.av_out = (T *)av;
    e.z_out = (T *)z;
    e.g = make_prox<T>(g);
    return launch_rows<T>(ctx, RM_AFINITO_INIT, a, e);
}

template <typename T>
static int32_t afinito_steps_t(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double alpha, double tol_b,
                               int64_t nsteps, const int64_t *idx, void *table, void *meta, void *av, void *z,
                               void *hat_gamma_dev, int64_t *done_host, int64_t *trials_host)
{
    AFinitoArgs<T> a{};
    a.A = (const T *)p->A;
    a.b = (const T *)p->b;
    a.ld = p->ld;
    a.d = p->d;
    a.N = p->N;
    a.lam = (T)p->lam;
    a.nsteps = nsteps;
    a.idx = idx;
    a.alpha = (T)alpha;
    a.tol_b = (T)tol_b;
    a.invN = T(1) / (T)p->N_total;
    a.Nf = (T)p->N_total;
    a.Nd = (double)p->N_total;
    a.g = make_prox<T>(g);
    a.table = (T *)table;
    a.meta = (T *)meta;
    a.av = (T *)av;
    a.z = (T *)z;
    a.hg = (T *)hat_gamma_dev;
    a.counters = reinterpret_cast<long long *>(ctx->scal);
    const ciao_shard_table &sh = ctx->shards;
    const bool sharded = sh.nshards > 0;
    if (sharded) {   // row-sharded problem: data rows, table rows and scalars of the other shards are peer memory (as the SAGA chain)
        shard_args<T>(ctx, p, a, true);
        for (int k = 0; k < CIAO_MAX_SHARDS; ++k) a.shM[k] = k < sh.nshards ? (T *)sh.meta[k] : nullptr;
    }
    long long c[2] = {0, 0};
    if (!sharded || sh.owner) {
        CIAO_TRY(launch_afinito<T>(ctx, p->loss, a));
        CIAO_HIP(hipMemcpyAsync(c, ctx->scal, sizeof c, hipMemcpyDeviceToHost, ctx->stream));
        CIAO_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (sharded && ctx->hook) {
        // av and z as the chains' hand-over; hat_gamma and the two counters as three Float64 (a Float32 is exact in one, a count
        // of steps below 2^53 too) behind them, the non-owners contributing zeros
        CIAO_TRY(broadcast_from_owner<T>(ctx, p->d, av, z, nsteps));
        double t[3] = {0.0, 0.0, 0.0};
        if (sh.owner) {
            T hgv;
            CIAO_HIP(hipMemcpyAsync(&hgv, hat_gamma_dev, sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
            CIAO_HIP(hipStreamSynchronize(ctx->stream));
            t[0] = (double)hgv, t[1] = (double)c[0], t[2] = (double)c[1];
        }
        CIAO_HIP(hipMemcpyAsync(ctx->scal, t, sizeof t, hipMemcpyHostToDevice, ctx->stream));
        CIAO_TRY(allreduce_hook(ctx, ctx->scal, 3, CIAO_F64));
        CIAO_HIP(hipMemcpyAsync(t, ctx->scal, sizeof t, hipMemcpyDeviceToHost, ctx->stream));
        CIAO_HIP(hipStreamSynchronize(ctx->stream));
        const T hgv = (T)t[0];
        CIAO_HIP(hipMemcpyAsync(hat_gamma_dev, &hgv, sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        CIAO_HIP(hipStreamSynchronize(ctx->stream));
        c[0] = (long long)t[1], c[1] = (long long)t[2];
    }
    if (done_host) *done_host = c[0];
    if (trials_host) *trials_host = c[1];
    return CIAO_OK;
}

// what the batch-parallel kernels' ProshiArgs and the chain's ProshiChainArgs have in common
template <typename T, template <typename> class Args>
static Args<T> proshi_args(const ciao_sepquad *f, const void *gam, void *table)
{
    Args<T> a{};
    a.Q = (const T *)f->Q;
    a.q = (const T *)f->q;
    a.ld = f->ld;
    a.d = f->d;
    a.N = f->N;
    a.eta = (T)f->eta;
    a.lo = (T)f->lo;
    a.hi = (T)f->hi;
    a.gam = (const T *)gam;
    a.invN = T(1) / (T)f->N_total;
    a.table = (T *)table;
    return a;
}

template <typename T>
static int32_t proshi_init_t(ciao_ctx *ctx, const ciao_sepquad *f, const ciao_prox_desc *g, const void *gam, const void *x0,
                             void *table, void *av, void *z, void *hat_gamma_dev)
{
    ProshiArgs<T> a = proshi_args<T, ProshiArgs>(f, gam, table);
    a.dense = f->dense;
    a.x = (const T *)x0;
    a.nrows = f->N;
    a.idx = nullptr;
    a.row0 = 0;
    Epilogue<T> e = epi_zero<T>();
    e.c_sum = T(1);            // av = sum_i s_i
    e.inv_extra = 2;           // hat_gamma = sum_i gam_i
    e.hg_out = (T *)hat_gamma_dev;
    e.av_out = (T *)av;
    e.z_out = (T *)z;          // z = (prox_{hat_gamma g}(av) - av) / hat_gamma
    e.zmode = 1;
    e.g = make_prox<T>(g);
    return launch_proshi<T>(ctx, true, a, e);
}

template <typename T>
static int32_t proshi_steps_t(ciao_ctx *ctx, const ciao_sepquad *f, const ciao_prox_desc *g, const void *gam, double hat_gamma,
                              int64_t nit, const BatchSrc &src, void *table, void *av, void *z)
{
    for (int64_t t = 0; t < nit; ++t) {
        const int64_t r = src.size(t);
        CIAO_REQUIRE(r >= 1 || (ctx->hook && r == 0), "ProShI batch %lld is empty", (long long)t);
        // Small batches of separable agents: a whole run of equal-sized batches is ONE coordinate-parallel launch
        // (proshi_chain_kernel) instead of two launches per iteration.  Crossover (option proshi_chain_max_batch, -1 = automatic),
        // measured at d = 1024 (tools/proshi_chain_time.py): a visit costs the chain 0.31-0.35 us in fp64, 0.24-0.26 in fp32; a
        // batch-parallel iteration 6.1-6.7 us whatever r.
        const int64_t lim = ctx->proshi_chain_max_batch >= 0 ? ctx->proshi_chain_max_batch : 18;
        if (!ctx->hook && !f->dense && r >= 1 && r <= lim) {
            const int64_t t1 = same_size_run(src, t, nit);
            ProshiChainArgs<T> c = proshi_args<T, ProshiChainArgs>(f, gam, table);
            c.hat_gamma = (T)hat_gamma;
            c.idx = src.idx(t);
            if (src.blocks()) CIAO_TRY(block_indices(ctx, src, t, t1, r, &c.idx));
            c.nvisits = (t1 - t) * r;
            c.batch = r;
            c.g = make_prox<T>(g);
            c.av = (T *)av;
            c.z = (T *)z;
            CIAO_TRY(launch_proshi_chain<T>(ctx, c));
            t = t1 - 1;
            continue;
        }
        ProshiArgs<T> a = proshi_args<T, ProshiArgs>(f, gam, table);
        a.dense = f->dense;
        a.x = (const T *)z;
        a.nrows = r;
        a.idx = src.idx(t);
        a.row0 = src.row0(t);
        Epilogue<T> e = epi_zero<T>();
        e.c_acc = T(1);        // av += sum_{i in batch} (s_i_new - s_i_old)
        e.acc_in = (const T *)av;
        e.c_sum = T(1);
        e.av_out = (T *)av;
        e.z_out = (T *)z;
        e.zmode = 1;
        e.tau = (T)hat_gamma;
        e.g = make_prox<T>(g);
        CIAO_TRY(launch_proshi<T>(ctx, false, a, e));
    }
    return CIAO_OK;
}

// a valid g for the sharing problem: its iterates are real, the complex NormL1 has no meaning for it (and no ProShI kernel implements it)
static int32_t check_real_prox(const ciao_prox_desc *g, const char *who)
{
    CIAO_TRY(check_prox(g));
    if (g && g->kind == CIAO_PROX_L1_COMPLEX) {
        set_error("%s: CIAO_PROX_L1_COMPLEX is not supported for the sharing problem (real iterates only)", who);
        return CIAO_ERR_UNSUPPORTED;
    }
    return CIAO_OK;
}

static int32_t check_sepquad(ciao_ctx *ctx, const ciao_sepquad *f)
{
    CIAO_REQUIRE(ctx && f, "ctx or problem is NULL");
    ctx->rowdot_A = nullptr;
    CIAO_REQUIRE(f->dtype == CIAO_F32 || f->dtype == CIAO_F64, "bad dtype %d", f->dtype);
    CIAO_REQUIRE(f->N >= 0 && f->d >= 1 && f->ld >= f->d && f->N_total >= f->N && f->N_total >= 1, "bad shape");
    CIAO_REQUIRE(f->dense == 0 || f->dense == 1, "ciao_sepquad.dense must be 0 or 1 (got %d)", f->dense);
    CIAO_REQUIRE(f->N == 0 || (f->Q && f->q), "Q or q is NULL");
    CIAO_REQUIRE(f->eta >= 0 && f->lo <= f->hi, "need eta >= 0 and lo <= hi");
    return CIAO_OK;
}

// the small one-launch kernels of these solvers, per type
template <typename T>
static void invsum_t(ciao_ctx *ctx, int nb, int64_t N, const void *gam)
{
    hipLaunchKernelGGL((invsum_kernel<T>), dim3(nb), dim3(256), 0, ctx->stream, N, (const T *)gam, ctx->scal);
}

template <typename T>
static void afinito_probe_t(ciao_ctx *ctx, const ciao_problem *p, int64_t i, const void *x0, const void *signs, double t)
{
    hipLaunchKernelGGL((afinito_probe_kernel<T>), dim3(1), dim3(WAVE), 0, ctx->stream, (const T *)p->A, (const T *)p->b, p->ld, p->d, p->loss,
                       (T)p->lam, i, (const T *)x0, (const T *)signs, (T)t, ctx->scal);
}

template <typename T>
static void proshi_solution_t(ciao_ctx *ctx, const ciao_sepquad *f, int64_t grid, const void *gam, const void *z, void *table)
{
    hipLaunchKernelGGL((proshi_solution_kernel<T>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, f->N, f->d, (const T *)gam, (const T *)z,
                       (T *)table);
}

}  // namespace ciao

using namespace ciao;

extern "C" {

int32_t ciao_hat_gamma(ciao_ctx *ctx, int32_t dtype, int64_t N, const void *gam, double *hat_gamma_host)
{
    CIAO_ENTER(ctx);
    CIAO_REQUIRE(ctx && hat_gamma_host, "ctx or output is NULL");
    CIAO_REQUIRE(dtype == CIAO_F32 || dtype == CIAO_F64, "bad dtype %d", dtype);
    CIAO_REQUIRE(N >= 0 && (N == 0 || gam), "N < 0 or gam is NULL");
    const int nb = 256;
    DISPATCH(dtype, invsum_t, ctx, nb, N, gam);
    CIAO_HIP(hipGetLastError());
    double part_data[256];
    CIAO_HIP(hipMemcpyAsync(part_data, ctx->scal, nb * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CIAO_HIP(hipStreamSynchronize(ctx->stream));
    double s = 0.0;
    for (int i = 0; i < nb; ++i) s += part_data[i];
    if (ctx->hook) {
        CIAO_HIP(hipMemcpyAsync(ctx->scal, &s, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        CIAO_TRY(allreduce_hook(ctx, ctx->scal, 1, CIAO_F64));
        CIAO_HIP(hipMemcpyAsync(&s, ctx->scal, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        CIAO_HIP(hipStreamSynchronize(ctx->stream));
    }
    *hat_gamma_host = 1.0 / s;
    return CIAO_OK;
}

int32_t ciao_finito_init(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *gam, double hat_gamma,
                         const void *x0, void *table, void *av, void *z)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_solve(ctx, p, g));
    CIAO_REQUIRE(x0 && av && z && ((table && gam) || p->N == 0), "NULL state vector / table / gam");
    CIAO_REQUIRE(hat_gamma > 0, "hat_gamma must be > 0");
    return DISPATCH(p->dtype, finito_init_t, ctx, p, g, gam, hat_gamma, x0, table, av, z);
}

// validation of a call's row blocks: inside [0, N), non-negative lengths (empty only on a row-sharded problem)
static int32_t check_blocks(const ciao_ctx *ctx, int64_t N, int64_t n, const int64_t *first_host, const int64_t *len_host, const char *what)
{
    CIAO_REQUIRE(n >= 0 && (n == 0 || (first_host && len_host)), "%s: n < 0 or NULL block arrays", what);
    for (int64_t t = 0; t < n; ++t) {
        CIAO_REQUIRE(len_host[t] >= 1 || (ctx->hook && len_host[t] == 0), "%s: batch %lld is empty", what, (long long)t);
        CIAO_REQUIRE(first_host[t] >= 0 && first_host[t] + len_host[t] <= N, "%s: batch %lld = rows [%lld, %lld) leaves [0, %lld)", what,
                     (long long)t, (long long)first_host[t], (long long)(first_host[t] + len_host[t]), (long long)N);
    }
    return CIAO_OK;
}

int32_t ciao_finito_steps(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *gam, double hat_gamma,
                          int64_t nit, const int64_t *bptr_host, const int64_t *bidx, void *table, void *av, void *z)
{
    CIAO_ENTER_BATCHABLE(ctx);
    CIAO_REQUIRE(!ctx->batch_open || (!ctx->hook && ctx->shards.nshards == 0), "a chain batch cannot run on a row-sharded problem");
    CIAO_TRY(check_solve(ctx, p, g));
    CIAO_REQUIRE(nit >= 0 && (nit == 0 || (bptr_host && (bidx || bptr_host[nit] == bptr_host[0]))), "nit < 0 or NULL batch arrays");
    CIAO_REQUIRE(nit == 0 || p->N > 0, "cannot sample from an empty problem");
    CIAO_REQUIRE(table && av && z && gam, "NULL state vector / table / gam");
    CIAO_REQUIRE(hat_gamma > 0, "hat_gamma must be > 0");
    const BatchSrc src{bptr_host, bidx};
    return DISPATCH(p->dtype, finito_steps_t, ctx, p, g, gam, hat_gamma, nit, src, table, av, z);
}

int32_t ciao_finito_steps_blocks(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *gam, double hat_gamma,
                                 int64_t nit, const int64_t *first_host, const int64_t *len_host, void *table, void *av, void *z)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_solve(ctx, p, g));
    CIAO_TRY(check_blocks(ctx, p->N, nit, first_host, len_host, "ciao_finito_steps_blocks"));
    CIAO_REQUIRE(nit == 0 || p->N > 0 || ctx->hook, "cannot take batches from an empty problem");
    CIAO_REQUIRE(table && av && z && gam, "NULL state vector / table / gam");
    CIAO_REQUIRE(hat_gamma > 0, "hat_gamma must be > 0");
    const BatchSrc src{nullptr, nullptr, first_host, len_host};
    return DISPATCH(p->dtype, finito_steps_t, ctx, p, g, gam, hat_gamma, nit, src, table, av, z);
}

int32_t ciao_lfinito_init(ciao_ctx *ctx, const ciao_problem *p, double hat_gamma, const void *x0, void *av, void *z,
                          void *z_full)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_REQUIRE(x0 && av && z && z_full, "NULL state vector");
    CIAO_REQUIRE(hat_gamma > 0, "hat_gamma must be > 0");
    return DISPATCH(p->dtype, lfinito_init_t, ctx, p, hat_gamma, x0, av, z, z_full);
}

int32_t ciao_lfinito_iterate(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *gam, double hat_gamma,
                             int64_t nb, const int64_t *bptr_host, const int64_t *bidx, void *av, void *z, void *z_full)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_solve(ctx, p, g));
    CIAO_REQUIRE(nb >= 0 && (nb == 0 || (bptr_host && (bidx || bptr_host[nb] == bptr_host[0]))), "nb < 0 or NULL batch arrays");
    CIAO_REQUIRE(av && z && z_full && gam, "NULL state vector / gam");
    CIAO_REQUIRE(hat_gamma > 0, "hat_gamma must be > 0");
    const BatchSrc src{bptr_host, bidx};
    return DISPATCH(p->dtype, lfinito_iterate_t, ctx, p, g, gam, hat_gamma, nb, src, av, z, z_full);
}

int32_t ciao_lfinito_iterate_blocks(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *gam, double hat_gamma,
                                    int64_t nb, const int64_t *first_host, const int64_t *len_host, void *av, void *z, void *z_full)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_solve(ctx, p, g));
    CIAO_TRY(check_blocks(ctx, p->N, nb, first_host, len_host, "ciao_lfinito_iterate_blocks"));
    CIAO_REQUIRE(av && z && z_full && gam, "NULL state vector / gam");
    CIAO_REQUIRE(hat_gamma > 0, "hat_gamma must be > 0");
    const BatchSrc src{nullptr, nullptr, first_host, len_host};
    return DISPATCH(p->dtype, lfinito_iterate_t, ctx, p, g, gam, hat_gamma, nb, src, av, z, z_full);
}

int32_t ciao_afinito_probe(ciao_ctx *ctx, const ciao_problem *p, int64_t i, const void *x0, const void *signs, double t,
                           double *nmg_host)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_problem(ctx, p));
    CIAO_REQUIRE(x0 && signs && nmg_host && t > 0, "NULL argument or t <= 0");
    CIAO_REQUIRE(p->loss != CIAO_LOSS_ZERO && i >= 0 && i < p->N, "sample index %lld outside [0, %lld) or no data terms", (long long)i,
                 (long long)p->N);
    DISPATCH(p->dtype, afinito_probe_t, ctx, p, i, x0, signs, t);
    CIAO_HIP(hipGetLastError());
    CIAO_HIP(hipMemcpyAsync(nmg_host, ctx->scal, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    CIAO_HIP(hipStreamSynchronize(ctx->stream));
    return CIAO_OK;
}

int32_t ciao_afinito_init(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double alpha, const void *x0,
                          void *table, void *meta, void *av, void *z, void *hat_gamma_dev, const void *gam_override)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_solve(ctx, p, g));
    CIAO_REQUIRE(x0 && av && z && hat_gamma_dev && ((table && meta) || p->N == 0), "NULL state vector / table / meta");
    CIAO_REQUIRE(alpha > 0 && alpha < 1, "alpha must be in (0, 1)");
    CIAO_REQUIRE(p->loss != CIAO_LOSS_ZERO, "adaptive Finito needs data terms (the Lipschitz probe of Zero() is degenerate)");
    CIAO_REQUIRE(p->N >= 1 || ctx->shards.nshards > 0, "adaptive Finito needs at least one term");
    CIAO_REQUIRE(!ctx->hook || ctx->shards.nshards > 0,
                 "adaptive Finito is a sequential chain: on a row-sharded problem it needs a shard table (ciao_ctx_set_shards) with "
                 "the table and meta shards");
    CIAO_TRY(check_shards(ctx, p, false));
    return DISPATCH(p->dtype, afinito_init_t, ctx, p, g, alpha, x0, table, meta, av, z, hat_gamma_dev, gam_override);
}

int32_t ciao_afinito_steps(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double alpha, double tol_b,
                           int64_t nsteps, const int64_t *idx, void *table, void *meta, void *av, void *z, void *hat_gamma_dev,
                           int64_t *done_host, int64_t *trials_host)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_solve(ctx, p, g));
    CIAO_REQUIRE(nsteps >= 0 && (nsteps == 0 || idx), "nsteps < 0 or idx is NULL");
    CIAO_REQUIRE(((table && meta) || ctx->shards.nshards > 0) && av && z && hat_gamma_dev, "NULL state vector / table / meta");
    CIAO_REQUIRE(alpha > 0 && alpha < 1 && tol_b > 0, "need 0 < alpha < 1 and tol_b > 0");
    CIAO_REQUIRE(p->loss != CIAO_LOSS_ZERO && (p->N >= 1 || ctx->shards.nshards > 0), "adaptive Finito needs data terms");
    CIAO_REQUIRE(!ctx->hook || ctx->shards.nshards > 0,
                 "adaptive Finito is a sequential chain: on a row-sharded problem it needs a shard table (ciao_ctx_set_shards) with "
                 "the table and meta shards");
    CIAO_TRY(check_shards(ctx, p, true));
    if (ctx->shards.nshards > 0 && ctx->shards.owner)
        for (int k = 0; k < ctx->shards.nshards; ++k)
            CIAO_REQUIRE(ctx->shards.row0[k + 1] == ctx->shards.row0[k] || ctx->shards.meta[k],
                         "shard %d has no meta pointer on the chain owner (adaptive Finito)", k);
    if (nsteps == 0) {
        if (done_host) *done_host = 0;
        if (trials_host) *trials_host = 0;
        return CIAO_OK;
    }
    return DISPATCH(p->dtype, afinito_steps_t, ctx, p, g, alpha, tol_b, nsteps, idx, table, meta, av, z, hat_gamma_dev, done_host,
                    trials_host);
}

int32_t ciao_proshi_init(ciao_ctx *ctx, const ciao_sepquad *f, const ciao_prox_desc *g, const void *gam, const void *x0,
                         void *table, void *av, void *z, void *hat_gamma_dev)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_sepquad(ctx, f));
    CIAO_TRY(check_real_prox(g, "ciao_proshi_init"));
    CIAO_REQUIRE(x0 && av && z && hat_gamma_dev && ((table && gam) || f->N == 0), "NULL state vector / table / gam");
    return DISPATCH(f->dtype, proshi_init_t, ctx, f, g, gam, x0, table, av, z, hat_gamma_dev);
}

int32_t ciao_proshi_steps(ciao_ctx *ctx, const ciao_sepquad *f, const ciao_prox_desc *g, const void *gam, double hat_gamma,
                          int64_t nit, const int64_t *bptr_host, const int64_t *bidx, void *table, void *av, void *z)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_sepquad(ctx, f));
    CIAO_TRY(check_real_prox(g, "ciao_proshi_steps"));
    CIAO_REQUIRE(nit >= 0 && (nit == 0 || (bptr_host && (bidx || bptr_host[nit] == bptr_host[0]))), "nit < 0 or NULL batch arrays");
    CIAO_REQUIRE(table && gam && av && z, "NULL state vector / table / gam");
    CIAO_REQUIRE(hat_gamma > 0, "hat_gamma must be > 0");
    const BatchSrc src{bptr_host, bidx};
    return DISPATCH(f->dtype, proshi_steps_t, ctx, f, g, gam, hat_gamma, nit, src, table, av, z);
}

int32_t ciao_proshi_steps_blocks(ciao_ctx *ctx, const ciao_sepquad *f, const ciao_prox_desc *g, const void *gam, double hat_gamma,
                                 int64_t nit, const int64_t *first_host, const int64_t *len_host, void *table, void *av, void *z)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_sepquad(ctx, f));
    CIAO_TRY(check_real_prox(g, "ciao_proshi_steps_blocks"));
    CIAO_TRY(check_blocks(ctx, f->N, nit, first_host, len_host, "ciao_proshi_steps_blocks"));
    CIAO_REQUIRE(table && gam && av && z, "NULL state vector / table / gam");
    CIAO_REQUIRE(hat_gamma > 0, "hat_gamma must be > 0");
    const BatchSrc src{nullptr, nullptr, first_host, len_host};
    return DISPATCH(f->dtype, proshi_steps_t, ctx, f, g, gam, hat_gamma, nit, src, table, av, z);
}

int32_t ciao_proshi_solution(ciao_ctx *ctx, const ciao_sepquad *f, const void *gam, const void *z, void *table)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_sepquad(ctx, f));
    CIAO_REQUIRE((table && gam && z) || f->N == 0, "NULL argument");
    if (f->N == 0) return CIAO_OK;
    int64_t grid = (f->N * f->d + 255) / 256;
    if (grid > (int64_t)ctx->num_cu * 16) grid = (int64_t)ctx->num_cu * 16;
    DISPATCH(f->dtype, proshi_solution_t, ctx, f, grid, gam, z, table);
    CIAO_HIP(hipGetLastError());
    return CIAO_OK;
}

}  // extern "C"

// api_core.hip -- the library's error state, the context's life cycle and options, and the checks every entry point starts with.
// The only unit that bakes CIAO_BUILD_FLAGS (an experiment build recompiles it whatever else it reuses: tools/exp_build.sh).

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <new>

#include "api_internal.h"

namespace ciao {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

int32_t hip_fail(hipError_t e, const char *what)
{
    set_error("HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
    return CIAO_ERR_HIP;
}

int32_t ensure(ciao_ctx *ctx, void **buf, size_t *have, size_t need)
{
    if (*have >= need) return CIAO_OK;
    // growing a workspace buffer: wait for work that may still read the old one, then reallocate
    CIAO_HIP(hipStreamSynchronize(ctx->stream));
    if (*buf) CIAO_HIP(hipFree(*buf));
    *buf = nullptr;
    *have = 0;
    size_t cap = need + need / 4 + 256;
    hipError_t e = hipMalloc(buf, cap);
    if (e != hipSuccess) {
        set_error("workspace allocation of %zu bytes failed: %s", cap, hipGetErrorString(e));
        return CIAO_ERR_ALLOC;
    }
    *have = cap;
    return CIAO_OK;
}

int32_t check_problem(ciao_ctx *ctx, const ciao_problem *p)
{
    CIAO_REQUIRE(ctx, "ctx is NULL");
    // Any entry point may overwrite the vector the cached a_i'z_full belong to; only ciao_svrg_iterate (which restores
    // the key after this check) and ciao_svrg_inner (which never writes z_full) keep the cache alive.
    ctx->rowdot_A = nullptr;
    CIAO_REQUIRE(p, "problem is NULL");
    CIAO_REQUIRE(p->dtype == CIAO_F32 || p->dtype == CIAO_F64, "problem.dtype must be CIAO_F32 or CIAO_F64 (got %d)", p->dtype);
    CIAO_REQUIRE(p->loss >= CIAO_LOSS_LS && p->loss <= CIAO_LOSS_LS_COMPLEX, "unknown loss kind %d", p->loss);
    CIAO_REQUIRE(p->loss != CIAO_LOSS_LS_COMPLEX || (p->d % 2 == 0 && p->ld % 2 == 0),
                 "complex problems store (re, im) pairs: d and ld count reals and must be even (got d=%lld ld=%lld)", (long long)p->d,
                 (long long)p->ld);
    CIAO_REQUIRE(p->N >= 0 && p->d >= 1, "need N >= 0 and d >= 1 (got N=%lld d=%lld)", (long long)p->N, (long long)p->d);
    CIAO_REQUIRE(p->ld >= p->d, "row stride ld=%lld < d=%lld", (long long)p->ld, (long long)p->d);
    CIAO_REQUIRE(p->N_total >= p->N && p->N_total >= 1, "N_total=%lld must be >= max(N,1)", (long long)p->N_total);
    if (p->N > 0 && p->loss != CIAO_LOSS_ZERO) {   // Zero() terms carry no data (SVRG.jl:58)
        CIAO_REQUIRE(p->A, "problem.A is NULL");
        CIAO_REQUIRE(p->b, "problem.b is NULL");
    }
    return CIAO_OK;
}

int32_t check_prox(const ciao_prox_desc *g)
{
    if (!g) return CIAO_OK;
    CIAO_REQUIRE(g->kind >= CIAO_PROX_ZERO && g->kind <= CIAO_PROX_L1_COMPLEX, "unknown prox kind %d", g->kind);
    if (g->kind == CIAO_PROX_L1 || g->kind == CIAO_PROX_L1_COMPLEX) CIAO_REQUIRE(g->lam >= 0.0, "NormL1 lambda must be >= 0");
    return CIAO_OK;
}

int32_t check_pair(const ciao_problem *p, const ciao_prox_desc *g)
{
    const int kind = g ? g->kind : CIAO_PROX_ZERO;
    if (p->loss == CIAO_LOSS_LS_COMPLEX)
        CIAO_REQUIRE(kind == CIAO_PROX_ZERO || kind == CIAO_PROX_L1_COMPLEX,
                     "a complex problem takes g = Zero or CIAO_PROX_L1_COMPLEX (got prox kind %d)", kind);
    else
        CIAO_REQUIRE(kind != CIAO_PROX_L1_COMPLEX, "CIAO_PROX_L1_COMPLEX needs a complex problem (CIAO_LOSS_LS_COMPLEX)");
    return CIAO_OK;
}

}  // namespace ciao

using namespace ciao;

extern "C" {

int32_t ciao_abi_version(void) { return CIAO_ABI_VERSION; }

const char *ciao_last_error(void) { return g_err; }

#ifndef CIAO_BUILD_FLAGS
#define CIAO_BUILD_FLAGS ""
#endif
const char *ciao_build_flags(void) { return CIAO_BUILD_FLAGS; }

int32_t ciao_ctx_create(int32_t device, void *stream, ciao_ctx **out)
{
    CIAO_REQUIRE(out, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    CIAO_HIP(hipGetDeviceCount(&ndev));
    CIAO_REQUIRE(device >= 0 && device < ndev, "device %d out of range (have %d)", device, ndev);
    DeviceGuard dg(device);   // allocate on `device`, leave the caller's current device as it was
    hipDeviceProp_t prop;
    CIAO_HIP(hipGetDeviceProperties(&prop, device));
    ciao_ctx *ctx = new (std::nothrow) ciao_ctx();
    if (!ctx) {
        set_error("out of host memory");
        return CIAO_ERR_ALLOC;
    }
    ctx->device = device;
    ctx->stream = (hipStream_t)stream;
    ctx->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    hipError_t e = hipMalloc((void **)&ctx->scal, 4096 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&ctx->errflag, sizeof(int));
    if (e == hipSuccess) e = hipMemsetAsync(ctx->errflag, 0, sizeof(int), ctx->stream);
    if (e != hipSuccess) {
        delete ctx;
        return hip_fail(e, "ctx scratch allocation");
    }
    *out = ctx;
    return CIAO_OK;
}

int32_t ciao_ctx_destroy(ciao_ctx *ctx)
{
    if (!ctx) return CIAO_OK;
    DeviceGuard dg(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (void *buf : {ctx->partial, ctx->mrhs_ptrs, ctx->wide_box, ctx->pextra, ctx->sumbuf, ctx->rowdot, ctx->monx, ctx->idxbuf, ctx->cert,
                      (void *)ctx->scal, (void *)ctx->errflag, (void *)ctx->peer_counter, ctx->batch_dev})
        if (buf) (void)hipFree(buf);
    if (ctx->batch_host) (void)hipHostFree(ctx->batch_host);
    if (ctx->batch_ev) (void)hipEventDestroy(ctx->batch_ev);
    for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
    delete ctx;
    return CIAO_OK;
}

int32_t ciao_ctx_set_stream(ciao_ctx *ctx, void *stream)
{
    CIAO_ENTER(ctx);
    ctx->stream = (hipStream_t)stream;
    return CIAO_OK;
}

int32_t ciao_ctx_synchronize(ciao_ctx *ctx)
{
    CIAO_ENTER(ctx);
    int flag = 0;
    CIAO_HIP(hipMemcpyAsync(&flag, ctx->errflag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    CIAO_HIP(hipStreamSynchronize(ctx->stream));
    if (flag) {
        CIAO_HIP(hipMemsetAsync(ctx->errflag, 0, sizeof(int), ctx->stream));
        if (flag == 2) {
            set_error("adaptive Finito init: grad f_i(x0 .+ 1) == grad f_i(x0) for the samples with gamma_i = -1 in meta; the reference "
                      "now probes random points (Finito_adaptive.jl:78-85): resolve them with ciao_afinito_probe and the host's "
                      "draws, then repeat ciao_afinito_init with gam_override");
            return CIAO_ERR_UNSUPPORTED;
        }
        if (flag == 3) {
            set_error("internal: a wave of the wave-specialised chain kernel gave up waiting for another (chain_ws_kernel spin limit); "
                      "results since the last synchronize are invalid -- option chain_no_ws=1 selects the previous chain kernel");
            return CIAO_ERR_HIP;
        }
        if (flag == 4) {
            set_error("peer all-reduce: a rank's flag never arrived (ciao_ctx_set_peers: every rank must make the same reductions in "
                      "the same order); results since the last synchronize are invalid");
            return CIAO_ERR_HOOK;
        }
        if (flag == 5) {
            set_error("internal: a workgroup of the several-workgroup chain (chain_wide_kernel, rows beyond 8192 elements) never saw "
                      "another's partial dot product within 4 s -- the chain's workgroups were not all resident (a GPU shared with other "
                      "work?); results since the last synchronize are invalid -- option chain_no_wide=1 selects the one-workgroup kernel");
            return CIAO_ERR_HIP;
        }
        if (flag == 6) {
            set_error("internal: a workgroup of the cluster sweep (rows_long_kernel, rows beyond 64 KiB) never saw another's partial dot "
                      "product within 4 s -- the grid was not all resident (a GPU shared with other work?); results since the last "
                      "synchronize are invalid -- option long_rows=0 selects the generic kernel");
            return CIAO_ERR_HIP;
        }
        set_error("a sample index was outside [0, N): results since the last synchronize are invalid");
        return CIAO_ERR_ARG;
    }
    return CIAO_OK;
}

int32_t ciao_ctx_set_monitor(ciao_ctx *ctx, const ciao_prox_desc *g, double *obj_dev)
{
    CIAO_ENTER(ctx);
    CIAO_TRY(check_prox(g));
    ctx->monitor = obj_dev;
    ctx->monitor_has_g = (g != nullptr);
    if (g) ctx->monitor_g = *g;
    return CIAO_OK;
}

int32_t ciao_ctx_set_option(ciao_ctx *ctx, const char *key, int64_t value)
{
    CIAO_ENTER(ctx);
    CIAO_REQUIRE(ctx && key, "ctx or key is NULL");
    if (!strcmp(key, "sweep_blocks_per_cu")) {
        CIAO_REQUIRE(value >= 0 && value <= 16, "sweep_blocks_per_cu must be in 0..16 (0 = automatic)");
        ctx->sweep_blocks_per_cu = value;
    } else if (!strcmp(key, "sweep_multi")) {
        ctx->sweep_multi = value != 0;
    } else if (!strcmp(key, "split_max_rows")) {
        CIAO_REQUIRE(value >= -1, "split_max_rows must be >= -1");
        ctx->split_max_rows = value;
    } else if (!strcmp(key, "small_i")) {
        CIAO_REQUIRE(value == 0 || value == 8 || value == 16, "small_i must be 0, 8 or 16");
        ctx->small_i = value;
    } else if (!strcmp(key, "split_all")) {
        ctx->split_all = value != 0;
    } else if (!strcmp(key, "split_blocks_per_cu")) {
        CIAO_REQUIRE(value >= 0 && value <= 16, "split_blocks_per_cu must be in 0..16");
        ctx->split_blocks_per_cu = value;
    } else if (!strcmp(key, "long_rows")) {
        ctx->long_rows = value != 0;
    } else if (!strcmp(key, "long_j")) {
        CIAO_REQUIRE(value == 0 || value == 4 || value == 8, "long_j must be 0, 4 or 8");
        ctx->long_j = value;
    } else if (!strcmp(key, "sweep_grid")) {
        CIAO_REQUIRE(value >= 0 && value <= 65535, "sweep_grid must be in 0..65535");
        ctx->sweep_grid = value;
    } else if (!strcmp(key, "sweep_prefetch")) {
        ctx->sweep_prefetch = value < 0 ? -1 : (value != 0);
    } else if (!strcmp(key, "chain_max_batch")) {
        CIAO_REQUIRE(value >= -1, "chain_max_batch must be >= -1 (-1 = automatic)");
        ctx->chain_max_batch = value;
    } else if (!strcmp(key, "svrg_cache_rowdots")) {
        ctx->svrg_cache_rowdots = value != 0;
        ctx->rowdot_A = nullptr;
    } else if (!strcmp(key, "proshi_chain_max_batch")) {
        CIAO_REQUIRE(value >= -1, "proshi_chain_max_batch must be >= -1 (-1 = automatic)");
        ctx->proshi_chain_max_batch = value;
    } else if (!strcmp(key, "chain_four_waves")) {
        ctx->chain_four_waves = value;
    } else if (!strcmp(key, "chain_big")) {
        ctx->chain_big = value != 0;
    } else if (!strcmp(key, "chain_no_dma")) {
        ctx->chain_no_dma = value != 0;
    } else if (!strcmp(key, "chain_no_wide")) {
        ctx->chain_no_wide = value != 0;
    } else if (!strcmp(key, "chain_no_ws")) {
        ctx->chain_no_ws = value != 0;
    } else if (!strcmp(key, "small_mfma")) {
        ctx->small_mfma = value;
    } else if (!strcmp(key, "wrow_rows_per_wave")) {
        ctx->wrow_rows_per_wave = value;
    } else if (!strcmp(key, "small_wrow")) {
        ctx->small_wrow = value;
    } else if (!strcmp(key, "small_mfma_table")) {
        ctx->small_mfma_table = value;
    } else if (!strcmp(key, "small_nb")) {
        CIAO_REQUIRE(value == 0 || (value >= 2 && value <= 4), "small_nb must be 0 or 2..4");
        ctx->small_nb = value;
    } else if (!strcmp(key, "multi_rhs_off")) {
        ctx->mrhs_off = value != 0;
    } else if (!strcmp(key, "mscore_off")) {
        ctx->mscore_off = value != 0;
    } else if (!strcmp(key, "peer_timeout_s")) {
        CIAO_REQUIRE(value >= 1 && value <= 86400, "peer_timeout_s must be in 1..86400");
        ctx->peer_timeout_s = value;
    } else if (!strcmp(key, "chain_ws_issuers")) {
        CIAO_REQUIRE(value >= 0 && value <= 2, "chain_ws_issuers must be 0 (automatic), 1 or 2");
        ctx->chain_ws_issuers = value;
    } else if (!strcmp(key, "force_generic")) {
        ctx->force_generic = value != 0;
    } else {
        set_error("unknown option '%s'", key);
        return CIAO_ERR_ARG;
    }
    return CIAO_OK;
}

int32_t ciao_ctx_timing_enable(ciao_ctx *ctx, int32_t enable)
{
    CIAO_ENTER(ctx);
    ctx->timing = enable != 0;
    return CIAO_OK;
}

int32_t ciao_ctx_timing_read(ciao_ctx *ctx, double *total_ms_host, int64_t *launches_host)
{
    CIAO_ENTER(ctx);
    CIAO_REQUIRE(ctx && total_ms_host && launches_host, "NULL argument");
    CIAO_HIP(hipStreamSynchronize(ctx->stream));
    double tot = 0.0;
    for (size_t i = 0; i + 1 < ctx->ev_used; i += 2) {
        float ms = 0.f;
        CIAO_HIP(hipEventElapsedTime(&ms, ctx->ev_pool[i], ctx->ev_pool[i + 1]));
        tot += ms;
    }
    *total_ms_host = tot;
    *launches_host = (int64_t)(ctx->ev_used / 2);
    ctx->ev_used = 0;
    return CIAO_OK;
}

const char *ciao_ctx_last_kernel(ciao_ctx *ctx) { return ctx ? ctx->last_kernel.c_str() : ""; }

}  // extern "C"

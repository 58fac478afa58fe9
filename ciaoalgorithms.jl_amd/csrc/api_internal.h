// api_internal.h -- what more than one of the API units (api_*.hip: the extern "C" entry points of libciao_hip.so, declared in
// include/ciao_hip.h) uses: the argument checks, the argument blocks every pass starts from, the type dispatch.
//
// Each entry point validates its arguments on the host (shapes must match what the kernels and their grids assume
// BEFORE anything is launched), builds the kernel argument structs and enqueues the kernels on the ctx's stream.
// Nothing there computes on the CPU: if the HIP runtime or the device is missing the calls fail with CIAO_ERR_HIP.
#pragma once

#include "ciao_ctx.h"
#include "launch.h"

namespace ciao {

#define DISPATCH(dtype, fn, ...) ((dtype) == CIAO_F64 ? fn<double>(__VA_ARGS__) : fn<float>(__VA_ARGS__))

// ---- argument checks (api_core.hip; check_shards: api_comm.hip) -----------------------------------------------------------
int32_t check_problem(ciao_ctx *ctx, const ciao_problem *p);
int32_t check_prox(const ciao_prox_desc *g);
// a complex problem takes g = Zero or the complex NormL1; a real problem never the complex NormL1
int32_t check_pair(const ciao_problem *p, const ciao_prox_desc *g);
// the three above, in this order: what an entry point that takes a problem and a g starts with
inline int32_t check_solve(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g)
{
    CIAO_TRY(check_problem(ctx, p));
    CIAO_TRY(check_prox(g));
    return check_pair(p, g);
}
// a shard table must describe exactly the problem the call is about
int32_t check_shards(const ciao_ctx *ctx, const ciao_problem *p, bool need_table);

// no pointer among these has one of its low three bits set (NULL passes: an optional buffer that is absent)
template <typename... P>
inline bool aligned8(const P *...p)
{
    return ((reinterpret_cast<uintptr_t>(p) | ...) & 7u) == 0;
}

// ---- the argument blocks a pass starts from -----------------------------------------------------------------------------------
template <typename T>
static RowsArgs<T> rows_args(const ciao_problem *p)
{
    RowsArgs<T> a{};
    a.A = (p->loss == CIAO_LOSS_ZERO) ? nullptr : (const T *)p->A;
    a.b = (p->loss == CIAO_LOSS_ZERO) ? nullptr : (const T *)p->b;
    a.ld = p->ld;
    a.d = p->d;
    a.loss = p->loss;
    a.lam = (T)p->lam;
    a.row0 = 0;
    a.nrows = p->N;
    a.idx = nullptr;
    a.invN = T(1) / (T)p->N_total;
    a.N = p->N;
    a.gam_uniform = T(1);
    a.hat_gamma = T(0);
    return a;
}

template <typename T>
static Epilogue<T> epi_zero()
{
    Epilogue<T> e{};
    e.p0 = T(1);
    return e;
}

// a chain's argument block (ChainArgs<T>, AFinitoArgs<T>) over a shard table: indices are GLOBAL rows, every shard's base pointer is
// valid on this device
template <typename T, typename Args>
inline void shard_args(const ciao_ctx *ctx, const ciao_problem *p, Args &a, bool with_table)
{
    const ciao_shard_table &sh = ctx->shards;
    a.nshards = sh.nshards;
    a.N = p->N_total;
    for (int k = 0; k < CIAO_MAX_SHARDS; ++k) {
        const bool on = k < sh.nshards;
        a.shA[k] = on ? (const T *)sh.A[k] : nullptr;
        a.shb[k] = on ? (const T *)sh.b[k] : nullptr;
        a.shT[k] = (on && with_table) ? (T *)sh.table[k] : nullptr;
    }
    for (int k = 0; k <= CIAO_MAX_SHARDS; ++k) a.sh_row0[k] = k <= sh.nshards ? sh.row0[k] : sh.row0[sh.nshards];
}

// ---- shared by api_solvers.hip (which defines them, for float and double) and api_finito.hip ------------------------------------
template <typename T>
ChainArgs<T> chain_args(const ciao_problem *p, const ciao_prox_desc *g);
template <typename T>
int32_t broadcast_from_owner(ciao_ctx *ctx, int64_t d, void *u, void *v, int64_t nsteps);
template <typename T>
int32_t prox_launch(ciao_ctx *ctx, int64_t d, const ciao_prox_desc *g, const T *x, T gamma, T scale, T *y);
// the objective monitor (ciao_ctx_set_monitor; api_solvers.hip says how it rides on a full pass)
template <typename T>
inline void monitor_begin(const ciao_ctx *ctx, const ciao_problem *p, RowsArgs<T> &a, Epilogue<T> &e)
{
    if (!ctx->monitor) return;
    a.want_fval = 1;
    e.obj_out = ctx->monitor;
    e.obj_scale = 1.0 / (double)p->N_total;
}

template <typename T>
int32_t monitor_end(ciao_ctx *ctx, int64_t d, const void *x);

}  // namespace ciao

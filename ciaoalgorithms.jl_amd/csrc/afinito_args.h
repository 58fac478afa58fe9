// afinito_args.h -- the argument block of the adaptive Finito chain kernels (afinito_kernels.h, which says what the fields hold);
// no kernel here.
#pragma once

#include "ciao_common.h"

namespace ciao {

template <typename T>
struct AFinitoArgs {
    const T *A;
    const T *b;
    int64_t ld, d, N;
    T lam;
    int64_t nsteps;
    const int64_t *idx;
    T alpha, tol_b, invN, Nf;
    double Nd;             // N_total as the reference uses it in `0.5 * iter.N * iter.α / γ` (Float64 whatever R, :128)
    ProxD<T> g;
    T *table, *meta, *av, *z;
    T *hg;                // device scalar: hat_gamma (in/out)
    long long *counters;  // [0] steps completed, [1] backtracking trials (out)
    int *errflag;
    // Row-sharded problem (ciao_ctx_set_shards, as ChainArgs): shard k = global rows [sh_row0[k], sh_row0[k+1]) with its data rows,
    // its rows of the s-table and its per-sample scalars in allocations of their own (possibly another GPU's); idx holds GLOBAL rows.
    int nshards;
    const T *shA[CIAO_MAX_SHARDS];
    const T *shb[CIAO_MAX_SHARDS];
    T *shT[CIAO_MAX_SHARDS];
    T *shM[CIAO_MAX_SHARDS];
    int64_t sh_row0[CIAO_MAX_SHARDS + 1];
};

}  // namespace ciao

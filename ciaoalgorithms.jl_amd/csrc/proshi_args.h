// proshi_args.h -- the argument blocks of the ProShI kernels (proshi_kernels.h): the batch-parallel rows kernels' and the
// coordinate-parallel chain's; no kernel here.
#pragma once

#include "ciao_common.h"

namespace ciao {

template <typename T>
struct ProshiArgs {
    const T *Q, *q;        // N x ld each
    int64_t ld, d, N;
    T eta, lo, hi;
    const T *gam;          // per-agent stepsizes
    T invN;
    const T *x;            // INIT: x0 ; STEP: z
    T *table;              // N x d
    int64_t nrows;
    const int64_t *idx;    // STEP: batch members, or nullptr = the contiguous rows row0 .. row0+nrows; INIT: nullptr (all rows)
    int64_t row0;
    T *partial;
    int64_t pstride;
    T *pextra;
    int *errflag;
    int dense;             // Q holds N dense d x d blocks (row k of agent i at Q + (i*d + k)*ld) instead of N diagonals
};

// a run of equal-sized small batches as one launch (proshi_chain_kernel)
template <typename T>
struct ProshiChainArgs {
    const T *Q, *q;
    int64_t ld, d, N;
    T eta, lo, hi;
    const T *gam;
    T invN, hat_gamma;
    const int64_t *idx;        // visited agents, batch after batch
    int64_t nvisits, batch;    // every batch has `batch` members
    ProxD<T> g;
    T *table, *av, *z;
    int *errflag;
};

}  // namespace ciao

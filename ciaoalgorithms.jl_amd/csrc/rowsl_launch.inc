// rowsl_launch.inc -- host side of rows_long_kernel (rowsl_kernels.h: a cluster of workgroups per row, rows beyond 64 KiB) for one
// real type (CIAO_T): how many segments and clusters, and the launch.

#include <algorithm>

#include "ciao_ctx.h"
#include "launch.h"
#include "rowsl_kernels.h"

namespace ciao {

namespace {
template <typename T, int J>
const void *long_kernel(int mode)
{
    switch (mode) {
        case RM_GRAD: return reinterpret_cast<const void *>(&rows_long_kernel<T, J, RM_GRAD>);
        case RM_GRAD2: return reinterpret_cast<const void *>(&rows_long_kernel<T, J, RM_GRAD2>);
        case RM_SAGA_INIT: return reinterpret_cast<const void *>(&rows_long_kernel<T, J, RM_SAGA_INIT>);
        case RM_FINITO_INIT: return reinterpret_cast<const void *>(&rows_long_kernel<T, J, RM_FINITO_INIT>);
        case RM_FINITO_BATCH: return reinterpret_cast<const void *>(&rows_long_kernel<T, J, RM_FINITO_BATCH>);
    }
    return nullptr;
}
template <typename T>
const void *long_kernel_j(int mode, int J)
{
    return J == 8 ? long_kernel<T, 8>(mode) : long_kernel<T, 4>(mode);
}
}  // namespace

// J chunks per thread, S segments per row, C clusters: the grid is C * S workgroups, never more than are resident at once ON AN IDLE
// chip: the clusters spin on their siblings' words, so a GPU shared with other work (another process, another stream's kernels) can
// leave a cluster waiting for a workgroup that has no slot -- bounded (4 s, then error 6 at the next synchronize, which names option
// long_rows=0: the generic kernel).  A cooperative launch would make the runtime check the same residency figure, not the sharing.
template <>
int32_t long_plan<CIAO_T>(ciao_ctx *ctx, int mode, int64_t d, int64_t nrows, int *J_out, int *S_out, int *C_out)
{
    using T = CIAO_T;
    constexpr int VEC = 16 / (int)sizeof(T);
    const int64_t nchunks = d / VEC;
    // measured (tools/long_rows_time.py, profiles/r04_long_rows.txt): 32 KiB segments stream fastest in the read-only modes and the
    // inits (fp64 d = 32768: 5.5 against 3.5 TB/s; the SAGA init 5.9 against 4.7), the Finito batch -- row and table row in
    // registers -- with 16 KiB ones (4.9 against 4.3)
    int J = ctx->long_j == 8 ? 8 : (ctx->long_j == 4 ? 4 : (mode == RM_FINITO_BATCH ? 4 : LONG_J_DEFAULT));
    const void *kern = long_kernel_j<T>(mode, J);
    if (!kern || nrows < 1) return CIAO_ERR_UNSUPPORTED;
    const int64_t S = (nchunks + (int64_t)J * ROWS_BLOCK - 1) / ((int64_t)J * ROWS_BLOCK);
    if (S > LONG_SMAX) return CIAO_ERR_UNSUPPORTED;
    // (asked of the runtime once per kernel -- type, J and mode -- and ctx, not on every launch -- every Finito batch on such rows came through here: ADVICE r4)
    static_assert(RM_AFINITO_INIT < 8, "long_occ has eight slots per (type, J): one per rows mode");
    int &occ = ctx->long_occ[sizeof(T) == 8 ? 1 : 0][J == 8 ? 1 : 0][mode & 7];
    if (occ == 0) {
        int o = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, kern, ROWS_BLOCK, 0) != hipSuccess || o < 1) {
            (void)hipGetLastError();
            o = -1;
        }
        occ = o;
    }
    if (occ < 1) return CIAO_ERR_UNSUPPORTED;
    int64_t bpc = ctx->split_blocks_per_cu > 0 ? ctx->split_blocks_per_cu : (J == 8 ? LONG_BPC_J8 : LONG_BPC_J4);
    bpc = std::min<int64_t>(bpc, occ);
    const int64_t cap = (int64_t)ctx->num_cu * bpc;
    const int64_t C = std::min<int64_t>(nrows, cap / S);
    if (C < 1) return CIAO_ERR_UNSUPPORTED;
    *J_out = J;
    *S_out = (int)S;
    *C_out = (int)C;
    return CIAO_OK;
}

template <>
int32_t launch_long<CIAO_T>(ciao_ctx *ctx, int mode, int J, int S, int C, RowsArgs<CIAO_T> &a)
{
    using T = CIAO_T;
    const int nword = (mode == RM_GRAD2 ? 2 : 1) * WideWord<T>::N;
    const size_t bytes = (size_t)LONG_NBUF * C * S * nword * sizeof(unsigned long long);
    CIAO_TRY(ensure(ctx, &ctx->wide_box, &ctx->wide_box_bytes, bytes));
    CIAO_HIP(hipMemsetAsync(ctx->wide_box, 0, bytes, ctx->stream));   // sequence numbers start at 1: a cleared word matches none
    LongArgs la{};
    la.box = (unsigned long long *)ctx->wide_box;
    la.S = S;
    la.C = C;
    const dim3 grid((unsigned)(C * S)), block(ROWS_BLOCK);
#define CIAO_LONG_CASE(MM)                                                                                  \
    case MM:                                                                                                \
        if (J == 8)                                                                                         \
            hipLaunchKernelGGL((rows_long_kernel<T, 8, MM>), grid, block, 0, ctx->stream, a, la);           \
        else                                                                                                \
            hipLaunchKernelGGL((rows_long_kernel<T, 4, MM>), grid, block, 0, ctx->stream, a, la);           \
        break;
    switch (mode) {
        CIAO_LONG_CASE(RM_GRAD)
        CIAO_LONG_CASE(RM_GRAD2)
        CIAO_LONG_CASE(RM_SAGA_INIT)
        CIAO_LONG_CASE(RM_FINITO_INIT)
        CIAO_LONG_CASE(RM_FINITO_BATCH)
        default: set_error("internal: rows_long_kernel in mode %d", mode); return CIAO_ERR_ARG;
    }
#undef CIAO_LONG_CASE
    return CIAO_OK;
}

}  // namespace ciao

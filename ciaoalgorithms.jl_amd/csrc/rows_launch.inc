// rows_launch.inc -- host dispatch of the rows kernels for one real type (included by rows_f32.hip / rows_f64.hip
// with CIAO_T defined, so the two instantiation sets compile in parallel).

#include <algorithm>
#include <string>

#include "ciao_ctx.h"
#include "launch.h"
#include "proshi_kernels.h"
#include "rows_kernels.h"

namespace ciao {

namespace {

template <typename T, int MODE, int PF>
int32_t launch_fast_pf(ciao_ctx *ctx, int K, int grid, RowsArgs<T> &a)
{
    switch (K) {
        case 1: hipLaunchKernelGGL((rows_fast_kernel<T, 1, MODE, PF>), dim3(grid), dim3(ROWS_BLOCK), 0, ctx->stream, a); break;
        case 2: hipLaunchKernelGGL((rows_fast_kernel<T, 2, MODE, PF>), dim3(grid), dim3(ROWS_BLOCK), 0, ctx->stream, a); break;
        case 4: hipLaunchKernelGGL((rows_fast_kernel<T, 4, MODE, PF>), dim3(grid), dim3(ROWS_BLOCK), 0, ctx->stream, a); break;
        case 8: hipLaunchKernelGGL((rows_fast_kernel<T, 8, MODE, PF>), dim3(grid), dim3(ROWS_BLOCK), 0, ctx->stream, a); break;
        case 16: hipLaunchKernelGGL((rows_fast_kernel<T, 16, MODE, PF>), dim3(grid), dim3(ROWS_BLOCK), 0, ctx->stream, a); break;
        default: set_error("internal: bad K %d", K); return CIAO_ERR_UNSUPPORTED;
    }
    return CIAO_OK;
}

// short rows: R rows per wave per iteration so that R * rowbytes = 8 KiB (rows_multi_kernel)
template <typename T, int MODE>
int32_t launch_multi(ciao_ctx *ctx, int K, int grid, RowsArgs<T> &a)
{
    switch (K) {
        case 2: hipLaunchKernelGGL((rows_multi_kernel<T, 2, 4, MODE>), dim3(grid), dim3(ROWS_BLOCK), 0, ctx->stream, a); break;
        case 4: hipLaunchKernelGGL((rows_multi_kernel<T, 4, 2, MODE>), dim3(grid), dim3(ROWS_BLOCK), 0, ctx->stream, a); break;
        default: set_error("internal: bad K %d for the multi-row kernel", K); return CIAO_ERR_UNSUPPORTED;
    }
    return CIAO_OK;
}

template <typename T, int MODE>
int32_t launch_fast(ciao_ctx *ctx, int K, int grid, RowsArgs<T> &a)
{
    if constexpr (MODE == RM_GRAD || MODE == RM_GRAD2) {
        if (ctx->sweep_multi && (K == 2 || K == 4)) return launch_multi<T, MODE>(ctx, K, grid, a);   // 2 and 4 KiB rows
    }
    // the gradient sweeps come in two pipelining flavours (ctx option "sweep_prefetch"); table modes use occupancy only
    if constexpr (MODE == RM_GRAD || MODE == RM_GRAD2) {
        // automatic: the register pipeline only pays for short rows (2 KiB), see sweep_shape() below
        const int64_t rowb = (int64_t)K * WAVE * 16;
        const bool pf = ctx->sweep_prefetch < 0 ? (rowb == 2048) : (ctx->sweep_prefetch != 0);
        if (pf) return launch_fast_pf<T, MODE, 1>(ctx, K, grid, a);
    }
    return launch_fast_pf<T, MODE, 0>(ctx, K, grid, a);
}

// one launch with dynamic LDS: above the default 64 KiB the ceiling has to be raised per kernel (160 KiB per CU on gfx950)
template <typename Args>
int32_t launch_with_lds(ciao_ctx *ctx, void (*kern)(Args), int64_t grid, int block, size_t lds, Args &a)
{
    if (lds > 60 * 1024)
        CIAO_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(block), lds, ctx->stream, a);
    return CIAO_OK;
}

template <typename T, int MODE>
int32_t launch_generic(ciao_ctx *ctx, int nw, int grid, size_t lds, RowsArgs<T> &a)
{
    if (lds == 0) {   // rows too long for LDS: iterate and per-wave accumulators in global memory (rows_generic_kernel GLOBAL_ACC)
        hipLaunchKernelGGL((rows_generic_kernel<T, 4, MODE, true>), dim3(grid), dim3(4 * WAVE), 0, ctx->stream, a);
        return CIAO_OK;
    }
    if (nw == 4) return launch_with_lds(ctx, &rows_generic_kernel<T, 4, MODE>, grid, 4 * WAVE, lds, a);
    return launch_with_lds(ctx, &rows_generic_kernel<T, 1, MODE>, grid, WAVE, lds, a);
}

template <typename T, int MODE>
int32_t launch_cplx(ciao_ctx *ctx, int grid, RowsArgs<T> &a)
{
    hipLaunchKernelGGL((rows_cplx_kernel<T, MODE>), dim3((unsigned)grid), dim3(ROWS_BLOCK), 0, ctx->stream, a);
    return CIAO_OK;
}

template <typename T, int MODE>
int32_t launch_csplit(ciao_ctx *ctx, int J, int grid, RowsArgs<T> &a)
{
    switch (J) {
        case 1: hipLaunchKernelGGL((rows_csplit_kernel<T, 1, MODE>), dim3((unsigned)grid), dim3(ROWS_BLOCK), 0, ctx->stream, a); break;
        case 2: hipLaunchKernelGGL((rows_csplit_kernel<T, 2, MODE>), dim3((unsigned)grid), dim3(ROWS_BLOCK), 0, ctx->stream, a); break;
        case 4: hipLaunchKernelGGL((rows_csplit_kernel<T, 4, MODE>), dim3((unsigned)grid), dim3(ROWS_BLOCK), 0, ctx->stream, a); break;
        case 8: hipLaunchKernelGGL((rows_csplit_kernel<T, 8, MODE>), dim3((unsigned)grid), dim3(ROWS_BLOCK), 0, ctx->stream, a); break;
        case 16: hipLaunchKernelGGL((rows_csplit_kernel<T, 16, MODE>), dim3((unsigned)grid), dim3(ROWS_BLOCK), 0, ctx->stream, a); break;
        default: set_error("internal: bad J %d", J); return CIAO_ERR_UNSUPPORTED;
    }
    return CIAO_OK;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// one workgroup per row; MASKED handles any 16-byte aligned row of up to J*4096 bytes; scalar = element-wise chunks for
// rows with no alignment (always masked)
template <typename T, int MODE>
int32_t launch_split(ciao_ctx *ctx, int J, bool masked, bool scalar, int grid, RowsArgs<T> &a)
{
    constexpr int VEC = 16 / sizeof(T);
#define CIAO_SPLIT_CASE(JJ)                                                                                                    \
    case JJ:                                                                                                                   \
        if (scalar)                                                                                                            \
            hipLaunchKernelGGL((rows_split_kernel<T, JJ, MODE, true, 1>), dim3(grid), dim3(ROWS_BLOCK), 0, ctx->stream, a);    \
        else if (masked)                                                                                                       \
            hipLaunchKernelGGL((rows_split_kernel<T, JJ, MODE, true, VEC>), dim3(grid), dim3(ROWS_BLOCK), 0, ctx->stream, a);  \
        else if constexpr ((MODE == RM_GRAD2 || MODE == RM_FINITO_BATCH) && JJ <= 4) /* exact shapes are K <= 16: J <= 4 */   \
            hipLaunchKernelGGL((rows_split_kernel<T, JJ, MODE, false, VEC>), dim3(grid), dim3(ROWS_BLOCK), 0, ctx->stream, a); \
        else                                                                                                                   \
            hipLaunchKernelGGL((rows_split_kernel<T, JJ, MODE, true, VEC>), dim3(grid), dim3(ROWS_BLOCK), 0, ctx->stream, a);  \
        break;
    switch (J) {
        CIAO_SPLIT_CASE(1)
        CIAO_SPLIT_CASE(2)
        CIAO_SPLIT_CASE(4)
        CIAO_SPLIT_CASE(8)
        CIAO_SPLIT_CASE(16)
        default: set_error("internal: bad J %d", J); return CIAO_ERR_UNSUPPORTED;
    }
#undef CIAO_SPLIT_CASE
    return CIAO_OK;
}

}  // namespace

namespace {
// finalize the per-block partials (+ all-reduce hook) + epilogue; shared by the rows and ProShI launches
// finalize on 256 threads (up to 256 partials: one round of loads) or 1024 (rows_kernels.h FIN_THREADS_MANY)
#define CIAO_FINALIZE(...)                                                                                                        \
    do {                                                                                                                          \
        if (grid > 256)                                                                                                           \
            hipLaunchKernelGGL((finalize_kernel<T, FIN_THREADS_MANY>), dim3(fgrid), dim3(FIN_THREADS_MANY), 0, ctx->stream, __VA_ARGS__); \
        else                                                                                                                      \
            hipLaunchKernelGGL((finalize_kernel<T, FIN_THREADS>), dim3(fgrid), dim3(FIN_THREADS), 0, ctx->stream, __VA_ARGS__);   \
    } while (0)
int32_t finish_reduction(ciao_ctx *ctx, int64_t d, int grid, int64_t pstride, const Epilogue<CIAO_T> &ep, bool raw_only)
{
    using T = CIAO_T;
    // ---- finalize (+ all-reduce hook) + epilogue ---------------------------------------------------------------------
    const int fcols = FIN_BYTES / (int)sizeof(T);
    const int fgrid = (int)((d + fcols - 1) / fcols);
    const PeerDev nopeers{};
    if (ctx->peer_world > 0) {
        // one-shot peer all-reduce fused into the pair of kernels that exists anyway (peer_kernels.h): finalize stores the raw sum
        // into every rank's mailbox and releases this rank's flag; the epilogue waits for the world's flags and adds the slots in
        // rank order.  No collective call, no extra launch.
        if (d + 1 > ctx->peer_max_elems) {
            set_error("the peer mailboxes hold %lld elements, this reduction has %lld (ciao_peer_mailbox_create)", (long long)ctx->peer_max_elems,
                      (long long)(d + 1));
            return CIAO_ERR_ARG;
        }
        const PeerDev pd = peer_dev(ctx);
        CIAO_FINALIZE(
                           (const T *)ctx->partial, pstride, grid, (const T *)ctx->pextra, d, (T *)ctx->sumbuf, ep, pd);
        if (raw_only)
            hipLaunchKernelGGL((peer_recv_kernel<T>), dim3((unsigned)((d + 1 + 255) / 256)), dim3(256), 0, ctx->stream, (T *)ctx->sumbuf, d + 1, pd);
        else
            hipLaunchKernelGGL((peer_epilogue_kernel<T>), dim3((unsigned)((d + 255) / 256)), dim3(256), 0, ctx->stream, d, ep, pd);
    } else if (ctx->hook || raw_only) {
        CIAO_FINALIZE(
                           (const T *)ctx->partial, pstride, grid, (const T *)ctx->pextra, d, (T *)ctx->sumbuf, ep, nopeers);
        CIAO_HIP(hipGetLastError());
        if (ctx->hook) CIAO_TRY(allreduce_hook(ctx, ctx->sumbuf, d + 1, sizeof(T) == 8 ? CIAO_F64 : CIAO_F32));
        if (!raw_only)
            hipLaunchKernelGGL((epilogue_kernel<T>), dim3((unsigned)((d + 255) / 256)), dim3(256), 0, ctx->stream,
                               (const T *)ctx->sumbuf, d, ep);
    } else {
        CIAO_FINALIZE(
                           (const T *)ctx->partial, pstride, grid, (const T *)ctx->pextra, d, (T *)nullptr, ep, nopeers);
    }
    CIAO_HIP(hipGetLastError());
    return CIAO_OK;
}
#undef CIAO_FINALIZE

// the workspace of a launch that leaves nparts partial d-vectors (and an extra scalar each) for finish_reduction: grown on
// demand, the kernel's arguments (RowsArgs or ProshiArgs) pointed at it; the partials' stride is a.pstride
template <typename Args>
int32_t reduction_workspace(ciao_ctx *ctx, int64_t d, int64_t nparts, Args &a)
{
    using T = CIAO_T;
    a.pstride = (d + 63) / 64 * 64;
    CIAO_TRY(ensure(ctx, &ctx->partial, &ctx->partial_bytes, (size_t)nparts * (size_t)a.pstride * sizeof(T)));
    CIAO_TRY(ensure(ctx, &ctx->pextra, &ctx->pextra_bytes, (size_t)nparts * sizeof(T)));
    CIAO_TRY(ensure(ctx, &ctx->sumbuf, &ctx->sumbuf_bytes, (size_t)(d + 1) * sizeof(T)));
    a.partial = (T *)ctx->partial;
    a.pextra = (T *)ctx->pextra;
    a.errflag = ctx->errflag;
    return CIAO_OK;
}

// ---- which kernel, on what grid ------------------------------------------------------------------------------------------
// The five families, in the order they are tried:
//   WAVE_ROW   rows_fast_kernel / rows_multi_kernel   d = 64*VEC*{1,2,4,8,16} exactly, 16-byte aligned rows
//   SPLIT      rows_split_kernel                       a workgroup per row: small / medium batches on those shapes; every
//                                                      other row of whole 16-byte chunks (masked tail) or of single
//                                                      elements (scalar) up to 64 KiB / 4096 elements
//   SMALL      rows_small_kernel                       several rows per wave: contiguous sweeps over rows under 1 KiB
//   SMALLM     rows_smallm_kernel                      ... the GRAD sweeps among them on the matrix cores (dense rows of 17 .. 256 elements)
//   LONG       rows_long_kernel                        rows of whole 16-byte chunks beyond 64 KiB: a cluster of workgroups per row
//   GENERIC    rows_generic_kernel                     anything else
enum RowsKind { RK_WAVE_ROW, RK_SPLIT, RK_SMALL, RK_SMALLM, RK_SMALLB, RK_WROW, RK_GENERIC, RK_CPLX, RK_CSPLIT, RK_LONG };

struct RowsPlan {
    RowsKind kind = RK_GENERIC;
    int K = 0;              // WAVE_ROW: 16-byte chunks per lane
    int J = 0;              // SPLIT: chunks per thread
    bool masked = false;    // SPLIT: predicated tail
    bool scalar = false;    // SPLIT: one element per chunk
    int small_i = 16;       // SMALL: elements per lane and iteration
    int nw = 0;             // GENERIC: waves per block
    size_t lds = 0;         // SMALL / GENERIC: dynamic LDS bytes (GENERIC with 0: accumulators in global memory, one per wave)
    int parts_per_block = 1;   // partial d-vectors each block writes (4 for the global-accumulator generic kernel)
    int long_S = 0, long_C = 0;   // LONG: segments per row, clusters (grid = S * C; ONE partial per cluster)
    int64_t grid = 1;
    int block = ROWS_BLOCK;
};

int32_t plan_rows(const ciao_ctx *ctx, int mode, const RowsArgs<CIAO_T> &a, RowsPlan &pl)
{
    using T = CIAO_T;
    if (a.loss == CIAO_LOSS_LS_COMPLEX) {
        // complex T: rows of whole 16-byte chunks up to 64 KiB stream through rows_csplit_kernel (one workgroup per row, the
        // grid rule of the real workgroup-per-row kernel); everything else takes rows_cplx_kernel (one partial per wave)
        constexpr int CV = 16 / sizeof(T);
        const int64_t crowb = a.d * (int64_t)sizeof(T);
        const bool ctable = (mode == RM_SAGA_INIT || mode == RM_FINITO_INIT || mode == RM_FINITO_BATCH);
        if (!ctx->force_generic && mode != RM_AFINITO_INIT && a.d % CV == 0 && a.d / CV >= 64 && a.d / CV <= 16 * ROWS_BLOCK &&
            aligned16(a.A) && (a.ld * (int64_t)sizeof(T)) % 16 == 0 && aligned16(a.x1) && (mode != RM_GRAD2 || aligned16(a.x2)) &&
            (!ctable || aligned16(a.table))) {
            int j = 1;
            while ((int64_t)j * ROWS_BLOCK < a.d / CV) j *= 2;
            pl.kind = RK_CSPLIT;
            pl.J = j;
            int64_t bpc = 1;
            const int64_t resident = j == 1 ? 6 : (j == 2 ? 5 : (j == 4 ? 4 : (j == 8 ? 2 : 1)));
            if (a.nrows > 16384) {
                bpc = (49152 + crowb / 2) / crowb;
                bpc = bpc < 1 ? 1 : (bpc > resident ? resident : bpc);
            } else if (crowb <= 8192) {   // (the real kernel's rule for batches on rows of up to 8 KiB, below)
                const int64_t by_bytes = crowb > 4096 ? 2 : (crowb > 2048 ? 4 : resident);
                bpc = std::max<int64_t>(1, std::min<int64_t>(by_bytes, a.nrows / ((int64_t)ctx->num_cu * 4)));
            }
            if (ctx->split_blocks_per_cu > 0) bpc = ctx->split_blocks_per_cu;
            pl.grid = std::max<int64_t>(1, std::min<int64_t>(a.nrows, (int64_t)ctx->num_cu * bpc));
            return CIAO_OK;
        }
        pl.kind = RK_CPLX;
        pl.parts_per_block = ROWS_WAVES;
        pl.grid = std::max<int64_t>(1, std::min<int64_t>((a.nrows + ROWS_WAVES - 1) / ROWS_WAVES, ctx->num_cu));
        return CIAO_OK;
    }
    constexpr int VEC = 16 / sizeof(T);
    const int64_t d = a.d;
    const int64_t rowb = d * (int64_t)sizeof(T);
    const bool two = (mode == RM_GRAD2);
    const bool table = (mode == RM_SAGA_INIT || mode == RM_FINITO_INIT || mode == RM_FINITO_BATCH || mode == RM_AFINITO_INIT);
    const bool rows16 = aligned16(a.A) && (a.ld * (int64_t)sizeof(T)) % 16 == 0 && (!table || aligned16(a.table));
    const bool fast_ok = !ctx->force_generic;

    // ---- WAVE_ROW shape? ----
    int K = 0;
    if (fast_ok && d % (WAVE * VEC) == 0 && rows16) {
        const int64_t k = d / (WAVE * VEC);
        if (k == 1 || k == 2 || k == 4 || k == 8 || k == 16) K = (int)k;
    }
    // ---- SPLIT on 16-byte chunks? ----
    int JS = 0;
    bool masked = false, scalar = false;
    if (fast_ok && mode != RM_AFINITO_INIT && d % VEC == 0 && d / VEC <= 16 * ROWS_BLOCK && rows16 && aligned16(a.x1) &&
        (!two || aligned16(a.x2))) {
        const int64_t nch = d / VEC;
        int j = 1;
        while ((int64_t)j * ROWS_BLOCK < nch) j *= 2;
        if (K > 0) {
            // measured on MI355X (tools/finito_batch_time.py, d=4096 fp32): r = 64 / 256 / 1024 / 8192 rows take 6.9 / 10.4 /
            // 19.2 / 82-89 us per batch here against 51.8 (as a chain) / 14.3 / 22.0 / 94.5 us one wave per row; from r = 16384
            // on the two are level (5.2 TB/s) and the wave-per-row kernel pulls ahead (5.6 vs 5.1-5.5 TB/s at r = 65536)
            const int64_t lim = ctx->split_max_rows >= 0 ? ctx->split_max_rows : 16384;
            const bool batch = (a.idx || a.nrows < a.N) && (mode == RM_GRAD2 || mode == RM_FINITO_BATCH);   // index list or row block
            if (batch && nch == (int64_t)j * ROWS_BLOCK && j <= 8 && a.nrows <= lim) JS = j;
            if (ctx->split_all && nch >= 64) {   // tuning experiment: the workgroup-per-row kernel for every mode and size
                JS = j;
                masked = true;
            }
        } else if (nch >= 64) {   // shorter rows leave most of a workgroup idle (d = 50 fp64: 0.5 TB/s; d = 300: 2.6)
            JS = j;
            masked = true;
        }
    }
    // ---- SPLIT on single elements: rows with no 16-byte structure, 256 .. 4096 elements ----
    if (fast_ok && K == 0 && JS == 0 && mode != RM_AFINITO_INIT && d >= 256 && d <= 16 * ROWS_BLOCK) {
        int j = 1;
        while ((int64_t)j * ROWS_BLOCK < d) j *= 2;
        JS = j;
        masked = scalar = true;
    }
    // ---- SMALL: contiguous sweeps over rows of at most 256 elements that nothing above takes ----
    // (padded rows too: the group is then a strided stretch, ld < 2^24 keeps the in-group offsets in 32 bits)
    const bool small = fast_ok && K == 0 && JS == 0 && !a.idx && d >= 1 && d <= 256 && a.ld < (1 << 24) &&
                       (mode == RM_GRAD || mode == RM_SAGA_INIT || mode == RM_FINITO_INIT);
    // ---- SMALLB: the batch modes (Finito batch, LFinito batch sweep) on such rows, index list or row block, any stride ----
    const bool smallb = fast_ok && K == 0 && JS == 0 && d >= 1 && d <= 256 && (mode == RM_GRAD2 || mode == RM_FINITO_BATCH);

    // ---- SMALLM: of those, everything over DENSE rows of 17 .. 256 elements that comes as one block of rows (no index list) on the
    // matrix cores: GRAD, GRAD2, and the table modes (whose table block is dense by construction: stride d)
    const bool smallm_tab = (mode == RM_FINITO_BATCH);
    const bool smallm = ((small && (mode == RM_GRAD || ctx->small_mfma_table != 0)) || (smallb && !a.idx && (mode == RM_GRAD2 || ctx->small_mfma_table != 0))) &&
                        ctx->small_mfma != 0 && d >= 17 && a.ld == d && a.A != nullptr && aligned16(a.A) && (a.row0 * rowb) % 16 == 0 &&
                        (!table || aligned16(a.table)) && (int64_t)smallm_lds<T>(d, 2, smallm_tab) + 8192 <= 160 * 1024;

    // ---- LONG: rows of whole 16-byte chunks beyond the workgroup-per-row kernel's 4096 chunks ----
    if (fast_ok && ctx->long_rows && JS == 0 && K == 0 && mode != RM_AFINITO_INIT && a.A != nullptr && d % VEC == 0 && d / VEC > 16 * ROWS_BLOCK && rows16 &&
        aligned16(a.x1) && (!two || aligned16(a.x2))) {
        int lj = 0, ls = 0, lc = 0;
        if (long_plan<T>(const_cast<ciao_ctx *>(ctx), mode, d, a.nrows, &lj, &ls, &lc) == CIAO_OK) {
            pl.kind = RK_LONG;
            pl.J = lj;
            pl.long_S = ls;
            pl.long_C = lc;
            pl.grid = (int64_t)ls * lc;
            return CIAO_OK;
        }
    }
    if (JS > 0) {
        pl.kind = RK_SPLIT;
        pl.J = JS;
        pl.masked = masked;
        pl.scalar = scalar;
        // batches: one row per workgroup up to one workgroup per CU -- more blocks only add partials for finalize to sum
        // (r = 1024: 19.6 / 22.4 / 29.1 us per batch at 1 / 2 / 4 blocks per CU).  Long sweeps (bench.py --d D
        // --blocks-per-cu B, fp64 GRAD, TB/s): 8 KB rows 5.2 / 6.5 / 5.9 at B = 3 / 5 / 8; 12 KB 5.1 / 6.9 / 6.1 at 2 / 4 / 6;
        // 24 KB 4.4 / 6.7 / 5.6 at 1 / 2 / 3; 32 KB 5.2 / 6.9 / 6.1 at 1 / 2 / 3 -> about 48 KB in flight per CU, but never
        // more workgroups than are resident at once (6 / 5 / 4 / 2 / 1 per CU for J = 1 / 2 / 4 / 8 / 16), or the surplus
        // queues behind the first round
        int64_t bpc = 1;
        const int64_t resident = JS == 1 ? 6 : (JS == 2 ? 5 : (JS == 4 ? 4 : (JS == 8 ? 2 : 1)));
        if (a.nrows > 16384) {
            bpc = (49152 + rowb / 2) / (rowb > 0 ? rowb : 1);
            bpc = bpc < 1 ? 1 : (bpc > resident ? resident : bpc);
        } else if (rowb <= 8192) {
            // rows of up to 8 KiB leave a CU idle with one workgroup on it: batches of a few thousand rows and more take several,
            // as long as a workgroup keeps four rows (round 5, with the 1024-thread finalize the extra partials cost one
            // round of loads: d = 300 fp32 r = 4096 / 16 384 27.2 -> 19.0 / 84.5 -> 34.9 us per batch, d = 784 fp64 33.6 -> 28.7 / 109.5 -> 74.8;
            // profiles/r05_midrow_batches.txt).  Longer rows stay at one workgroup per CU: their partials are as long as they are
            // (d = 4096 fp32: r = 2048 29.7 us on 256 workgroups, 31.0 on 512)
            // (measured best: 2 per CU for rows of 4-8 KiB -- d = 1024 fp64 r = 4096 / 16 384 34.3 -> 30.9 / 111.7 -> 92.8, three and more are
            // slower again --, 3-4 for 2-4 KiB, up to the residency below that)
            const int64_t by_bytes = rowb > 4096 ? 2 : (rowb > 2048 ? 4 : resident);
            bpc = std::min<int64_t>(by_bytes, a.nrows / ((int64_t)ctx->num_cu * 4));
            bpc = bpc < 1 ? 1 : bpc;
        }
        if (ctx->split_blocks_per_cu > 0) bpc = ctx->split_blocks_per_cu;
        pl.grid = std::min<int64_t>(a.nrows, (int64_t)ctx->num_cu * bpc);
    } else if (K > 0) {
        pl.kind = RK_WAVE_ROW;
        pl.K = K;
        // one row per wave while that still fits one block per CU; beyond that at least 4 rows per wave (measured: r = 4096
        // rows run 1.4x faster on 256 blocks than on 1024, r = 256 rows 1.7x faster on 64 blocks than on 16)
        const int64_t g1 = (a.nrows + ROWS_WAVES - 1) / ROWS_WAVES;
        const int64_t g4 = (a.nrows + 4 * ROWS_WAVES - 1) / (4 * ROWS_WAVES);
        pl.grid = g1 <= ctx->num_cu ? g1 : (g4 > ctx->num_cu ? g4 : ctx->num_cu);
        // Persistent grid size.  Measured with non-temporal row loads (tools/tune_sweep.py, profiles/): HBM streams fastest
        // with about 8-12 MB of loads in flight chip-wide (32-48 KiB per CU); more waves than that LOSE bandwidth (7.1 TB/s
        // at 256 blocks vs 6.5 TB/s at 1024 for 8 KiB rows).  So the grid shrinks as the rows grow:
        //   row bytes   >=16384   8192   4096   2048   <=1024
        //   blocks          192    256    512   1024     2048      (x num_cu/256; 4 waves each, one row per wave in flight)
        // 2 / 4 KiB rows run rows_multi_kernel (8 KiB per wave in flight): best at 1024 / 512 blocks (7.1 / 7.2 TB/s);
        // the read+write table modes are flat above ~2 blocks per CU (grid scan of round 1, profiles/README.md)
        int64_t cap;
        if (ctx->sweep_blocks_per_cu > 0) {
            cap = (int64_t)ctx->num_cu * ctx->sweep_blocks_per_cu;
        } else if (table) {
            cap = (rowb >= 2048 ? 512 : 1024) * (int64_t)ctx->num_cu / 256;
        } else {
            const bool multi = ctx->sweep_multi && (K == 2 || K == 4);
            const int64_t base = rowb >= 16384 ? 192 : (rowb >= 8192 ? 256 : (rowb >= 4096 ? 512 : (rowb >= 2048 ? (multi ? 1024 : 768) : 2048)));
            cap = base * ctx->num_cu / 256;
        }
        pl.grid = std::min(pl.grid, cap);
    } else if (smallb && (!smallm || a.nrows <= 8192) && ctx->small_wrow != 0 && wrow_plan<T>(mode, a, &pl.K, &pl.J)) {
        // (batches of up to 8192 rows given as a row block too -- Finito: 12.7 against 15.9 us at r = 4096, d = 50 fp64, 13.0 against 18.7 at
        // d = 100 fp32; an LFinito iteration in batches of 2048: 4.3 against 7.3 ms at d = 100 fp64, 4.6 against 10.0 at d = 255 fp32; level
        // at 16 384, the tiles ahead beyond -- profiles/r05_wrow_blocks.txt)
        // Finito batches the matrix-core tiles do not take -- every index list (the reference's default sweeping = 1), and row blocks of
        // shapes whose tiles do not fit LDS: one wave per row, two rows in flight per wave, eight waves per SIMD (rowsw_kernels.h; pl.K
        // = elements per chunk, pl.J = chunks per lane)
        pl.kind = RK_WROW;
        {   // two workgroups per CU, each of 2 x (the waves per SIMD the registers allow) waves: rowsw_kernels.h WrowWaves
            const int bw = wrow_block_waves<T>(pl.K, pl.J);
            pl.block = bw * WAVE;
            // a small batch is cut into FOUR rows per wave: one row per wave makes four times the workgroups, as many partial d-vectors
            // for finalize to add and a block-level reduction per row (r = 16 384 at d = 50 fp64: 24.5 us per batch at one row per wave,
            // 21.6 at four, 21.2 at eight; r = 4096: 18.8 / 16.6 / 16.3; profiles/r05_small_batches.txt; option wrow_rows_per_wave)
            const int64_t rpw = ctx->wrow_rows_per_wave > 0 ? ctx->wrow_rows_per_wave : 4;
            // ... but first one workgroup on every CU (r = 4096 at d = 100 fp64: 16.2 us per batch on 86 workgroups of four rows per wave,
            // 14.9 on 256)
            const int64_t by_rpw = (a.nrows + bw * rpw - 1) / (bw * rpw), one_each = std::min<int64_t>(ctx->num_cu, (a.nrows + bw - 1) / bw);
            pl.grid = std::max<int64_t>(1, std::min<int64_t>(std::max(by_rpw, one_each), (int64_t)ctx->num_cu * 2));
        }
    } else if (smallb && !smallm) {
        pl.kind = RK_SMALLB;
        pl.scalar = (a.idx != nullptr) || a.ld != a.d;   // (reused for this kind: the rows are gathered, not one dense block)
        // 8 elements per lane in both precisions: the Finito batch keeps row AND table row of two groups in flight, and 16 per lane
        // leave one wave per SIMD (fp64 d = 50 / 100 / 255, r = 65536 blocks: 1.50 / 2.10 / 2.94 TB/s at 16, 1.68 / 2.39 / 3.56 at 8)
        pl.small_i = 8;
#define CIAO_SMALLB_BYTES(II) (pl.scalar ? (two ? smallb_wave_bytes<T, RM_GRAD2, II, true>() : smallb_wave_bytes<T, RM_FINITO_BATCH, II, true>()) \
                                         : (two ? smallb_wave_bytes<T, RM_GRAD2, II, false>() : smallb_wave_bytes<T, RM_FINITO_BATCH, II, false>()))
        pl.lds = (size_t)ROWS_WAVES * CIAO_SMALLB_BYTES(8);
#undef CIAO_SMALLB_BYTES
        int64_t G = (int64_t)WAVE * pl.small_i / d;
        if (G > WAVE) G = WAVE;
        const int64_t ngroups = (a.nrows + G - 1) / G;
        pl.grid = std::max<int64_t>(1, std::min<int64_t>((ngroups + ROWS_WAVES - 1) / ROWS_WAVES, (int64_t)ctx->num_cu * (pl.small_i == 8 ? 8 : 4)));
    } else if (smallm) {
        // the row dots as MFMAs over tiles of 16 rows staged by LDS-DMA, the rank-1 accumulation as FMAs on the registers the MFMAs
        // read (rowsm_kernels.h).  Measured (profiles/r04_small_mfma.txt, N = 4M, TB/s): fp32 d = 50 / 100 / 200 / 255 5.3 / 5.6 / 5.6 / 5.8
        // against 4.2 / 4.2 / 3.8 / 4.5 on rows_small_kernel; fp64 d = 50 / 120 5.8 / 5.9 against 5.3 / 5.5 (fp64 rows beyond 144
        // elements do not fit two tile buffers per wave in LDS and stay there).  A ring of nb tile buffers per wave (option small_nb):
        // deeper rings cost resident waves and were slower at every shape, so two.  Resident workgroups per CU are set by LDS (8 KiB
        // of margin per workgroup: a grid sized for one workgroup more than fits runs a second, half-empty round)
        pl.kind = RK_SMALLM;
        const int64_t budget = 160 * 1024;
        int nb = 2;
        if (ctx->small_nb >= 2 && ctx->small_nb <= 4 && (int64_t)smallm_lds<T>(d, (int)ctx->small_nb, smallm_tab) + 8192 <= budget &&
            (ctx->small_nb - 2) * ((16 * rowb + 1023) / 1024 + 1) <= 63)
            nb = (int)ctx->small_nb;
        pl.small_i = nb;
        pl.lds = smallm_lds<T>(d, nb, smallm_tab);
        const int64_t bpc = std::max<int64_t>(1, std::min<int64_t>(8, budget / ((int64_t)pl.lds + 8192)));
        const int64_t ntiles = (a.nrows + 15) / 16;
        pl.grid = std::min<int64_t>((ntiles + ROWS_WAVES - 1) / ROWS_WAVES, (int64_t)ctx->num_cu * bpc);
    } else if (small) {
        pl.kind = RK_SMALL;
        // measured (4M rows, TB/s at 16 / 8 elements per lane): fp64 d=50 4.3 / 3.9, d=127 4.5 / 4.0; fp32 d=50 2.7 / 3.4,
        // d=255 2.8 / 3.4; d=5 fp64 2.0 / 3.0 (a group holds at most 64 rows, so tiny rows cannot fill the larger group).
        // Round 4: with the row scalars read by global loads (they were FLAT loads against a scratch slot) fp64 d=50 / 120 run 5.2 /
        // 5.5 TB/s and fp32 d=50 / 100 / 200 / 255 4.2 / 4.2 / 3.8 / 4.5; 16-byte chunks per lane instead of single elements were
        // tried on top and are SLOWER (fp32 3.1 / 3.1 / 2.7, fp64 4.1 / 4.4: profiles/r04_small_sweeps.txt) -- the per-chunk tail
        // test costs more than the narrower loads do
        pl.small_i = ctx->small_i > 0 ? (int)ctx->small_i : ((sizeof(T) == 4 || d <= 8) ? 8 : 16);
        pl.lds = (size_t)ROWS_WAVES * (WAVE * pl.small_i + 2 * WAVE) * sizeof(T);
        int64_t G = (int64_t)WAVE * pl.small_i / d;   // rows per wave-iteration
        if (G > WAVE) G = WAVE;
        const int64_t ngroups = (a.nrows + G - 1) / G;
        pl.grid = std::min<int64_t>((ngroups + ROWS_WAVES - 1) / ROWS_WAVES, (int64_t)ctx->num_cu * (pl.small_i == 8 ? 8 : 4));
    } else {
        pl.kind = RK_GENERIC;
        const size_t per = (size_t)d * sizeof(T);
        const size_t nx = two ? 2 : 1;
        const size_t lds_cap = 144 * 1024;   // of the CU's 160 KiB
        if ((nx + 4) * per <= lds_cap) {
            pl.nw = 4;
            pl.lds = (nx + 4) * per;
        } else if ((nx + 1) * per <= lds_cap) {
            pl.nw = 1;
            pl.lds = (nx + 1) * per;
        } else {
            // rows of any length: nothing staged in LDS, one partial per wave in the workspace (d = 16384 fp64 and beyond)
            pl.nw = 4;
            pl.lds = 0;
            pl.parts_per_block = 4;
        }
        pl.block = pl.nw * WAVE;
        const int64_t g1 = (a.nrows + pl.nw - 1) / pl.nw;
        const int64_t g4 = (a.nrows + 4 * pl.nw - 1) / (4 * pl.nw);
        pl.grid = g1 <= ctx->num_cu ? g1 : (g4 > ctx->num_cu ? g4 : ctx->num_cu);
        int64_t cap = ctx->sweep_blocks_per_cu > 0
                          ? (int64_t)ctx->num_cu * ctx->sweep_blocks_per_cu
                          : (table ? (rowb >= 2048 ? 512 : 1024)
                                   : (rowb >= 16384 ? 192 : (rowb >= 8192 ? 256 : (rowb >= 4096 ? 512 : (rowb >= 2048 ? 768 : 2048))))) *
                                (int64_t)ctx->num_cu / 256;
        if (pl.nw == 1) cap *= 4;
        if (pl.parts_per_block > 1) cap = std::min<int64_t>(cap, (int64_t)ctx->num_cu);   // grid x 4 partial d-vectors of >= 72 KiB each
        pl.grid = std::min(pl.grid, cap);
    }
    if (ctx->sweep_grid > 0 && pl.grid > ctx->sweep_grid) pl.grid = ctx->sweep_grid;
    if (pl.grid < 1) pl.grid = 1;
    return CIAO_OK;
}

int32_t dispatch_rows(ciao_ctx *ctx, int mode, const RowsPlan &pl, RowsArgs<CIAO_T> &a)
{
    using T = CIAO_T;
    const int grid = (int)pl.grid;
#define CIAO_MODE_SWITCH(CALL, WITH_AFINITO)                                                     \
    switch (mode) {                                                                              \
        case RM_GRAD: return CALL(RM_GRAD);                                                      \
        case RM_GRAD2: return CALL(RM_GRAD2);                                                    \
        case RM_SAGA_INIT: return CALL(RM_SAGA_INIT);                                            \
        case RM_FINITO_INIT: return CALL(RM_FINITO_INIT);                                        \
        case RM_FINITO_BATCH: return CALL(RM_FINITO_BATCH);                                      \
        case RM_AFINITO_INIT:                                                                    \
            if (WITH_AFINITO) return CALL##_AF();                                                \
            break;                                                                               \
    }
    switch (pl.kind) {
        case RK_CSPLIT:
#define CIAO_CALL_CSPLIT(MM) launch_csplit<T, MM>(ctx, pl.J, grid, a)
#define CIAO_CALL_CSPLIT_AF() CIAO_ERR_ARG
            CIAO_MODE_SWITCH(CIAO_CALL_CSPLIT, false)
#undef CIAO_CALL_CSPLIT
#undef CIAO_CALL_CSPLIT_AF
            break;
        case RK_CPLX:
#define CIAO_CALL_CPLX(MM) launch_cplx<T, MM>(ctx, grid, a)
#define CIAO_CALL_CPLX_AF() launch_cplx<T, RM_AFINITO_INIT>(ctx, grid, a)
            CIAO_MODE_SWITCH(CIAO_CALL_CPLX, true)
#undef CIAO_CALL_CPLX
#undef CIAO_CALL_CPLX_AF
            break;
        case RK_SMALL:
#define CIAO_SMALL_LAUNCH(MM)                                                                                                          \
    if (pl.small_i == 8 && a.ld == a.d)                                                                                               \
        hipLaunchKernelGGL((rows_small_kernel<T, MM, 8, false>), dim3((unsigned)grid), dim3(ROWS_BLOCK), pl.lds, ctx->stream, a);     \
    else if (pl.small_i == 8)                                                                                                         \
        hipLaunchKernelGGL((rows_small_kernel<T, MM, 8, true>), dim3((unsigned)grid), dim3(ROWS_BLOCK), pl.lds, ctx->stream, a);      \
    else if (a.ld == a.d)                                                                                                             \
        hipLaunchKernelGGL((rows_small_kernel<T, MM, 16, false>), dim3((unsigned)grid), dim3(ROWS_BLOCK), pl.lds, ctx->stream, a);    \
    else                                                                                                                              \
        hipLaunchKernelGGL((rows_small_kernel<T, MM, 16, true>), dim3((unsigned)grid), dim3(ROWS_BLOCK), pl.lds, ctx->stream, a);
            if (mode == RM_GRAD) {
                CIAO_SMALL_LAUNCH(RM_GRAD)
            } else if (mode == RM_SAGA_INIT) {
                CIAO_SMALL_LAUNCH(RM_SAGA_INIT)
            } else {
                CIAO_SMALL_LAUNCH(RM_FINITO_INIT)
            }
#undef CIAO_SMALL_LAUNCH
            return CIAO_OK;
        case RK_SMALLM:
            a.small_nb = pl.small_i;
            return launch_smallm<T>(ctx, mode, grid, pl.lds, a);
        case RK_WROW:
            return launch_wrow<T>(ctx, mode, pl.K, pl.J, grid, a);
        case RK_SMALLB:
#define CIAO_SMALLB_LAUNCH_G(MM, GG) \
    hipLaunchKernelGGL((rows_smallb_kernel<T, MM, 8, GG>), dim3((unsigned)grid), dim3(ROWS_BLOCK), pl.lds, ctx->stream, a);
#define CIAO_SMALLB_LAUNCH(MM)                                                                                                   \
    if (pl.scalar) {                                                                                                             \
        CIAO_SMALLB_LAUNCH_G(MM, true)                                                                                           \
    } else {                                                                                                                     \
        CIAO_SMALLB_LAUNCH_G(MM, false)                                                                                          \
    }
            if (mode == RM_GRAD2) {
                CIAO_SMALLB_LAUNCH(RM_GRAD2)
            } else {
                CIAO_SMALLB_LAUNCH(RM_FINITO_BATCH)
            }
#undef CIAO_SMALLB_LAUNCH
#undef CIAO_SMALLB_LAUNCH_G
            return CIAO_OK;
        case RK_LONG:
            return launch_long<T>(ctx, mode, pl.J, pl.long_S, pl.long_C, a);
        case RK_SPLIT:
#define CIAO_CALL_SPLIT(MM) launch_split<T, MM>(ctx, pl.J, pl.masked, pl.scalar, grid, a)
#define CIAO_CALL_SPLIT_AF() CIAO_ERR_ARG
            CIAO_MODE_SWITCH(CIAO_CALL_SPLIT, false)
#undef CIAO_CALL_SPLIT
#undef CIAO_CALL_SPLIT_AF
            break;
        case RK_WAVE_ROW:
#define CIAO_CALL_FAST(MM) launch_fast<T, MM>(ctx, pl.K, grid, a)
#define CIAO_CALL_FAST_AF() launch_fast<T, RM_AFINITO_INIT>(ctx, pl.K, grid, a)
            CIAO_MODE_SWITCH(CIAO_CALL_FAST, true)
#undef CIAO_CALL_FAST
#undef CIAO_CALL_FAST_AF
            break;
        case RK_GENERIC:
#define CIAO_CALL_GEN(MM) launch_generic<T, MM>(ctx, pl.nw, grid, pl.lds, a)
#define CIAO_CALL_GEN_AF() launch_generic<T, RM_AFINITO_INIT>(ctx, pl.nw, grid, pl.lds, a)
            CIAO_MODE_SWITCH(CIAO_CALL_GEN, true)
#undef CIAO_CALL_GEN
#undef CIAO_CALL_GEN_AF
            break;
    }
#undef CIAO_MODE_SWITCH
    set_error("internal: bad rows mode %d", mode);
    return CIAO_ERR_ARG;
}

std::string rows_kernel_name(const ciao_ctx *ctx, int mode, const RowsPlan &pl)
{
    using T = CIAO_T;
    const char *ty = sizeof(T) == 8 ? "f64" : "f32";
    const bool table = (mode == RM_SAGA_INIT || mode == RM_FINITO_INIT || mode == RM_FINITO_BATCH || mode == RM_AFINITO_INIT);
    char buf[160];
    switch (pl.kind) {
        case RK_CSPLIT:
            snprintf(buf, sizeof buf, "rows_csplit_kernel<%s,J%d,mode%d> (cplx) grid=%lld block=%d", ty, pl.J, mode, (long long)pl.grid, pl.block);
            break;
        case RK_CPLX:
            snprintf(buf, sizeof buf, "rows_cplx_kernel<%s,mode%d> grid=%lld block=%d", ty, mode, (long long)pl.grid, pl.block);
            break;
        case RK_SMALL:
            snprintf(buf, sizeof buf, "rows_small_kernel<%s,mode%d,I%d> grid=%lld block=%d", ty, mode, pl.small_i, (long long)pl.grid, pl.block);
            break;
        case RK_SMALLM:
            snprintf(buf, sizeof buf, "rows_smallm_kernel<%s,mode%d,ring%d> grid=%lld block=%d", ty, mode, pl.small_i, (long long)pl.grid, pl.block);
            break;
        case RK_WROW:
            snprintf(buf, sizeof buf, "rows_wrow_kernel<%s,%s,K%d,mode%d> grid=%lld block=%d", ty, pl.K == 1 ? "elements" : "chunks", pl.J, mode,
                     (long long)pl.grid, pl.block);
            break;
        case RK_SMALLB:
            snprintf(buf, sizeof buf, "rows_smallb_kernel<%s,mode%d,I%d,%s> grid=%lld block=%d", ty, mode, pl.small_i,
                     pl.scalar ? "gather" : "dense", (long long)pl.grid, pl.block);
            break;
        case RK_LONG:
            snprintf(buf, sizeof buf, "rows_long_kernel<%s,J%d,mode%d> segments=%d clusters=%d grid=%lld block=%d", ty, pl.J, mode, pl.long_S,
                     pl.long_C, (long long)pl.grid, pl.block);
            break;
        case RK_SPLIT:
            snprintf(buf, sizeof buf, "rows_split_kernel<%s,J%d,mode%d%s> grid=%lld block=%d", ty, pl.J, mode,
                     pl.scalar ? ",scalar" : (pl.masked ? ",masked" : ""), (long long)pl.grid, pl.block);
            break;
        case RK_WAVE_ROW: {
            const bool multi = ctx->sweep_multi && !table && (pl.K == 2 || pl.K == 4);
            snprintf(buf, sizeof buf, "%s<%s,K%d,mode%d> grid=%lld block=%d", multi ? "rows_multi_kernel" : "rows_fast_kernel", ty, pl.K, mode,
                     (long long)pl.grid, pl.block);
            break;
        }
        default:
            snprintf(buf, sizeof buf, "rows_generic_kernel<%s,NW%d,mode%d%s> grid=%lld block=%d", ty, pl.nw, mode,
                     pl.parts_per_block > 1 ? ",global_acc" : "", (long long)pl.grid, pl.block);
    }
    return buf;
}

// HIP events around the dominant kernel of an entry point, on the stream it runs on (bench.py roofline): records the start
// event now and hands back the stop event for the caller to record behind its launch
int32_t timing_begin(ciao_ctx *ctx, hipEvent_t *stop)
{
    *stop = nullptr;
    if (!ctx->timing) return CIAO_OK;
    if (ctx->ev_used + 2 > ctx->ev_pool.size()) {
        hipEvent_t e0, e1;
        CIAO_HIP(hipEventCreate(&e0));
        CIAO_HIP(hipEventCreate(&e1));
        ctx->ev_pool.push_back(e0);
        ctx->ev_pool.push_back(e1);
    }
    hipEvent_t ev0 = ctx->ev_pool[ctx->ev_used];
    *stop = ctx->ev_pool[ctx->ev_used + 1];
    ctx->ev_used += 2;
    CIAO_HIP(hipEventRecord(ev0, ctx->stream));
    return CIAO_OK;
}

// rows kernel -> finalize (-> all-reduce hook -> epilogue).  raw_only: stop after the (all-reduced) raw sum is in
// ctx->sumbuf[0..d) with the extra scalar at [d]; no epilogue.
int32_t launch_rows_impl(ciao_ctx *ctx, int mode, RowsArgs<CIAO_T> &a, const Epilogue<CIAO_T> &ep, bool raw_only)
{
    const int64_t d = a.d;
    RowsPlan pl;
    CIAO_TRY(plan_rows(ctx, mode, a, pl));
    const int64_t nparts = pl.kind == RK_LONG ? pl.long_C : pl.grid * pl.parts_per_block;
    CIAO_TRY(reduction_workspace(ctx, d, nparts, a));

    hipEvent_t ev1 = nullptr;
    CIAO_TRY(timing_begin(ctx, &ev1));
    CIAO_TRY(dispatch_rows(ctx, mode, pl, a));
    CIAO_HIP(hipGetLastError());
    if (ev1) CIAO_HIP(hipEventRecord(ev1, ctx->stream));
    ctx->last_kernel = rows_kernel_name(ctx, mode, pl);
    return finish_reduction(ctx, d, (int)nparts, a.pstride, ep, raw_only);
}
}  // namespace

template <>
int32_t launch_rows<CIAO_T>(ciao_ctx *ctx, int mode, RowsArgs<CIAO_T> &a, const Epilogue<CIAO_T> &ep)
{
    return launch_rows_impl(ctx, mode, a, ep, false);
}

// raw variant: leave the (all-reduced) sum and extra in ctx->sumbuf, no epilogue (used by ciao_objective)
template <>
int32_t launch_rows_raw<CIAO_T>(ciao_ctx *ctx, int mode, RowsArgs<CIAO_T> &a)
{
    Epilogue<CIAO_T> ep{};
    return launch_rows_impl(ctx, mode, a, ep, true);
}

// ---- ProShI: agent rows of a separable quadratic (proshi_kernels.h) --------------------------------------------------------
namespace {
enum ProshiKind { PK_DENSE, PK_VEC, PK_ROWS };

struct ProshiPlan {
    ProshiKind kind = PK_ROWS;
    int J = 0;             // VEC: 16-byte chunks per thread
    int nw = 0;            // ROWS: waves per block
    size_t lds = 0;        // DENSE / ROWS: dynamic LDS bytes
    int64_t grid = 1;      // workgroups, each leaving one partial d-vector
    int block = 256;
    bool timed = true;     // timing events around the launch
};

int32_t plan_proshi(const ciao_ctx *ctx, const ProshiArgs<CIAO_T> &a, ProshiPlan &pl)
{
    using T = CIAO_T;
    const int64_t d = a.d;
    constexpr int64_t PV = 16 / sizeof(T);
    int64_t cap;
    if (a.dense) {
        pl.kind = PK_DENSE;
        pl.lds = (size_t)d * sizeof(T);
        if (pl.lds > 64 * 1024) {
            set_error("ProShI with dense Quadratic terms covers d*%zu bytes <= 64 KiB (got d=%lld)", sizeof(T), (long long)d);
            return CIAO_ERR_UNSUPPORTED;
        }
        pl.grid = a.nrows;
        cap = (int64_t)ctx->num_cu * 4;
    } else if (!ctx->force_generic && d % PV == 0 && d / PV <= 8 * 256 && aligned16(a.Q) && aligned16(a.q) && aligned16(a.table) &&
               aligned16(a.x) && (a.ld * (int64_t)sizeof(T)) % 16 == 0) {
        // ---- vectorised path: 16-byte aligned rows of at most 32 KiB ----
        pl.kind = PK_VEC;
        const int64_t nch = d / PV;
        pl.J = nch <= 256 ? 1 : (nch <= 512 ? 2 : (nch <= 1024 ? 4 : 8));
        // one agent row per workgroup; from eight agents per CU on, two workgroups per CU (each with the next agent's rows in flight:
        // r = 4096 at d = 1024 fp64 41.7 -> 35.8 us, r = 8192 78 -> 62; below that the second set of partials costs more than it hides)
        pl.grid = a.nrows;
        // (rows of up to 2 KiB, batches of 4096 agents and more: four -- d = 256 fp64 r = 16 384 / 65 536 57.0 -> 44.2 / 188 -> 128 us; at 4 KiB and
        // beyond two stay best: profiles/r05_midrow_batches.txt)
        const int64_t auto_bpc = (d * (int64_t)sizeof(T) <= 2048 && a.nrows >= 4096) ? 4 : (a.nrows >= 8 * (int64_t)ctx->num_cu ? 2 : 1);
        cap = (int64_t)ctx->num_cu * (ctx->split_blocks_per_cu > 0 ? ctx->split_blocks_per_cu : auto_bpc);
    } else {
        pl.kind = PK_ROWS;
        pl.timed = false;   // inherited behaviour: the generic kernel has never recorded timing events
        const size_t per = (size_t)d * sizeof(T), lds_cap = 144 * 1024;
        pl.nw = 4;
        if (5 * per > lds_cap) pl.nw = 1;
        pl.lds = (size_t)(1 + pl.nw) * per;
        if (pl.lds > lds_cap) {
            set_error("ProShI covers 2*d*%zu bytes <= 144 KiB of LDS (got d=%lld)", sizeof(T), (long long)d);
            return CIAO_ERR_UNSUPPORTED;
        }
        pl.block = pl.nw * WAVE;
        pl.grid = (a.nrows + pl.nw - 1) / pl.nw;
        cap = (int64_t)ctx->num_cu * (pl.nw == 4 ? 2 : 8);
    }
    if (pl.grid > cap) pl.grid = cap;
    if (pl.grid < 1) pl.grid = 1;
    return CIAO_OK;
}

template <bool INIT>
int32_t dispatch_proshi_phase(ciao_ctx *ctx, const ProshiPlan &pl, ProshiArgs<CIAO_T> &a)
{
    using T = CIAO_T;
    const dim3 grid((unsigned)pl.grid), block(pl.block);
    switch (pl.kind) {
        case PK_DENSE: hipLaunchKernelGGL((proshi_dense_kernel<T, INIT>), grid, block, pl.lds, ctx->stream, a); return CIAO_OK;
        case PK_VEC:
            switch (pl.J) {
                case 1: hipLaunchKernelGGL((proshi_vec_kernel<T, INIT, 1>), grid, block, 0, ctx->stream, a); return CIAO_OK;
                case 2: hipLaunchKernelGGL((proshi_vec_kernel<T, INIT, 2>), grid, block, 0, ctx->stream, a); return CIAO_OK;
                case 4: hipLaunchKernelGGL((proshi_vec_kernel<T, INIT, 4>), grid, block, 0, ctx->stream, a); return CIAO_OK;
                case 8: hipLaunchKernelGGL((proshi_vec_kernel<T, INIT, 8>), grid, block, 0, ctx->stream, a); return CIAO_OK;
            }
            set_error("internal: bad J %d", pl.J);
            return CIAO_ERR_UNSUPPORTED;
        default:
            return pl.nw == 4 ? launch_with_lds(ctx, &proshi_rows_kernel<T, INIT, 4>, pl.grid, pl.block, pl.lds, a)
                              : launch_with_lds(ctx, &proshi_rows_kernel<T, INIT, 1>, pl.grid, pl.block, pl.lds, a);
    }
}

int32_t dispatch_proshi(ciao_ctx *ctx, bool init, const ProshiPlan &pl, ProshiArgs<CIAO_T> &a)
{
    return init ? dispatch_proshi_phase<true>(ctx, pl, a) : dispatch_proshi_phase<false>(ctx, pl, a);
}

std::string proshi_kernel_name(bool init, const ProshiPlan &pl)
{
    const char *ty = sizeof(CIAO_T) == 8 ? "f64" : "f32", *phase = init ? "init" : "step";
    const long long grid = (long long)pl.grid;
    char buf[128];
    switch (pl.kind) {
        case PK_DENSE: snprintf(buf, sizeof buf, "proshi_dense_kernel<%s,%s> grid=%lld block=%d", ty, phase, grid, pl.block); break;
        case PK_VEC: snprintf(buf, sizeof buf, "proshi_vec_kernel<%s,%s,J%d> grid=%lld block=%d", ty, phase, pl.J, grid, pl.block); break;
        default: snprintf(buf, sizeof buf, "proshi_rows_kernel<%s,%s,NW%d> grid=%lld block=%d", ty, phase, pl.nw, grid, pl.block);
    }
    return buf;
}
}  // namespace

// plan -> workspace -> kernel -> finalize + epilogue, as launch_rows_impl
template <>
int32_t launch_proshi<CIAO_T>(ciao_ctx *ctx, bool init, ProshiArgs<CIAO_T> &a, const Epilogue<CIAO_T> &ep)
{
    ProshiPlan pl;
    CIAO_TRY(plan_proshi(ctx, a, pl));
    CIAO_TRY(reduction_workspace(ctx, a.d, pl.grid, a));

    hipEvent_t ev1 = nullptr;
    if (pl.timed) CIAO_TRY(timing_begin(ctx, &ev1));
    CIAO_TRY(dispatch_proshi(ctx, init, pl, a));
    CIAO_HIP(hipGetLastError());
    if (ev1) CIAO_HIP(hipEventRecord(ev1, ctx->stream));
    ctx->last_kernel = proshi_kernel_name(init, pl);
    return finish_reduction(ctx, a.d, (int)pl.grid, a.pstride, ep, false);
}

// a run of small batches, one thread per coordinate: no partials, no finalize, no timing events
template <>
int32_t launch_proshi_chain<CIAO_T>(ciao_ctx *ctx, ProshiChainArgs<CIAO_T> &c)
{
    using T = CIAO_T;
    c.errflag = ctx->errflag;
    const int64_t grid = (c.d + 255) / 256;
    CIAO_TRY(launch_with_lds(ctx, &proshi_chain_kernel<T>, grid, 256, proshi_chain_lds_bytes<T>(), c));
    CIAO_HIP(hipGetLastError());
    char nm[128];
    snprintf(nm, sizeof nm, "proshi_chain_kernel<%s> grid=%lld block=256 visits=%lld batch=%lld", sizeof(T) == 8 ? "f64" : "f32",
             (long long)grid, (long long)c.nvisits, (long long)c.batch);
    ctx->last_kernel = nm;
    return CIAO_OK;
}

}  // namespace ciao

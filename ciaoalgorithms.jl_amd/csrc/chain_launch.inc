// chain_launch.inc -- host dispatch of the chain kernels for one real type (CIAO_T).
//
// launch_chain is one pipeline, as launch_rows and launch_proshi are (rows_launch.inc): plan_chain decides everything and touches
// nothing, dispatch_chain launches what the plan says, chain_kernel_name prints the plan.  launch_afinito keeps its own structure.

#include <initializer_list>
#include <string>

#include "ciao_ctx.h"
#include "launch.h"
#include "chain_kernels.h"
#include "chain_ws_kernels.h"
#include "chain_wide_kernels.h"

namespace ciao {

// launch_dma<T, ALG, LOSS> (the LDS-DMA fast chain) is defined in chain_dma_launch.inc and instantiated in its own translation
// units (chain_dma{0..4}_f32/f64.hip: one per algorithm), launch_ws in chain_ws_launch.inc, so that the build spreads over the cores.
#define CIAO_DMA_EXTERN(AA)                                                                                             \
    extern template int32_t launch_dma<CIAO_T, AA, CIAO_LOSS_LS>(ciao_ctx *, int, int, bool, ChainArgs<CIAO_T> &);      \
    extern template int32_t launch_dma<CIAO_T, AA, CIAO_LOSS_LOGISTIC>(ciao_ctx *, int, int, bool, ChainArgs<CIAO_T> &);
CIAO_DMA_EXTERN(CA_SVRG)
CIAO_DMA_EXTERN(CA_SVRGC)
CIAO_DMA_EXTERN(CA_SAGA)
CIAO_DMA_EXTERN(CA_FINITO)
CIAO_DMA_EXTERN(CA_LFINITO)
#undef CIAO_DMA_EXTERN
extern template int32_t launch_ws<CIAO_T, CA_SAGA, CIAO_LOSS_LS>(ciao_ctx *, int, bool, ChainArgs<CIAO_T> &);
extern template int32_t launch_ws<CIAO_T, CA_SAGA, CIAO_LOSS_LOGISTIC>(ciao_ctx *, int, bool, ChainArgs<CIAO_T> &);

namespace {
inline bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

constexpr int64_t RING_MAX_BYTES = 8 * CHAIN_NT * 16;   // 32 KiB rows: the longest the LDS-DMA ring takes (complex rows: half of it)

// "These rows can take the LDS-DMA ring": whole 16-byte chunks, at most max_bytes; the row stride and every pointer of `ptrs` 16-byte
// aligned (a null pointer passes; ld = 0: no data rows to step over)
template <typename T>
bool ring_eligible(int64_t d, int64_t ld, int64_t max_bytes, std::initializer_list<const void *> ptrs)
{
    const int64_t rowb = d * (int64_t)sizeof(T);
    if (rowb % 16 != 0 || rowb > max_bytes || (ld * (int64_t)sizeof(T)) % 16 != 0) return false;
    for (const void *p : ptrs)
        if (!al16(p)) return false;
    return true;
}

// ... asked of a chain's arguments: the state vectors always, the data rows unless the loss is Zero() (those rows alias av), the table
// where the algorithm keeps one; over a shard table every non-empty shard's bases (local or peer-mapped) in place of A and table
template <typename T>
bool chain_ring_eligible(const ChainArgs<T> &a, int64_t max_bytes, bool need_table)
{
    if (!ring_eligible<T>(a.d, 0, max_bytes, {a.av, a.z, a.zf, a.w})) return false;
    auto bases = [&](const void *A, const void *table) {
        return (a.loss == CIAO_LOSS_ZERO || ring_eligible<T>(a.d, a.ld, max_bytes, {A})) && (!need_table || al16(table));
    };
    if (a.nshards == 0) return bases(a.A, a.table);
    for (int k = 0; k < a.nshards; ++k)
        if (a.sh_row0[k + 1] != a.sh_row0[k] && !bases(a.shA[k], a.shT[k])) return false;
    return true;
}

// the row's 4 KiB class: J = row bytes / 4096 rounded up to a power of two; masked: the row ends short of J * 4096 bytes
inline int ring_row_class(int64_t rowb, bool *masked)
{
    int j = 1;
    while ((int64_t)j * CHAIN_NT * 16 < rowb) j *= 2;
    *masked = ((int64_t)j * CHAIN_NT * 16 != rowb);
    return j;
}

enum ChainKind {
    CK_REG,    // chain_kernel: the register ring, rows with no 16-byte structure
    CK_DMA,    // chain_dma_kernel: the LDS-DMA ring
    CK_WS,     // chain_ws_kernel: the wave-specialised ring (SAGA / SAG)
    CK_WIDE,   // chain_wide_kernel: several workgroups
    CK_BIG,    // chain_big_kernel: any length, the state in the caller's vectors
    CK_CDMA,   // chain_cdma_kernel: complex rows on the LDS-DMA ring
    CK_CREG,   // chain_cplx_reg_kernel
    CK_CBIG    // chain_cplx_kernel
};

struct ChainPlan {
    ChainKind kind = CK_REG;
    int alg = 0;                // the algorithm the kernel is instantiated for ...
    int name_alg = 0;           // ... and the number the name prints (cached-dots SVRG on the register ring: 4 over the algorithm-0 kernel)
    int loss = CIAO_LOSS_LS;    // the real kernels' loss: Zero() is least squares ...
    bool zero = false;          // ... with lam = 0 on rows that alias av
    bool drop_gam = false;      // cached-dots SVRG on a kernel that recomputes a_i'z_full itself: the cache is not passed
    int E = 0;                  // REG: elements per thread
    bool full = false;          //      d is exactly E x block
    bool one_wave = false;      //      rows of up to 64 elements
    int name_J = 0;             // DMA / WS / CDMA: the J the name prints, the row's 4 KiB class
    int J = 0;                  //   ... and the kernel's own class (J, block, MASKED): 16-byte chunks per thread
    bool masked = false;
    int issuers = 0;            // WS: issuer waves
    int G = 0;                  // WIDE: workgroups
    int EP = 0;                 // CREG: complex entries per thread
    int grid = 1, block = CHAIN_NT;
};

template <typename T>
int32_t plan_chain(const ciao_ctx *ctx, int alg, const ChainArgs<T> &a, ChainPlan &pl)
{
    const int64_t rowb = a.d * (int64_t)sizeof(T);
    const bool cplx = (a.loss == CIAO_LOSS_LS_COMPLEX);
    const bool svrg = (alg == CA_SVRG || alg == CA_SVRGC), tab = (alg == CA_SAGA || alg == CA_FINITO);
    const bool known = svrg || tab || alg == CA_LFINITO;
    const bool ring_on = !ctx->chain_no_dma && !ctx->chain_big;
    const bool ring = !cplx && ring_on && chain_ring_eligible(a, RING_MAX_BYTES, tab);
    // only chain_dma_kernel (the LDS-DMA ring, one or four or eight waves) takes a batch: its launch site records
    if (ctx->batch_open && !(ring && (svrg || tab) && a.nshards == 0)) {
        set_error("a chain batch takes SVRG inner cycles, SAGA / SAG steps and small-batch Finito steps on real rows of whole 16-byte chunks, 16-byte aligned, "
                  "of at most 32 KiB, unsharded (got alg %d, d=%lld, %d-byte scalars)", alg, (long long)a.d, (int)sizeof(T));
        return CIAO_ERR_UNSUPPORTED;
    }
    if (cplx && a.nshards > 0) {
        set_error("complex problems cannot run over a shard table");
        return CIAO_ERR_UNSUPPORTED;
    }
    // d > 8192, and in fp64 already > 4096: beyond one workgroup's registers (the 32-elements-per-thread register ring spills in fp64:
    // 7.7-8.7 us per update measured at d = 5000 ... 8192, against 2.9 on three or four workgroups) and beyond the ring's 32 KiB
    const bool beyond = a.d > (sizeof(T) == 8 ? 4096 : 8192);
    const bool wide = !cplx && beyond && !ctx->chain_big && !ctx->chain_no_wide && a.nshards == 0 && a.d <= (int64_t)WIDE_NT * 8 * WIDE_GMAX &&
                      a.nsteps < 0xFFFFFFFFll && (a.loss == CIAO_LOSS_LS || a.loss == CIAO_LOSS_LOGISTIC || a.loss == CIAO_LOSS_ZERO);
    if (!known) {
        set_error("internal: bad chain alg %d", alg);
        return CIAO_ERR_ARG;
    }
    pl.alg = pl.name_alg = alg;
    pl.loss = (a.loss == CIAO_LOSS_LOGISTIC) ? CIAO_LOSS_LOGISTIC : CIAO_LOSS_LS;
    pl.zero = (a.loss == CIAO_LOSS_ZERO);
    if (cplx) {   // complex T: (re, im) pairs; no cached-dots instantiation
        pl.alg = pl.name_alg = svrg ? CA_SVRG : alg;
        // rows of whole 16-byte chunks up to 16 KiB, everything 16-byte aligned: the LDS-DMA ring of the real chains
        if (ring_on && chain_ring_eligible(a, RING_MAX_BYTES / 2, tab)) {
            pl.kind = CK_CDMA;
            pl.J = pl.name_J = ring_row_class(rowb, &pl.masked);
            return CIAO_OK;
        }
        const int64_t pairs = (a.d / 2 + CHAIN_NT - 1) / CHAIN_NT;   // complex entries per thread at 256 threads
        pl.EP = pairs <= 1 ? 1 : (pairs <= 2 ? 2 : (pairs <= 4 ? 4 : (pairs <= 8 ? 8 : 0)));
        if (pl.EP > 0 && !ctx->chain_big) {   // up to 2048 complex entries: state in registers, the next row in flight
            pl.kind = CK_CREG;
        } else {
            pl.kind = CK_CBIG;
            pl.block = CHAIN_BIG_NT;
        }
        return CIAO_OK;
    }
    if (wide) {   // SVRG / SAGA / Finito: the chain shared by G workgroups, each with its columns of the state in registers (chain_wide_kernels.h)
        pl.kind = CK_WIDE;
        pl.alg = pl.name_alg = svrg ? CA_SVRG : alg;
        pl.E = 8;   // columns per thread: 2048 per workgroup, up to 64 workgroups (131 072 elements)
        pl.G = pl.grid = (int)((a.d + (int64_t)WIDE_NT * pl.E - 1) / ((int64_t)WIDE_NT * pl.E));
        pl.block = WIDE_NT;
        return CIAO_OK;
    }
    if (beyond || ctx->chain_big) {   // (or forced, for tests): no per-thread register state
        if (a.nshards > 0) {
            set_error("a chain over a shard table needs rows of at most 32 KiB (got d=%lld)", (long long)a.d);
            return CIAO_ERR_UNSUPPORTED;
        }
        pl.kind = CK_BIG;
        pl.alg = pl.name_alg = svrg ? CA_SVRG : alg;
        pl.drop_gam = (alg == CA_SVRGC);
        pl.block = CHAIN_BIG_NT;
        return CIAO_OK;
    }
    if (ring) {
        bool masked;   // relative to the row's 4 KiB class
        pl.name_J = ring_row_class(rowb, &masked);
        // Short rows (up to 2 KiB: d <= 256 fp64 / 512 fp32, the shapes of most tabular problems) run on ONE wave: a lane
        // owns one or two 16-byte chunks as it does with four waves, but the reduced dot product reaches every lane through
        // an SGPR and the LDS exchange -- write, lgkmcnt(0), barrier, read: a third of a four-wave step -- does not exist.
        // Never over a shard table (a problem that needs several GPUs does not have 2 KiB rows, and the variants cost build time).
        // (fp64 rows of 2-4 KiB ran on one wave with four chunks per lane until round 5 -- 10 % faster than four waves in round 3,
        // 0.277 against 0.306 us; the four-wave step has shed more since: d = 512 fp64 SVRG 0.285 on four waves against 0.292 on
        // one, d = 384 0.291 against 0.314, Finito r = 1 0.39 against 0.45 -- and the one-wave variant parked 84-92 VGPRs in AGPRs)
        const bool one_wave = !ctx->chain_four_waves && a.nshards == 0 && rowb <= 2048;
        // SAGA / SAG on rows of more than 2 KiB up to 4 KiB (or shorter, over a shard table or with option chain_four_waves): the
        // wave-specialised chain, 0.36 against 0.41 us per update at BASELINE config #3; only the stager wave ever sees a shard
        // table.  The SVRG chains stay on chain_dma_kernel: their steps have no table traffic to take off the consumers, and the
        // barrier-free exchange costs them more than the DMA issue it saves (profiles/r03_chain_ws_ab.txt).  fp64 rows of 2-4 KiB:
        // d = 512 0.411 against 0.476 us per update (profiles/r05_stage_ptr_ab.txt).
        // A chain batch runs them on chain_dma_kernel, bitwise the same results: a batch is bound by the memory system, not by one
        // chain's latency, and the kernel-argument copy a batch needs costs this kernel 2 % of a step.
        // Rows of 8 KiB stay on chain_dma_kernel: seven waves leave a consumer 256 registers; the fp64 consumer of 8 KiB rows
        // needs more (1.84 us per update against 0.52), and the fp32 one fits but is slower than four do-everything waves (0.516
        // against 0.482 us; profiles/r04_saga_f64_and_sharded.txt); those instantiations are not built.
        if (alg == CA_SAGA && !ctx->chain_no_ws && !ctx->batch_open && pl.name_J == 1 && !one_wave && a.nsteps < ((int64_t)1 << 30)) {
            pl.kind = CK_WS;
            pl.J = 1;
            pl.masked = masked;
            // one issuer wave per 4 KiB of row per step at most (option chain_ws_issuers overrides: 1 or 2)
            pl.issuers = ctx->chain_ws_issuers > 0 ? (int)ctx->chain_ws_issuers : 2;
            pl.block = (WS_NCW + 1 + pl.issuers) * WAVE;
            return CIAO_OK;
        }
        pl.kind = CK_DMA;
        if (one_wave) {   // one chunk per lane up to 1 KiB, two up to 2 KiB; exact at their own sizes
            pl.J = rowb <= 1024 ? 1 : 2;
            pl.block = WAVE;
            pl.masked = (rowb != pl.J * 1024);
        } else {
            // Four waves up to 16 KiB rows, eight waves for 32 KiB rows.  Measured (SVRG, fp64, us per update): 16 KiB rows 0.62 on four
            // waves vs 0.68 on eight (the exchange among eight waves costs more than halving the per-thread work saves); 32 KiB rows
            // 0.94 vs 0.86 in round 2, 0.755 vs 0.570 (cached row dots) in round 4 (profiles/r04_chain_32k_ab.txt).
            pl.J = pl.name_J == 8 ? 4 : pl.name_J;
            pl.block = pl.name_J == 8 ? 2 * CHAIN_NT : CHAIN_NT;
            pl.masked = masked;
        }
        return CIAO_OK;
    }
    if (a.nshards > 0) {
        set_error("a chain over a shard table needs rows of whole 16-byte chunks, 16-byte aligned, of at most 32 KiB "
                  "(the LDS-DMA kernel; got d=%lld)", (long long)a.d);
        return CIAO_ERR_UNSUPPORTED;
    }
    pl.kind = CK_REG;
    if (alg == CA_SVRGC) {   // the register ring recomputes a_i'z_full itself (and holds no CA_SVRGC instantiation); the name keeps the 4
        pl.alg = CA_SVRG;
        pl.drop_gam = true;
    }
    // rows of up to 64 elements: ONE wave, one element per lane, no exchange.  Measured per SVRG update, one wave vs four: d=50 0.299
    // vs 0.345 us (fp64), 0.241 vs 0.288 (fp32); with 4 or 8 elements per lane this kernel's per-element work outweighs the exchange
    // (d=129 0.42 vs 0.38, d=511 0.75 vs 0.54), so those stay on four waves.
    pl.one_wave = !ctx->chain_four_waves && a.d <= WAVE;
    pl.block = pl.one_wave ? WAVE : CHAIN_NT;
    const int64_t per = (a.d + CHAIN_NT - 1) / CHAIN_NT;
    // (32: 4096 < d <= 8192 in fp32; the state spills a little (16-72 B), the chain stays available.  fp64 at 32 elements per thread is
    // NOT built -- 1-1.4 KB of scratch per lane: such rows are `beyond`)
    pl.E = pl.one_wave || per <= 1 ? 1 : (per <= 4 ? 4 : (per <= 8 ? 8 : (per <= 16 ? 16 : 32)));
    pl.full = (a.d == (int64_t)pl.E * pl.block);
    return CIAO_OK;
}

template <typename T, int ALG, int LOSS>
int32_t launch_chain_e(ciao_ctx *ctx, const ChainPlan &pl, ChainArgs<T> &a)
{
#define CIAO_CHAIN_CASE(EE, NT)                                                                                  \
    if (pl.full)                                                                                                 \
        hipLaunchKernelGGL((chain_kernel<T, EE, ALG, LOSS, true, NT>), dim3(1), dim3(NT), 0, ctx->stream, a);    \
    else                                                                                                         \
        hipLaunchKernelGGL((chain_kernel<T, EE, ALG, LOSS, false, NT>), dim3(1), dim3(NT), 0, ctx->stream, a);   \
    return CIAO_OK;
    if (pl.one_wave) {
        CIAO_CHAIN_CASE(1, WAVE)
    }
    switch (pl.E) {
        case 1: CIAO_CHAIN_CASE(1, CHAIN_NT)
        case 4: CIAO_CHAIN_CASE(4, CHAIN_NT)
        case 8: CIAO_CHAIN_CASE(8, CHAIN_NT)
        case 16: CIAO_CHAIN_CASE(16, CHAIN_NT)
        case 32:
            if constexpr (sizeof(T) == 4) {
                CIAO_CHAIN_CASE(32, CHAIN_NT)
            }
    }
#undef CIAO_CHAIN_CASE
    set_error("internal: bad E %d", pl.E);
    return CIAO_ERR_UNSUPPORTED;
}

// the real kernels of one (algorithm, loss)
template <typename T, int ALG, int LOSS>
int32_t dispatch_chain_real(ciao_ctx *ctx, const ChainPlan &pl, ChainArgs<T> &a, const WideArgs &wa)
{
    if (pl.kind == CK_DMA) return launch_dma<T, ALG, LOSS>(ctx, pl.J, pl.block, pl.masked, a);
    if constexpr (ALG == CA_SAGA) {
        if (pl.kind == CK_WS) return launch_ws<T, ALG, LOSS>(ctx, pl.issuers, pl.masked, a);
    }
    if constexpr (ALG != CA_SVRGC) {   // (cached-dots SVRG is the ring's alone)
        switch (pl.kind) {
            case CK_REG: return launch_chain_e<T, ALG, LOSS>(ctx, pl, a);
            case CK_WIDE: hipLaunchKernelGGL((chain_wide_kernel<T, 8, ALG, LOSS>), dim3((unsigned)pl.G), dim3(WIDE_NT), 0, ctx->stream, a, wa); return CIAO_OK;
            case CK_BIG: hipLaunchKernelGGL((chain_big_kernel<T, ALG, LOSS>), dim3(1), dim3(CHAIN_BIG_NT), 0, ctx->stream, a); return CIAO_OK;
            default: break;
        }
    }
    set_error("internal: chain kind %d for algorithm %d", (int)pl.kind, ALG);
    return CIAO_ERR_UNSUPPORTED;
}

template <typename T, int ALG>
int32_t dispatch_chain_cplx(ciao_ctx *ctx, const ChainPlan &pl, ChainArgs<T> &a)
{
    if (pl.kind == CK_CBIG) {
        hipLaunchKernelGGL((chain_cplx_kernel<T, ALG>), dim3(1), dim3(CHAIN_BIG_NT), 0, ctx->stream, a);
        return CIAO_OK;
    }
    switch (pl.EP) {
        case 1: hipLaunchKernelGGL((chain_cplx_reg_kernel<T, ALG, 1>), dim3(1), dim3(CHAIN_NT), 0, ctx->stream, a); break;
        case 2: hipLaunchKernelGGL((chain_cplx_reg_kernel<T, ALG, 2>), dim3(1), dim3(CHAIN_NT), 0, ctx->stream, a); break;
        case 4: hipLaunchKernelGGL((chain_cplx_reg_kernel<T, ALG, 4>), dim3(1), dim3(CHAIN_NT), 0, ctx->stream, a); break;
        default: hipLaunchKernelGGL((chain_cplx_reg_kernel<T, ALG, 8>), dim3(1), dim3(CHAIN_NT), 0, ctx->stream, a); break;
    }
    return CIAO_OK;
}

// Zero(): the least-squares form with lam = 0 gives exactly 0 for any finite "data"; every row (every shard's too) aliases the
// (finite) av vector with stride 0, which keeps the row prefetch branch-free
template <typename T>
void alias_zero_loss(ChainArgs<T> &a)
{
    a.lam = T(0);
    a.A = a.av;
    a.ld = 0;
    a.b = nullptr;
    for (int k = 0; k < a.nshards; ++k) {
        a.shA[k] = a.av;
        a.shb[k] = nullptr;
    }
}

template <typename T>
int32_t dispatch_chain(ciao_ctx *ctx, const ChainPlan &pl, ChainArgs<T> &a)
{
    if (pl.kind == CK_CDMA) return launch_cdma<T>(ctx, pl.alg, pl.J, pl.masked, a);
    if (pl.kind == CK_CREG || pl.kind == CK_CBIG) {
        switch (pl.alg) {
            case CA_SVRG: return dispatch_chain_cplx<T, CA_SVRG>(ctx, pl, a);
            case CA_SAGA: return dispatch_chain_cplx<T, CA_SAGA>(ctx, pl, a);
            case CA_FINITO: return dispatch_chain_cplx<T, CA_FINITO>(ctx, pl, a);
            default: return dispatch_chain_cplx<T, CA_LFINITO>(ctx, pl, a);
        }
    }
    WideArgs wa{};
    if (pl.kind == CK_WIDE) {   // the workgroups' mailbox
        wa.slice = (int64_t)WIDE_NT * pl.E;
        wa.G = pl.G;
        const size_t bytes = (size_t)2 * WIDE_GMAX * 4 * sizeof(unsigned long long);
        CIAO_TRY(ensure(ctx, &ctx->wide_box, &ctx->wide_box_bytes, bytes));
        CIAO_HIP(hipMemsetAsync(ctx->wide_box, 0, bytes, ctx->stream));   // step numbers start at 1: a cleared word matches none
        wa.box = (unsigned long long *)ctx->wide_box;
    }
    if (pl.zero) {
        alias_zero_loss(a);
        if (pl.kind == CK_WIDE) a.loss = CIAO_LOSS_LS;
    }
    if (pl.drop_gam) a.gam = nullptr;
#define CIAO_CHAIN_ALG(AA)                                                                               \
    case AA:                                                                                             \
        return pl.loss == CIAO_LOSS_LOGISTIC ? dispatch_chain_real<T, AA, CIAO_LOSS_LOGISTIC>(ctx, pl, a, wa) \
                                             : dispatch_chain_real<T, AA, CIAO_LOSS_LS>(ctx, pl, a, wa);
    switch (pl.alg) {
        CIAO_CHAIN_ALG(CA_SVRG)
        CIAO_CHAIN_ALG(CA_SVRGC)
        CIAO_CHAIN_ALG(CA_SAGA)
        CIAO_CHAIN_ALG(CA_FINITO)
        default: CIAO_CHAIN_ALG(CA_LFINITO)
    }
#undef CIAO_CHAIN_ALG
}

template <typename T>
std::string chain_kernel_name(const ChainPlan &pl, const ChainArgs<T> &a)
{
    auto n = [](const char *tag, int v) { return tag + std::to_string(v); };
    const std::string ty = sizeof(T) == 8 ? "<f64" : "<f32", alg = n(",alg", pl.name_alg);
    const std::string ring = n(",J", pl.name_J) + alg + (pl.masked ? ",masked" : "") + (a.nshards > 0 ? ",sharded" : "");
    std::string k;
    switch (pl.kind) {
        case CK_REG: k = "chain_kernel" + ty + n(",E", pl.E) + alg + (pl.full ? ",full" : ",masked"); break;
        case CK_DMA: k = "chain_dma_kernel" + ty + ring; break;
        case CK_WS: k = "chain_ws_kernel" + ty + ring + n(",issuers", pl.issuers); break;
        case CK_WIDE: k = "chain_wide_kernel" + ty + n(",E", pl.E) + alg; break;
        case CK_BIG: k = "chain_big_kernel" + ty + alg; break;
        case CK_CDMA: k = "chain_cdma_kernel" + ty + ring; break;
        case CK_CREG: k = "chain_cplx_reg_kernel" + ty + alg + n(",EP", pl.EP); break;
        default: k = "chain_cplx_kernel" + ty + alg; break;
    }
    char buf[160];
    snprintf(buf, sizeof buf, "%s> grid=%d block=%d steps=%lld", k.c_str(), pl.grid, pl.block, (long long)a.nsteps);
    return buf;
}
}  // namespace

// plan -> launch -> name, as launch_rows_impl; inside an open chain batch the launch is a record, and the name is the record's
template <>
int32_t launch_chain<CIAO_T>(ciao_ctx *ctx, int alg, ChainArgs<CIAO_T> &a)
{
    if (a.nsteps <= 0) return CIAO_OK;
    a.errflag = ctx->errflag;
    ChainPlan pl;
    CIAO_TRY(plan_chain(ctx, alg, a, pl));
    CIAO_TRY(dispatch_chain(ctx, pl, a));
    CIAO_HIP(hipGetLastError());
    const std::string name = chain_kernel_name(pl, a);
    if (ctx->batch_open && !ctx->batch.empty())
        ctx->batch.back().name = name;
    else
        ctx->last_kernel = name;
    return CIAO_OK;
}

namespace {
template <typename T, int LOSS, int J, bool MASKED, int NT, bool SHARDED = false>
int32_t launch_afinito_dma_jm(ciao_ctx *ctx, AFinitoArgs<T> &a)
{
    constexpr size_t lds = afinito_dma_lds_bytes<T, J, NT, SHARDED>();
    static_assert(lds <= 160 * 1024, "LDS budget");
    auto kern = &afinito_dma_kernel<T, J, LOSS, MASKED, NT, SHARDED>;
    if (lds > 60 * 1024)
        CIAO_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(1), dim3(NT), lds, ctx->stream, a);
    return CIAO_OK;
}

template <typename T, int LOSS, int J, int NT = CHAIN_NT>
int32_t launch_afinito_dma_j(ciao_ctx *ctx, bool masked, AFinitoArgs<T> &a)
{
    if constexpr (NT == CHAIN_NT) {   // a chain over a shard table: four waves whatever the row length
        if (a.nshards > 0)
            return masked ? launch_afinito_dma_jm<T, LOSS, J, true, NT, true>(ctx, a) : launch_afinito_dma_jm<T, LOSS, J, false, NT, true>(ctx, a);
    }
    return masked ? launch_afinito_dma_jm<T, LOSS, J, true, NT>(ctx, a) : launch_afinito_dma_jm<T, LOSS, J, false, NT>(ctx, a);
}

// J = row bytes / 4096 rounded up to a power of two (four waves); rows of up to 2 KiB run on ONE wave (J = 1 / 2 chunks per lane)
template <typename T, int LOSS>
int32_t launch_afinito_dma(ciao_ctx *ctx, int J, bool masked, AFinitoArgs<T> &a, int *block)
{
    const int64_t rowb = a.d * (int64_t)sizeof(T);
    *block = CHAIN_NT;
    if (J == 1 && !ctx->chain_four_waves && rowb <= 2048 && a.nshards == 0) {
        *block = WAVE;
        if (rowb <= 1024) return launch_afinito_dma_j<T, LOSS, 1, WAVE>(ctx, rowb != 1024, a);
        return launch_afinito_dma_j<T, LOSS, 2, WAVE>(ctx, rowb != 2048, a);
    }
    switch (J) {
        case 1: return launch_afinito_dma_j<T, LOSS, 1>(ctx, masked, a);
        case 2: return launch_afinito_dma_j<T, LOSS, 2>(ctx, masked, a);
        case 4: return launch_afinito_dma_j<T, LOSS, 4>(ctx, masked, a);
        case 8: return launch_afinito_dma_j<T, LOSS, 8>(ctx, masked, a);
        default: set_error("internal: bad J %d", J); return CIAO_ERR_UNSUPPORTED;
    }
}

// adaptive Finito on rows beyond one workgroup's registers (more than 32 KiB): the several-workgroup chain (chain_wide_kernels.h)
template <typename T>
int32_t launch_afinito_wide(ciao_ctx *ctx, int loss, AFinitoArgs<T> &a)
{
    constexpr int E = 8;
    WideArgs wa{};
    wa.slice = (int64_t)WIDE_NT * E;
    wa.G = (int)((a.d + wa.slice - 1) / wa.slice);
    const size_t bytes = (size_t)2 * WIDE_GMAX * AFW_WORDS * sizeof(unsigned long long);
    CIAO_TRY(ensure(ctx, &ctx->wide_box, &ctx->wide_box_bytes, bytes));
    CIAO_HIP(hipMemsetAsync(ctx->wide_box, 0, bytes, ctx->stream));   // exchange numbers start at 1: a cleared word matches none
    wa.box = (unsigned long long *)ctx->wide_box;
    if (loss == CIAO_LOSS_LOGISTIC)
        hipLaunchKernelGGL((afinito_wide_kernel<T, E, CIAO_LOSS_LOGISTIC>), dim3(wa.G), dim3(WIDE_NT), 0, ctx->stream, a, wa);
    else
        hipLaunchKernelGGL((afinito_wide_kernel<T, E, CIAO_LOSS_LS>), dim3(wa.G), dim3(WIDE_NT), 0, ctx->stream, a, wa);
    CIAO_HIP(hipGetLastError());
    char nm[128];
    snprintf(nm, sizeof nm, "afinito_wide_kernel<%s,E%d> grid=%d block=%d steps=%lld", sizeof(T) == 8 ? "f64" : "f32", E, wa.G, WIDE_NT,
             (long long)a.nsteps);
    ctx->last_kernel = nm;
    return CIAO_OK;
}
}  // namespace

template <>
int32_t launch_afinito<CIAO_T>(ciao_ctx *ctx, int loss, AFinitoArgs<CIAO_T> &a)
{
    using T = CIAO_T;
    const int64_t per = (a.d + CHAIN_NT - 1) / CHAIN_NT;
    const int E = per <= 1 ? 1 : (per <= 4 ? 4 : (per <= 8 ? 8 : (per <= 16 ? 16 : 0)));
    a.errflag = ctx->errflag;
    const int64_t rowb = a.d * (int64_t)sizeof(T);
    if (a.nshards > 0 && (loss == CIAO_LOSS_LS_COMPLEX || !ring_eligible<T>(a.d, a.ld, RING_MAX_BYTES, {a.av, a.z}))) {
        set_error("adaptive Finito over a shard table needs real rows of whole 16-byte chunks, at most 32 KiB, and 16-byte aligned vectors");
        return CIAO_ERR_UNSUPPORTED;
    }
    if (a.nshards == 0 && !ctx->chain_no_wide && !ctx->chain_big && (loss == CIAO_LOSS_LS || loss == CIAO_LOSS_LOGISTIC) &&
        rowb > RING_MAX_BYTES && a.d <= (int64_t)WIDE_NT * 8 * WIDE_GMAX && a.nsteps < 0x7FFFFFFFll)
        return launch_afinito_wide<T>(ctx, loss, a);
    // (rows of 16-32 KiB in fp32 are more than 16 elements per thread -- E == 0 -- and still fit the LDS-DMA ring)
    const bool dma_ok = loss != CIAO_LOSS_LS_COMPLEX && !ctx->chain_big &&
                        (a.nshards > 0 || (!ctx->chain_no_dma && ring_eligible<T>(a.d, a.ld, RING_MAX_BYTES, {a.A, a.table, a.meta, a.av, a.z})));
    if (!dma_ok && (E == 0 || loss == CIAO_LOSS_LS_COMPLEX || ctx->chain_big)) {
        // rows beyond the register-resident shapes, complex T, or forced (option chain_big, for tests): state in memory
        if (loss == CIAO_LOSS_LS_COMPLEX)
            hipLaunchKernelGGL((afinito_big_kernel<T, true>), dim3(1), dim3(CHAIN_BIG_NT), 0, ctx->stream, a, loss);
        else
            hipLaunchKernelGGL((afinito_big_kernel<T, false>), dim3(1), dim3(CHAIN_BIG_NT), 0, ctx->stream, a, loss);
        CIAO_HIP(hipGetLastError());
        char nm[128];
        snprintf(nm, sizeof nm, "afinito_big_kernel<%s%s> grid=1 block=%d steps=%lld", sizeof(T) == 8 ? "f64" : "f32",
                 loss == CIAO_LOSS_LS_COMPLEX ? ",cplx" : "", CHAIN_BIG_NT, (long long)a.nsteps);
        ctx->last_kernel = nm;
        return CIAO_OK;
    }
    const bool lg = (loss == CIAO_LOSS_LOGISTIC);
    // ---- LDS-DMA fast path: whole 4 KiB multiples per row, everything 16-byte aligned ----
    if (dma_ok) {
        bool masked;
        const int j = ring_row_class(rowb, &masked);
        {
            int block = CHAIN_NT;
            int32_t st = lg ? launch_afinito_dma<T, CIAO_LOSS_LOGISTIC>(ctx, j, masked, a, &block)
                            : launch_afinito_dma<T, CIAO_LOSS_LS>(ctx, j, masked, a, &block);
            CIAO_TRY(st);
            CIAO_HIP(hipGetLastError());
            char nm[128];
            snprintf(nm, sizeof nm, "afinito_dma_kernel<%s,J%d%s%s> grid=1 block=%d steps=%lld", sizeof(T) == 8 ? "f64" : "f32", j,
                     masked ? ",masked" : "", a.nshards > 0 ? ",sharded" : "", block, (long long)a.nsteps);
            ctx->last_kernel = nm;
            return CIAO_OK;
        }
    }
#define CIAO_AF_CASE(EE)                                                                                                  \
    case EE:                                                                                                              \
        if (lg)                                                                                                           \
            hipLaunchKernelGGL((afinito_chain_kernel<T, EE, CIAO_LOSS_LOGISTIC>), dim3(1), dim3(CHAIN_NT), 0, ctx->stream, a); \
        else                                                                                                              \
            hipLaunchKernelGGL((afinito_chain_kernel<T, EE, CIAO_LOSS_LS>), dim3(1), dim3(CHAIN_NT), 0, ctx->stream, a);  \
        break;
    switch (E) {
        CIAO_AF_CASE(1)
        CIAO_AF_CASE(4)
        CIAO_AF_CASE(8)
        CIAO_AF_CASE(16)
    }
#undef CIAO_AF_CASE
    CIAO_HIP(hipGetLastError());
    char buf[128];
    snprintf(buf, sizeof buf, "afinito_chain_kernel<%s,E%d> grid=1 block=%d steps=%lld", sizeof(T) == 8 ? "f64" : "f32", E, CHAIN_NT,
             (long long)a.nsteps);
    ctx->last_kernel = buf;
    return CIAO_OK;
}

}  // namespace ciao

/*
 * ciao_hip.h -- C ABI of libciao_hip.so: the finite-sum hot path of CIAOAlgorithms.jl (SVRG / SAGA+SAG / Finito /
 * LFinito iterate updates) as hand-written HIP kernels for gfx950 (MI355X).
 *
 * This is the drop-in boundary.  The reference (pure Julia) has no FFI of its own; the boundary is inserted exactly
 * where its iterables (L2) call the ProximalOperators.jl plugin API (L1):
 *      gradient!(y, f_i, x)      prox!(y, g, x, gamma)
 * and where the solver functors (L3) call Base.iterate on those iterables.  Each entry point below names the
 * reference lines (relative to /root/reference/src/algorithms/) whose work it performs.  INTEGRATION.md shows the
 * Julia `ccall` stubs that bind these symbols.
 *
 * Conventions
 *   - extern "C"; plain pointers and sizes; no C++/torch types; no exceptions cross the ABI.
 *   - every call returns int32 status: 0 = ok, negative = error (ciao_last_error() has the text).
 *   - all vectors/matrices are DEVICE pointers unless the parameter name ends in `_host`.  The caller owns every
 *     buffer (AMDGPU.jl ROCArray / torch tensor); the library never frees or reallocates them and only owns the
 *     private workspace inside ciao_ctx.
 *   - work is enqueued on the ctx's HIP stream; calls are asynchronous unless they return host data.
 *   - one ctx = one device + one stream; not thread-safe (the reference is single-threaded with a global RNG).
 *   - sample indices are int64, 0-BASED (the Julia wrapper subtracts 1).  The reference's RNG draws are an INPUT
 *     (index arrays), because Julia's stream is not reproducible outside Julia.
 *   - real type `R` of the reference = `dtype` here (f32 or f64); nothing is silently promoted
 *     (test/test_lasso.jl:74 asserts eltype).  Scalars cross the ABI as double and are rounded to R once.
 *   - data layout: A is row-major N x d with row stride `ld` elements (a Julia d x N column-major Matrix is exactly
 *     this with ld = d); the SAGA/Finito table is row-major N x d, stride d.
 *   - multi-GPU: rows are sharded; every entry point that sums over samples calls the ctx's all-reduce hook (if set)
 *     on the raw d-vector sum before its epilogue (see ciao_ctx_set_allreduce).
 */
#ifndef CIAO_HIP_H
#define CIAO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CIAO_ABI_VERSION 3   /* 3: ciao_shard_table grew by meta[8] (round 4 changed the layout under version 2: ADVICE r4) */

#if defined(__GNUC__)
#define CIAO_API __attribute__((visibility("default")))
#else
#define CIAO_API
#endif

enum {
    CIAO_OK = 0,
    CIAO_ERR_ARG = -1,         /* bad argument (null pointer, negative size, misaligned, index out of range) */
    CIAO_ERR_HIP = -2,         /* a HIP runtime call failed                                                */
    CIAO_ERR_UNSUPPORTED = -3, /* shape / operator family outside what the kernels cover                   */
    CIAO_ERR_ALLOC = -4,       /* workspace allocation failed                                              */
    CIAO_ERR_HOOK = -5         /* the all-reduce hook returned non-zero                                    */
};

enum { CIAO_F32 = 0, CIAO_F64 = 1 };

/* f_i families */
enum {
    CIAO_LOSS_LS = 0,       /* LeastSquares(a_i' (1 x d), [b_i], lam): f_i(x) = lam/2 (a_i'x - b_i)^2   test/test_lasso.jl:54 */
    CIAO_LOSS_LOGISTIC = 1, /* Precompose(LogisticLoss([y_i],1), a_i', 1): log(1+exp(-y_i a_i'x))        test/test_logistic_l1.jl:36 */
    CIAO_LOSS_ZERO = 2,     /* Zero(): the default F = fill(Zero(), N)                                   SVRG/SVRG.jl:58 */
    /* Complex T (src/CIAOAlgorithms.jl:3 RealOrComplex; test/test_lasso.jl:3 runs ComplexF32/64): LeastSquares with a complex
     * row and target, f_i(x) = lam/2 |a_i.x - b_i|^2, grad = lam conj(a_i) (a_i.x - b_i).  Every complex vector is stored as
     * interleaved (re, im) pairs of the REAL dtype -- what reinterpret(R, ::Vector{Complex{R}}) gives: d and ld count reals
     * (d = 2 x the complex length, even), A is N x ld, b holds N pairs, tables N x d.  Correctness path: one wave per row, no
     * tuning. */
    CIAO_LOSS_LS_COMPLEX = 3
};

/* g families (rows O3, O4) */
enum {
    CIAO_PROX_ZERO = 0, /* Zero(): prox = identity                       SVRG/SVRG.jl:49             */
    CIAO_PROX_L1 = 1,   /* NormL1(lam): soft threshold at gamma*lam      test/test_lasso.jl:59       */
    CIAO_PROX_BOX = 2,  /* IndBox(lo, hi): clamp, scalar or per-coordinate  test/test_sharing.jl:16   */
    CIAO_PROX_L1_COMPLEX = 3   /* NormL1(lam) on complex coordinates stored as (re, im) pairs: y = sign(x) max(|x| - gamma lam, 0)
                                  with the complex modulus and sign; d must be even */
};

/* Packed F = [f_1 .. f_N] (replaces the reference's Vector of N one-row operator objects, test/test_lasso.jl:50-58).
 * N is the number of rows RESIDENT on this device (the local shard); N_total the global count used for the 1/N
 * factors (== N on one GPU).  Sample indices, `gam` and the SAGA/Finito tables are indexed by LOCAL row. */
typedef struct {
    int32_t loss;      /* CIAO_LOSS_*                        */
    int32_t dtype;     /* CIAO_F32 / CIAO_F64                */
    int64_t N;         /* local rows                         */
    int64_t d;         /* features                           */
    int64_t ld;        /* row stride of A in elements (>= d) */
    int64_t N_total;   /* global N (for the 1/N factors)     */
    const void *A;     /* device, N x ld                     */
    const void *b;     /* device, N: targets b_i (LS) or labels y_i in {-1,+1} (logistic); NULL for ZERO */
    double lam;        /* LeastSquares lambda (ignored otherwise) */
} ciao_problem;

typedef struct {
    int32_t kind;       /* CIAO_PROX_*                                  */
    int32_t _pad;
    double lam;         /* NormL1 lambda                                */
    double lo, hi;      /* IndBox scalar bounds                         */
    const void *lo_vec; /* device d-vector of lower bounds, or NULL     */
    const void *hi_vec; /* device d-vector of upper bounds, or NULL     */
} ciao_prox_desc;

typedef struct ciao_ctx ciao_ctx; /* opaque: device id, stream, private workspace, all-reduce hook */

/* All-reduce hook: sum `count` elements of dtype at device pointer `buf` IN PLACE across all ranks, enqueued on
 * `stream` (a hipStream_t).  Return 0 on success.  With RCCL: ncclAllReduce(buf, buf, count, type, ncclSum, comm,
 * stream).  The Python host passes a closure around torch.distributed.all_reduce. */
typedef int32_t (*ciao_allreduce_fn)(void *user, void *buf, int64_t count, int32_t dtype, void *stream);

/* ---- library / context ------------------------------------------------------------------------------------- */
CIAO_API int32_t ciao_abi_version(void);
CIAO_API const char *ciao_last_error(void);
/* The extra compiler flags this library was built with: "" for the product build.  Experiment builds (timing macros, some
 * of which give wrong results; tools/exp_build.sh) report theirs here and are never written over the product library. */
CIAO_API const char *ciao_build_flags(void);
/* device >= 0; stream = hipStream_t to enqueue on (NULL = the device's default stream). */
CIAO_API int32_t ciao_ctx_create(int32_t device, void *stream, ciao_ctx **out);
CIAO_API int32_t ciao_ctx_destroy(ciao_ctx *ctx);
CIAO_API int32_t ciao_ctx_set_stream(ciao_ctx *ctx, void *stream);
CIAO_API int32_t ciao_ctx_synchronize(ciao_ctx *ctx);
CIAO_API int32_t ciao_ctx_set_allreduce(ciao_ctx *ctx, ciao_allreduce_fn fn, void *user); /* fn = NULL: single GPU */
/* The same without a host callback: `comm` is an ncclComm_t of RCCL spanning the ranks that share the rows; the library
 * then calls ncclAllReduce(buf, buf, count, ncclFloat|ncclDouble, ncclSum, comm, stream) itself wherever the hook would
 * be called.  RCCL is resolved at run time from `librccl_path` (NULL = "librccl.so"), so single-GPU hosts need no RCCL;
 * pass the library the communicator was created with.  comm = NULL removes it.  Replaces any hook set before. */
CIAO_API int32_t ciao_ctx_set_rccl(ciao_ctx *ctx, void *comm, const char *librccl_path);
/* Objective monitor (the step after the path; the reference has stop(state) = false, SVRG/SVRG.jl:55,70,
 * and computes the cost outside, test/test_lasso.jl:45-47).  obj_dev = device double[3], or NULL to switch it off.  While
 * set, every full pass over the rows -- ciao_full_gradient, ciao_proxgrad_step, ciao_svrg_init, the tail pass of
 * ciao_svrg_iterate (at the new z_full = the solution), ciao_lfinito_init, the full pass of ciao_lfinito_iterate (at
 * z_full) -- also leaves, for the point x the pass was taken at,
 *     obj_dev[1] = (1/N_total) sum_i f_i(x)    obj_dev[2] = g(x)    obj_dev[0] = obj_dev[1] + obj_dev[2]
 * where the f_i(x) are the values `gradient!` returns and the reference discards: they ride on the same sweep (no extra
 * pass over A; all-reduced with the d-vector on a row-sharded problem).  g (may be NULL = Zero) is copied. */
CIAO_API int32_t ciao_ctx_set_monitor(ciao_ctx *ctx, const ciao_prox_desc *g, double *obj_dev);
/* Tuning knobs (performance only, never results-changing beyond summation order); returns CIAO_ERR_ARG for unknown keys:
 *   "sweep_blocks_per_cu", "sweep_grid", "sweep_prefetch", "sweep_multi", "force_generic"   grid / variant of the rows kernels
 *   "chain_max_batch"      Finito / LFinito batches up to this size run as one sequential chain (-1 = measured crossover)
 *   "split_max_rows"       batches up to this size run one workgroup per row instead of one wave per row (-1 = 16384)
 *   "split_blocks_per_cu"  grid cap of that kernel (0 = automatic)
 *   "split_all"            experiment: that kernel for every mode and size (tools/tune_split.py)
 *   "small_i"              rows_small_kernel (rows under 1 KiB): elements per lane and iteration, 8 or 16 (0 = automatic)
 *   "small_mfma"           0: dense rows of 17 .. 256 elements do not take the matrix-core tile kernel (rows_smallm_kernel)
 *   "small_mfma_table"     0: ... its table modes (SAGA / Finito init, Finito batches over row blocks) are off, the sweeps stay
 *   "small_nb"             ... tile buffers per wave, 2 .. 4 (0 = automatic: 2)
 *   "small_wrow"           0: Finito / LFinito batches on rows of up to 256 elements do not take the one-wave-per-row kernel
 *                          (rows_wrow_kernel: index lists, and row blocks of up to 8192 rows) but rows_smallb_kernel / the tiles
 *   "wrow_rows_per_wave"   rows_wrow_kernel: rows a wave takes in a small batch before more workgroups are used (0 = 4)
 *   "multi_rhs_off"        1: ciao_full_gradient_multi / ciao_svrg_epoch_tail_multi run K single sweeps (testing)
 *   "mscore_off"           1: ciao_margin_stats_multi runs K times (row dots + per-sample reduction) instead of its one-pass kernel (testing)
 *   "peer_timeout_s"       wall-clock bound of a peer-mailbox wait, seconds (default 30)
 *   "chain_no_dma"         the register-ring chain instead of the LDS-DMA one;  "chain_big": the any-length kernels at any d
 *   "chain_four_waves"     rows of up to 2 KiB (fp64: 4 KiB) on the four-wave chain instead of the single-wave one
 *   "proshi_chain_max_batch"  ProShI batches up to this size run as one coordinate-parallel chain launch (-1 = measured crossover)
 *   "chain_no_ws"          SAGA / SAG chains on chain_dma_kernel instead of the wave-specialised chain_ws_kernel
 *   "chain_no_wide"        SVRG / SAGA chains on rows beyond 8192 elements on the one-workgroup kernel instead of chain_wide_kernel
 *   "chain_ws_issuers"     issuer waves of chain_ws_kernel, 1 or 2 (0 = automatic)
 *   "long_rows"            0: sweeps / batches on rows beyond 64 KiB on the generic kernel instead of rows_long_kernel (a cluster of
 *                          workgroups per row);  "long_j": its 16-byte chunks per thread, 4 or 8 (0 = automatic)
 *   "svrg_cache_rowdots"   0: the SVRG full pass does not store a_i'z_full at all (see ciao_svrg_iterate) */
CIAO_API int32_t ciao_ctx_set_option(ciao_ctx *ctx, const char *key, int64_t value);
/* Kernel timing for bench.py's roofline line: when enabled, every launch of the dominant streaming kernel of an entry
 * point (rows_fast_kernel / rows_generic_kernel) is bracketed by HIP events on the ctx's stream.  _read synchronises,
 * returns the summed device time of those launches and their count since the last read, and resets the counters. */
CIAO_API int32_t ciao_ctx_timing_enable(ciao_ctx *ctx, int32_t enable);
CIAO_API int32_t ciao_ctx_timing_read(ciao_ctx *ctx, double *total_ms_host, int64_t *launches_host);
/* Name + grid of the dominant kernel of the last entry point called (for bench.py / rocprof correlation). */
CIAO_API const char *ciao_ctx_last_kernel(ciao_ctx *ctx);

/* ---- L1 plugin API (ProximalOperators.jl calling convention) ---------------------------------------------- */
/* gradient!(y, F[i], x): y = grad f_i(x); if fval != NULL also *fval = f_i(x) (device scalar of dtype).
 * Call sites: SVRG/SVRG_basic.jl:60,74,75,89; SAGA_SAG/SAGA_basic.jl:43,56; Finito/Finito_basic.jl:78,112. */
CIAO_API int32_t ciao_gradient(ciao_ctx *ctx, const ciao_problem *p, int64_t i, const void *x, void *y, void *fval);
/* prox!(y, g, x, gamma): y = prox_{gamma g}(x); y may alias x.
 * Call sites: SVRG_basic.jl:80; SAGA_basic.jl:48,64; Finito_basic.jl:84,118; Finito_LFinito.jl:83,92. */
CIAO_API int32_t ciao_prox(ciao_ctx *ctx, int32_t dtype, int64_t d, const ciao_prox_desc *g, const void *x, double gamma,
                  void *y);

/* ---- the roofline sweep ------------------------------------------------------------------------------------ */
/* av = (1/N_total) sum_i grad f_i(x)       SVRG_basic.jl:58-63 (init) and :87-92 (epoch tail).
 * Reads every row of A exactly once. */
CIAO_API int32_t ciao_full_gradient(ciao_ctx *ctx, const ciao_problem *p, const void *x, void *av);
/* The same pass for K iterates over the same rows -- av[k] = (1/N_total) sum_i grad f_i(x[k]), k < K -- in ONE pass over A: with
 * K right-hand sides the contraction is GEMM-shaped (A Z, the link function, A' C) and runs on the matrix cores
 * (csrc/mrhs_kernels.h; north_star: "MFMA ... if the f_i gradients are expressed as a dense A.x contraction").  x and av are HOST
 * arrays of K device pointers (16-byte aligned d-vectors).  Not in the reference, which solves one problem per call
 * (SVRG_basic.jl:87-92 is the single pass): an extension for hosts that advance several solves together (a regularisation path,
 * folds: ciao_ctx_chain_batch_begin).  Shapes the kernel does not take (d other than 256 / 512 / 768 / 1024 -- and 128 in fp64 --, unaligned rows, a
 * row-sharded problem, the objective monitor) run as K single passes inside the call.  Each av[k] agrees with its own
 * ciao_full_gradient to rounding (another summation order), not bitwise. */
CIAO_API int32_t ciao_full_gradient_multi(ciao_ctx *ctx, const ciao_problem *p, int32_t K, const void *const *x, void *const *av);
/* Fused proximal-gradient step on the full gradient (the "full-gradient + prox sweep" of the north star; it is also
 * LFinito's `prox!` + full pass, Finito_LFinito.jl:83-88, in x-coordinates):
 *     av = (1/N_total) sum_i grad f_i(x);   y = prox_{gamma g}(x - gamma * av)          (y may alias x) */
CIAO_API int32_t ciao_proxgrad_step(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double gamma,
                           const void *x, void *av, void *y);
/* (1/N_total) sum_i f_i(x) + g(x) on the same sweep (the value `gradient!` returns and the reference discards;
 * test/test_lasso.jl:45 computes it outside).  *obj_host receives the value (synchronises). */
CIAO_API int32_t ciao_objective(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *x,
                       double *obj_host);
/* Optimality certificate at x.  out_host[0] = F(x) = (1/N) sum f_i(x), [1] = g(x) (L1 value; 0 for Zero/Box),
 * [2] = || x - prox_{gamma g}(x - gamma grad f(x)) ||_2 / gamma, [3] = || grad f(x) ||_inf, [4] = x . grad f(x),
 * [5] = max Box violation of x (0 otherwise).  av: NULL -> one full pass is made here (the objective monitor's sum armed for it; the
 * caller's monitor is neither read nor written); non-NULL -> the caller's grad f(x) is used, no pass over A, and out_host[0] is
 * left as the caller set it (F(x) where known, NaN otherwise).  Real T only (complex problems are refused); gamma > 0, finite.
 * The five reductions are bitwise reproducible: their order is a function of d alone.  Synchronises. */
CIAO_API int32_t ciao_certificate(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *x,
                                  const void *av, double gamma, double *out_host);
/* Row dots: out[i] = a_i'x for the N local rows (device memory, N elements of T) -- the predictions of a fitted model, per sample.
 * Not in the reference (its f_i are one-row operator objects; test/test_logistic_l1.jl forms A*x on the host).  One full pass, the
 * certificate's own; grad f(x) goes to the context's workspace.  Real T with data rows only (CIAO_LOSS_ZERO and complex problems are
 * refused).  On a row-sharded context: the local rows.  Does not synchronise. */
CIAO_API int32_t ciao_row_dots(ciao_ctx *ctx, const ciao_problem *p, const void *x, void *out);
/* Per-sample statistics of given row dots (device memory, N of T) against p->b, reduced on the device.  Logistic rows, t_i = b_i dots_i:
 * out_host[0] = sum_i log(1 + exp(-t_i)), [1] = E(s) = sum_i h(s sigma(-t_i)) with h(u) = u log u + (1-u) log(1-u) (the entropy of the
 * logistic dual at the point scaled by s), [2] = the number of samples with t_i <= 0 (misclassified), [3] = min_i t_i.  LeastSquares
 * rows, r_i = dots_i - b_i: [0] = sum_i r_i^2, [1] = sum_i b_i, [2] = sum_i b_i^2, [3] = max_i |r_i|.  Serves log-loss / accuracy /
 * RMSE / R^2 of a fitted model (the reference's tests compute them outside) and the logistic duality gap.  0 <= s <= 1; N >= 1; real
 * T with data rows only.  Bitwise reproducible: the order of every sum is a function of N alone.  Synchronises. */
CIAO_API int32_t ciao_margin_stats(ciao_ctx *ctx, const ciao_problem *p, const void *dots, double s, double *out_host);
/* EXTENSION beyond the reference (as ciao_full_gradient_multi is): the same statistics for K models in ONE pass over A -- model
 * selection over a regularisation path, folds or restarts.
 * x: HOST array of K device pointers (d-vectors of p->dtype, 16-byte aligned, as ciao_full_gradient_multi takes them).
 * s_host: K host doubles in [0,1], or NULL (= all 1).  out_host: 4*K host doubles.
 * out_host[4k .. 4k+4) holds exactly the four numbers ciao_margin_stats documents, for the row dots a_i'x_k over the N local rows at
 * s = s_k.  The N x K dots never exist in memory (csrc/mscore_kernels.h: the row dots on the matrix cores, the per-sample terms as
 * their epilogue).  Model k's four numbers are bitwise the same whatever K is, whichever place k has in the list and whatever the
 * other iterates hold (NaN included); the order of every sum is a function of (N, d, dtype) alone.  They agree with
 * ciao_row_dots + ciao_margin_stats to rounding (another order of addition), not bitwise.  1 <= K <= 256.  The one-pass kernel takes
 * every d <= 1024, every ld and every base of A; longer rows, iterates that are not 16-byte aligned and the option "mscore_off" run
 * as K times (the ciao_row_dots pass + the reduction of ciao_margin_stats) inside the call, bitwise what those two calls give.
 * Refused with CIAO_ERR_ARG and nothing launched: a NULL ctx, p, x or out_host, K outside 1..256, a NULL x[k], an s_k outside [0,1]
 * or NaN, N = 0, CIAO_LOSS_ZERO and complex problems.  On a row-sharded context: the LOCAL rows, as ciao_row_dots.  Synchronises. */
CIAO_API int32_t ciao_margin_stats_multi(ciao_ctx *ctx, const ciao_problem *p, int32_t K, const void *const *x,
                                         const double *s_host, double *out_host);
/* ciao_margin_stats_multi over a LIST of rows, with an offset per model: held-out rows of a fold scored for K
 * fitted models that each carry an intercept, in one pass over the rows named and without a gathered copy.
 * idx: M device int64 row numbers in [0, N), 8-byte aligned, any order, repeats allowed; or NULL: every row in order (M must be N).
 * offset_host: K host doubles, finite, or NULL; model k's per-sample terms see (double)(a_i'x_k) + offset_k, one double addition.
 * With NULL no addition is made.  s_host, out_host, x: as ciao_margin_stats_multi.
 * The call over idx gives BIT FOR BIT what the call with idx = NULL gives on the gathered copy A[idx], b[idx], for every ld, base and
 * alignment of A; with idx = NULL and offset_host = NULL it gives ciao_margin_stats_multi's bits.  A model's bits do not depend on K, on
 * its place in the list of models or on its neighbours.  An entry of idx outside [0, N) is a row that does not exist: no load is
 * issued for it and its samples are SKIPPED (not counted as zeros).  Columns [d, ld) and rows the list does not name are never read.
 * There is no in-call fallback here and the option "mscore_off" does not apply: refused with CIAO_ERR_ARG and nothing launched are
 * ciao_margin_stats_multi's cases and M < 1, idx not 8-byte aligned, a non-finite offset, idx = NULL with M != N, d > 1024 and an
 * x[k] that is not 16-byte aligned (score such a model with ciao_list_dots).  ciao_ctx_last_kernel: mscore_partial_kernel<rows,...>.
 * Synchronises. */
CIAO_API int32_t ciao_margin_stats_multi_rows(ciao_ctx *ctx, const ciao_problem *p, const int64_t *idx, int64_t M, int32_t K,
                                              const void *const *x, const double *offset_host, const double *s_host, double *out_host);
/* ciao_certificate with its per-sample terms.  out_host[0..5] are exactly ciao_certificate's six numbers (av = NULL: the call makes
 * its pass), [6..9] the four numbers of ciao_margin_stats on that pass's row dots with s = min(1, mu / ||grad f(x)||_inf) formed on
 * the device (mu = g->lam for CIAO_PROX_L1 with lam > 0; s = 1 otherwise, and where grad f(x) = 0).  For logistic rows and NormL1
 * the duality gap is out[0] + out[1] + out[7] / N (no counterpart in the reference: `stop(state) = false`, SVRG.jl:55).  Refused on a
 * row-sharded context (all-reduce hook or shard table set), for N = 0, CIAO_LOSS_ZERO and complex problems.  Synchronises. */
CIAO_API int32_t ciao_certificate_samples(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *x,
                                          double gamma, double *out_host);
/* EXTENSION beyond the reference (as ciao_full_gradient_multi is): gap-safe feature screening for l1 problems.  The reference has
 * no screening and no duality gap (`stop(state) = false`, SVRG.jl:55); DESIGN.md section 8.8 has the rule and its radii.
 * Column sums of squares: out[j] = sum_i A[i,j]^2 for j < d over the N resident rows; out is a device vector of d DOUBLES whatever
 * p->dtype is.  One pass over A (every element read once, squares formed and added in double), no atomics: bitwise reproducible
 * between runs, contexts, row strides and pointer alignments -- every order of addition is a function of (N, d) alone.  Real
 * CIAO_LOSS_LS / CIAO_LOSS_LOGISTIC problems; complex problems, CIAO_LOSS_ZERO (no A), N = 0 and NULL arguments are refused with
 * CIAO_ERR_ARG and nothing is launched.  On a row-sharded context: the LOCAL rows only, as ciao_row_dots (the caller sums the
 * ranks' vectors).  Workspace: at most 32 MiB of partial sums (8 d bytes where that is more).  Does not synchronise,
 * except where that workspace has to grow (the first call at a larger N x d waits for the stream and reallocates). */
CIAO_API int32_t ciao_col_sqnorms(ciao_ctx *ctx, const ciao_problem *p, double *out);
/* EXTENSION beyond the reference: the screening rule.  grad = grad f(x), a device d-vector of dtype; colsq = what ciao_col_sqnorms
 * wrote (device, d doubles); keep = d device bytes.  Per coordinate, in double, without contraction:
 *     keep[j] = !( s |grad_j| + kappa sqrt(colsq_j) < mu )
 * so that a NaN anywhere keeps the coordinate; *n_kept_host = the number of kept coordinates.  With s and kappa from the duality
 * gap every dropped coordinate is zero at the optimum.  0 <= s <= 1; kappa >= 0 (+inf allowed: keeps
 * everything; NaN refused); mu > 0 and finite; d >= 1; no NULL argument: otherwise CIAO_ERR_ARG.  Synchronises. */
CIAO_API int32_t ciao_screen(ciao_ctx *ctx, int32_t dtype, int64_t d, const void *grad, const double *colsq, double s, double kappa,
                             double mu, uint8_t *keep, int64_t *n_kept_host);
/* EXTENSION beyond the reference: the per-sample smoothness constants of a packed matrix.  The reference's tests form them on the host
 * from the rows, L_i = lam ||a_i||^2 (test/test_lasso.jl:52-56) and L_i = ||a_i||^2 / 4 (test/test_logistic_l1.jl:39), and every step
 * size follows from them (gamma = 1 / (7 max L), test_lasso.jl:164; gamma_i = alpha N / L_i, Finito_basic.jl:61-74).  DESIGN.md section 8.9.
 * Row sums of squares: out[i] = sum_j A[i,j]^2 for the N resident rows; out is a device vector of N DOUBLES whatever p->dtype is, or
 * NULL.  stats_host: 4 host doubles {max_i out[i], the smallest i that attains it (exact as a double), min_i out[i], sum_i out[i]},
 * or NULL; with out = NULL only the summary is produced and no N-vector exists anywhere.  One pass over A (every element read once,
 * squares formed and added in double), no atomics: bitwise reproducible between runs, contexts, row strides and pointer alignments
 * -- the order of addition of a row is a function of d alone, that of the summary of (N, d) alone.  A NaN anywhere in a row makes
 * that row's value NaN and the summary's max, min and sum NaN (argmax: the first such row), so that a step size derived from it is
 * NaN too.  CIAO_LOSS_LS, CIAO_LOSS_LOGISTIC and CIAO_LOSS_LS_COMPLEX problems (a complex row is its 2n reals: ||a_i||^2 is their
 * sum of squares).  CIAO_LOSS_ZERO (no A), N = 0, a NULL problem and out = stats_host = NULL are refused with CIAO_ERR_ARG and
 * nothing is launched.  On a row-sharded context: the LOCAL rows only, as ciao_row_dots and ciao_col_sqnorms.  Workspace: 128 KiB
 * of records.  Synchronises only where stats_host is non-NULL (and where that workspace is first allocated). */
CIAO_API int32_t ciao_row_sqnorms(ciao_ctx *ctx, const ciao_problem *p, double *out, double *stats_host);
/* EXTENSION beyond the reference: the column moments of a packed matrix, for standardising it where it lies.  The reference has no
 * counterpart (its tests build their matrices on the host); one l1 weight on columns of different scale penalises units, and
 * LeastSquares rows have no intercept unless A and b are centred.  DESIGN.md section 8.10.
 * Shifted sums over the N resident rows, for j < d:
 *     s1[j] = sum_i (A[i,j] - c_j)        s2[j] = sum_i (A[i,j] - c_j)^2
 * with c = shift, a device vector of d DOUBLES, or (shift = NULL) c_j = A[0,j], read by the kernel.  s1 and s2 are device vectors of d
 * DOUBLES whatever p->dtype is.  (double)a - c_j, its square and every addition are formed in double, without contraction.  Then
 * mean_j = c_j + s1[j] / N and M2_j = s2[j] - s1[j]^2 / N (N times the population variance), M2 with a relative error of at most
 * 2 (N + 3) 2^-53 s2 / M2: where that quotient is large, a second call with shift = the mean brings it to 1.  One pass over A (every
 * element read once), no atomics: bitwise reproducible between runs, contexts, row strides and pointer alignments -- every order of
 * addition is a function of (N, d) alone.  Real CIAO_LOSS_LS / CIAO_LOSS_LOGISTIC problems; complex problems, CIAO_LOSS_ZERO (no A)
 * and NULL ctx / p / s1 / s2 are refused with CIAO_ERR_ARG and nothing is launched.  N = 0: both vectors are set to zero, no kernel is
 * launched.  On a row-sharded context: the LOCAL rows only, as ciao_col_sqnorms (with shift = NULL each rank would shift by its own
 * first row: pass a common shift there).  Workspace: at most 32 MiB of partial sums (16 d bytes where that is more).  Does not
 * synchronise, except where that workspace has to grow. */
CIAO_API int32_t ciao_col_moments(ciao_ctx *ctx, const ciao_problem *p, const double *shift, double *s1, double *s2);
/* EXTENSION beyond the reference: centre and scale the columns of a packed matrix in one pass.  For i < N, j < d:
 *     out[i,j] = (T)( ((double)A[i,j] - center_j) * scale_j )
 * center, scale: device vectors of d DOUBLES; NULL center means 0, NULL scale means 1.  One subtraction and one multiplication in
 * double, without contraction, then one rounding to T.  out: device, N rows of stride ld_out >= d elements of p->dtype; the columns
 * [d, ld_out) of a row are not written.  out == p->A with ld_out == p->ld is allowed (in place: every element is read and written by
 * the same thread, a row is loaded before it is stored); any other overlap of the two matrices is refused.  N d elements read, N d
 * written; 16-byte accesses where both bases and both strides are multiples of 16 bytes.  Refusals as ciao_col_moments (NULL ctx /
 * p / out, complex problems, CIAO_LOSS_ZERO), plus ld_out < d: CIAO_ERR_ARG, nothing launched.  N = 0: nothing to do (out may then be NULL).  On a
 * row-sharded context: the local rows.  No workspace; does not synchronise. */
CIAO_API int32_t ciao_scale_columns(ciao_ctx *ctx, const ciao_problem *p, const double *center, const double *scale, void *out,
                                    int64_t ld_out);
/* EXTENSION beyond the reference: the second-order statistics of a packed matrix in one pass over its rows, on the matrix cores.
 * The reference has no counterpart (its tests form A'A on the host where they need the smoothness constant).  DESIGN.md section 8.12.
 * Over the N resident rows, for i, j < d:
 *     G[i * ldg + j] = sum_n A[n,i] A[n,j]      u[j] = sum_n A[n,j] b_n      colsum[j] = sum_n A[n,j]
 *     bsum[0] = sum_n b_n                       bsum[1] = sum_n b_n^2
 * (b: the targets of CIAO_LOSS_LS rows, the labels of CIAO_LOSS_LOGISTIC rows).  G: device, d rows of stride ldg >= d DOUBLES; both
 * triangles are written and G[i][j], G[j][i] hold the same bits; the columns [d, ldg) of a row are not written.  u, colsum: device
 * vectors of d DOUBLES; bsum: 2 device DOUBLES; each of the three may be NULL and the others' bits do not depend on it.  Every output
 * is double whatever p->dtype is: fp32 rows are converted to double where they become operands of v_mfma_f64_16x16x4_f64, so every
 * product of two fp32 elements is exact, every sum is formed in double, and a matrix stored as fp32 gives the bits the same values
 * stored as fp64 give.  One pass over A (the upper triangle of 128 x 128 tiles of G times P row partitions, then a fixed-order sum of a
 * tile's P partial tiles), no atomics: bitwise reproducible between runs, contexts, row strides and pointer alignments -- every order of
 * addition is a function of (N, d) alone.  Columns [d, ld) of a row are never read.  Real CIAO_LOSS_LS / CIAO_LOSS_LOGISTIC problems with
 * d <= 4096; complex problems, CIAO_LOSS_ZERO (no A), d > 4096, ldg < d and NULL ctx / p / G are refused with CIAO_ERR_ARG and nothing is
 * launched.  N = 0: every output is set to zero, no kernel is launched.  On a row-sharded context: the LOCAL rows only, as
 * ciao_col_moments (the ranks' matrices are not combined).  Workspace: at most 256 MiB of partial tiles.  Does not synchronise, except
 * where that workspace has to grow. */
CIAO_API int32_t ciao_gram(ciao_ctx *ctx, const ciao_problem *p, double *G, int64_t ldg, double *u, double *colsum, double *bsum);
/* EXTENSION beyond the reference: ciao_gram with a weight per row -- A' diag(w) A and the weighted sums, in the same one pass on the
 * matrix cores.  DESIGN.md section 8.13.  w: a device vector of N DOUBLES (the local rows') at any 8-byte-aligned address; nothing beyond
 * w[N-1] is read.  Over the N resident rows, for i, j < d:
 *     G[i * ldg + j] = sum_n w_n A[n,i] A[n,j]     u[j] = sum_n w_n A[n,j] b_n      colsum[j] = sum_n w_n A[n,j]
 *     bsum[0] = sum_n w_n b_n                      bsum[1] = sum_n w_n b_n^2        bsum[2] = sum_n w_n
 * bsum: 3 device DOUBLES here; G, ldg, u, colsum and the NULL rule as ciao_gram (u, colsum, bsum may each be NULL and the others' bits do
 * not depend on it).  WHERE THE WEIGHT ENTERS: exactly one operand of every product is w_n times an element -- w_n A[n,j] for G[i][j] with
 * i <= j (the other triangle is its mirror: both hold the same bits), w_n b_n for u and bsum[0..1], w_n for colsum and bsum[2] -- formed
 * in double with ONE rounding; the other operand is the raw element, and no square root of w is taken.  So any finite weight is allowed,
 * negative ones included; integer weights on integer rows stay exact; w = 1 gives ciao_gram's bits (1 a is exact, the order of addition
 * is the same); 0/1 weights give the statistics of a row subset without copying rows.  A weight of zero does NOT mask a non-finite
 * element: 0 inf = NaN.  Plan, tiles, workspace and the order of addition are ciao_gram's: a function of (N, d) alone, not of ld, of
 * the bases of A or w, of p->dtype, of the NULL outputs or of the values of w; bitwise reproducible.  Refused with CIAO_ERR_ARG and
 * nothing launched: a NULL or misaligned w, and everything ciao_gram refuses (complex problems, CIAO_LOSS_ZERO, d > 4096, ldg < d,
 * NULL ctx / p / G).  N = 0: every output is set to zero, no kernel is launched (w may then be NULL).  On a row-sharded context: the
 * LOCAL rows only.
 * Workspace: ciao_gram's.  Does not synchronise, except where that workspace has to grow. */
CIAO_API int32_t ciao_gram_weighted(ciao_ctx *ctx, const ciao_problem *p, const double *w, double *G, int64_t ldg, double *u, double *colsum,
                                    double *bsum);
/* EXTENSION beyond the reference: the statistics of a LIST of rows at the cost of the rows touched -- ciao_gram / ciao_gram_weighted over
 * the gathered matrix A[idx], b[idx] without forming it.  DESIGN.md section 8.15.  idx: a device vector of M int64 row numbers (LOCAL rows
 * on a row-sharded context) at any 8-byte-aligned address, in any order, repeats allowed (a bootstrap resample, a random fold); nothing
 * beyond idx[M-1] is read.  List position m plays the part the row number plays in ciao_gram: the panel row and b are read at idx[m], the
 * weight (w: M device DOUBLES at any 8-byte-aligned address, or NULL for the unweighted statistics) at the POSITION m, so a bootstrap's
 * counts or w[idx] go in directly; nothing beyond w[M-1] is read.  bsum: 2 device doubles without w, 3 with it; G, ldg, u, colsum and the
 * NULL rule as ciao_gram.  Plan, tiles, workspace, order of addition and the final kernels are ciao_gram's for (M, d): the outputs are BIT
 * FOR BIT those of ciao_gram (with w: of ciao_gram_weighted) on the gathered copy, for every ld, base and alignment of A, idx and w;
 * idx = 0 .. N-1 gives ciao_gram's bits on A itself.  A is read only: the rows named by the list, columns [0, d) of them.
 * An entry outside [0, N) names a row that does not exist: the kernel issues no load for it and the row is zero in both operands (the
 * ones of the augmented column included, so it counts in no sum); Context.gram(rows=) refuses such a list BEFORE any launch -- the
 * predicate is there so that this raw entry point cannot read out of bounds.  Refused with CIAO_ERR_ARG and nothing launched: a NULL or
 * misaligned idx (M = 0 aside), M < 0, a misaligned w, and everything ciao_gram refuses.  M = 0: every output is set to zero, no kernel is
 * launched.  Workspace: ciao_gram's.  Does not synchronise, except where that workspace has to grow. */
CIAO_API int32_t ciao_gram_rows(ciao_ctx *ctx, const ciao_problem *p, const int64_t *idx, int64_t M, const double *w, double *G, int64_t ldg,
                                double *u, double *colsum, double *bsum);
/* EXTENSION beyond the reference: a matrix-vector product and its adjoint over a LIST of rows, the first-order passes of a problem on a
 * row subset (a training fold, held-out rows, a bootstrap resample) at the cost of the rows touched.  DESIGN.md section 8.16.
 *     ciao_list_dots     out[m] = a_{idx[m]}' x                 m = 0 .. M-1   (M device doubles)
 *     ciao_list_combine  out[j] = sum_m c[m] A[idx[m], j]       j = 0 .. d-1   (d device doubles)
 * idx: M device int64 row numbers (LOCAL rows on a row-sharded context) at any 8-byte-aligned address, any order, repeats allowed, or
 * NULL: position = row, and M must equal p->N.  x: d device elements of p->dtype; c: M device DOUBLES, one per list position, at any
 * 8-byte-aligned address.  Products and sums in double.  Both give BIT FOR BIT what the same call with idx = NULL gives on the gathered
 * copy A[idx] (c unchanged), for every ld, base and alignment of A, idx, x and c: the order of addition of a row's dot product is a
 * function of d alone (one row has one bit pattern at every position of every list), that of the combination of (M, d) alone.  A is
 * read only: the rows named, columns [0, d) of them; nothing beyond idx[M-1] / c[M-1].  An entry outside [0, N) issues no load:
 * out[m] = 0 in the dots, no term in the combination (Context.list_dots / list_combine refuse such a list before any launch).
 * Refused with CIAO_ERR_ARG and nothing launched: NULL ctx / p / x / c / out; M < 0; idx = NULL with M != N; idx, c or out not aligned
 * to 8 bytes; complex problems; CIAO_LOSS_ZERO; d > 4096.  M = 0: nothing is launched (ciao_list_combine sets out to d zeros).
 * Workspace of ciao_list_combine: ciao_col_sqnorms' partial d-vectors.  Neither synchronises, except where that workspace has to grow. */
CIAO_API int32_t ciao_list_dots(ciao_ctx *ctx, const ciao_problem *p, const int64_t *idx, int64_t M, const void *x, double *out);
CIAO_API int32_t ciao_list_combine(ciao_ctx *ctx, const ciao_problem *p, const int64_t *idx, int64_t M, const double *c, double *out);
/* EXTENSION beyond the reference: cyclic coordinate descent with covariance updates for the lasso on a Gram matrix (glmnet's inner loop),
 * K models in one launch, one workgroup each.  DESIGN.md section 8.14.  Everything is DOUBLE and on the device:
 *     min_x (c/2)(x'G x - 2 u'x + const) + mu_k ||x||_1,   tau[k] = mu_k / c
 * G: d x d at row stride ldg (symmetric: only ROW j is read for coordinate j, never a column beyond d-1); u: d; inv: d, inv[j] = 1 / G[j][j]
 * where that is > 0 and 0 elsewhere (the kernel never divides); tau: K; X: K vectors of d at stride ldx, the warm starts on entry and the
 * results on exit; R: K vectors of d at stride ldr, or NULL: the final r = u - G x as accumulated; stat: K x 4 doubles {sweeps made,
 * non-zero updates made, largest change of the last completed full sweep, state}.
 *     start      r = u; for j ascending with x_j != 0: r_i -= x_j G[j][i]
 *     update(j)  rho = r_j + G_jj x_j; a = |rho| - tau; x+ = 0 if a <= 0, else copysign(a, rho) inv_j; delta = x+ - x_j; delta not finite:
 *                the model ends at once, state 2, x_j unchanged; delta != 0: r_i -= delta G[j][i] for all i, then x_j = x+;
 *                change = G_jj delta^2; the support changes if exactly one of x_j, x+ is 0
 *     loop       a full sweep (j = 0 .. d-1); largest change <= tol and support unchanged: state 1 (converged).  Otherwise active sweeps
 *                (only the j with x_j != 0 at their turn) until one has largest change <= tol, then a full sweep again.  Every sweep counts
 *                against max_sweeps; the budget spent: state 0 (call again from the returned X).
 * Every product is rounded before it is added and no sum over coordinates is formed: the results are a function of the inputs' bits alone,
 * not of K, of a model's place among the K, of ldg / ldx / ldr, of the bases or of the run (host_route.host_gram_cd reproduces them in
 * numpy).  Refused with CIAO_ERR_ARG and nothing launched: NULL ctx / G / u / inv / tau / X / stat; d < 1 or > 4096; K < 1 or > 4096;
 * ldg < d, ldx < d, ldr < d with R given; a base not aligned to 8 bytes; tol < 0 or NaN; max_sweeps < 1 or > 1024 (this bounds one
 * launch's time).  Does not synchronise. */
CIAO_API int32_t ciao_gram_cd(ciao_ctx *ctx, int64_t d, int64_t K, const double *G, int64_t ldg, const double *u, const double *inv,
                              const double *tau, double *X, int64_t ldx, double tol, int32_t max_sweeps, double *R, int64_t ldr, double *stat);
/* EXTENSION beyond the reference: ciao_gram_cd with bounds, a penalty factor per coordinate, a ridge term, and a Gram matrix, u and tol
 * per model (non-negative and box-constrained lasso, adaptive lasso, elastic net, every fold of a cross-validation in ONE launch).
 * DESIGN.md section 8.17.  Model k minimises over lo_kj <= x_j <= hi_kj
 *     1/2 x'G x - u_k'x + sum_j t_kj |x_j| + (ridge_k / 2) sum_j x_j^2,   G = G + gsel[k] sg,   t_kj = tau[k] pf_kj (one rounded product)
 * G: nsets matrices of d x d at row stride ldg, sg elements apart (sg is not looked at with nsets = 1); gsel: K int32 set numbers, or NULL:
 * set 0 for all; u, inv, pf, lo, hi: model k's d elements start at k times the vector's stride, a stride of 0 shares one vector among all
 * models; inv_kj = 1 / (G_jj + ridge_k) where that is > 0, else 0 (the ridge enters nowhere else); pf, lo, hi may each be NULL: 1, -inf,
 * +inf; tau, tol: K; X, R, stat, max_sweeps: as ciao_gram_cd.
 *     update(j)  ciao_gram_cd's with a = |rho| - t_kj and, after x+ is formed:  if (x+ > hi_kj) x+ = hi_kj;  if (x+ < lo_kj) x+ = lo_kj
 *                (comparisons: a NaN goes through to state 2); the sweep loop is ciao_gram_cd's with tol[k]
 *     state 3    the model cannot run and ends at once, its rows of X and R untouched, nothing of G read for it, the other models
 *                unaffected: gsel[k] outside [0, nsets); tol[k] < 0 or NaN; a pf_kj < 0 or NaN; a t_kj NaN; lo_kj > 0, hi_kj < 0, or
 *                either NaN
 * With pf, lo, hi NULL or at their defaults and one set, X, R and stat are ciao_gram_cd's bit for bit; in general they are a function of
 * the model's own inputs' bits alone (host_route.host_gram_cd_general reproduces them in numpy).  Refused with CIAO_ERR_ARG and nothing
 * launched: what ciao_gram_cd refuses (tol: NULL); nsets < 1; sg < (d-1) ldg + d with nsets > 1; a stride of u, inv, pf, lo or hi that
 * is neither 0 nor >= d; a base not aligned to 8 bytes (gsel: 4).  Does not synchronise. */
CIAO_API int32_t ciao_gram_cd_general(ciao_ctx *ctx, int64_t d, int64_t K, const double *G, int64_t ldg, int64_t sg, int64_t nsets,
                                      const int32_t *gsel, const double *u, int64_t ldu, const double *inv, int64_t ldinv, const double *tau,
                                      const double *pf, int64_t ldpf, const double *lo, int64_t ldlo, const double *hi, int64_t ldhi,
                                      double *X, int64_t ldx, const double *tol, int32_t max_sweeps, double *R, int64_t ldr, double *stat);

/* ---- SVRG / SVRG++  (SVRG/SVRG_basic.jl) -------------------------------------------------------------------- */
/* Base.iterate(iter), :57-66: av = full gradient at x0; z_full = x0; z = 0; w = x0. */
CIAO_API int32_t ciao_svrg_init(ciao_ctx *ctx, const ciao_problem *p, const void *x0, void *av, void *z, void *z_full,
                       void *w);
/* The inner cycle :73-82 for the m draws idx[0..m) (device int64, 0-based LOCAL rows):
 *     temp = gamma*(grad f_i(z_full) - grad f_i(w) - av) + w ; w = prox_{gamma g}(temp) ; z += w.
 * Strictly sequential in w: runs as one persistent workgroup (replicas-only across GPUs). */
CIAO_API int32_t ciao_svrg_inner(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double gamma, int64_t m,
                        const int64_t *idx, const void *av, void *z, const void *z_full, void *w);
/* Base.iterate(iter, state), :71-96 = inner cycle + tail (z_full = z/m; basic: w = z_full; z = 0) + full pass.
 * (`state.m *= 2` of SVRG++ is host bookkeeping; pass the current m.)
 * The full pass also stores a_i'z_full per row in the ctx workspace (N scalars).  With reuse_rowdots != 0 the CALLER
 * vouches that A and z_full still hold exactly what the previous ciao_svrg_init / ciao_svrg_iterate on this ctx left in
 * them (nothing wrote to either from outside, not even in place); the inner cycle then reads those N scalars instead of
 * recomputing the second dot product of every step (0.39 vs 0.50 us per update at d = 1024 fp64).
 * The library additionally requires that the previous call on this ctx was one of those two (or ciao_svrg_inner) with
 * the same A, z_full and N; anything else recomputes.  With reuse_rowdots == 0 nothing cached is ever read: the safe
 * choice for a host that hands the state vectors to user code between calls.  The host mirrors track this themselves
 * (solvers.py: torch's in-place version counters of z_full, A and b). */
CIAO_API int32_t ciao_svrg_iterate(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double gamma, int64_t m,
                          const int64_t *idx, int32_t plus, int32_t reuse_rowdots, void *av, void *z, void *z_full, void *w);
/* The second half of ciao_svrg_iterate on its own, :84-92: z_full = z / m; basic (plus == 0): w = z_full; z = 0; then the full
 * pass av = (1/N) sum_i grad f_i(z_full).  ciao_svrg_inner followed by this IS ciao_svrg_iterate with reuse_rowdots == 0, bit for
 * bit; it exists for hosts that run the inner cycles of several solves as one chain batch (ciao_ctx_chain_batch_begin) and
 * finish each solve's outer iteration afterwards. */
CIAO_API int32_t ciao_svrg_epoch_tail(ciao_ctx *ctx, const ciao_problem *p, int64_t m, int32_t plus, void *av, void *z,
                             void *z_full, void *w);
/* ... for K solves over the same rows at once (host arrays of K device pointers): every solve's tail, then the K full passes as
 * ONE pass over A (ciao_full_gradient_multi).  K calls of ciao_svrg_epoch_tail to rounding. */
CIAO_API int32_t ciao_svrg_epoch_tail_multi(ciao_ctx *ctx, const ciao_problem *p, int32_t K, int64_t m, int32_t plus, void *const *av,
                                   void *const *z, void *const *z_full, void *const *w);

/* ---- the sequential chains on a row-sharded problem ("one chain on one GPU pulling remote rows over xGMI") --
 * The inner loops of SVRG and SAGA are one dependent chain and do not shard: on a problem whose rows do not fit one GPU
 * (BASELINE config #4: 80M x 1024) exactly ONE rank, the chain owner, runs the chain and reads the rows of the other shards
 * through peer-mapped pointers (hipIpcOpenMemHandle / peer access: the loads travel over xGMI; all indices are known up front,
 * SVRG_basic.jl:73, so the rows are prefetched through the same LDS-DMA ring as local ones).  Same arithmetic, same order:
 * the chain's results are bitwise those of the unsharded chain on the concatenated rows.
 *   shard k = GLOBAL rows [row0[k], row0[k+1]) (contiguous block partition, row0[0] = 0, row0[nshards] = N_total);
 *   A[k], b[k] (and table[k] for SAGA): device pointers valid on THIS device for shard k's rows (its own shard: the
 *   local pointers); every A[k] has the row stride of the local problem.  Non-owners pass the same nshards / row0 and
 *   may leave the pointers NULL. */
#define CIAO_MAX_SHARDS 8
typedef struct {
    int32_t nshards;
    int32_t owner;                          /* != 0 on the one rank that runs the chains */
    int64_t row0[CIAO_MAX_SHARDS + 1];
    const void *A[CIAO_MAX_SHARDS];
    const void *b[CIAO_MAX_SHARDS];
    void *table[CIAO_MAX_SHARDS];           /* SAGA gradient table / adaptive Finito s-table shards (NULL when only SVRG is run) */
    void *meta[CIAO_MAX_SHARDS];            /* adaptive Finito: the per-sample scalars of the shard's rows (n x 4 x 4; NULL otherwise) */
} ciao_shard_table;
/* Installs (copies) the shard table; NULL removes it.  While one is set AND an all-reduce hook is installed,
 * ciao_svrg_inner / ciao_svrg_iterate / ciao_saga_steps / ciao_afinito_init / ciao_afinito_steps are valid on the row-sharded
 * problem (adaptive Finito: every rank initialises its own rows' table and scalars in one all-reduced sweep; the owner's chain
 * then reads and writes the other shards' table rows and scalars, and av, z, hat_gamma and the two counters reach every rank;
 * rows must be whole 16-byte chunks of at most 32 KiB): `idx` then holds GLOBAL rows,
 * the owner runs the chain, every other rank skips it, and the iterates the chain produced (z, w; for SAGA z, av) reach all
 * ranks through one all-reduce of 2d scalars in which the non-owners contribute zeros; the tail and the full pass of
 * ciao_svrg_iterate then run sharded as usual.  (The a_i'z_full cache is not used across shards.) */
CIAO_API int32_t ciao_ctx_set_shards(ciao_ctx *ctx, const ciao_shard_table *shards);
/* ---- one-shot peer all-reduce (SURVEY.md sections 5 / 8e, the "tuned alternative" to ncclAllReduce; no reference counterpart) --
 * The all-reduce of the d+1 scalars of a sweep / batch is latency, not bandwidth (4-16 KB over 7 direct xGMI links).  With
 * peers set, the kernel that produces a rank's raw sum writes it straight into a slot of EVERY rank's mailbox and releases a
 * flag, and the kernel that applies the epilogue waits for the world's flags and adds the slots in rank order (bitwise the
 * same sum on every rank): no collective call and no extra launch per reduction (csrc/peer_kernels.h).
 *   _mailbox_create: this rank's mailbox, fine-grained device memory for reductions of up to max_elems elements (d + 1, or
 *                    2 d for the sharded chains' hand-over); share it with ciao_ipc_export / _open.  _destroy frees it.
 *   ciao_ctx_set_peers: mailboxes[r] = rank r's mailbox as mapped on THIS device (mailboxes[rank] = its own); world <= 8.  Every
 *                    rank calls it with freshly created mailboxes at the same point of its program and from then on makes
 *                    the same reductions in the same order.  Replaces any all-reduce hook / RCCL communicator; NULL or world 0
 *                    turns it off.  A rank whose flag never arrives is reported by ciao_ctx_synchronize (CIAO_ERR_HOOK). */
CIAO_API int32_t ciao_peer_mailbox_create(ciao_ctx *ctx, int64_t max_elems, void **mailbox_out, int64_t *bytes_out);
CIAO_API int32_t ciao_peer_mailbox_destroy(ciao_ctx *ctx, void *mailbox);
CIAO_API int32_t ciao_ctx_set_peers(ciao_ctx *ctx, int32_t rank, int32_t world, void *const *mailboxes, int64_t max_elems);
/* Sharing a device allocation with the chain owner's process (plain HIP IPC, no torch / AMDGPU.jl needed):
 * _export: handle_out = 64 bytes describing the allocation that contains dev_ptr, *offset_out = dev_ptr's offset in it;
 * _open (in the other process, on the device that will read it): *dev_ptr_out = the mapped pointer + offset;
 * _close: unmaps what _open returned (pass the same dev_ptr and offset). */
CIAO_API int32_t ciao_ipc_export(const void *dev_ptr, void *handle_out, int64_t *offset_out);
CIAO_API int32_t ciao_ipc_open(const void *handle, int64_t offset, void **dev_ptr_out);
CIAO_API int32_t ciao_ipc_close(void *dev_ptr, int64_t offset);

/* ---- SAGA / SAG  (SAGA_SAG/SAGA_basic.jl) ------------------------------------------------------------------- */
/* Base.iterate(iter), :41-48: table[i] = grad f_i(x0); av = sum/N; z = prox_{gamma g}((1-gamma) x0). */
CIAO_API int32_t ciao_saga_init(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double gamma,
                       const void *x0, void *table, void *av, void *z);
/* nsteps consecutive Base.iterate(iter,state), :53-68, with the draws idx[0..nsteps) (device int64). */
CIAO_API int32_t ciao_saga_steps(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double gamma, int32_t sag,
                        int64_t nsteps, const int64_t *idx, void *table, void *av, void *z);

/* ---- several independent chains at once ----------------------------------------------------------------------- */
/* A chain (the SVRG inner cycle SVRG_basic.jl:73-82, the SAGA / SAG steps SAGA_basic.jl:53-68) is one workgroup on one of the
 * GPU's 256 compute units: sequential by definition.  A host that runs SEVERAL solves over the same rows -- a
 * regularisation path (g = NormL1(lambda_k)), cross-validation folds (index streams over different row subsets), restarts --
 * has that many independent chains.  Between _begin and _end the calls of ciao_svrg_inner, ciao_saga_steps and ciao_finito_steps
 * (index-list form, every iteration's batch of the same size, small enough to run as a sequential chain: option "chain_max_batch";
 * the default Finito has batches of one sample, Finito.jl:50) on this ctx are
 * RECORDED instead of launched (every other entry point returns CIAO_ERR_ARG meanwhile); _end(launch = 1) checks that no chain
 * writes state another one touches (SVRG writes w, z; SAGA and Finito z, av and their table; CIAO_ERR_ARG otherwise), and launches them as one
 * grid per kernel variant with one workgroup per chain, on the ctx's stream; _end(launch = 0) drops the records.  Each chain's
 * results are bitwise those of the same call made alone.  Takes the chains of the LDS-DMA kernels: real scalars, rows of whole
 * 16-byte chunks of at most 32 KiB, 16-byte aligned, unsharded (CIAO_ERR_UNSUPPORTED from the recording call otherwise: the batch
 * stays open and that call is not part of it).  No counterpart in the reference, which solves one problem per call. */
CIAO_API int32_t ciao_ctx_chain_batch_begin(ciao_ctx *ctx);
CIAO_API int32_t ciao_ctx_chain_batch_end(ciao_ctx *ctx, int32_t launch);

/* ---- Finito / MISO  (Finito/Finito_basic.jl) ---------------------------------------------------------------- */
/* hat_gamma = 1 / sum_i (1/gam_i)  over the LOCAL rows then all-reduced (Finito_basic.jl:82). Synchronises. */
CIAO_API int32_t ciao_hat_gamma(ciao_ctx *ctx, int32_t dtype, int64_t N, const void *gam, double *hat_gamma_host);
/* Base.iterate(iter), :76-84: table[i] = x0 - (gam_i/N) grad f_i(x0); av = hat_gamma sum_i table[i]/gam_i;
 * z = prox_{hat_gamma g}(av).  gam: device N-vector of per-sample stepsizes (built by the host from :61-74). */
CIAO_API int32_t ciao_finito_init(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *gam,
                         double hat_gamma, const void *x0, void *table, void *av, void *z);
/* nit consecutive Base.iterate(iter,state), :109-118.  Iteration t uses the samples
 * bidx[bptr_host[t] .. bptr_host[t+1]) (bidx: device int64, LOCAL rows; bptr_host: HOST int64[nit+1]); the batch
 * choice (:95-108) is host logic.  Small batches run as one persistent chain; large ones batch-parallel.
 * The samples of one batch must be distinct, as every batch the reference can build is (sample(1:N, r, replace=false),
 * :97, or a static block, :49-59): the members of a batch are updated concurrently. */
CIAO_API int32_t ciao_finito_steps(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *gam,
                          double hat_gamma, int64_t nit, const int64_t *bptr_host, const int64_t *bidx,
                          void *table, void *av, void *z);

/* The same for batches that are contiguous blocks of LOCAL rows -- every static batch of sweeping 2 and 3 is one
 * (Finito_basic.jl:52-58), on a row-sharded problem too (the local members of a contiguous global block are a contiguous
 * local block under both ownership rules of the host mirror): iteration t updates rows first_host[t] .. first_host[t] +
 * len_host[t] - 1 (HOST int64[nit] each).  No index array exists: nothing is built or uploaded per batch (8 bytes per
 * sample and iteration otherwise -- for LFinito a whole N-index array per iteration) and a sharded host needs no per-batch
 * membership test.  The kernels are the same and so is their speed (measured: 12.0 vs 12.0 us per batch at r = 256,
 * 45.1 vs 46.2 at r = 4096, d = 4096 fp32); results are bitwise those of ciao_finito_steps on arange(first, first+len). */
CIAO_API int32_t ciao_finito_steps_blocks(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *gam,
                                 double hat_gamma, int64_t nit, const int64_t *first_host, const int64_t *len_host,
                                 void *table, void *av, void *z);

/* ---- LFinito  (Finito/Finito_LFinito.jl) -------------------------------------------------------------------- */
/* Base.iterate(iter), :66-72: av = x0 - (hat_gamma/N) sum_i grad f_i(x0); z = z_full = av (state ctor :27-37). */
CIAO_API int32_t ciao_lfinito_init(ciao_ctx *ctx, const ciao_problem *p, double hat_gamma, const void *x0, void *av,
                          void *z, void *z_full);
/* One Base.iterate(iter,state), :82-100: z_full = prox(av); av = z_full - (hat_gamma/N) sum grad f_i(z_full);
 * then for each of the nb batches, in the order given: z = prox(av); av += sum_{i in batch} [ (hat_gamma/N)
 * (grad f_i(z_full) - grad f_i(z)) + (hat_gamma/gam_i)(z - z_full) ]. */
CIAO_API int32_t ciao_lfinito_iterate(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *gam,
                             double hat_gamma, int64_t nb, const int64_t *bptr_host, const int64_t *bidx,
                             void *av, void *z, void *z_full);

/* The same with the batches given as contiguous row blocks (LFinito's batches are ALWAYS the static blocks of
 * Finito_LFinito.jl:44-49; sweeping 3 only permutes their order, :89): see ciao_finito_steps_blocks. */
CIAO_API int32_t ciao_lfinito_iterate_blocks(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, const void *gam,
                                    double hat_gamma, int64_t nb, const int64_t *first_host, const int64_t *len_host,
                                    void *av, void *z, void *z_full);

/* ---- adaptive Finito  (Finito/Finito_adaptive.jl) -------------------------------- */
/* For the row-structured f_i here grad f_i = c_i a_i, so the reference's N x d gradient table is N scalars: `meta` is a
 * device N x 4 x 4 array of R: per sample FOUR identical copies of {c_i, f_i(x_i), gamma_i, a_i'x_i} (one per wave of
 * the step kernel, which makes every read follow its write in one wave's program order); `table` is the N x d table of points
 * x_i; `hat_gamma_dev` is a DEVICE scalar of R (it changes during backtracking).
 * Base.iterate(iter), :59-98: x_i = x0; gamma_i = alpha / L_i with L_i = ||grad f_i(x0 .+ 1) - grad f_i(x0)|| / (sqrt(d) N);
 * hat_gamma = 1/sum 1/gamma_i; av = hat_gamma (sum x_i/gamma_i - sum grad f_i / N); z = prox_{hat_gamma g}(av).
 * The reference's random re-probe (:78-85: when grad f_i(x0 .+ 1) == grad f_i(x0), i.e. for a row whose entries sum to zero,
 * it probes at x0 .+ rand(t*[-1,1]) with t = 1, 2, 4, ...) needs RNG draws, which are a HOST input on this path: such
 * samples get gamma_i = -1 in meta and the next ciao_ctx_synchronize returns CIAO_ERR_UNSUPPORTED.  The host then resolves
 * them in increasing i with ciao_afinito_probe and its own +-1 draws (gamma_i = alpha / (nmg / (t sqrt(d)) / N) with the t
 * AFTER its doubling, as the reference has it, :82-88) and repeats this call with `gam_override`: a device N-vector of R
 * whose entries > 0 are taken as gamma_i (the others are computed as before); NULL = none. */
CIAO_API int32_t ciao_afinito_init(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double alpha,
                                   const void *x0, void *table, void *meta, void *av, void *z, void *hat_gamma_dev,
                                   const void *gam_override);
/* One retry of that probe for sample i: *nmg_host = || grad f_i(x0 + t*signs) - grad f_i(x0) || (signs: device d-vector of
 * +-1 in R; for CIAO_LOSS_LS_COMPLEX d/2 real +-1 entries, added to the real parts as rand(t*[-1,1], size(x0)) does, and
 * sqrt(length(x0)) in the host's formula counts the d/2 complex entries).  Synchronises. */
CIAO_API int32_t ciao_afinito_probe(ciao_ctx *ctx, const ciao_problem *p, int64_t i, const void *x0, const void *signs, double t,
                                    double *nmg_host);
/* nsteps consecutive Base.iterate(iter,state), :120-152, for the samples idx[0..nsteps) (the selection :105-118 is host
 * logic).  Synchronises; *done_host = steps completed (< nsteps iff a stepsize fell below tol_b/N: the reference then
 * warns and ends the iteration, :123-126), *trials_host = backtracking trials taken.  Julia's promotions are kept for
 * R = Float32: the model value `0.5 * iter.N * iter.α / γ ...` and the comparison are Float64, `γ *= 0.8` is a Float64
 * product rounded back (:128-136).  Rows of any length and complex T run afinito_big_kernel (state in the caller's vectors);
 * meta for complex T: copies 0/2 hold {Re c, f_i, gamma_i, Re a_i.x_i}, copies 1/3 the imaginary parts (c = lam res). */
CIAO_API int32_t ciao_afinito_steps(ciao_ctx *ctx, const ciao_problem *p, const ciao_prox_desc *g, double alpha,
                                    double tol_b, int64_t nsteps, const int64_t *idx, void *table, void *meta, void *av,
                                    void *z, void *hat_gamma_dev, int64_t *done_host, int64_t *trials_host);

/* ---- ProShI  (ProShI/ProShI_basic.jl) ------------------------------------------------ */
/* minimize (1/N) sum_i f_i(x_i) + g(sum_i x_i): the solution is the whole N x d table.  Operator family of the reference's
 * own test (test/test_sharing.jl:16-25): f_i = Sum(Quadratic(Q_i, q_i), SqrDistL2(IndBox(lo, hi), eta)).
 *   dense = 0: Q_i = diagm(Q[i,:]) as that test builds it; grad f_i(x)_k = Q_ik x_k + q_ik + eta (x_k - clamp(x_k, lo, hi)),
 *              element-wise in each agent's own row.
 *   dense = 1: a full d x d matrix per agent (ProShI_basic.jl:113 calls the operator's generic gradient!, which for Quadratic
 *              is Q_i x + q_i): Q holds N row-major blocks, row k of agent i at Q + (i*d + k)*ld; needs d*sizeof(T) <= 64 KiB. */
typedef struct {
    int32_t dtype;     /* CIAO_F32 / CIAO_F64                                  */
    int32_t dense;     /* 0: Q holds the N diagonals; 1: N dense d x d blocks  */
    int64_t N;         /* local agents (rows)                                  */
    int64_t d;
    int64_t ld;        /* row stride of Q and q in elements (>= d)             */
    int64_t N_total;   /* global number of agents (the 1/N factor)             */
    const void *Q;     /* device N x ld diagonals, or (dense) N*d x ld rows    */
    const void *q;     /* device N x ld: their linear terms                    */
    double eta, lo, hi; /* SqrDistL2(IndBox(lo, hi), eta); eta = 0 drops it    */
} ciao_sepquad;
/* Base.iterate(iter), :76-87: table_i = x0 - (gam_i/N) grad f_i(x0); hat_gamma = sum gam_i (written to the device scalar
 * hat_gamma_dev); av = sum_i table_i; z = (prox_{hat_gamma g}(av) - av) / hat_gamma. */
CIAO_API int32_t ciao_proshi_init(ciao_ctx *ctx, const ciao_sepquad *f, const ciao_prox_desc *g, const void *gam,
                                  const void *x0, void *table, void *av, void *z, void *hat_gamma_dev);
/* nit consecutive Base.iterate(iter,state), :109-121; iteration t updates the agents bidx[bptr_host[t]..bptr_host[t+1])
 * (device int64, LOCAL rows): av -= s_i; s_i += gam_i z; s_i -= (gam_i/N) grad f_i(s_i); av += s_i; then the z update. */
CIAO_API int32_t ciao_proshi_steps(ciao_ctx *ctx, const ciao_sepquad *f, const ciao_prox_desc *g, const void *gam,
                                   double hat_gamma, int64_t nit, const int64_t *bptr_host, const int64_t *bidx,
                                   void *table, void *av, void *z);
/* The same for batches that are contiguous blocks of local agents (sweeping 2 and 3, ProShI_basic.jl:50-57). */
CIAO_API int32_t ciao_proshi_steps_blocks(ciao_ctx *ctx, const ciao_sepquad *f, const ciao_prox_desc *g, const void *gam,
                                 double hat_gamma, int64_t nit, const int64_t *first_host, const int64_t *len_host,
                                 void *table, void *av, void *z);
/* solution(state), :127-132: table_i += gam_i z for every agent, IN PLACE (as the reference does). */
CIAO_API int32_t ciao_proshi_solution(ciao_ctx *ctx, const ciao_sepquad *f, const void *gam, const void *z, void *table);

/* ==================================================================================================================
 * Everything above is the drop-in surface: the entry points a reference-side binding needs for this path.
 * The declarations below are NOT part of it.  They are helpers the benchmark, the tests and the Python host mirror use
 * (synthetic data generated on the device; the host-side batch sampler of the injected index stream) and are only
 * visible with CIAO_BENCH_API defined.
 * ================================================================================================================== */
#ifdef CIAO_BENCH_API
/* ---- synthetic data (bench / tests): counter-based generator, reproducible per (seed, row, col) ------------- */
/* out[i*ld + k] = scale * N(0,1) for rows row0 .. row0+nrows, keyed by the GLOBAL (row, col). */
CIAO_API int32_t ciao_synth_normal(ciao_ctx *ctx, int32_t dtype, void *out, int64_t nrows, int64_t d, int64_t ld,
                          int64_t row0, uint64_t seed, double scale);
/* b = A x_true + noise*N(0,1) (LS targets) or sign(...) (logistic labels when `labels` != 0). */
CIAO_API int32_t ciao_synth_targets(ciao_ctx *ctx, const ciao_problem *p, const void *x_true, double noise, int32_t labels,
                           int64_t row0, uint64_t seed, void *b_out);

/* ---- host-side helper: the batch draws of Finito / ProShI with sweeping = 1 ------------------------------------ */
/* n consecutive `sample(1:N, r, replace=false)` (Finito_basic.jl:97, ProShI_basic.jl:97) from the injected
 * counter-based index stream (splitmix64(seed), outputs pos, pos+1, ...: DESIGN.md "index streams"; Julia's own RNG is
 * not reproducible outside Julia), written 0-based to the HOST array out_host[n*r]; *pos_out_host = the stream
 * position after the draws.  Rule per batch: draw as many uniform candidates as are still missing, append, drop
 * repeats keeping first occurrences, until r distinct indices are held.  Needs 2r <= N (the wrapper shuffles
 * otherwise).  Pure host code, no ctx: it exists because a device batch takes 10-50 us and an interpreted host cannot
 * draw batches at that rate. */
CIAO_API int32_t ciao_sample_batches(uint64_t seed, uint64_t pos, int64_t N, int64_t r, int64_t n, int64_t *out_host,
                            uint64_t *pos_out_host);
/* m i.i.d. uniform draws from 0..N-1 of the same stream (outputs pos .. pos+m-1; the rule of `rand(state.ind, m)`,
 * SVRG_basic.jl:73, and `rand(1:N)`, SAGA_basic.jl:55, on the injected stream: ((splitmix64 >> 32) * N) >> 32), written to the
 * DEVICE array out_dev[m] on the ctx's stream: an epoch's 10^7 indices cost the host a second and 80 MB of PCIe, the device
 * microseconds.  Needs 0 < N < 2^32. */
CIAO_API int32_t ciao_sample_uniform(ciao_ctx *ctx, uint64_t seed, uint64_t pos, int64_t N, int64_t m, int64_t *out_dev);
/* The peer all-reduce (ciao_ctx_set_peers) on a device buffer of its own, as two kernels (send, wait + add): what bench.py
 * times as allreduce_us_per_step for that collective, and what tests hold against a host-staged sum. */
CIAO_API int32_t ciao_peer_allreduce(ciao_ctx *ctx, int32_t dtype, int64_t count, void *buf);

#endif /* CIAO_BENCH_API */

#ifdef __cplusplus
}
#endif
#endif /* CIAO_HIP_H */

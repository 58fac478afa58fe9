// gramcdg_kernels.h -- the general form of the coordinate descent of gramcd_kernels.h (ciao_gram_cd_general):
//      min_x  1/2 x'G x - u_k'x + sum_j t_kj |x_j| + (ridge_k / 2) sum_j x_j^2      over lo_kj <= x_j <= hi_kj,     G = G[gsel[k]]
// K models in one launch, each with its own Gram matrix out of `nsets`, its own u, inv, penalty factors, bounds and tol.  The ridge term
// enters through the host's inv_kj = 1 / (G_jj + ridge_k) alone (0 where that denominator is not > 0): the kernel never divides.
//
// The method, to the bit (host_route.host_gram_cd_general is its numpy mirror; every product is rounded before it is added):
//   refusal    gsel[k] outside [0, nsets); tol[k] < 0 or NaN; a pf_kj < 0 or NaN; a t_kj = (tau_k pf_kj) NaN; lo_kj > 0, hi_kj < 0 or
//              either NaN: the model ends at once with state 3, its rows of X and R untouched, nothing of G read for it
//   start      t_kj = tau_k pf_kj, one rounded product;  r = u_k;  for j ascending with x_j != 0:  r_i <- r_i - (x_j G_ji)
//   update(j)  rho = r_j + (G_jj x_j);  a = |rho| - t_kj;  x+ = 0 if a <= 0, else copysign(a, rho) inv_kj;  if (x+ > hi) x+ = hi;
//              if (x+ < lo) x+ = lo  (comparisons, not fmin / fmax: a NaN in x+ goes through);  delta = x+ - x_j;  the rest -- state 2,
//              the update of r, change = G_jj (delta delta), the support rule, the full / active sweep loop -- is gramcd_kernels.h's,
//              with tol[k] for tol
// With pf, lo, hi NULL (or 1, -inf, +inf) and one set the bits are ciao_gram_cd's: tau 1.0 is exact and the clamp moves nothing.
//
// The kernel is gramcd_kernel's: one workgroup per model, the decision wave-uniform in every thread, element i of r on one thread for
// the whole launch, the row requested before delta is known, two barriers per non-zero update.  New: t_kj is a fourth LDS array beside
// x, r and the diagonal (4 d doubles, d rounded up to even: 128 KiB at d = 4096), and a byte per coordinate says which sides are open
// (bit 0: hi_kj > 0, bit 1: lo_kj < 0; 4 KiB more), then 16 bytes for the flag through which the workgroup agrees on a refusal (an LDS word and
// two barriers: the library's block-wide OR made the compiler take inv, lo and hi of every update through vector loads, whose wait
// also waited for the row in front of the first barrier: 1.3-1.5 x the time per update).  lo, hi and inv of the coordinate that moves come from global memory behind the row
// request.  The 64-at-a-time idle test passes over exactly the coordinates at x_j = 0 whose update gives delta = 0: a <= 0, or x+ on a
// closed side (rho > t with hi = 0, rho < -t with lo = 0), which the clamp returns to 0.  That holds for a finite a and inv_kj >= 0; a
// coordinate whose inv_kj is negative or NaN has both bits set, and a non-finite a takes its turn, so the bits never depend on the test
// (the mirror has none).  CIAO_GRAMCDG_PLAIN_IDLE (an experiment macro) puts gramcd_kernel's test back, to time what the flags buy.
//
// What is never read: columns [d, ldg) of a row of G, anything beyond element d-1 of a model's u / inv / pf / lo / hi or of its row of X,
// anything beyond element K-1 of tau / tol / gsel.  16-byte loads where the base of G, ldg and the set stride allow and the pair lies
// wholly in [0, d); element loads otherwise.
#pragma once

#include "gramcd_kernels.h"

namespace ciao {

struct GramCdgPlan {
    int block;       // threads per workgroup
    int vec16;       // 1: 16-byte row loads
    int grid;        // K
    int lds;         // bytes of dynamic LDS
};

// a pure function of (d, ldg, sg, the alignment of G, K); sg: the set stride, 0 with one set
inline GramCdgPlan gramcdg_plan(int64_t d, int64_t ldg, int64_t sg, bool g_aligned16, int64_t K)
{
    GramCdgPlan pl;
    pl.block = d <= GRAMCD_SMALL_D ? GRAMCD_SMALL_BLOCK : GRAMCD_LARGE_BLOCK;
    pl.vec16 = g_aligned16 && ldg % 2 == 0 && sg % 2 == 0;
    pl.grid = (int)K;
    const int64_t dp = (d + 1) & ~(int64_t)1;
    pl.lds = (int)(4 * dp * (int64_t)sizeof(double) + ((d + 15) & ~(int64_t)15) + 16);      // x, r, diag, t; the open-side bytes; the refusal flag
    return pl;
}

struct GramCdgArgs {
    const double *G;
    const int32_t *gsel;   // K, or NULL: set 0 for all
    const double *u, *inv;
    const double *tau;     // K
    const double *pf;      // or NULL: 1
    const double *lo;      // or NULL: -inf
    const double *hi;      // or NULL: +inf
    const double *tol;     // K
    double *X;
    double *R;             // or NULL
    double *stat;          // K x 4: sweeps, non-zero updates, largest change of the last full sweep, state
    int64_t ldg, sg, ldu, ldinv, ldpf, ldlo, ldhi, ldx, ldr;
    int d;
    int nsets;
    int max_sweeps;
};

template <int BLOCK, bool VEC>
__global__ __launch_bounds__(BLOCK) void gramcdg_kernel(GramCdgArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char gramcdg_smem[];
    const int d = a.d;
    const int dp = (d + 1) & ~1;
    double *x = reinterpret_cast<double *>(gramcdg_smem);
    double *r = x + dp;
    double *diag = r + dp;
    double *tk = diag + dp;
    unsigned char *open = reinterpret_cast<unsigned char *>(tk + dp);
    int *refused = reinterpret_cast<int *>(open + ((d + 15) & ~15));
    const int t = (int)threadIdx.x;
    const int k = (int)blockIdx.x;
    double *Xk = a.X + (int64_t)k * a.ldx;
    const double *__restrict__ uk = a.u + (int64_t)k * a.ldu;
    const double *__restrict__ invk = a.inv + (int64_t)k * a.ldinv;
    const double *__restrict__ pfk = a.pf ? a.pf + (int64_t)k * a.ldpf : nullptr;
    const double *__restrict__ lok = a.lo ? a.lo + (int64_t)k * a.ldlo : nullptr;
    const double *__restrict__ hik = a.hi ? a.hi + (int64_t)k * a.ldhi : nullptr;
    const double tau = a.tau[k];
    const double tol = a.tol[k];
    const int set = a.gsel ? a.gsel[k] : 0;
    double g[GRAMCD_PER_THREAD];

    // the vectors of the model into LDS, and what it cannot run on found on the way
    if (t == 0)
        *refused = 0;
    __syncthreads();
    bool refuse = !(set >= 0 && set < a.nsets) || !(tol >= 0.0);
    for (int i = t; i < d; i += BLOCK) {
        const double pf = pfk ? pfk[i] : 1.0;
        const double lo = lok ? lok[i] : -__builtin_huge_val();
        const double hi = hik ? hik[i] : __builtin_huge_val();
        const double iv = invk[i];
        const double ti = tau * pf;
        refuse |= !(pf >= 0.0) || ti != ti || !(lo <= 0.0) || !(hi >= 0.0);
        const bool wild = !(iv >= 0.0);
        x[i] = Xk[i];
        r[i] = uk[i];
        tk[i] = ti;
        open[i] = (unsigned char)((hi > 0.0 || wild ? 1 : 0) | (lo < 0.0 || wild ? 2 : 0));
    }
    int sweeps = 0, state = 3;
    double nupd = 0.0, last_full = 0.0;
    // the same answer in every thread.  Refused: state 3, X and R as they were, nothing of G read.  (One exit for both ways, with every
    // global store after the sweeps: inv, lo and hi of the coordinate that moves then come through the scalar cache, and the row stays
    // in flight across the first barrier.)
    if (refuse)
        *refused = 1;
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane(*refused) == 0) {
    const double *__restrict__ G = a.G + (int64_t)set * a.sg;
    for (int i = t; i < d; i += BLOCK)
        diag[i] = G[(int64_t)i * a.ldg + i];
    __syncthreads();
    // start: r = u - G x, one row per non-zero of the warm start, in ascending order (gramcd_kernel's)
    for (int j = 0; j < d; ++j) {
        {
            const int jl = j + (t & 63);
            const unsigned long long m = __ballot(jl < d && x[jl] != 0.0);
            if (m == 0ull) {
                j += 63;
                continue;
            }
            j += __builtin_ctzll(m);
        }
        const double xj = gramcd_uniform(x[j]);
        if (xj != 0.0) {
            gramcd_load_row<BLOCK, VEC>(G + (int64_t)j * a.ldg, d, t, g);
            gramcd_axpy<BLOCK, VEC>(r, d, t, xj, g);
        }
    }
    __syncthreads();

    bool active = false;      // the kind of the sweep about to run
    while (true) {
        if (sweeps >= a.max_sweeps) {
            state = 0;
            break;
        }
        ++sweeps;
        double big = 0.0;
        bool support = false, bad = false;
        for (int j = 0; j < d; ++j) {
            // the first coordinate from j on that can move, 64 at a time (gramcd_kernel's walk).  At x_j = 0 the test is sign-aware: a
            // coordinate whose x+ lands on a closed side is clamped back to 0 and takes no turn.
            const int jl = j + (t & 63);
            double xl = 0.0, rl = 0.0, gl = 0.0, tl = 0.0;
            bool can = false;
            if (jl < d) {
                xl = x[jl];
                rl = r[jl];
                gl = diag[jl];
                tl = tk[jl];
                const double rho = rl + gl * xl;
                const double av = fabs(rho) - tl;
#ifdef CIAO_GRAMCDG_PLAIN_IDLE
                can = xl != 0.0 || (!active && !(av <= 0.0));
#else
                const int op = open[jl];
                const bool side = rho > 0.0 ? (op & 1) != 0 : rho < 0.0 ? (op & 2) != 0 : true;
                can = xl != 0.0 || (!active && !(av <= 0.0) && (side || !(av <= 1.79769313486231570815e308)));
#endif
            }
            const unsigned long long m = __ballot(can);
            if (m == 0ull) {
                j += 63;
                continue;
            }
            const int lane = __builtin_ctzll(m);
            j += lane;
            const double xj = gramcd_lane(xl, lane);
            const double rj = gramcd_lane(rl, lane);
            const double gjj = gramcd_lane(gl, lane);
            const double tj = gramcd_lane(tl, lane);
            const double rho = rj + gjj * xj;
            const double av = fabs(rho) - tj;
            if (av <= 0.0 && xj == 0.0)
                continue;                                   // x+ = 0 = x_j: nothing moves
            gramcd_load_row<BLOCK, VEC>(G + (int64_t)j * a.ldg, d, t, g);   // requested before delta is known: G is read only
            double xp = av <= 0.0 ? 0.0 : copysign(av, rho) * invk[j];
            const double hi = hik ? hik[j] : __builtin_huge_val();
            const double lo = lok ? lok[j] : -__builtin_huge_val();
            if (xp > hi)
                xp = hi;
            if (xp < lo)
                xp = lo;
            const double delta = xp - xj;
            if (!(fabs(delta) <= 1.79769313486231570815e308)) {
                bad = true;
                break;
            }
            if (delta != 0.0) {
                __syncthreads();                            // every thread has decided coordinate j from the r of before
                gramcd_axpy<BLOCK, VEC>(r, d, t, delta, g);
                if ((VEC ? (j >> 1) : j) % BLOCK == t)
                    x[j] = xp;
                __syncthreads();
                nupd += 1.0;
                const double ch = gjj * (delta * delta);
                if (ch > big)
                    big = ch;
                if ((xj == 0.0) != (xp == 0.0))
                    support = true;
            }
        }
        if (bad) {
            state = 2;
            break;
        }
        if (!active) {
            last_full = big;
            if (big <= tol && !support) {
                state = 1;
                break;
            }
            active = true;
        } else if (big <= tol) {
            active = false;
        }
    }
    // every write of x and r was followed by a barrier
    for (int i = t; i < d; i += BLOCK) {
        Xk[i] = x[i];
        if (a.R)
            a.R[(int64_t)k * a.ldr + i] = r[i];
    }
    }
    if (t == 0) {
        double *st = a.stat + 4 * (int64_t)k;
        st[0] = (double)sweeps;
        st[1] = nupd;
        st[2] = last_full;
        st[3] = (double)state;
    }
}

}  // namespace ciao

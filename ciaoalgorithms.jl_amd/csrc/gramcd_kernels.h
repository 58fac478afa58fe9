// gramcd_kernels.h -- cyclic coordinate descent with covariance updates for the d-space lasso (ciao_gram_cd):
//      min_x (c/2)(x'G x - 2 u'x + sum b^2) + mu ||x||_1          tau = mu / c
// on a precomputed Gram matrix, K models (K values of tau, K warm starts) in one launch.  A strictly sequential chain per model: one
// workgroup owns one model, grid = K, and nothing crosses between workgroups.  G is read only, ROW j for coordinate j.
//
// The method, to the bit (host_route.host_gram_cd is its numpy mirror; every product is rounded before it is added: contraction is off):
//   start      r = u; for j ascending with x_j != 0:  r_i <- r_i - (x_j G_ji)  for all i
//   update(j)  rho = r_j + (G_jj x_j);  a = |rho| - tau;  x+ = 0 if a <= 0, else copysign(a, rho) inv_j  (a NaN goes through: a NaN in rho
//              makes x+ NaN);  delta = x+ - x_j;  delta not finite: the model ends with state 2, x_j unchanged;  delta != 0:
//              r_i <- r_i - (delta G_ji) for all i, then x_j <- x+;  change = G_jj (delta delta);  the support changes if exactly one of
//              x_j, x+ is 0
//   sweeps     full: update(j) for j = 0 .. d-1;  active: only the j with x_j != 0 at their turn
//   loop       full sweep; largest change <= tol and support unchanged: state 1.  Otherwise active sweeps until one has largest change
//              <= tol, then a full sweep again.  Every sweep counts against max_sweeps; the budget spent: state 0.
// The largest change is a max: exact in any order.  No sum over coordinates is formed anywhere.
//
// The kernel.  x, r and the diagonal of G live in LDS (3 d doubles, d rounded up to even: 96 KiB at d = 4096).  The decision for coordinate
// j (rho, x+, delta) is computed by EVERY thread from LDS broadcasts made wave-uniform, so every branch is a scalar branch and every
// barrier is reached by all.  Element i of r belongs to ONE thread for the whole launch (thread i % BLOCK with element loads; pair i / 2
// to thread (i / 2) % BLOCK with 16-byte loads), which reads G_ji and rewrites r_i: per element one product, one subtraction, whatever
// the block size or the load kind -- the bits do not depend on either.  Coordinates that cannot move (a <= 0 and x_j = 0; in an active
// sweep x_j = 0) cost no row, no barrier and no turn of their own: every wave tests 64 of them at once, a lane each, and a ballot names
// the first that can.  For that one the row is requested first, then delta is formed; a non-zero delta costs TWO
// barriers: one before r is rewritten (a slower thread may still be deciding an earlier coordinate from the r of before), one after (the
// next decision reads the new r).  The row's latency covers the first.
//
// What is never read: columns [d, ldg) of a row of G, anything beyond u[d-1], inv[d-1], tau[K-1], row k of X beyond its d elements.
// 16-byte loads where the base of G and ldg allow and the pair lies wholly in [0, d); element loads otherwise.
#pragma once

#include "ciao_common.h"

namespace ciao {

constexpr int GRAMCD_MAX_D = 4096;
constexpr int GRAMCD_MAX_K = 4096;
constexpr int GRAMCD_MAX_SWEEPS = 1024;
constexpr int GRAMCD_SMALL_BLOCK = 256;     // d <= GRAMCD_SMALL_D
constexpr int GRAMCD_LARGE_BLOCK = 1024;
constexpr int GRAMCD_SMALL_D = 1024;
constexpr int GRAMCD_PER_THREAD = 4;        // elements of r a thread owns at most: GRAMCD_SMALL_D / 256 = GRAMCD_MAX_D / 1024

struct GramCdPlan {
    int block;       // threads per workgroup
    int vec16;       // 1: 16-byte row loads
    int grid;        // K
    int lds;         // bytes of dynamic LDS
};

// a pure function of (d, ldg, the alignment of G, K)
inline GramCdPlan gramcd_plan(int64_t d, int64_t ldg, bool g_aligned16, int64_t K)
{
    GramCdPlan pl;
    pl.block = d <= GRAMCD_SMALL_D ? GRAMCD_SMALL_BLOCK : GRAMCD_LARGE_BLOCK;
    pl.vec16 = g_aligned16 && ldg % 2 == 0;
    pl.grid = (int)K;
    pl.lds = (int)(3 * ((d + 1) & ~(int64_t)1) * (int64_t)sizeof(double));
    return pl;
}

struct GramCdArgs {
    const double *G;
    const double *u;
    const double *inv;
    const double *tau;
    double *X;
    double *R;       // or NULL
    double *stat;    // K x 4: sweeps, non-zero updates, largest change of the last full sweep, state
    int64_t ldg, ldx, ldr;
    double tol;
    int d;
    int max_sweeps;
};

// the value lane 0 holds, as a wave-uniform double (every lane holds the same bits here: what it buys is scalar branches)
__device__ __forceinline__ double gramcd_uniform(double v)
{
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
    const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// the value lane `lane` (wave-uniform) holds, as a wave-uniform double
__device__ __forceinline__ double gramcd_lane(double v, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// the elements of row `row` this thread owns, into registers.  VEC: W = 2 and slot m holds elements 2 q, 2 q + 1 with q = t + m BLOCK.
template <int BLOCK, bool VEC>
__device__ __forceinline__ void gramcd_load_row(const double *__restrict__ row, int d, int t, double (&g)[GRAMCD_PER_THREAD])
{
    if constexpr (VEC) {
#pragma unroll
        for (int m = 0; m < GRAMCD_PER_THREAD / 2; ++m) {
            const int i = 2 * (t + m * BLOCK);
            if (i + 1 < d) {
                const double2 v = *reinterpret_cast<const double2 *>(row + i);
                g[2 * m] = v.x;
                g[2 * m + 1] = v.y;
            } else {
                g[2 * m] = i < d ? row[i] : 0.0;
                g[2 * m + 1] = 0.0;
            }
        }
    } else {
#pragma unroll
        for (int m = 0; m < GRAMCD_PER_THREAD; ++m) {
            const int i = t + m * BLOCK;
            g[m] = i < d ? row[i] : 0.0;
        }
    }
}

// r_i <- r_i - (s g_i) for the elements this thread owns
template <int BLOCK, bool VEC>
__device__ __forceinline__ void gramcd_axpy(double *__restrict__ r, int d, int t, double s, const double (&g)[GRAMCD_PER_THREAD])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int m = 0; m < GRAMCD_PER_THREAD; ++m) {
        const int i = VEC ? 2 * (t + (m >> 1) * BLOCK) + (m & 1) : t + m * BLOCK;
        if (i < d) {
            const double p = s * g[m];
            r[i] = r[i] - p;
        }
    }
}

template <int BLOCK, bool VEC>
__global__ __launch_bounds__(BLOCK) void gramcd_kernel(GramCdArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char gramcd_smem[];
    const int d = a.d;
    const int dp = (d + 1) & ~1;
    double *x = reinterpret_cast<double *>(gramcd_smem);
    double *r = x + dp;
    double *diag = r + dp;
    const int t = (int)threadIdx.x;
    const int k = (int)blockIdx.x;
    const double *__restrict__ G = a.G;
    double *Xk = a.X + (int64_t)k * a.ldx;
    const double tau = a.tau[k];
    const double tol = a.tol;
    double g[GRAMCD_PER_THREAD];

    for (int i = t; i < d; i += BLOCK) {
        x[i] = Xk[i];
        r[i] = a.u[i];
        diag[i] = G[(int64_t)i * a.ldg + i];
    }
    __syncthreads();
    // start: r = u - G x, one row per non-zero of the warm start, in ascending order.  x does not change here and a thread touches
    // its own elements of r only: no barrier until the end.
    for (int j = 0; j < d; ++j) {
        {
            const int jl = j + (t & 63);      // the next non-zero of the warm start, 64 coordinates at a time (as in the sweeps below)
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

    int sweeps = 0, state = 0;
    double nupd = 0.0, last_full = 0.0;
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
            // the first coordinate from j on that can move, 64 at a time: lane l of EVERY wave forms the decision's own test for
            // coordinate j + l (r does not change between two updates, so this is the test its turn would make), and the ballot is
            // the same wave-uniform mask in every wave.  Coordinates that cannot move are passed over without a turn of their own;
            // the one that can takes its x_j, r_j and G_jj from the lane that tested it.
            const int jl = j + (t & 63);
            double xl = 0.0, rl = 0.0, gl = 0.0;
            bool can = false;
            if (jl < d) {
                xl = x[jl];
                rl = r[jl];
                gl = diag[jl];
                can = xl != 0.0 || (!active && !(fabs(rl + gl * xl) - tau <= 0.0));
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
            const double rho = rj + gjj * xj;
            const double av = fabs(rho) - tau;
            if (av <= 0.0 && xj == 0.0)
                continue;                                   // x+ = 0 = x_j: nothing moves
            gramcd_load_row<BLOCK, VEC>(G + (int64_t)j * a.ldg, d, t, g);   // requested before delta is known: G is read only
            const double xp = av <= 0.0 ? 0.0 : copysign(av, rho) * a.inv[j];
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
    if (t == 0) {
        double *st = a.stat + 4 * (int64_t)k;
        st[0] = (double)sweeps;
        st[1] = nupd;
        st[2] = last_full;
        st[3] = (double)state;
    }
}

}  // namespace ciao

// api_synth.hip -- data and indices made where they are used: synthetic rows and targets on the device (a benchmark's N x d matrix
// never crosses the host), the index stream on the device, and the host sampler of batches without replacement.

#include <algorithm>
#include <vector>

#include "api_internal.h"

namespace ciao {

// ---- synthetic data -------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
// standard normal keyed by (seed, row, col): Box-Muller on two 32-bit uniforms of one 64-bit hash
__device__ __forceinline__ float normal_at(uint64_t seed, uint64_t row, uint64_t col)
{
    uint64_t h = mix64(seed + 0x9E3779B97F4A7C15ULL * (row * 0x100000001B3ULL + col + 1));
    h = mix64(h ^ (row << 1) ^ 0xD1B54A32D192ED03ULL);
    const float u1 = ((float)(uint32_t)(h >> 32) + 1.0f) * (1.0f / 4294967296.0f);   // (0,1]
    const float u2 = (float)(uint32_t)h * (1.0f / 4294967296.0f);                    // [0,1)
    return sqrtf(-2.0f * __logf(u1)) * __cosf(6.28318530717958647692f * u2);
}

template <typename T>
__global__ void __launch_bounds__(256)
    synth_normal_kernel(T *out, int64_t nrows, int64_t d, int64_t ld, int64_t row0, uint64_t seed, T scale)
{
    const int64_t total = nrows * d;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t r = t / d, c = t - r * d;
        out[r * ld + c] = scale * (T)normal_at(seed, (uint64_t)(row0 + r), (uint64_t)c);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) synth_targets_kernel(const T *A, int64_t N, int64_t d, int64_t ld, const T *x_true,
                                                           T noise, int labels, int64_t row0, uint64_t seed, T *b)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < N; i += nw) {
        const T *ap = A + i * ld;
        T dot = T(0);
        for (int64_t e = lane; e < d; e += WAVE) dot += ap[e] * x_true[e];
        dot = wave_allsum(dot);
        T v = dot + noise * (T)normal_at(seed ^ 0xABCDEF0123456789ULL, (uint64_t)(row0 + i), 0xFFFFFFFFULL);
        if (labels) v = v >= T(0) ? T(1) : T(-1);
        if (lane == 0) b[i] = v;
    }
}

template <typename T>
static void synth_normal_t(ciao_ctx *ctx, int64_t grid, void *out, int64_t nrows, int64_t d, int64_t ld, int64_t row0, uint64_t seed, double scale)
{
    hipLaunchKernelGGL((synth_normal_kernel<T>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, (T *)out, nrows, d, ld, row0, seed, (T)scale);
}

template <typename T>
static void synth_targets_t(ciao_ctx *ctx, int64_t grid, const ciao_problem *p, const void *x_true, double noise, int32_t labels, int64_t row0,
                            uint64_t seed, void *b_out)
{
    hipLaunchKernelGGL((synth_targets_kernel<T>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, (const T *)p->A, p->N, p->d, p->ld,
                       (const T *)x_true, (T)noise, (int)labels, row0, seed, (T *)b_out);
}

}  // namespace ciao

using namespace ciao;

extern "C" {

int32_t ciao_synth_normal(ciao_ctx *ctx, int32_t dtype, void *out, int64_t nrows, int64_t d, int64_t ld, int64_t row0,
                          uint64_t seed, double scale)
{
    CIAO_ENTER(ctx);
    CIAO_REQUIRE(ctx && (out || nrows == 0), "ctx or out is NULL");
    CIAO_REQUIRE(dtype == CIAO_F32 || dtype == CIAO_F64, "bad dtype %d", dtype);
    CIAO_REQUIRE(nrows >= 0 && d >= 1 && ld >= d, "bad shape");
    if (nrows == 0) return CIAO_OK;
    const int64_t total = nrows * d;
    int64_t grid = (total + 255) / 256;
    if (grid > (int64_t)ctx->num_cu * 32) grid = (int64_t)ctx->num_cu * 32;
    DISPATCH(dtype, synth_normal_t, ctx, grid, out, nrows, d, ld, row0, seed, scale);
    CIAO_HIP(hipGetLastError());
    return CIAO_OK;
}

int32_t ciao_synth_targets(ciao_ctx *ctx, const ciao_problem *p, const void *x_true, double noise, int32_t labels,
                           int64_t row0, uint64_t seed, void *b_out)
{
    CIAO_ENTER(ctx);
    CIAO_REQUIRE(ctx && p && x_true && (b_out || p->N == 0), "NULL argument");
    CIAO_REQUIRE(p->dtype == CIAO_F32 || p->dtype == CIAO_F64, "bad dtype");
    CIAO_REQUIRE(p->N >= 0 && p->d >= 1 && p->ld >= p->d && (p->A || p->N == 0), "bad problem shape");
    if (p->N == 0) return CIAO_OK;
    int64_t grid = (p->N + 3) / 4;
    if (grid > (int64_t)ctx->num_cu * 8) grid = (int64_t)ctx->num_cu * 8;
    DISPATCH(p->dtype, synth_targets_t, ctx, grid, p, x_true, noise, labels, row0, seed, b_out);
    CIAO_HIP(hipGetLastError());
    return CIAO_OK;
}

// ---- host helper: n x sample(1:N, r, replace=false) from the splitmix64 index stream (sampling.py is its reference) ----
namespace {
inline uint64_t splitmix_at(uint64_t seed, uint64_t k)   // output number k (0-based) of the stream: counter-based
{
    uint64_t z = seed + (k + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void __launch_bounds__(256) sample_uniform_kernel(uint64_t seed, uint64_t pos, uint64_t N, int64_t m, int64_t *out)
{
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < m; k += (int64_t)gridDim.x * 256) {
        uint64_t z = seed + (pos + (uint64_t)k + 1) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        out[k] = (int64_t)(((z >> 32) * N) >> 32);
    }
}
}  // namespace

int32_t ciao_sample_uniform(ciao_ctx *ctx, uint64_t seed, uint64_t pos, int64_t N, int64_t m, int64_t *out_dev)
{
    CIAO_ENTER(ctx);
    CIAO_REQUIRE(N > 0 && N < (1ll << 32) && m >= 0 && (out_dev || m == 0), "need 0 < N < 2^32, m >= 0 and an output array");
    if (m == 0) return CIAO_OK;
    const int64_t grid = std::min<int64_t>((m + 255) / 256, (int64_t)ctx->num_cu * 8);
    hipLaunchKernelGGL(sample_uniform_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, seed, pos, (uint64_t)N, m, out_dev);
    CIAO_HIP(hipGetLastError());
    return CIAO_OK;
}

int32_t ciao_sample_batches(uint64_t seed, uint64_t pos, int64_t N, int64_t r, int64_t n, int64_t *out_host,
                            uint64_t *pos_out_host)
{
    CIAO_REQUIRE(N > 0 && N < (1ll << 32) && r >= 1 && 2 * r <= N && n >= 0, "need 0 < N < 2^32, r >= 1, 2r <= N, n >= 0");
    CIAO_REQUIRE((out_host || n == 0) && pos_out_host, "NULL output");
    // open-addressing set of the indices held by the current batch: one 8-byte word per slot = (batch tag << 32) | index, so
    // a probe touches one cache line and nothing is cleared between batches (a stale tag reads as an empty slot)
    uint64_t cap = 16;
    while (cap < (uint64_t)(2 * r)) cap <<= 1;
    std::vector<uint64_t> slots;
    try {
        slots.assign(cap, 0);
    } catch (...) {   // nothing may unwind through the C ABI
        set_error("out of host memory (%llu hash slots)", (unsigned long long)cap);
        return CIAO_ERR_ALLOC;
    }
    uint32_t tag = 0;
    for (int64_t t = 0; t < n; ++t) {
        if (++tag == 0) {   // 2^32 batches later the tags would repeat: start over with clean slots
            std::fill(slots.begin(), slots.end(), 0);
            tag = 1;
        }
        int64_t *out = out_host + t * r;
        int64_t have = 0;
        while (have < r) {
            const int64_t need = r - have;   // one round: as many candidates as are still missing (>= 1)
            for (int64_t c = 0; c < need; ++c) {
                const uint64_t u = splitmix_at(seed, pos++) >> 32;
                const uint64_t v = (u * (uint64_t)N) >> 32;   // uniform in 0..N-1, the rule of IndexStream.rand_indices
                const uint64_t word = ((uint64_t)tag << 32) | v;
                uint64_t h = ((v * 0x9E3779B97F4A7C15ull) >> 24) & (cap - 1);
                bool seen = false;
                while ((slots[h] >> 32) == tag) {
                    if (slots[h] == word) {
                        seen = true;
                        break;
                    }
                    h = (h + 1) & (cap - 1);
                }
                if (!seen) {
                    slots[h] = word;
                    out[have++] = (int64_t)v;
                }
            }
        }
    }
    *pos_out_host = pos;
    return CIAO_OK;
}

}  // extern "C"

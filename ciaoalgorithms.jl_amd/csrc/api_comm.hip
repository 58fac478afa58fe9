// api_comm.hip -- what a context knows of the other ranks: the all-reduce hook (the host's, RCCL called directly, or the library's own
// peer mailboxes, peer_kernels.h), the shard table of a row-sharded problem, and the IPC helpers that map another rank's memory.

#include <dlfcn.h>
#include <string.h>

#include "api_internal.h"
#include "peer_kernels.h"

namespace ciao {

int32_t check_shards(const ciao_ctx *ctx, const ciao_problem *p, bool need_table)
{
    const ciao_shard_table &sh = ctx->shards;
    if (sh.nshards == 0) return CIAO_OK;
    CIAO_REQUIRE(sh.row0[sh.nshards] == p->N_total, "the shard table covers %lld rows but the problem has N_total = %lld",
                 (long long)sh.row0[sh.nshards], (long long)p->N_total);
    if (sh.owner && p->loss != CIAO_LOSS_ZERO)
        for (int k = 0; k < sh.nshards; ++k) {
            if (sh.row0[k + 1] == sh.row0[k]) continue;
            CIAO_REQUIRE(sh.A[k] && sh.b[k], "shard %d has rows but no data pointers on the chain owner", k);
            CIAO_REQUIRE(!need_table || sh.table[k], "shard %d has no table pointer on the chain owner (SAGA)", k);
        }
    return CIAO_OK;
}

// the two halves of a peer reduction as kernels of their own
template <typename T>
static int32_t peer_reduce_t(void *buf, int64_t count, const PeerDev &pd, hipStream_t stream)
{
    const unsigned grid = (unsigned)((count + 255) / 256);
    hipLaunchKernelGGL((peer_send_kernel<T>), dim3(grid), dim3(256), 0, stream, (const T *)buf, count, pd);
    hipLaunchKernelGGL((peer_recv_kernel<T>), dim3(grid), dim3(256), 0, stream, (T *)buf, count, pd);
    return hipGetLastError() == hipSuccess ? 0 : CIAO_ERR_HIP;
}

}  // namespace ciao

using namespace ciao;

extern "C" {

int32_t ciao_ctx_set_allreduce(ciao_ctx *ctx, ciao_allreduce_fn fn, void *user)
{
    CIAO_ENTER(ctx);
    ctx->hook = fn;
    ctx->hook_user = user;
    return CIAO_OK;
}

// the library's own all-reduce hook: RCCL called directly (no host-language callback per reduction)
static int32_t rccl_hook(void *user, void *buf, int64_t count, int32_t dtype, void *stream)
{
    ciao_ctx *ctx = static_cast<ciao_ctx *>(user);
    const int nccl_type = (dtype == CIAO_F64) ? 8 : 7;   // ncclFloat64 / ncclFloat32 (rccl.h)
    const int r = ctx->rccl_allreduce(buf, buf, (size_t)count, nccl_type, /*ncclSum*/ 0, ctx->rccl_comm, (hipStream_t)stream);
    if (r != 0) {
        set_error("ncclAllReduce failed with %d (%s)", r, ctx->rccl_errstr ? ctx->rccl_errstr(r) : "?");
        return r;
    }
    return 0;
}

int32_t ciao_ctx_set_rccl(ciao_ctx *ctx, void *comm, const char *librccl_path)
{
    CIAO_ENTER(ctx);
    if (!comm) {
        if (ctx->hook == rccl_hook) {
            ctx->hook = nullptr;
            ctx->hook_user = nullptr;
        }
        ctx->rccl_comm = nullptr;
        return CIAO_OK;
    }
    const char *path = librccl_path ? librccl_path : "librccl.so";
    void *h = dlopen(path, RTLD_NOW | RTLD_LOCAL);   // the same handle again if the host has loaded it already
    if (!h) {
        set_error("cannot load RCCL from '%s': %s", path, dlerror());
        return CIAO_ERR_ARG;
    }
    void *f = dlsym(h, "ncclAllReduce");
    if (!f) {
        set_error("'%s' has no ncclAllReduce", path);
        dlclose(h);
        return CIAO_ERR_ARG;
    }
    if (ctx->rccl_lib && ctx->rccl_lib != h) dlclose(ctx->rccl_lib);
    ctx->rccl_lib = h;
    ctx->rccl_allreduce = reinterpret_cast<int (*)(const void *, void *, size_t, int, int, void *, hipStream_t)>(f);
    ctx->rccl_errstr = reinterpret_cast<const char *(*)(int)>(dlsym(h, "ncclGetErrorString"));
    ctx->rccl_comm = comm;
    ctx->hook = rccl_hook;
    ctx->hook_user = ctx;
    return CIAO_OK;
}

// ---- one-shot peer all-reduce (peer_kernels.h) ---------------------------------------------------------------------------
static int64_t peer_slot_bytes_for(int64_t max_elems) { return ((max_elems * 8 + 255) / 256) * 256; }

int32_t ciao_peer_mailbox_create(ciao_ctx *ctx, int64_t max_elems, void **mailbox_out, int64_t *bytes_out)
{
    CIAO_ENTER(ctx);
    CIAO_REQUIRE(mailbox_out && max_elems >= 1, "NULL argument or max_elems < 1");
    const size_t bytes = (size_t)(PEER_HDR + 2 * PEER_MAX * peer_slot_bytes_for(max_elems));
    void *m = nullptr;
    // fine-grained device memory: written by the other GPUs over xGMI while this GPU's kernels read it
    CIAO_HIP(hipExtMallocWithFlags(&m, bytes, hipDeviceMallocFinegrained));
    CIAO_HIP(hipMemset(m, 0, bytes));
    CIAO_HIP(hipDeviceSynchronize());
    *mailbox_out = m;
    if (bytes_out) *bytes_out = (int64_t)bytes;
    return CIAO_OK;
}

int32_t ciao_peer_mailbox_destroy(ciao_ctx *ctx, void *mailbox)
{
    CIAO_ENTER(ctx);
    if (mailbox) CIAO_HIP(hipFree(mailbox));
    return CIAO_OK;
}

// the library's peer hook on an arbitrary buffer (chain-owner broadcasts, bench): the two halves as kernels of their own
static int32_t peer_hook(void *user, void *buf, int64_t count, int32_t dtype, void *stream)
{
    ciao_ctx *ctx = static_cast<ciao_ctx *>(user);
    if (count > ctx->peer_max_elems) {
        set_error("the peer mailboxes hold %lld elements, this reduction has %lld", (long long)ctx->peer_max_elems, (long long)count);
        return CIAO_ERR_ARG;
    }
    return DISPATCH(dtype, peer_reduce_t, buf, count, peer_dev(ctx), (hipStream_t)stream);
}

int32_t ciao_ctx_set_peers(ciao_ctx *ctx, int32_t rank, int32_t world, void *const *mailboxes, int64_t max_elems)
{
    CIAO_ENTER(ctx);
    if (!mailboxes || world <= 0) {   // off: what the peers displaced (a user hook, the RCCL communicator) is back in place
        if (ctx->hook == peer_hook) {
            ctx->hook = ctx->peer_saved ? ctx->peer_saved_hook : nullptr;
            ctx->hook_user = ctx->peer_saved ? ctx->peer_saved_user : nullptr;
        }
        ctx->peer_saved = false;
        ctx->peer_world = 0;
        return CIAO_OK;
    }
    CIAO_REQUIRE(world >= 1 && world <= PEER_MAX && rank >= 0 && rank < world, "world must be in 1..%d and rank in [0, world) (got %d, %d)",
                 PEER_MAX, world, rank);
    CIAO_REQUIRE(max_elems >= 1, "max_elems < 1");
    for (int r = 0; r < world; ++r) CIAO_REQUIRE(mailboxes[r], "mailbox %d is NULL", r);
    if (!ctx->peer_counter) {
        CIAO_HIP(hipMalloc((void **)&ctx->peer_counter, sizeof(unsigned int)));
        CIAO_HIP(hipMemset(ctx->peer_counter, 0, sizeof(unsigned int)));
    }
    for (int r = 0; r < PEER_MAX; ++r) ctx->peer_mail[r] = r < world ? static_cast<unsigned char *>(mailboxes[r]) : nullptr;
    ctx->peer_world = world;
    ctx->peer_rank = rank;
    // The sequence number lives WITH the mailboxes, so that a group that is set again (off and on; another ctx) continues instead of
    // restarting at 1 and meeting flags of an earlier life that happen to equal the new numbers.  It is read from THIS
    // RANK'S OWN flag in its own mailbox -- the two words (one per parity) that only this rank's kernels ever write: every rank made
    // the same reductions, so every rank reads the same number, and no peer can change what is read.  (Until round 5 the maximum over
    // ALL ranks' flags was taken: a rank that finished set_peers first and started reduction last+1 wrote its flag into a slower
    // rank's mailbox before that rank read it, the slow rank started at last+1 and the two stayed one number -- one parity -- apart
    // until both timed out: ADVICE r4.)  Fresh mailboxes read 0.
    {
        CIAO_HIP(hipStreamSynchronize(ctx->stream));
        unsigned int flags[2 * PEER_MAX * 16];
        static_assert(sizeof flags == PEER_HDR, "the header is two parities of eight 64-byte flag lines");
        CIAO_HIP(hipMemcpy(flags, mailboxes[rank], sizeof flags, hipMemcpyDeviceToHost));
        unsigned int last = 0;
        for (int par = 0; par < 2; ++par) last = flags[(par * PEER_MAX + rank) * 16] > last ? flags[(par * PEER_MAX + rank) * 16] : last;
        ctx->peer_seq = last;
    }
    ctx->peer_max_elems = max_elems;
    ctx->peer_slot_bytes = peer_slot_bytes_for(max_elems);
    if (ctx->hook != peer_hook) {   // remember what is displaced (set twice in a row: the first one's memory stands)
        ctx->peer_saved_hook = ctx->hook;
        ctx->peer_saved_user = ctx->hook_user;
        ctx->peer_saved = true;
    }
    ctx->hook = peer_hook;
    ctx->hook_user = ctx;
    return CIAO_OK;
}

int32_t ciao_peer_allreduce(ciao_ctx *ctx, int32_t dtype, int64_t count, void *buf)
{
    CIAO_ENTER(ctx);
    CIAO_REQUIRE(ctx->peer_world > 0, "no peers are set (ciao_ctx_set_peers)");
    CIAO_REQUIRE(buf && count >= 1 && (dtype == CIAO_F64 || dtype == CIAO_F32), "NULL buffer, count < 1 or unknown dtype");
    const int32_t st = peer_hook(ctx, buf, count, dtype, (void *)ctx->stream);
    return st == 0 ? CIAO_OK : (st < 0 ? st : CIAO_ERR_HOOK);
}

int32_t ciao_ctx_set_shards(ciao_ctx *ctx, const ciao_shard_table *shards)
{
    CIAO_ENTER(ctx);
    ctx->rowdot_A = nullptr;
    if (!shards) {
        ctx->shards = ciao_shard_table{};
        return CIAO_OK;
    }
    CIAO_REQUIRE(shards->nshards >= 1 && shards->nshards <= CIAO_MAX_SHARDS, "nshards must be in 1..%d (got %d)", CIAO_MAX_SHARDS,
                 shards->nshards);
    CIAO_REQUIRE(shards->row0[0] == 0, "row0[0] must be 0");
    for (int k = 0; k < shards->nshards; ++k)
        CIAO_REQUIRE(shards->row0[k + 1] >= shards->row0[k], "row0 must be non-decreasing (shard %d)", k);
    ctx->shards = *shards;
    return CIAO_OK;
}

int32_t ciao_ipc_export(const void *dev_ptr, void *handle_out, int64_t *offset_out)
{
    CIAO_REQUIRE(dev_ptr && handle_out && offset_out, "NULL argument");
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "the ABI documents 64-byte handles");
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    CIAO_HIP(hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)dev_ptr));
    hipIpcMemHandle_t h;
    CIAO_HIP(hipIpcGetMemHandle(&h, (void *)base));
    memcpy(handle_out, &h, sizeof h);
    *offset_out = (int64_t)((const char *)dev_ptr - (const char *)base);
    return CIAO_OK;
}

int32_t ciao_ipc_open(const void *handle, int64_t offset, void **dev_ptr_out)
{
    CIAO_REQUIRE(handle && dev_ptr_out && offset >= 0, "NULL argument or negative offset");
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof h);
    void *base = nullptr;
    CIAO_HIP(hipIpcOpenMemHandle(&base, h, hipIpcMemLazyEnablePeerAccess));
    *dev_ptr_out = (char *)base + offset;
    return CIAO_OK;
}

int32_t ciao_ipc_close(void *dev_ptr, int64_t offset)
{
    CIAO_REQUIRE(dev_ptr && offset >= 0, "NULL argument or negative offset");
    CIAO_HIP(hipIpcCloseMemHandle((char *)dev_ptr - offset));
    return CIAO_OK;
}

}  // extern "C"

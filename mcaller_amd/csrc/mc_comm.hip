// mc_comm.hip -- RCCL, loaded on first use (the library is only needed by multi-GPU jobs): the communicator of a context and the
// all-reduce of its per-site counts.  Host code only.
#include "mc_ctx.h"

#include <dlfcn.h>
#include <rccl/rccl.h>
namespace {
struct Rccl {
    void *h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl g_rccl;

int rccl_load() {
    if (g_rccl.h) return 0;
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) {
        mc_set_error("cannot load librccl.so: %s", dlerror());
        return -15;
    }
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(h, "ncclCommInitRank");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(h, "ncclCommDestroy");
    g_rccl.AllReduce = (decltype(g_rccl.AllReduce))dlsym(h, "ncclAllReduce");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.CommDestroy || !g_rccl.AllReduce || !g_rccl.GetErrorString) {
        mc_set_error("librccl.so lacks an expected symbol");
        dlclose(h);
        return -15;
    }
    g_rccl.h = h;
    return 0;
}
}  // namespace

#define RCCL_TRY(expr)                                                                              \
    do {                                                                                            \
        ncclResult_t _r = (expr);                                                                   \
        if (_r != ncclSuccess) {                                                                    \
            mc_set_error("%s failed: %s", #expr, g_rccl.GetErrorString(_r));                        \
            return -15;                                                                             \
        }                                                                                           \
    } while (0)

static_assert(sizeof(ncclUniqueId) == MC_UNIQUE_ID_BYTES, "ncclUniqueId size");

extern "C" int mc_comm_available(void) { return rccl_load(); }

extern "C" int mc_comm_unique_id(uint8_t *out) {
    if (int rc = rccl_load()) return rc;
    ncclUniqueId id;
    RCCL_TRY(g_rccl.GetUniqueId(&id));
    memcpy(out, &id, sizeof(id));
    return 0;
}

extern "C" int mc_comm_init(mc_ctx *c, int32_t world, int32_t rank, const uint8_t *unique_id) {
    HIP_TRY(hipSetDevice(c->device));
    if (world < 1 || rank < 0 || rank >= world) {
        mc_set_error("mc_comm_init: rank %d of %d", rank, world);
        return -12;
    }
    if (int rc = rccl_load()) return rc;
    mc_comm_destroy(c);
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof(id));
    ncclComm_t comm = nullptr;
    RCCL_TRY(g_rccl.CommInitRank(&comm, world, id, rank));
    c->comm = comm;
    c->comm_world = world;
    return 0;
}

extern "C" int mc_comm_destroy(mc_ctx *c) {
    if (c && c->comm && g_rccl.h) {
        (void)hipSetDevice(c->device);
        (void)g_rccl.CommDestroy((ncclComm_t)c->comm);
    }
    if (c) c->comm = nullptr;
    return 0;
}

extern "C" int mc_site_allreduce(mc_ctx *c, int32_t *n_meth, int32_t *n_total, int64_t *first_row, float *ms) {
    HIP_TRY(hipSetDevice(c->device));
    if (!c->site_cnt) {
        mc_set_error("mc_site_allreduce: call mc_site_counts first");
        return -12;
    }
    const int64_t ns = c->site_n;
    if (ms) *ms = 0.f;
    if (c->comm && c->comm_world > 1 && ns > 0) {
        HIP_TRY(hipEventRecord(c->ev[0], c->site_stream));
        RCCL_TRY(g_rccl.AllReduce(c->site_cnt, c->site_cnt, (size_t)ns * 2, ncclInt32, ncclSum, (ncclComm_t)c->comm, c->site_stream));
        RCCL_TRY(g_rccl.AllReduce(c->site_first, c->site_first, (size_t)ns, ncclInt64, ncclMin, (ncclComm_t)c->comm, c->site_stream));
        HIP_TRY(hipEventRecord(c->ev[1], c->site_stream));
        HIP_TRY(hipStreamSynchronize(c->site_stream));
        if (ms) HIP_TRY(hipEventElapsedTime(ms, c->ev[0], c->ev[1]));
    }
    return mc_site_counts_fetch(c, n_meth, n_total, first_row);
}

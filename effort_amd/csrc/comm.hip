// Multi-GPU: one process per GPU, RCCL over xGMI (the reference is single-device, helpers/gpu.swift:36-38).  The only unit that sees rccl.h.
#include <dlfcn.h>
#include <rccl/rccl.h>          // types only: the library is opened when the first communicator is asked for (rccl(), below)

#include "host.h"

using namespace effort;

// RCCL is bound at RUN time, when the first communicator is asked for: a single-GPU host needs no librccl to load this library,
// and a process that has one mapped already (PyTorch-ROCm brings its own copy) gets THAT one -- dlopen by soname returns the copy
// already in the process -- so two RCCLs never meet in one address space; a plain C / Swift host gets the system ROCm's.
struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
};
static const RcclApi& rccl() {
    static RcclApi api = [] {
        RcclApi a;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
            a.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (a.lib) break;
        }
        if (!a.lib) return a;
        a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(a.lib, "ncclGetUniqueId"));
        a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(a.lib, "ncclCommInitRank"));
        a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(a.lib, "ncclCommDestroy"));
        a.AllGather = reinterpret_cast<decltype(a.AllGather)>(dlsym(a.lib, "ncclAllGather"));
        a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(a.lib, "ncclGetErrorString"));
        a.ok = a.GetUniqueId && a.CommInitRank && a.CommDestroy && a.AllGather && a.GetErrorString;
        return a;
    }();
    return api;
}

extern "C" int effort_comm_unique_id(void* id_out) {
    if (!id_out) return EFFORT_ERR_ARG;
    static_assert(sizeof(ncclUniqueId) == EFFORT_COMM_ID_BYTES, "effort_hip.h: EFFORT_COMM_ID_BYTES");
    if (!rccl().ok) return EFFORT_ERR_COMM;
    return rccl().GetUniqueId(static_cast<ncclUniqueId*>(id_out)) == ncclSuccess ? EFFORT_OK : EFFORT_ERR_COMM;
}
extern "C" int effort_comm_create(effort_ctx* c, int rank, int world, const void* id) {
    if (!c || !id || world < 1 || rank < 0 || rank >= world) return fail(c, EFFORT_ERR_ARG, "comm_create: bad argument");
    if (c->comm) return fail(c, EFFORT_ERR_ARG, "comm_create: the context has a communicator already");
    hipSetDevice(c->device);
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    if (!rccl().ok) return fail(c, EFFORT_ERR_COMM, "comm_create: librccl.so could not be opened (dlopen) -- multi-GPU needs RCCL");
    const ncclResult_t r = rccl().CommInitRank(&c->comm, world, uid, rank);
    if (r != ncclSuccess) { c->comm = nullptr; snprintf(c->err, sizeof(c->err), "ncclCommInitRank: %s", rccl().GetErrorString(r)); return EFFORT_ERR_COMM; }
    c->commRank = rank; c->commWorld = world;
    return EFFORT_OK;
}
// effort_destroy's part: the streams are synchronised already.
void comm_release(effort_ctx* c) {
    if (c->comm) rccl().CommDestroy(c->comm);
    c->comm = nullptr;
}
extern "C" int effort_comm_destroy(effort_ctx* c) {
    if (!c) return EFFORT_ERR_ARG;
    if (c->comm) { hipSetDevice(c->device); effort_sync(c); comm_release(c); c->commRank = 0; c->commWorld = 1; }
    return EFFORT_OK;
}
extern "C" int effort_comm_rank(effort_ctx* c) { return c ? c->commRank : EFFORT_ERR_ARG; }
extern "C" int effort_comm_world(effort_ctx* c) { return c ? c->commWorld : EFFORT_ERR_ARG; }
// All-gather of the ranks' output slices on the context's stream, after the multiplies that wrote them (the lanes are joined):
// recv = [world][count] f32.  send may be recv + rank*count (in place).
extern "C" int effort_allgather_outputs(effort_ctx* c, const float* send, float* recv, int count) {
    if (!c || !send || !recv || count < 1) return fail(c, EFFORT_ERR_ARG, "allgather_outputs: bad argument");
    if (!c->comm) return fail(c, EFFORT_ERR_ARG, "allgather_outputs: no communicator (effort_comm_create)");
    JOIN_TRY(c);
    const ncclResult_t r = rccl().AllGather(send, recv, (size_t)count, ncclFloat, c->comm, c->stream);
    if (r != ncclSuccess) { snprintf(c->err, sizeof(c->err), "ncclAllGather: %s", rccl().GetErrorString(r)); return EFFORT_ERR_COMM; }
    return EFFORT_OK;
}

// capi_comm.cpp -- see capi_internal.h
#include "multi_internal.h"
#include <dlfcn.h>

// ---- multi-GPU: one process drives ndev devices (the reference's localisation node is one process,
// rmcl_localization.cpp:482-552); RCCL communicators of ncclCommInitAll, resolved with dlopen so that single-GPU users never
// load the library ---------------------------------------------------------------------------------------------
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
};
static RcclApi g_rccl;

static bool rccl_load(std::string& err) {
  static std::mutex mtx;   // two threads may create their first communicator at the same time
  std::lock_guard<std::mutex> lock(mtx);
  if (g_rccl.lib) return true;
  void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
  if (!lib) { err = std::string("dlopen(librccl.so.1): ") + dlerror(); return false; }
#define RCCL_SYM(field, name)                                                       \
  g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(lib, name));        \
  if (!g_rccl.field) { err = std::string("librccl lacks ") + name; dlclose(lib); return false; }
  RCCL_SYM(CommInitAll, "ncclCommInitAll") RCCL_SYM(CommDestroy, "ncclCommDestroy") RCCL_SYM(AllGather, "ncclAllGather")
  RCCL_SYM(AllReduce, "ncclAllReduce") RCCL_SYM(GroupStart, "ncclGroupStart") RCCL_SYM(GroupEnd, "ncclGroupEnd")
  RCCL_SYM(GetErrorString, "ncclGetErrorString") RCCL_SYM(CommCount, "ncclCommCount")
#undef RCCL_SYM
  g_rccl.lib = lib;
  return true;
}

#define NCCLCHK(expr)                                                                                          \
  do {                                                                                                         \
    const ncclResult_t r_ = (expr);                                                                            \
    if (r_ != ncclSuccess) return fail(RMCLHIP_ERR_HIP, std::string(#expr) + ": " + g_rccl.GetErrorString(r_)); \
  } while (0)

// ---- the debug trace (multi_internal.h) ----
static std::atomic<bool> g_trace_on{false};
static std::mutex g_trace_mtx;
static std::string g_trace;
RMCL_INTERNAL void trace(char what, uint32_t rank) {
  if (!g_trace_on.load(std::memory_order_relaxed)) return;
  std::lock_guard<std::mutex> lock(g_trace_mtx);
  g_trace += what;
  g_trace += std::to_string(rank);
  g_trace += ' ';
}
RMCL_INTERNAL void trace_mark(const char* label) {
  if (!g_trace_on.load(std::memory_order_relaxed)) return;
  std::lock_guard<std::mutex> lock(g_trace_mtx);
  g_trace += label;
  g_trace += ' ';
}

rmclhip_status rmclhip_debug_trace(int on, char* buf, size_t cap) {
  // on = 1: start (clears), on = 0: stop; buf (nullable) receives what was recorded so far
  std::lock_guard<std::mutex> lock(g_trace_mtx);
  if (buf && cap) {
    const size_t n = std::min(cap - 1, g_trace.size());
    std::memcpy(buf, g_trace.data(), n);
    buf[n] = 0;
  }
  if (on) g_trace.clear();
  g_trace_on = on != 0;
  return RMCLHIP_OK;
}

// ---- creation ----
RMCL_INTERNAL rmclhip_status device_list_check(const char* who_, const int* devices, uint32_t ndev, bool refuse_duplicates, NullDevices null_means,
                                               std::vector<int>* out) {
  const std::string who(who_);
  if (ndev == 0 || ndev > 64) return fail(RMCLHIP_ERR_INVALID, who + ": ndev must be 1..64");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(RMCLHIP_ERR_NO_DEVICE, "no HIP device available (librmclhip has no CPU fallback)");
  std::vector<int> devs(ndev);
  for (uint32_t i = 0; i < ndev; ++i) {
    devs[i] = devices ? devices[i] : (null_means == NullDevices::kCountUp ? static_cast<int>(i) : 0);
    if (devs[i] < 0 || devs[i] >= count) return fail(RMCLHIP_ERR_INVALID, who + ": device index out of range");
    for (uint32_t j = 0; refuse_duplicates && j < i; ++j)
      if (devs[j] == devs[i]) return fail(RMCLHIP_ERR_INVALID, who + ": duplicate device");
  }
  out->swap(devs);
  return RMCLHIP_OK;
}

void rmclhip_comm_destroy(rmclhip_comm* c) {
  if (!c) return;
  for (size_t i = 0; i < c->devices.size(); ++i) {
    (void)hipSetDevice(c->devices[i]);
    if (i < c->streams.size() && c->streams[i]) { (void)hipStreamSynchronize(c->streams[i]); (void)hipStreamDestroy(c->streams[i]); }
    if (i < c->comms.size() && c->comms[i] && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comms[i]);
    if (i < c->ev_in.size() && c->ev_in[i]) (void)hipEventDestroy(c->ev_in[i]);
    if (i < c->ev_out.size() && c->ev_out[i]) (void)hipEventDestroy(c->ev_out[i]);
  }
  delete c;
}

rmclhip_status rmclhip_comm_create(const int* devices, uint32_t ndev, rmclhip_comm** out) {
  ApiGuard guard_("rmclhip_comm_create");
  if (!out) return fail(RMCLHIP_ERR_INVALID, "comm_create: out is null");
  *out = nullptr;
  std::vector<int> devs;   // refused lists never load RCCL
  if (rmclhip_status st = device_list_check("comm_create", devices, ndev, true, NullDevices::kCountUp, &devs)) return st;
  std::string err;
  if (!rccl_load(err)) return fail(RMCLHIP_ERR_UNSUPPORTED, "comm_create: " + err);
  rmclhip_comm* c = new rmclhip_comm();
  c->devices = devs;
  c->comms.resize(ndev);
  const ncclResult_t r = g_rccl.CommInitAll(c->comms.data(), static_cast<int>(ndev), devs.data());
  if (r != ncclSuccess) {
    delete c;
    return fail(RMCLHIP_ERR_HIP, std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(r));
  }
  c->streams.resize(ndev);
  for (uint32_t i = 0; i < ndev; ++i) {
    (void)hipSetDevice(devs[i]);
    if (hipStreamCreateWithFlags(&c->streams[i], hipStreamNonBlocking) != hipSuccess) {
      rmclhip_comm_destroy(c);
      return fail(RMCLHIP_ERR_HIP, "comm_create: hipStreamCreate failed");
    }
  }
  *out = c;
  return RMCLHIP_OK;
}

uint32_t rmclhip_comm_size(const rmclhip_comm* c) { return c ? static_cast<uint32_t>(c->devices.size()) : 0u; }

// The loopback communicator (see struct rmclhip_comm): same interface, no RCCL, ranks may share a device.
rmclhip_status rmclhip_comm_create_loopback(const int* devices, uint32_t ndev, rmclhip_comm** out) {
  ApiGuard guard_("rmclhip_comm_create_loopback");
  if (!out) return fail(RMCLHIP_ERR_INVALID, "comm_create_loopback: out is null");
  *out = nullptr;
  std::vector<int> devs;
  if (rmclhip_status st = device_list_check("comm_create_loopback", devices, ndev, false, NullDevices::kAllZero, &devs)) return st;
  rmclhip_comm* c = new rmclhip_comm();
  c->loopback = true;
  c->devices = devs;
  c->streams.assign(ndev, nullptr);
  c->ev_in.assign(ndev, nullptr);
  c->ev_out.assign(ndev, nullptr);
  for (uint32_t i = 0; i < ndev; ++i) {
    hipError_t e = hipSetDevice(c->devices[i]);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->streams[i], hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_in[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_out[i], hipEventDisableTiming);
    if (e != hipSuccess) { rmclhip_comm_destroy(c); return fail(RMCLHIP_ERR_HIP, std::string("comm_create_loopback: ") + hipGetErrorString(e)); }
  }
  *out = c;
  return RMCLHIP_OK;
}

rmclhip_status rmclhip_comm_loopback_set_reduce_rotation(rmclhip_comm* c, uint32_t first_rank) {
  if (!c || !c->loopback) return fail(RMCLHIP_ERR_INVALID, "comm_loopback_set_reduce_rotation: a loopback communicator is needed");
  c->reduce_rotation = first_rank % static_cast<uint32_t>(c->devices.size());
  return RMCLHIP_OK;
}

/* how many ranks the communicator's collectives span: ncclCommCount of the first rank's communicator for RCCL, the rank list's size for
 * the loopback stand-in (bench.py records it beside its sharded figures: a scaling run shows that RCCL saw N ranks) */
rmclhip_status rmclhip_comm_collective_ranks(rmclhip_comm* c, uint32_t* n_ranks, int* is_rccl) {
  if (!c || !n_ranks) return fail(RMCLHIP_ERR_INVALID, "comm_collective_ranks: null");
  if (is_rccl) *is_rccl = c->loopback ? 0 : 1;
  if (c->loopback) { *n_ranks = static_cast<uint32_t>(c->devices.size()); return RMCLHIP_OK; }
  int cnt = 0;
  if (g_rccl.CommCount == nullptr) return fail(RMCLHIP_ERR_UNSUPPORTED, "comm_collective_ranks: ncclCommCount not resolved");
  NCCLCHK(g_rccl.CommCount(c->comms[0], &cnt));
  *n_ranks = static_cast<uint32_t>(cnt);
  return RMCLHIP_OK;
}

// ---- the collectives (multi_internal.h) ----
// every rank's stream waits until all ranks' streams have reached this point (loopback collectives only)
static hipError_t loopback_barrier(rmclhip_comm* c, std::vector<hipEvent_t>& evs) {
  const size_t world = c->devices.size();
  for (size_t r = 0; r < world; ++r) {
    hipError_t e = hipSetDevice(c->devices[r]);
    if (e == hipSuccess) e = hipEventRecord(evs[r], c->streams[r]);
    if (e != hipSuccess) return e;
  }
  for (size_t r = 0; r < world; ++r) {
    hipError_t e = hipSetDevice(c->devices[r]);
    for (size_t s = 0; s < world && e == hipSuccess; ++s)
      if (s != r) e = hipStreamWaitEvent(c->streams[r], evs[s], 0);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

RMCL_INTERNAL rmclhip_status comm_allgather(rmclhip_comm* c, const void* const* send, void* const* recv, size_t bytes) {
  const uint32_t world = static_cast<uint32_t>(c->devices.size());
  if (bytes == 0) return RMCLHIP_OK;
  if (!c->loopback) {
    NCCLCHK(g_rccl.GroupStart());
    for (uint32_t r = 0; r < world; ++r) {
      (void)hipSetDevice(c->devices[r]);
      const ncclResult_t nr = g_rccl.AllGather(send[r], recv[r], bytes, ncclChar, c->comms[r], c->streams[r]);
      if (nr != ncclSuccess) { (void)g_rccl.GroupEnd(); return fail(RMCLHIP_ERR_HIP, std::string("ncclAllGather: ") + g_rccl.GetErrorString(nr)); }
    }
    NCCLCHK(g_rccl.GroupEnd());
    return RMCLHIP_OK;
  }
  HIPCHK(loopback_barrier(c, c->ev_in));      // every rank's send buffer is complete
  for (uint32_t r = 0; r < world; ++r) {
    HIPCHK(hipSetDevice(c->devices[r]));
    for (uint32_t sr = 0; sr < world; ++sr)
      HIPCHK(hipMemcpyAsync(static_cast<char*>(recv[r]) + static_cast<size_t>(sr) * bytes, send[sr], bytes, hipMemcpyDefault, c->streams[r]));
  }
  HIPCHK(loopback_barrier(c, c->ev_out));     // ... and nobody overwrites it before every rank has read it
  return RMCLHIP_OK;
}

RMCL_INTERNAL rmclhip_status comm_allreduce_f64(rmclhip_comm* c, const double* const* send, double* const* recv, uint32_t count, bool is_max) {
  const uint32_t world = static_cast<uint32_t>(c->devices.size());
  if (count == 0) return RMCLHIP_OK;
  if (!c->loopback) {
    NCCLCHK(g_rccl.GroupStart());
    for (uint32_t r = 0; r < world; ++r) {
      (void)hipSetDevice(c->devices[r]);
      const ncclResult_t nr = g_rccl.AllReduce(send[r], recv[r], count, ncclDouble, is_max ? ncclMax : ncclSum, c->comms[r], c->streams[r]);
      if (nr != ncclSuccess) { (void)g_rccl.GroupEnd(); return fail(RMCLHIP_ERR_HIP, std::string("ncclAllReduce: ") + g_rccl.GetErrorString(nr)); }
    }
    NCCLCHK(g_rccl.GroupEnd());
    return RMCLHIP_OK;
  }
  HIPCHK(loopback_barrier(c, c->ev_in));
  // (RCCL chooses its own order of summation; the stand-in can be told to choose another one -- a result that must not depend on the
  // library's order is tested by rotating it)
  std::vector<const double*> rot(world);
  for (uint32_t k = 0; k < world; ++k) rot[k] = send[(k + c->reduce_rotation) % world];
  for (uint32_t r = 0; r < world; ++r) {
    HIPCHK(hipSetDevice(c->devices[r]));
    HIPCHK(launch_loopback_allreduce(rot.data(), world, recv[r], count, is_max, c->streams[r]));
  }
  HIPCHK(loopback_barrier(c, c->ev_out));
  return RMCLHIP_OK;
}

RMCL_INTERNAL rmclhip_status comm_wait_all(rmclhip_comm* c) {
  for (uint32_t r = 0; r < c->devices.size(); ++r) {
    HIPCHK(hipSetDevice(c->devices[r]));
    HIPCHK(hipStreamSynchronize(c->streams[r]));
    trace('W', r);
  }
  return RMCLHIP_OK;
}

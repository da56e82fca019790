// multi_internal.h -- what the translation units of "several devices in one process" share (capi_comm.cpp, capi_rcc_sharded.cpp,
// capi_pf_sharded.cpp): the communicator, the block partition, the device-list check, the collectives and the debug trace.
#pragma once
#include "capi_internal.h"
#include <rccl/rccl.h>   // types only: the library is resolved with dlopen when the first communicator is created (capi_comm.cpp)

struct rmclhip_comm {
  std::vector<int> devices;
  std::vector<ncclComm_t> comms;
  std::vector<hipStream_t> streams;   // one collective stream per device
  // rmclhip_comm_create_loopback: an in-process stand-in for RCCL (every "rank" is a stream of this process, ranks may share a
  // device): collectives are device-to-device copies / one small kernel, ordered with events.  It exists so that the ndev > 1 code
  // paths of the sharded entry points run -- and are checked against the unsharded results -- on a box with ONE GPU.
  bool loopback = false;
  std::vector<hipEvent_t> ev_in, ev_out;
  uint32_t reduce_rotation = 0;   // loopback only (rmclhip_comm_loopback_set_reduce_rotation): the all-reduce adds the ranks starting at this one
};

// contiguous block partition of n items over `world` ranks: rank's block, and the largest block -- what every shard
// is padded to, so that the collectives run on equal counts
RMCL_INTERNAL inline void shard_bounds(uint32_t n, uint32_t rank, uint32_t world, uint32_t* lo, uint32_t* hi) {
  const uint32_t base = n / world, rem = n % world;
  *lo = rank * base + std::min(rank, rem);
  *hi = *lo + base + (rank < rem ? 1u : 0u);
}
RMCL_INTERNAL inline uint32_t shard_cap(uint32_t n, uint32_t world) { return n / world + (n % world ? 1u : 0u); }

// the device list of a create function (capi_comm.cpp): ndev must be 1..64 and every index a device of this machine, else
// RMCLHIP_ERR_INVALID "<who>: ..." (RMCLHIP_ERR_NO_DEVICE without any device).  A null list means 0 .. ndev-1, or ndev times device 0.
enum class NullDevices { kCountUp, kAllZero };
RMCL_INTERNAL rmclhip_status device_list_check(const char* who, const int* devices, uint32_t ndev, bool refuse_duplicates, NullDevices null_means,
                                               std::vector<int>* out);

// ---- the collectives the sharded entry points use, on every rank's collective stream (nothing here waits on the host) ----
// all-gather of `bytes` per rank: recv[r][s * bytes ..] = send[s][0 .. bytes) for every rank r and s
RMCL_INTERNAL rmclhip_status comm_allgather(rmclhip_comm* c, const void* const* send, void* const* recv, size_t bytes);
// all-reduce of `count` doubles (sum or max): recv[r] = op over s of send[s], identical on every rank
RMCL_INTERNAL rmclhip_status comm_allreduce_f64(rmclhip_comm* c, const double* const* send, double* const* recv, uint32_t count, bool is_max);
// the host waits for every rank's collective stream (ONE wait per rank, after everything of a phase has been enqueued); traces W<r>
RMCL_INTERNAL rmclhip_status comm_wait_all(rmclhip_comm* c);

// debug trace of the sharded entry points (rmclhip_debug_trace): "E<r>" = rank r's work of a phase enqueued, "W<r>" = the host waited
// for rank r.  A phase that scales reads E0 E1 ... W0 W1 ...; E0 W0 E1 W1 serialises the devices.
RMCL_INTERNAL void trace(char what, uint32_t rank);
RMCL_INTERNAL void trace_mark(const char* label);

// capi_internal.h -- what the translation units of the C ABI (include/rmclhip.h) share: the handle structs, the error plumbing and the
// internal functions one file defines and another calls.  Round 5 split the former capi.cpp (4 300 lines) by handle type:
//   capi_map.cpp       context, map / scene upload, host-side algebra, device memory helpers
//   capi_rcc.cpp       the correspondence operator: models, datasets, find, reduction, the moments' hand-over to the host, pose batches
//   capi_micp.cpp      the MICP corrections of that operator, one sensor and N, each a dispatcher over its loop forms (kernels: micp.hip)
//   capi_rcc_tune.cpp  tuning knobs, autotune, measurement aids (include/rmclhip_bench.h) and diagnostics (include/rmclhip_lab.h) of that operator
//   capi_segment.cpp   map segmentation of that operator: trace into its own scratch, labels, compacted outlier clouds (kernels: segment.hip)
//   capi_pc2scan.cpp   PointCloud2 bytes -> range image of a spherical model, as a free function and as an operator's dataset (kernels: pc2scan.hip)
//   capi_deskew.cpp    PointCloud2 bytes + per-point times + the scan's motion -> OnDn model + dataset of an operator, or a compensated cloud; the host helpers (kernel: deskew.hip)
//   capi_pf.cpp        particle-filter sensor update, motion update, resamplers
//   capi_field.cpp     the map's distance field: layout, what both layouts' builds and create entry points share, the coarse-to-fine build, download, lookup, and the sensor update of correspondence_type 1 answered from it (kernels: field_build.hip, field.hip)
//   capi_band_field.cpp the banded distance field: layout, the coarse build, classification, the bricks' fill, download (kernels: field_build.hip; the lookups are field.hip's)
//   capi_stein.cpp     the Stein variational step of a cloud on a filter handle's field: parameters, scratch, the iterations' launches, counts (kernels: stein.hip)
//   capi_refine.cpp    the damped Gauss-Newton refinement of particles on a distance field: parameters, launch, counts (kernel: refine.hip)
//   capi_particles.cpp the particle cloud's initialisations (uniform, pose + covariance, on the surface), the recovery injection and the visualisation channels (kernels: particles.hip)
//   capi_surface_sample.cpp the surface sampler: parameters, the build of the face weights, info; the recovery averages (host) (kernels: surface_sample.hip, the scan of resample.hip)
//   capi_hypotheses.cpp the single-device pose estimate and the pose hypotheses: clusters of the occupied bins (kernels: hypotheses.hip)
//   capi_pose_information.cpp the point-to-plane information matrix of a find's correspondences and its host algebra: covariance, degeneracy (kernels: pose_information.hip)
//   several devices in one process (what the three share: multi_internal.h):
//   capi_comm.cpp      communicators (RCCL resolved with dlopen / the in-process loopback), their two collectives, the debug trace of the sharded entry points
//   capi_rcc_sharded.cpp pose batches sharded over one operator replica per device (no collective)
//   capi_pf_sharded.cpp the sharded particle filter: one filter replica per device, every sharded twin of a single-device entry point
// Host-side orchestration only: device memory, streams, launches.  There is no CPU compute path: without a HIP device every compute
// entry point fails with RMCLHIP_ERR_NO_DEVICE.
// Ownership: every allocation is a member (or a local) of type DevBuf, PinnedBuf or MappedBuf below and goes with its owner; a
// plain pointer in a handle is borrowed or points into one of them, and says so.  A destroy function sets the handle's device, waits
// for its stream, destroys what has an order (graph, events, stream), drops the references it holds and deletes the handle.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../include/rmclhip.h"
#include "../../include/rmclhip_bench.h"
#include "../../include/rmclhip_lab.h"
#include "bvh_build.h"
#include "devmath.h"
#include "kernels.h"
#include "lab_hooks.h"

using namespace rmclhip;

static_assert(sizeof(rmclhip_transform) == sizeof(xform), "Transform layout");
static_assert(sizeof(rmclhip_cross_statistics) == sizeof(cstats), "CrossStatistics layout");
static_assert(sizeof(rmclhip_particle_attributes) == 36, "ParticleAttributes layout");
static_assert(sizeof(rmclhip_range_measurement) == 64, "RangeMeasurement layout");
static_assert(sizeof(rmclhip_spherical_model) == 32, "SphericalModel layout");

// internal symbols shared by the translation units of the library: never exported
#define RMCL_INTERNAL __attribute__((visibility("hidden")))

extern RMCL_INTERNAL thread_local std::string g_err;   // rmclhip_last_error (capi_map.cpp)

inline rmclhip_status fail(rmclhip_status st, const std::string& msg) {
  g_err = msg;
  return st;
}

#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ == kLabMissing)                                                                        \
      return fail(RMCLHIP_ERR_UNSUPPORTED, std::string(#expr) + ": this kernel variant is an experiment that lives in " \
                  "librmclhip_lab.so, which is not loaded (include/rmclhip_lab.h)");              \
    if (e_ != hipSuccess)                                                                         \
      return fail(RMCLHIP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));            \
  } while (0)

// a HIP call of the entry point `who` (capi_field.cpp): on failure the error is cleared and becomes RMCLHIP_ERR_NOMEM (out of memory)
// or RMCLHIP_ERR_HIP, with the message "<who>: <HIP's error string>"
RMCL_INTERNAL rmclhip_status hip_status(const std::string& who, hipError_t e);
#define HIPCHK_AS(who, expr)                                          \
  do {                                                                \
    if (rmclhip_status st_ = hip_status(who, (expr))) return st_;     \
  } while (0)

inline xform to_x(const rmclhip_transform* T) {
  xform r;
  std::memcpy(&r, T, sizeof(r));
  return r;
}
inline void from_x(const xform& x, rmclhip_transform* T) { std::memcpy(T, &x, sizeof(x)); }
inline cstats to_cs(const rmclhip_cross_statistics* s) {
  cstats r;
  std::memcpy(&r, s, sizeof(r));
  return r;
}
inline void from_cs(const cstats& c, rmclhip_cross_statistics* s) { std::memcpy(s, &c, sizeof(c)); }

// RMCLHIP_DEBUG=1: report which API call leaves a HIP error behind
struct ApiGuard {
  const char* name;
  explicit ApiGuard(const char* n) : name(n) {}
  ~ApiGuard() {
    static const bool on = std::getenv("RMCLHIP_DEBUG") != nullptr;
    if (on) {
      const hipError_t e = hipPeekAtLastError();
      if (e != hipSuccess) std::fprintf(stderr, "[rmclhip debug] %s leaves HIP error: %s\n", name, hipGetErrorString(e));
    }
  }
};

// ---- owned memory ----------------------------------------------------------------------------------
// Every byte of device, pinned and host-mapped memory the library holds belongs to one of three move-only owners, which free it in
// their destructors: a handle's destroy function names no buffer.  These two functions are the only callers of HIP's allocation and
// free functions in this directory (tests/test_abi.py; rmclhip_malloc / rmclhip_free, which hand memory to the caller, excepted).  They
// keep the two process-wide counts rmclhip_debug_live_bytes reads -- allocation is never on a per-call path, every buffer is grow-only --
// and report a failed free under RMCLHIP_DEBUG.
enum MemKind { kMemDevice = 0, kMemPinned = 1, kMemMapped = 2 };
extern RMCL_INTERNAL std::atomic<uint64_t> g_live_bytes[2];   // [0] device, [1] pinned + host-mapped (capi_map.cpp)

// *p: the allocation (null on failure); *d (kMemMapped only): its device alias
RMCL_INTERNAL inline hipError_t mem_alloc(MemKind kind, size_t bytes, void** p, void** d = nullptr) {
  hipError_t e = kind == kMemDevice   ? hipMalloc(p, bytes)
                 : kind == kMemPinned ? hipHostMalloc(p, bytes, hipHostMallocDefault)
                                      : hipHostMalloc(p, bytes, hipHostMallocMapped | hipHostMallocCoherent);
  if (e != hipSuccess) { *p = nullptr; return e; }
  if (kind == kMemMapped && (e = hipHostGetDevicePointer(d, *p, 0)) != hipSuccess) {
    (void)hipHostFree(*p);
    *p = *d = nullptr;
    return e;
  }
  g_live_bytes[kind != kMemDevice].fetch_add(bytes, std::memory_order_relaxed);
  return hipSuccess;
}
RMCL_INTERNAL inline void mem_free(MemKind kind, void* p, size_t bytes) {
  if (!p) return;
  const hipError_t e = kind == kMemDevice ? hipFree(p) : hipHostFree(p);
  g_live_bytes[kind != kMemDevice].fetch_sub(bytes, std::memory_order_relaxed);
  if (e != hipSuccess && std::getenv("RMCLHIP_DEBUG"))
    std::fprintf(stderr, "[rmclhip debug] %s(%p) -> %s\n", kind == kMemDevice ? "hipFree" : "hipHostFree", p, hipGetErrorString(e));
}

// device (DevBuf) or pinned host memory (PinnedBuf: hipHostMallocDefault, staging a device copies into and the host reads), grow-only
// (RCCEmbree.cpp:28-33): reserve keeps what is large enough and otherwise replaces it, contents lost.  (Hidden: an out-of-line copy
// of a header template's member is otherwise an exported weak symbol of the library.)
template <typename T, MemKind K>
struct RMCL_INTERNAL OwnedBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  OwnedBuf() = default;
  OwnedBuf(const OwnedBuf&) = delete;
  OwnedBuf& operator=(const OwnedBuf&) = delete;
  OwnedBuf(OwnedBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  OwnedBuf& operator=(OwnedBuf&& o) noexcept {
    if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
    return *this;
  }
  ~OwnedBuf() { release(); }
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    const hipError_t e = mem_alloc(K, n * sizeof(T), reinterpret_cast<void**>(&p));
    if (e == hipSuccess) cap = n;
    return e;
  }
  void release() {
    mem_free(K, p, cap * sizeof(T));
    p = nullptr;
    cap = 0;
  }
};
template <typename T> using DevBuf = OwnedBuf<T, kMemDevice>;
template <typename T> using PinnedBuf = OwnedBuf<T, kMemPinned>;

// host-mapped coherent memory, which a kernel writes through d and the host reads through h: results, status blocks, completion tags.
// Grow-only as above; both pointers are null after a failed reserve.
template <typename T>
struct RMCL_INTERNAL MappedBuf {
  T* h = nullptr;
  T* d = nullptr;  // device alias of h
  size_t cap = 0;  // elements
  MappedBuf() = default;
  MappedBuf(const MappedBuf&) = delete;
  MappedBuf& operator=(const MappedBuf&) = delete;
  MappedBuf(MappedBuf&& o) noexcept : h(o.h), d(o.d), cap(o.cap) { o.h = o.d = nullptr; o.cap = 0; }
  MappedBuf& operator=(MappedBuf&& o) noexcept {
    if (this != &o) { release(); h = o.h; d = o.d; cap = o.cap; o.h = o.d = nullptr; o.cap = 0; }
    return *this;
  }
  ~MappedBuf() { release(); }
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    const hipError_t e = mem_alloc(kMemMapped, n * sizeof(T), reinterpret_cast<void**>(&h), reinterpret_cast<void**>(&d));
    if (e == hipSuccess) cap = n;
    return e;
  }
  void release() {
    mem_free(kMemMapped, h, cap * sizeof(T));
    h = d = nullptr;
    cap = 0;
  }
};

// the temporary device buffers of a build: count (at least one) elements each, freed when the build leaves, however it leaves
struct BuildScratch {
  std::vector<DevBuf<uint8_t>> owned;
  template <typename T>
  hipError_t alloc(T** out, size_t count) {
    owned.emplace_back();
    const hipError_t e = owned.back().reserve(std::max<size_t>(count, 1u) * sizeof(T));
    *out = reinterpret_cast<T*>(owned.back().p);
    return e;
  }
};

// Upload on the handle's OWN stream, then wait for it.  A plain hipMemcpy runs on the null stream, which the handles'
// hipStreamNonBlocking streams do not synchronise with: a copy from pageable memory may return once the data is staged,
// and a kernel enqueued on the handle's stream right afterwards is then not ordered behind the DMA.  (Observed as a
// 1-in-200 deviation of 5e-7 rad in a correction issued immediately after set_dataset, tools/flaky_g5.py.)
inline hipError_t upload_on(hipStream_t s, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  if (bytes == 0) return hipSuccess;
  hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return e;
}

// PointCloud2 -> scan (capi_pc2scan.cpp): grow-only scratch of one owner (a context's free function, an operator): the per-cell keys
// of the winner resolution, the range image, the per-workgroup counts and the host-mapped totals (created by the first call)
struct Pc2ScanScratch {
  DevBuf<unsigned long long> keys;
  DevBuf<float> ranges;
  DevBuf<uint32_t> block_counts;        // 3 per workgroup of points, then 1 per workgroup of cells
  MappedBuf<uint32_t> h_counters;       // {finite, in image, in range, cells filled}
};

// ROBUST MICP (capi_robust.cpp): grow-only scratch of one owner (a context's free function, an operator) -- two sets of partial rows,
// the scale selection's histograms and keys, the small device block the kernels keep between launches, and the host-mapped block
// their last launches write the results into (no copy launch: the call waits for the stream and reads them)
struct RobustDevBlock { RobustScale scale; xform state[2]; };
struct RobustOutBlock { RobustScale scale; RobustLoopOut loop; RobustStats stats; };
struct RobustScratch {
  DevBuf<double> partials;
  DevBuf<uint32_t> sel, keys;
  DevBuf<float> weights;
  DevBuf<RobustDevBlock> dev;
  MappedBuf<RobustOutBlock> out;
  // the rig loop (rmclhip_micp_correct_once_robust), on the rig's FIRST sensor: its state between launches and the host-mapped copy
  DevBuf<RobustRigState> rig;
  MappedBuf<RobustRigState> rig_out;
};

struct rmclhip_ctx {
  int device = 0;
  hipDeviceProp_t props;
  // map / rcc / pf / resampler handles keep a pointer to their context: each holds a reference, and
  // rmclhip_ctx_destroy only drops the creator's, so destroying the context before its children is safe
  std::atomic<int> refs{1};
  std::atomic<int> wait_block{0};   // rmclhip_ctx_set_wait_mode: 0 = spin on the completion tag, 1 = block in hipStreamSynchronize
  // rmclhip_statistics_p2l (the free function on caller-owned views): stream, partial rows, host-mapped result + tag, created by the
  // first call under the mutex, which also serialises the calls of one context
  std::mutex p2l_mtx;
  hipStream_t p2l_stream = nullptr;
  DevBuf<double> p2l_partials;
  MappedBuf<cstats> p2l_h_stats;        // [0] the result
  MappedBuf<unsigned long long> p2l_h_done;
  uint32_t p2l_seq = 0;
  DevBuf<double> pinfo_partials, pinfo_rows;   // rmclhip_pose_information_p2l: its rows per workgroup and its result row, same stream and mutex
  RobustScratch robust;                        // rmclhip_statistics_p2l_robust, same stream and mutex
  // rmclhip_pointcloud2_to_scan (the free function): its own stream and scratch, created by the first call under its mutex
  std::mutex pc2_mtx;
  hipStream_t pc2_stream = nullptr;
  Pc2ScanScratch pc2;
  DevBuf<uint8_t> pc2_raw;              // staged host bytes
  DevBuf<uint8_t> deskew_aux;           // rmclhip_pointcloud2_deskew (capi_deskew.cpp), same stream and mutex: the four counters
  // rmclhip_particles_* (capi_particles.cpp): their stream and the visualisation pack's device staging, created by the first call
  // under the mutex, which also serialises the calls of one context
  std::mutex part_mtx;
  hipStream_t part_stream = nullptr;
  DevBuf<float> part_viz;
  bool part_timing = false;              // rmclhip_debug_particles_timing (include/rmclhip_lab.h): bracket those calls with the two events
  hipEvent_t part_ev0 = nullptr, part_ev1 = nullptr;
  float part_last_ms = 0.f;
  ~rmclhip_ctx();                       // capi_map.cpp: the streams and events; the buffers free themselves after it
};

inline void ctx_retain(rmclhip_ctx* c) { c->refs.fetch_add(1); }
inline void ctx_release(rmclhip_ctx* c) {
  if (c && c->refs.fetch_sub(1) == 1) delete c;
}

struct rmclhip_map {
  rmclhip_ctx* ctx = nullptr;
  std::atomic<int> refs{1};
  BvhInfo info;
  DevBuf<uint32_t> d_nodes;
  DevBuf<uint32_t> d_qnodes;  // Node4Q twins
  DevBuf<uint32_t> d_frontier;   // frontier table (layout.h kFrontierDepth): n_frontier x 8 dwords {lo.xyz hi.x | hi.yz ref pad}
  uint32_t n_frontier = 0;
  DevBuf<uint32_t> d_frontier_pf;   // ... of the filter's tree (find kind 24 walks d_qnodes_pf)
  uint32_t n_frontier_pf = 0;
  // group boxes of the two tables (bvh_build.h frontier_groups_of): 16 x 8 dwords behind each table in ITS allocation, null for a table of <= 64 entries
  const uint32_t* d_frontier_groups = nullptr;   // inside d_frontier
  const uint32_t* d_frontier_groups_pf = nullptr;   // inside d_frontier_pf
  DevBuf<uint32_t> d_qnodes_pf;  // Node4Q array of the particle filter's own tree (leaves <= kPfLeafTris, same records)
  DevBuf<uint32_t> d_cnodes;  // Node4C twins
  DevBuf<uint32_t> d_cnodes16;  // Node16C twins (maps of up to kMaxNodes16 nodes; find kind 32 descends two levels per pass on them), else null
  DevBuf<uint32_t> d_tris;
  uint64_t bytes = 0;
  // near grid of the closest-point queries (kernels.h NearGrid): built on the first rmclhip_rcc_find_cpc of any operator of this map
  // near grids (ensure_near_grid): slot 0 = cells near the surface only (scan points), slot 1 = every cell (the filter's beam ends).
  // A slot is built once under the mutex and never changes or moves afterwards -- other operators' launches may be reading it --
  // and both live until the map is released.
  std::mutex grid_mtx;
  struct GridSlot { bool ready = false, failed = false; NearGrid g = {}; DevBuf<uint32_t> cells; };   // g.cells is cells.p
  GridSlot grid_slot[2];
  std::vector<uint32_t> scene_first_face;  // map_create_scene: first global face id of every instance, + the total (else empty)
};

// rmclhip_field_refine / rmclhip_pf_refine (capi_refine.cpp): grow-only scratch of one owner -- the beams' device records, the result
// rows when the caller gives none but asks for the counts, the three counters -- and what the call in flight needs to finish
struct RefineScratch {
  DevBuf<float> beams;
  DevBuf<uint32_t> rows, counters;
  const uint32_t* rows_src = nullptr;   // where the rows of the call in flight land (the caller's device memory or `rows`); null: none were asked for
};

// rmclhip_pf_stein_step (capi_stein.cpp): grow-only scratch of a filter handle, freed with it -- the cell list (table, counts, prefix
// sums, every particle's word), the drives, the bins' records, the counters and the result rows when the caller gives none but asks
// for the counts.  The beams use RefineScratch's buffer.  events: rmclhip_debug_stein_timing (include/rmclhip_lab.h)
struct SteinScratch {
  DevBuf<unsigned long long> table, incl, block_tot;
  DevBuf<uint32_t> words3, slot_of, records, counters, rows;   // words3: count | listed | cursor
  DevBuf<float> drive;
  bool timing = false;
  hipEvent_t events[kSteinEvents] = {nullptr, nullptr, nullptr, nullptr};
  float last_ms[kSteinEvents - 1u] = {0.f, 0.f, 0.f};
  ~SteinScratch() {
    for (hipEvent_t e : events) if (e) (void)hipEventDestroy(e);
  }
};

// the distance field of a map (capi_field.cpp): the lattice, immutable once built; handles that read it (rmclhip_pf_set_field) hold a
// reference.  `stream` and the two staging buffers serve rmclhip_field_query / _download alone, one call at a time (mtx).
struct rmclhip_field {
  rmclhip_ctx* ctx = nullptr;
  rmclhip_map* map = nullptr;
  std::atomic<int> refs{1};
  rmclhip_field_info info{};
  DevBuf<float> d_lat;
  // a banded field (capi_band_field.cpp): d_lat is null, the three arrays of BANDED DISTANCE FIELD instead; info is the logical
  // geometry with the actual bytes
  bool banded = false;
  rmclhip_band_field_info band{};
  DevBuf<uint32_t> d_table;
  DevBuf<float> d_coarse, d_bricks;
  uint64_t accounted = 0;          // what the field has added to its map's device_bytes
  std::mutex mtx;
  hipStream_t stream = nullptr;
  DevBuf<float> d_q_points, d_q_out;
  RefineScratch refine;            // rmclhip_field_refine, under mtx
};

struct rmclhip_rcc {
  rmclhip_ctx* ctx = nullptr;
  rmclhip_map* map = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  xform Tsb = xidentity();
  // model
  ModelKind kind = kModelNone;
  uint32_t W = 0, H = 0;
  rmclhip_interval range{0.f, 0.f};
  f3 orig{0.f, 0.f, 0.f};
  float pin_fc[4] = {1.f, 1.f, 0.f, 0.f};  // pinhole fx, fy, cx, cy
  DevBuf<float> d_model_tab;
  // params
  float max_dist = 1.0f, adaptive_max_dist_min = 1.0f;
  // dataset
  DevBuf<float> d_ds_points;
  DevBuf<uint8_t> d_ds_mask;
  // what the kernels read: the handle's own copies above, or device memory borrowed from the caller
  // (rmclhip_rcc_set_dataset_view: Correspondences_::dataset lives in the caller's rm::Memory<.., VRAM_HIP>)
  const float* ds_pts = nullptr;     // d_ds_points or the caller's view
  const uint8_t* ds_msk = nullptr;   // d_ds_mask or the caller's view
  uint32_t n_dataset = 0;
  bool ds_has_mask = false;
  // model buffers
  DevBuf<uint8_t> d_hits;
  DevBuf<float> d_ranges, d_points, d_normals;
  DevBuf<uint32_t> d_face_ids;
  uint32_t n_model = 0;      // per pose
  uint32_t nposes_last = 0;
  bool descent_wide = true;   // ... on the 16-wide twins when the map has them (A/B: rmclhip_rcc_set_descent's max_levels bit 31 clears it)
  uint32_t descent_final_cap = 64, descent_levels = 24;   // kind 32's cooperative descent (rmclhip_rcc_set_descent, include/rmclhip_lab.h)
  // pose batches in world order (kernels.hip launch_batch_tile_order; A/B knob rmclhip_rcc_set_batch_order): keys | sorted keys, values | sorted values, sort scratch
  int xcd_mapping_override = -1;   // A/B knob (rmclhip_rcc_set_descent bits 29..30): -1 = the tuned / default mapping
  uint32_t tuned_xcd_mapping = 0;  // rmclhip_rcc_autotune's choice among 0 / 1 / 2 (FindParams::xcd_mapping); 0 = the default
  uint32_t batch_order = 64;   // 0 = pose-major; else the granule (workgroups per XCD turn)
  DevBuf<uint32_t> d_ord_scratch, d_ord_vals;
  uint32_t last_order_n = 0, last_order_ngroups = 0;   // entries / workgroups per pose of the last batch launch's order, 0 = it went pose-major (rmclhip_debug_batch_order)
  bool descent_carry = false;   // kind 32: accepted candidates stay undivided through the cooperative leaf loop (traverse.hip.h TriPending); set by the autotune where it measures faster, or by rmclhip_rcc_set_descent's bit 16
  uint32_t descent_leaf_cap = 24;   // kind 32: a wave one of whose rays enters more final leaves than this starts at the root (lab: rmclhip_rcc_set_descent)
  uint32_t out_mask = RMCLHIP_OUT_ALL;   // rmclhip_rcc_set_outputs: which model buffers find / find_batch write
  // reduction
  DevBuf<double> d_partials;
  DevBuf<double> d_pinfo_partials, d_pinfo_rows;   // rmclhip_rcc_pose_information[_batch] (capi_pose_information.cpp): rows per workgroup, result rows per pose
  RobustScratch robust;            // the robust entry points (capi_robust.cpp)
  MappedBuf<cstats> h_stats;
  DevBuf<MicpState> d_state;
  MappedBuf<MicpState> h_state;
  DevBuf<uint32_t> d_counter;
  // device-resident MICP loop as a static hipGraph: per-call inputs travel in one 256-B H2D copy
  PinnedBuf<MicpCall> h_call;
  DevBuf<MicpCall> d_call;
  hipGraphExec_t micp_exec = nullptr;
  hipGraph_t micp_graph = nullptr;
  struct MicpKey {
    uint32_t n_iter = 0, W = 0, H = 0, n_dataset = 0;
    int kind = 0, variant = 0, tile = 0, has_mask = 0;
    const void* ptrs[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool operator==(const MicpKey& o) const { return std::memcmp(this, &o, sizeof(MicpKey)) == 0; }
  } micp_key;
  bool use_graph = true;           // rmclhip_rcc_set_variant bit 9 clears it: the chain is enqueued directly
  bool graph_dirty = true;         // set by setModel / set_variant: by-value launch arguments changed
  // moment form of the schedule-(R) loop (launch_micp_fast): tried first when the previous corrections say the gate
  // decisions are stable; the per-iteration form above is the fallback and the reference for the result
  int fast_mode = 1;               // rmclhip_rcc_set_micp_fast: 0 off, 1 automatic with the iterations on the host (default), 3 / 4 device loops (A/B)
  DevBuf<double> d_fast_partials;
  DevBuf<unsigned long long> d_fast_mask;
  DevBuf<double> d_fold_rows;         // hand-over area of the loop launch's folding workgroups (kernels.h: kMicpFoldBlocks)
  DevBuf<uint32_t> d_join_flags;      // (first sensor of rmclhip_micp_correct_once) the other sensors' "my rows are complete" words
  hipEvent_t ev_join = nullptr;       // rmclhip_micp_correct_once: this sensor's find (+ moment pass) ran on its own stream; the loop's stream waits for it
  uint32_t* d_fold_flags = nullptr;   // inside d_fold_rows, behind the rows
  uint32_t last_fast_rows = 0, last_fast_words = 0;   // partial rows / mask words of the last moment-form attempt (diagnostics)
  MappedBuf<MicpFastStatus> h_fast_status;
  MappedBuf<unsigned long long> h_done;         // completion tags: [0] this handle's chains, [1] the N-sensor loop
  uint32_t done_seq = 0;                        // sequence number of the last polled call (never 0 in a tag)
  // closest-point correspondences, tracking: record index per dataset point of the previous find_cpc (see rmclhip_rcc_find_cpc)
  DevBuf<uint32_t> d_cpc_rec;
  const uint32_t* cpc_rec_ptr = nullptr;        // d_cpc_rec.p when the records were written (never dereferenced)
  const float* cpc_rec_pts = nullptr;           // the dataset the records were computed for
  uint32_t cpc_rec_n = 0;
  bool cpc_tracking = true;
  bool cpc_bounded = false;        // rmclhip_rcc_set_cpc_bounded: search only within max_dist
  bool cpc_grid = true;            // rmclhip_rcc_set_cpc_grid: points without a tracking seed start from the map's near grid
  float fast_rho_cap = 0.02f, fast_tau_cap = 0.1f;   // bounds on |2 sin(theta/2)| and |t| of the pre-transforms
  uint32_t fast_holdoff = 0;       // corrections to skip the attempt for (after repeated overflows)
  uint32_t fast_overflows = 0;     // consecutive
  rmclhip_micp_fast_info fast_info = {};
  // Round 4 -- iterations on the host (micp_host.h): what k_micp_publish hands over, and the host's verified copy of it
  MappedBuf<MicpHostBlock> h_mom;
  MicpMomentSet mset;                  // valid for the model buffers + dataset it was formed from; dropped by whatever changes either
  bool mset_pending = false;           // a publish is in flight on the stream (speculating find): its tag carries mset_seq
  uint32_t mset_seq = 0;
  float pend_lo = 0.f, pend_hi = 0.f, pend_rho = 0.f, pend_tau = 0.f;   // band and caps the in-flight set is formed for
  uint32_t mset_passes = 0;            // moment passes computeCrossStatistics ran since the last find (at most 2)
  MicpFastStatus last_fast = {};       // outcome of the last moment-form attempt, whichever side ran the iterations
  // the reference's unchanged caller loop (micp_localization.cpp:900-964): find(), then computeCrossStatistics() per iteration
  uint32_t ccs_since_find = 0;         // computeCrossStatistics calls since the last find
  bool ccs_loop = false;               // the last find was followed by such calls: the next find forms the moments in its epilogue
  float ccs_last_maxd = 0.f;           // max_dist' of the last call (the band of the next speculation is centred on it)
  float ccs_max_rho = 0.f, ccs_max_tau = 0.f;   // largest pre-transform since the last find
  rmclhip_ccs_info ccs_info = {};
  // N-sensor loop (rmclhip_micp_correct_once): call block + state of the first sensor, kept between calls
  DevBuf<uint8_t> d_multi_blob;
  MappedBuf<MicpMultiState> h_multi_state;
  MappedBuf<MicpMultiFastStatus> h_multi_status;
  uint32_t multi_holdoff = 0, multi_overflows = 0;
  // batch
  DevBuf<uint8_t> d_raw;           // staged PointCloud2 bytes (set_input_pointcloud2)
  DevBuf<xform> d_Tbm, d_Tsm, d_Tms, d_Tdelta;
  DevBuf<cstats> d_bstats;
  // correct_batch's results leave through host-mapped staging: the solve launch writes them there, the call returns on its completion
  // tag and copies them out -- no device-to-host copy launches, no stream synchronisation
  MappedBuf<xform> h_bT;
  MappedBuf<cstats> h_bS;
  // map segmentation (capi_segment.cpp): grow-only scratch of its trace {ranges, normals}, the staged measured ranges, labels when the
  // caller wants none, the per-workgroup counts; the totals arrive in host-mapped memory (created by the first call)
  DevBuf<float> d_seg_ranges, d_seg_normals, d_seg_real;
  DevBuf<uint8_t> d_seg_labels;
  DevBuf<uint32_t> d_seg_block_counts;
  MappedBuf<uint32_t> h_seg_counts;
  // rmclhip_rcc_set_input_pointcloud2_scan (capi_pc2scan.cpp): the model as set_model_spherical received it (the trig tables alone do
  // not give the bins back), the range image the dataset was made of and the keys, grow-only; host bytes are staged in d_raw
  rmclhip_spherical_model sph_model{{0.f, 0.f, 0u}, {0.f, 0.f, 0u}, {0.f, 0.f}};
  Pc2ScanScratch pc2;
  DevBuf<uint8_t> d_deskew_aux;    // rmclhip_rcc_set_input_pointcloud2_deskewed (capi_deskew.cpp): the four counters
  bool capturing = false;          // inside hipStreamBeginCapture: no synchronisation allowed
  int variant = 15;       // traversal kind: 0 wave-packet, 1 one lane per ray (while-while), 2 four lanes per ray
                          // (quad-cooperative), 15 automatic: quad while the launch is bound by the slowest ray's
                          // chain of dependent fetches (few rays in flight), one lane per ray once the chip is full
  int tile_override = 0;  // 1 + log2(tile width), 0 = automatic
  // rmclhip_rcc_autotune[_batch]: the kind measured fastest for the current (map, model), for single scans / pose batches (0 = the
  // rule), and whether its rays start at the frontier (kinds 23 / 24 without it are round 2's kinds 19 / 22)
  int tuned_kind = 0, tuned_batch_kind = 0;
  int tuned_tile = 0;              // 1 + log2(tile width) measured best by rmclhip_rcc_autotune (0 = the rule's shape)
  int last_moment_find_kind = 0;   // what enqueue_find_with_moments launched last (it may replace the rule's 24 by 23) ...
  bool last_moment_find_tiled = false;   // ... and whether it left one moment row per workgroup (epilogue) or per 1024 elements (pass)
  bool tuned_frontier = true, tuned_batch_frontier = true;
  DevBuf<float> d_tile_planes;     // plane table of the frontier start for the current (model, tiling): 16 floats per tile
  bool tile_planes_ok = false;
  float ang_aspect = 0.0f;         // spherical models: |row spacing / column spacing| in angle (0: unknown -- the other models)
  float last_find_ms = 0.f, last_reduce_ms = 0.f;
  bool reduce_timing_pending = false;
  bool find_timing_pending = false;   // a speculating find returned on its tag: ev0 / ev1 still hold its timing
  bool kernel_timing = false;         // rmclhip_rcc_set_kernel_timing: bracket find / computeCrossStatistics with HIP events (two
                                      // hipEventRecord + one hipEventElapsedTime per call: opt-in since round 4)
};

// A pinned, host-mapped completion tag of a handle whose synchronous calls launch kernels and return nothing through the host (the
// filter's update / motion update, the tournament): a one-thread launch behind the chain stores {seq, 0}, the host polls it -- ~7 us
// sooner than the stream's own completion signal reaches hipStreamSynchronize (measured on the synchronous find, round 4).
struct ChainTag {
  MappedBuf<unsigned long long> word;
  uint32_t seq = 0;
  hipError_t create() {
    const hipError_t e = word.reserve(1);
    if (e == hipSuccess) *word.h = 0ull;
    return e;
  }
  // wait for the end of what `stream` holds (BLOCK wait mode, or no tag: hipStreamSynchronize)
  hipError_t wait_chain_end(const rmclhip_ctx* ctx, hipStream_t stream) {
    if (word.h == nullptr || ctx->wait_block.load(std::memory_order_relaxed)) return hipStreamSynchronize(stream);
    seq = (seq == 0xFFFFFFFFu) ? 1u : seq + 1u;
    if (const hipError_t e = launch_host_tag(word.d, seq, stream)) return e;
    const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(20);
    volatile const unsigned long long* tag = word.h;
    for (uint32_t spins = 0;; ++spins) {
      if (*tag == static_cast<unsigned long long>(seq)) { std::atomic_thread_fence(std::memory_order_acquire); return hipSuccess; }
#if defined(__x86_64__) || defined(__i386__)
      __builtin_ia32_pause();
#endif
      if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() > t_end) return hipStreamSynchronize(stream);
    }
  }
};

// computeCrossStatistics and every correction read {hits, points, normals} of the operator's model buffers (Correspondences.hpp:81-85)
inline bool micp_outputs_selected(const rmclhip_rcc* r) { return (r->out_mask & RMCLHIP_OUT_MICP) == RMCLHIP_OUT_MICP; }
constexpr const char* kNeedMicpOutputs =
    "the operator's {hits, points, normals} outputs are deselected (rmclhip_rcc_set_outputs): nothing to reduce";

// whatever is about to rewrite the model buffers or the dataset: the published moments summarise the old ones
static inline void drop_moment_set(rmclhip_rcc* r) {
  r->mset.valid = false;
  r->mset_pending = false;
  r->mset_passes = 0;
}

// what a reduction over the operator's correspondences covers: the dataset or the last find's model buffers, whichever is shorter
inline uint32_t nred_of(const rmclhip_rcc* r) { return std::min(r->n_dataset, r->n_model); }

// the streaming reduction's parameter block over `n` correspondences of ONE scan of the operator, pre-transform the identity, into its
// own partial rows; the caller sets what differs (nposes, Tpre, Tpre_dev)
inline ReduceParams reduce_params(const rmclhip_rcc* r, uint32_t n, float max_dist, uint32_t nblocks) {
  ReduceParams p;
  std::memset(&p, 0, sizeof(p));
  p.dataset_points = r->ds_pts; p.dataset_mask = r->ds_has_mask ? r->ds_msk : nullptr;
  p.model_points = r->d_points.p; p.model_normals = r->d_normals.p; p.model_mask = r->d_hits.p;
  p.n = n; p.nposes = 1; p.max_dist = max_dist;
  p.Tpre = xidentity();
  p.partials = r->d_partials.p; p.nblocks = nblocks;
  return p;
}

struct rmclhip_pf {
  rmclhip_ctx* ctx = nullptr;
  rmclhip_map* map = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  rmclhip_pf_params params{2.0f, 100.0f, 100.0f, 0.0f, {0.05f, 80.0f}, 10000u, 0u};
  DevBuf<float> d_beams;
  PinnedBuf<float> h_beams;  // staging
  hipEvent_t ev_beams = nullptr;      // behind the last copy out of h_beams
  bool beams_copy_pending = false;
  float* errors_dev = nullptr;   // rmclhip_pf_set_error_output: the caller's device memory
  int variant = 0;
  uint32_t refill_thr = 0, tail_lanes = 8;  // schedule knobs of the round-3 kernel (0: from `refill`); rmclhip_pf_set_schedule
  // rmclhip_pf_set_mapping: 0 beam-minor blocks of ~2048 rays (default), 1 particle-minor blocks (measured neutral, kept for A/B); nothing else is accepted
  bool cpc_grid = true;            // correspondence_type 1: seed every closest-point query from the map's near grid (A/B: rmclhip_pf_set_mapping bit 8 clears it)
  ChainTag tag;                    // completion tag of the synchronous kernel-only calls (update, motion update, extract_weights)
  bool slot_order = false;         // rmclhip_pf_set_variant bit 11
  bool accum = true;               // order-independent likelihood accumulation (round 5 default: no error scratch, no in-order chain); rmclhip_pf_set_variant bit 12 clears it (A/B: rounds 3 / 4)
  DevBuf<double> d_gpow;           // g^i, i = 0 .. n_beams, g = max_n_meas / (max_n_meas + 1): its merge weights
  uint32_t gpow_beams = 0, gpow_max = 0;
  bool evals_global = true;        // k_pf_update_v3 keeps a workgroup's beam errors in global scratch, not LDS (A/B: rmclhip_pf_set_mapping bit 9 clears it)
  DevBuf<float> d_evals;           // [n_particles * n_beams], grow-only
  int mapping = 0;
  uint32_t map_ppb = 0;            // particles per workgroup of the particle-minor mapping (0: 32)
  const uint32_t* order = nullptr; // slot -> particle (device), borrowed or d_order
  uint32_t order_n = 0;
  DevBuf<uint32_t> d_order;
  bool beams_at_origin = false;  // of the beams uploaded last: all start at the sensor origin
  bool legacy = false;      // A/B: the round-2 kernel (k_pf_update_persist)
  bool big_blocks = false;  // A/B: 4096 rays per workgroup
  bool pf_tree = true;      // quantised nodes of the filter's own tree (leaves <= kPfLeafTris); false: the map's tree (A/B)
  bool full_nodes = false;  // A/B: persistent lanes on the 128-B nodes instead of their 64-B quantised twins
  int refill = 4;  // 0: rounds of one ray per lane; 1..4: persistent lanes (dynamic ray fetch), refill when 8/16/32/48
                   // lanes of a wave are idle (default 48: the refill block also evaluates the finished beams, which
                   // pays off with many lanes at once; measured best on sphere and room)
  // the surface constraint (capi_surface.cpp): rmclhip_pf_set_surface; the class counts of the last constrained launch land in
  // h_surf (pinned, 4 words) behind that launch on `stream`
  bool surface_on = false;
  rmclhip_surface_params surface{};
  DevBuf<uint32_t> d_surf;
  PinnedBuf<uint32_t> h_surf;
  uint32_t* surf_faces = nullptr;  // rmclhip_debug_surface_faces: the caller's device memory, one word per particle of the next constrained launches
  RefineScratch refine;            // rmclhip_pf_refine (capi_refine.cpp)
  SteinScratch stein;              // rmclhip_pf_stein_step (capi_stein.cpp)
  rmclhip_field* field = nullptr;  // rmclhip_pf_set_field (capi_field.cpp): correspondence_type 1 is answered from this lattice; the handle holds a reference
};

// GladiatorResamplerGPU analogue: owns a stream and the scratch of the {sum, max} reduction
struct rmclhip_resampler {
  rmclhip_ctx* ctx = nullptr;
  hipStream_t stream = nullptr;
  DevBuf<double> d_psum;
  DevBuf<float> d_pmax, d_out;
  PinnedBuf<float> h_out;  // {sum, max}
  ChainTag tag;            // completion tag of the tournament (a kernel-only synchronous call)
  PinnedBuf<unsigned long long> h_res;   // residual resampling's {sum, max, expect, n_draws} + the draws' total (5 words)
  // residual resampling: {double sum, double max, u64 expect, u64 n_draws} on the device, the draws' particle / count / prefix sums
  DevBuf<unsigned long long> d_res_stats, d_res_incl, d_res_btot;
  DevBuf<uint32_t> d_res_idx, d_res_cnt;
  // adaptive count (capi_adaptive.cpp): the bin table (grown to a power of two >= 2 n, cleared per call) and its two counters (landing
  // in h_res[5]); the systematic resampler's prefix sums and block totals
  DevBuf<unsigned long long> d_kld_table, d_sys_incl, d_sys_btot;
  DevBuf<uint32_t> d_kld_cnt;
  // pose hypotheses (capi_hypotheses.cpp), grow-only as the bin table: four 32-bit words per table word {parent, rank, bins, particles},
  // one 64-bit word per table word (weight) followed by the counters, the particles' labels, the cluster records (4 words per occupied
  // bin) followed by the kMaxHypotheses winners; the moment passes' partials (256 * 32) + result (32), also rmclhip_particles_pose_estimate's
  DevBuf<uint32_t> d_hyp_u32, d_hyp_labels;
  DevBuf<unsigned long long> d_hyp_u64, d_hyp_rec;
  DevBuf<double> d_hyp_mom;
};


// the launch reduce_enqueue issues after the reduction: k_reduce_finalize (kTailStats) or k_batch_solve (kTailBatchSolve)
struct ReduceTail {
  uint32_t mode = kTailNone;
  cstats* stats_out = nullptr;          // kTailStats; kTailBatchSolve (nullable there)
  xform* Tdelta_out = nullptr;          // kTailBatchSolve
  unsigned long long* done = nullptr;   // host-mapped completion tag (kTailStats, one pose)
  uint32_t seq = 0;                     // ... and the sequence number it must carry
};

// what the tag's sum covers: `base` always; the `extra` blocks only when *code == 0 (a status block's "done", the exits that
// also wrote a state block) or when there is no code word
struct DoneCheck {
  const void* base = nullptr; size_t base_bytes = 0;
  const volatile uint32_t* code = nullptr;
  const void* extra[3] = {nullptr, nullptr, nullptr}; size_t extra_bytes[3] = {0, 0, 0};
};

// residual resampling (ResidualResamplerCPU.cpp:55-203) in three enqueue phases, each followed by ONE wait of the caller:
//   A prepare: statistics + how many copies a draw inserts on average  -> h_res[0..3]
//   B draws  : a block of draws that fills the cloud with a margin     -> h_res[4] = copies these draws insert (repeat doubled if short)
//   C fill   : the slots [first, first + count) of the new cloud
struct ResidualJob {
  rmclhip_resampler* r = nullptr;
  hipStream_t st = nullptr;
  const rmclhip_transform* poses = nullptr; const rmclhip_particle_attributes* attrs = nullptr;
  rmclhip_transform* poses_new = nullptr; rmclhip_particle_attributes* attrs_new = nullptr;
  uint32_t n_particles = 0, n_new = 0, first = 0, count = 0;
  const rmclhip_gladiator_config* cfg = nullptr;
  uint64_t seed = 0; uint32_t step = 0;
  double want = 0.0;
  uint32_t n_draws = 0;
  bool filled = false;     // phase B's draws cover the new cloud
  bool active = false;     // count != 0 && n_new != 0
};

// ---- defined in one file, called from another --------------------------------------------------------
RMCL_INTERNAL rmclhip_status rebuild_tile_planes(rmclhip_rcc* r, bool keep_tuning = false);
RMCL_INTERNAL int find_variant(const rmclhip_rcc* r, uint32_t nposes);
RMCL_INTERNAL void fill_find_params(rmclhip_rcc* r, FindParams& p, uint32_t nposes, int kind = -1);
RMCL_INTERNAL rmclhip_status ensure_model_buffers(rmclhip_rcc* r, size_t n_total);
RMCL_INTERNAL rmclhip_status find_enqueue(rmclhip_rcc* r, const xform& Tbm, bool* speculate = nullptr);
RMCL_INTERNAL rmclhip_status reduce_enqueue(rmclhip_rcc* r, const xform& Tpre, const xform* Tpre_dev, float max_dist, uint32_t nposes, const ReduceTail& tail);
// capi_rcc.cpp, shared by find / computeCrossStatistics and the corrections (capi_micp.cpp): sequence numbers and completion tags, the
// gate and its band, the moment epilogue of a find and the host's verified copy of what it publishes, the caps a served loop leaves
RMCL_INTERNAL uint32_t next_seq(rmclhip_rcc* r);
RMCL_INTERNAL hipError_t wait_done(const rmclhip_ctx* ctx, volatile const unsigned long long* tag, uint32_t seq, const DoneCheck& chk, hipStream_t stream);
RMCL_INTERNAL hipError_t wait_chain_end(rmclhip_rcc* r);
RMCL_INTERNAL float adaptive_max_dist(const rmclhip_rcc* r, double p);
RMCL_INTERNAL void gate_band(const rmclhip_rcc* r, float centre, float* lo, float* hi);
RMCL_INTERNAL hipError_t wait_moments(rmclhip_rcc* r, uint32_t seq, float lo, float hi, float rho_cap, float tau_cap);
RMCL_INTERNAL void learn_caps(rmclhip_rcc* r, float max_rho, float max_tau);
RMCL_INTERNAL rmclhip_status arm_moment_epilogue(rmclhip_rcc* r, FindParams& fp, int fv, uint32_t nred, float lo, float hi, float rho_cap, float tau_cap, uint32_t* nb_out, uint32_t* wpb_out);
RMCL_INTERNAL rmclhip_status enqueue_find_with_moments(rmclhip_rcc* r, const xform& Tsm, float lo, float hi, float rho_cap, float tau_cap, uint32_t seq, bool epilogue_allowed);
RMCL_INTERNAL rmclhip_status find_batch_enqueue(rmclhip_rcc* r, const rmclhip_transform* Tbm, uint32_t nposes);
RMCL_INTERNAL rmclhip_status batch_order_enqueue(rmclhip_rcc* r, FindParams& p, int variant);   // pose batches in world order (capi_rcc_tune.cpp)
RMCL_INTERNAL rmclhip_status ensure_near_grid(rmclhip_map* m, hipStream_t stream, bool full, const NearGrid** out);
RMCL_INTERNAL rmclhip_status map_upload(rmclhip_ctx* ctx, const BvhHost& bvh, rmclhip_map** out);
// forget rates outside [0, 1] or NaN, non-finite noise widths, a trans_dist_metric above 1: RMCLHIP_ERR_INVALID (rmclhip.h states the rule)
RMCL_INTERNAL rmclhip_status resampler_config_check(const char* who, const rmclhip_gladiator_config* cfg);
RMCL_INTERNAL rmclhip_status gladiator_enqueue(rmclhip_resampler* r, const rmclhip_transform* poses_dev, const rmclhip_particle_attributes* attrs_dev, uint32_t n_particles, rmclhip_transform* poses_new_dev, rmclhip_particle_attributes* attrs_new_dev, uint32_t first, uint32_t count, const rmclhip_gladiator_config* cfg, uint64_t seed, uint32_t step, hipStream_t st);
RMCL_INTERNAL rmclhip_status residual_prepare_enqueue(ResidualJob& j);
RMCL_INTERNAL rmclhip_status residual_fill_enqueue(ResidualJob& j, bool want_n_draws);
RMCL_INTERNAL rmclhip_status residual_draws_enqueue(ResidualJob& j, bool first_try);
RMCL_INTERNAL void residual_draws_done(ResidualJob& j);
RMCL_INTERNAL rmclhip_status residual_check(ResidualJob& j);
// capi_particles.cpp: argument checks of the two initialisations (the pose form also factors the covariance) and their launches on `st`;
// the sharded entry points check once and enqueue per rank
struct ParticlesPoseJob { xform Tlm; float L[36]; double chol_err; };
RMCL_INTERNAL rmclhip_status particles_uniform_check(const char* who, uint32_t first, uint32_t count, const float* bb_min, const float* bb_max);
RMCL_INTERNAL rmclhip_status particles_pose_check(const char* who, uint32_t first, uint32_t count, const rmclhip_transform* Tlm, const double* covariance,
                                                  ParticlesPoseJob* job);
// capi_particles.cpp: the range check of every initialisation, and the context's particle stream (created by the first call; the caller
// holds ctx->part_mtx)
RMCL_INTERNAL rmclhip_status particles_range_check(const std::string& who, uint32_t first, uint32_t count);
RMCL_INTERNAL rmclhip_status particles_stream(rmclhip_ctx* ctx);
// capi_surface_sample.cpp: the surface sampler.  Immutable once built; its launches run on the context's particle stream (under
// ctx->part_mtx) or, for a sharded filter's replicas, on the rank's collective stream.  d_count / h_count: the injected slots of the
// call in flight (device word, pinned host word).
struct rmclhip_surface_sampler {
  rmclhip_ctx* ctx = nullptr;
  rmclhip_map* map = nullptr;
  rmclhip_surface_sample_params params{};
  rmclhip_surface_sample_info info{};
  DevBuf<uint32_t> d_rec;
  DevBuf<unsigned long long> d_incl;
  DevBuf<uint32_t> d_count;
  PinnedBuf<uint32_t> h_count;
};
RMCL_INTERNAL rmclhip_status surface_sample_params_check(const std::string& who, const rmclhip_surface_sample_params* p);
RMCL_INTERNAL SurfaceSampleView surface_sample_view(const rmclhip_surface_sampler* sm);
// the threshold of an injection (RMCLHIP_ERR_INVALID for p outside [0, 1] or NaN), and its launch on s with the count's clear in front
// and the count's copy to sm->h_count behind it (no wait; a threshold of 0 enqueues nothing and zeroes *h_count)
RMCL_INTERNAL rmclhip_status surface_inject_threshold(const std::string& who, double p_inject, unsigned long long* out);
RMCL_INTERNAL rmclhip_status surface_inject_enqueue(rmclhip_surface_sampler* sm, xform* poses, void* attrs, uint32_t first, uint32_t count,
                                                    unsigned long long threshold, uint64_t seed, uint32_t step, hipStream_t s);
// capi_surface.cpp: the surface constraint's argument check, and the two launches on f->stream with the copy of their class counts to
// f->h_surf behind them (no wait).  pf_motion_enqueue: the motion update of the handle, constrained when rmclhip_pf_set_surface says so;
// noise: null = the deterministic update, else the sampled odometry model's draw per particle (capi_motion_noise.cpp).
RMCL_INTERNAL rmclhip_status surface_params_check(const char* who, const rmclhip_surface_params* p);
RMCL_INTERNAL rmclhip_status pf_motion_enqueue(rmclhip_pf* f, xform* poses, void* attrs, uint32_t n, const xform& T_bnew_bold, double forget_rate,
                                               uint32_t max_n_meas, bool collision, const MotionNoiseKernelParams* noise = nullptr);
// capi_motion_noise.cpp: the parameters' check, sigma of a step (rmclhip_motion_noise_sigma_host under the caller's name), and the
// check of a noisy call's sigma with the kernel's view of it -- *on is false when all six are zero: the deterministic launch
RMCL_INTERNAL rmclhip_status motion_noise_params_check(const char* who, const rmclhip_motion_noise_params* p);
RMCL_INTERNAL rmclhip_status motion_noise_sigma(const char* who, const rmclhip_motion_noise_params* p, const rmclhip_transform* T, float* sigma_out);
RMCL_INTERNAL rmclhip_status motion_noise_kernel_params(const char* who, const float* sigma, uint64_t seed, uint32_t step, uint32_t first,
                                                        MotionNoiseKernelParams* out, bool* on);
RMCL_INTERNAL rmclhip_status pf_surface_enqueue(rmclhip_pf* f, xform* poses, void* attrs, uint32_t n, const rmclhip_surface_params& sp, uint32_t max_n_meas);
// capi_adaptive.cpp: the checks and launches the pose hypotheses share with the adaptive count.  kld_table_words: the size of the bin
// table count_bins_run fills for n particles; resampler_stats: the likelihoods' maximum, landed on the host
inline uint64_t kld_table_words(uint32_t n) { uint64_t words = 64; while (words < 2ull * n) words <<= 1; return words; }
RMCL_INTERNAL rmclhip_status kld_bins_check(const char* who, const rmclhip_kld_params* p);
RMCL_INTERNAL rmclhip_status resampler_stats(rmclhip_resampler* r, const rmclhip_particle_attributes* attrs_dev, uint32_t n, float* max_out);
RMCL_INTERNAL rmclhip_status count_bins_run(rmclhip_resampler* r, const rmclhip_transform* poses_dev, const rmclhip_particle_attributes* attrs_dev,
                                            uint32_t n, const rmclhip_kld_params* p, float max_l, uint32_t* k_out, uint32_t* n_counted_out);
// capi_hypotheses.cpp: the argument check and the single-device path of the pose hypotheses (the sharded filter runs it on rank 0's
// gathered cloud); labels_dev: nullable
RMCL_INTERNAL rmclhip_status pose_hypotheses_check(const char* who, rmclhip_resampler* r, const rmclhip_kld_params* bins, uint32_t max_hypotheses,
                                                   rmclhip_pose_hypothesis* out, uint32_t* n_out, uint32_t* n_clusters_out);
RMCL_INTERNAL rmclhip_status pose_hypotheses_run(const char* who, rmclhip_resampler* r, const rmclhip_transform* poses_dev,
                                                 const rmclhip_particle_attributes* attrs_dev, uint32_t n, const rmclhip_kld_params* bins,
                                                 uint32_t max_hypotheses, rmclhip_pose_hypothesis* out, uint32_t* n_out, uint32_t* n_clusters_out,
                                                 uint32_t* labels_dev);
// capi_rcc.cpp: the stream and host-mapped scratch of the free functions on caller-owned views (rmclhip_statistics_p2l,
// rmclhip_pose_information_p2l), created by the first call; the caller holds ctx->p2l_mtx
RMCL_INTERNAL rmclhip_status ctx_p2l_ensure(rmclhip_ctx* ctx);
// capi_pose_information.cpp: a result row of launch_pose_information[_robust] -> A, g, rss, n_meas
RMCL_INTERNAL void pose_information_unpack_row(const double* row, rmclhip_pose_information* out);
// capi_field.cpp: a reference less on a field (the last one frees it; null: nothing), and the sensor update answered from f->field
RMCL_INTERNAL void field_release(rmclhip_field* fd);
RMCL_INTERNAL rmclhip_status pf_field_enqueue(rmclhip_pf* f, const rmclhip_transform* poses, rmclhip_particle_attributes* attrs, uint32_t n, uint32_t n_beams,
                                              const rmclhip_transform* Tsb);
// capi_field.cpp: the kernels' view of a field
RMCL_INTERNAL FieldView field_view(const rmclhip_field* fd);
// capi_field.cpp: the geometry of a field over a box (banded: the logical lattice of a banded field, not capped by max_nodes)
RMCL_INTERNAL rmclhip_status field_layout(const std::string& who, const float* bmin, const float* bmax, const rmclhip_field_params* params,
                                          rmclhip_field_info* out, bool banded);
// capi_field.cpp: what rmclhip_field_create and rmclhip_field_create_banded share.  field_create_check: the refusals that come before
// the layout (RMCLHIP_OK leaves *out null); field_new: refuses a map without faces, else a handle with `info` that holds its context,
// its map and a stream of its own and is given up with field_release; field_build_params: the map and the geometry of a level, nothing
// else set; field_level_step: launches the level of `stride` and cn[3] nodes on s, then makes it the level the next one is seeded from
RMCL_INTERNAL rmclhip_status field_create_check(const std::string& who, const rmclhip_ctx* ctx, const rmclhip_map* map, rmclhip_field** out);
RMCL_INTERNAL rmclhip_status field_new(const std::string& who, rmclhip_ctx* ctx, rmclhip_map* map, const rmclhip_field_info& info, rmclhip_field** out);
RMCL_INTERNAL FieldBuildParams field_build_params(const rmclhip_field* fd);
RMCL_INTERNAL hipError_t field_level_step(FieldBuildParams& p, uint32_t stride, const uint32_t* cn, uint32_t* rec_out, float* dist_out, hipStream_t s);
// capi_band_field.cpp: RMCLHIP_ERR_INVALID if `field` is banded and max_dist exceeds its band (null or dense: RMCLHIP_OK)
RMCL_INTERNAL rmclhip_status field_band_check(const std::string& who, const rmclhip_field* field, float max_dist);
// capi_refine.cpp: the refinement in two halves, so that the sharded filter has every device's launch in flight before it waits for any.
// refine_check refuses what the header lists (params null: the defaults are written to *out); refine_enqueue uploads the beams and
// launches on `stream`; refine_finish waits for the stream and ADDS this call's counts to *stats (nullable)
RMCL_INTERNAL rmclhip_status refine_check(const std::string& who, const void* poses_dev, uint32_t n, const rmclhip_range_measurement* beams, uint32_t n_beams,
                                          const rmclhip_transform* Tsb, const rmclhip_refine_params* params, rmclhip_refine_params* out);
// refine_kernel_params: what the refine and the Stein kernels read of a field, a cloud, its beams (device records) and the parameters;
// rows and counters are left null
RMCL_INTERNAL RefineKernelParams refine_kernel_params(const rmclhip_field* field, rmclhip_transform* poses_dev, uint32_t n, const float* beams_dev,
                                                      uint32_t n_beams, const rmclhip_transform* Tsb, const rmclhip_refine_params& params);
RMCL_INTERNAL rmclhip_status refine_enqueue(const rmclhip_field* field, hipStream_t stream, RefineScratch& sc, rmclhip_transform* poses_dev, uint32_t n,
                                            const rmclhip_range_measurement* beams, uint32_t n_beams, const rmclhip_transform* Tsb,
                                            const rmclhip_refine_params& params, rmclhip_refine_result* results_dev, bool want_stats);
RMCL_INTERNAL rmclhip_status refine_finish(hipStream_t stream, RefineScratch& sc, uint32_t n, rmclhip_refine_stats* stats);
//@@DECLS@@

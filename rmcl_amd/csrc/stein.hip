// stein.hip -- a Stein variational step of the particle cloud on the map's distance field (include/rmclhip.h, STEIN STEP ON THE FIELD,
// states the arithmetic; tests/stein_ref.py restates it in numpy).  One iteration is seven launches on one stream:
//
//   k_stein_drive     one wave per particle, four per workgroup: refine's pass at the pose and its first solve (refine_step.hip.h) --
//                     the particle's own move, six floats.
//   k_stein_insert    one lane per particle: the key of its translation bin into an open-addressing table (the probe of
//                     k_kld_count_bins), the word's particle count.  Lanes of a wave that share a word add ONCE (their number), so a
//                     converged cloud issues one atomic per wave, not 64 on one word.
//   k_stein_decide    one lane per particle: listed or thinned away -- a function of the particle's index and its bin's count alone --
//                     and the word's listed count, added the same way.
//   k_scan_*          resample.hip's exact prefix sums over the listed counts: where every bin's records start.
//   k_stein_scatter   one lane per listed particle: its 64-byte record {position, index, rotation, drive} behind its bin's start.  The
//                     order inside a bin is the atomics'; nothing reads it as an order.
//   k_stein_pair      one wave per particle: the (at most 27) bins around its own are probed by one lane each, the lanes stride over a
//                     bin's contiguous records, every pair inside the kernel's support adds to 13 sums of 64-bit integers per lane,
//                     an integer butterfly totals them -- exact, so the same for any order of the records --, and the move is
//                     limited and applied by refine's rules.  No atomics.
//
// A particle's pose is rewritten by its own wave alone and read by no other: neighbours are read from the records, which hold the
// poses of the iteration's start.
#include "kld_bins.hip.h"
#include "refine_step.hip.h"

namespace rmclhip {
namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;       // slot_of: the particle's pose is not finite
constexpr uint32_t kListedBit = 0x80000000u;    // slot_of: the particle is listed (a table has at most 2^27 words)

// the bin of a translation on the free axes, index + 8192 (14 bits); a locked axis is ignored (kld_bins.hip.h: bin_lin of width 0)
__device__ __forceinline__ void stein_bins(const f3& t, uint32_t mask, float width, uint32_t (&b)[3]) {
  b[0] = static_cast<uint32_t>(bin_lin(t.x, (mask & 1u) ? width : 0.0f));
  b[1] = static_cast<uint32_t>(bin_lin(t.y, (mask & 2u) ? width : 0.0f));
  b[2] = static_cast<uint32_t>(bin_lin(t.z, (mask & 4u) ? width : 0.0f));
}
__device__ __forceinline__ unsigned long long stein_key(uint32_t bx, uint32_t by, uint32_t bz) {
  return static_cast<unsigned long long>(bx) | (static_cast<unsigned long long>(by) << 14) | (static_cast<unsigned long long>(bz) << 28);
}

// Q(x) = int64(rint(double(x) * 2^32))
__device__ __forceinline__ long long stein_q(float x) { return static_cast<long long>(rint(static_cast<double>(x) * 4294967296.0)); }

__device__ __forceinline__ long long stein_wave_sum(long long x) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, 64);
  return x;
}

// every lane with `on` adds 1 to words[slot]: the lanes of the wave that name the same word add once, through the lowest of them.
// Returns what the word held before this wave's add plus the lane's rank among its lanes; *group (nullable): how many lanes shared
// the add, in its leading lane, 0 in every other.  Every lane of the wave must call.
__device__ __forceinline__ uint32_t stein_add_per_word(uint32_t* __restrict__ words, uint32_t slot, bool on, uint32_t* group) {
  const uint32_t lane = threadIdx.x & 63u;
  unsigned long long todo = __ballot(on);
  uint32_t before = 0u;
  if (group) *group = 0u;
  while (todo != 0ull) {   // wave-uniform
    const int leader = __ffsll(static_cast<long long>(todo)) - 1;
    const uint32_t s = __shfl(slot, leader, 64);
    const unsigned long long same = __ballot(on && slot == s);
    const uint32_t k = static_cast<uint32_t>(__popcll(same));
    uint32_t old = 0u;
    if (lane == static_cast<uint32_t>(leader)) {
      old = atomicAdd(&words[s], k);
      if (group) *group = k;
    }
    old = __shfl(old, leader, 64);
    if (on && slot == s) before = old + static_cast<uint32_t>(__popcll(same & ((1ull << lane) - 1ull)));
    todo &= ~same;
  }
  return before;
}

// ---------------------------------------------------------------------------------------------
// 1. the drive
// ---------------------------------------------------------------------------------------------
template <bool kBanded>
__global__ void __launch_bounds__(256) k_stein_drive(const SteinKernelParams p) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t pi = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (pi >= p.r.n_particles) return;   // the whole wave leaves
  const xform pose = p.r.poses[pi];
  const bool finite = surface_pose_finite(pose);
  RefineSums S;
  refine_pass<kBanded>(p.r, pose, lane, S);
  double delta[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool ok = false;
  if (finite && S.n_used != 0u)   // wave-uniform
    ok = refine_solve(S.A, S.b, p.r.dof_mask & 0x3Fu, static_cast<double>(p.r.lambda0), p.r.max_step_trans, p.r.max_step_rot, delta);
  if (lane != 0u) return;
  float* d = p.drive + static_cast<size_t>(kSteinDriveStride) * pi;
#pragma unroll
  for (int k = 0; k < 6; ++k) d[k] = ok ? static_cast<float>(delta[k]) : 0.0f;
  d[6] = 0.0f; d[7] = 0.0f;
  if (p.rows != nullptr) {
    uint32_t* row = p.rows + 4u * static_cast<size_t>(pi);
    row[0] = __float_as_uint(static_cast<float>(S.C));
    row[1] = S.n_used;
  }
  if (!finite) atomicAdd(p.counters + 0, 1u);
  else if (S.n_used == 0u) atomicAdd(p.counters + 1, 1u);
}

// ---------------------------------------------------------------------------------------------
// 2. the cell list
// ---------------------------------------------------------------------------------------------
// table: mask + 1 words, all kEmptySlot on entry; count: zero on entry.  No lane leaves before the ballots.
__global__ void __launch_bounds__(kBlock) k_stein_insert(const SteinKernelParams p, unsigned long long mask) {
  const uint32_t n = p.r.n_particles;
  const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  uint32_t slot = kNoSlot;
  bool inserted = false;
  if (i < n) {
    const xform T = p.r.poses[i];
    if (surface_pose_finite(T)) {
      uint32_t b[3];
      stein_bins(T.t, p.r.dof_mask, 1.001f * p.h_trans, b);
      const unsigned long long key = stein_key(b[0], b[1], b[2]);
      // at most n keys, >= 2 n words: the probe meets its key or an empty word before it has gone round (adaptive.hip)
      unsigned long long sl = mix64(key) & mask;
      for (;;) {
        unsigned long long cur = __atomic_load_n(&p.table[sl], __ATOMIC_RELAXED);
        if (cur == kEmptySlot) {
          cur = atomicCAS(&p.table[sl], kEmptySlot, key);
          if (cur == kEmptySlot) { inserted = true; break; }
        }
        if (cur == key) break;
        sl = (sl + 1ull) & mask;
      }
      slot = static_cast<uint32_t>(sl);
    }
  }
  uint32_t group = 0u;
  const uint32_t before = stein_add_per_word(p.count, slot, slot != kNoSlot, &group);
  // a bin is thinned when its count passes max_per_bin: exactly one add per such bin takes it from <= max_per_bin to beyond
  const bool crossed = group != 0u && before <= p.max_per_bin &&
                       static_cast<unsigned long long>(before) + group > static_cast<unsigned long long>(p.max_per_bin);
  const unsigned long long m_ins = __ballot(inserted), m_thin = __ballot(crossed);
  if ((threadIdx.x & 63u) == 0u) {
    if (m_ins) atomicAdd(p.counters + 2, static_cast<uint32_t>(__popcll(m_ins)));
    if (m_thin) atomicAdd(p.counters + 3, static_cast<uint32_t>(__popcll(m_thin)));
  }
  if (i < n) p.slot_of[i] = slot;
}

// listed: every particle of a bin of at most max_per_bin; of a fuller bin those with uint64(r) * count < uint64(max_per_bin) << 32,
// r = word 0 of draw 8 of the resamplers' stream at (index, step)
__global__ void __launch_bounds__(kBlock) k_stein_decide(const SteinKernelParams p) {
  const uint32_t n = p.r.n_particles;
  const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  const uint32_t slot = (i < n) ? p.slot_of[i] : kNoSlot;
  bool listed = false;
  if (slot != kNoSlot) {
    const uint32_t c = p.count[slot];
    listed = c <= p.max_per_bin;
    if (!listed) {
      uint32_t r[4];
      philox4x32_10(static_cast<uint32_t>(i), p.step, 8u, 0u, p.key0, p.key1, r);
      listed = static_cast<unsigned long long>(r[0]) * c < (static_cast<unsigned long long>(p.max_per_bin) << 32);
    }
  }
  (void)stein_add_per_word(p.listed, slot, listed, nullptr);
  if (listed) p.slot_of[i] = slot | kListedBit;
}

// incl: the inclusive prefix sums of `listed`; cursor: zero on entry
__global__ void __launch_bounds__(kBlock) k_stein_scatter(const SteinKernelParams p) {
  const uint32_t n = p.r.n_particles;
  const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  const uint32_t v = (i < n) ? p.slot_of[i] : kNoSlot;
  const bool listed = v != kNoSlot && (v & kListedBit) != 0u;
  const uint32_t slot = v & ~kListedBit;
  const uint32_t rank = stein_add_per_word(p.cursor, slot, listed, nullptr);
  if (!listed) return;
  const unsigned long long pos = (p.incl[slot] - p.listed[slot]) + rank;
  if (pos >= n) return;   // (never: the listed counts sum to at most n)
  const xform T = p.r.poses[i];
  const float* d = p.drive + static_cast<size_t>(kSteinDriveStride) * i;
  uint4* rec = reinterpret_cast<uint4*>(p.records + static_cast<size_t>(kSteinRecordWords) * pos);
  rec[0] = make_uint4(__float_as_uint(T.t.x), __float_as_uint(T.t.y), __float_as_uint(T.t.z), static_cast<uint32_t>(i));
  rec[1] = make_uint4(__float_as_uint(T.R.x), __float_as_uint(T.R.y), __float_as_uint(T.R.z), __float_as_uint(T.R.w));
  rec[2] = make_uint4(__float_as_uint(d[0]), __float_as_uint(d[1]), __float_as_uint(d[2]), __float_as_uint(d[3]));
  rec[3] = make_uint4(__float_as_uint(d[4]), __float_as_uint(d[5]), 0u, 0u);
}

// ---------------------------------------------------------------------------------------------
// 3. pair sums and the move
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_stein_pair(const SteinKernelParams p, unsigned long long tmask) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t pi = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (pi >= p.r.n_particles) return;   // the whole wave leaves
  const xform pose = p.r.poses[pi];
  const uint32_t mask = p.r.dof_mask & 0x3Fu;
  uint32_t* row = (p.rows != nullptr) ? p.rows + 4u * static_cast<size_t>(pi) : nullptr;
  if (!surface_pose_finite(pose)) {   // untouched, nobody's neighbour (it has no record)
    if (lane == 0u && row != nullptr) { row[2] = 0u; row[3] = 0u; }
    return;
  }
  const float h_trans = p.h_trans, h_rot = p.h_rot;
  const quat qi_conj = {-pose.R.x, -pose.R.y, -pose.R.z, pose.R.w};
  uint32_t b[3];
  stein_bins(pose.t, mask, 1.001f * h_trans, b);
  long long W = 0ll, D[6] = {0ll, 0ll, 0ll, 0ll, 0ll, 0ll}, R[6] = {0ll, 0ll, 0ll, 0ll, 0ll, 0ll};
  uint32_t n_nb = 0u;
  // lanes 0 .. 26 each probe one of the 3 x 3 x 3 bins around the particle's own (one per locked axis), so the probes' dependent loads
  // run side by side and not one bin after the other; the table is at most half full, so a probe meets its key or an empty word
  uint32_t my_listed = 0u, my_count = 0u;
  unsigned long long my_start = 0ull;
  if (lane < 27u) {
    const int dx = static_cast<int>(lane % 3u) - 1, dy = static_cast<int>((lane / 3u) % 3u) - 1, dz = static_cast<int>(lane / 9u) - 1;
    const int nx = static_cast<int>(b[0]) + dx, ny = static_cast<int>(b[1]) + dy, nz = static_cast<int>(b[2]) + dz;
    // a locked axis has its one bin; a bin index is 0 .. 16383: what lies beyond does not exist (no wrap)
    const bool exists = ((mask & 1u) || dx == 0) && ((mask & 2u) || dy == 0) && ((mask & 4u) || dz == 0) && nx >= 0 && nx <= 16383 &&
                        ny >= 0 && ny <= 16383 && nz >= 0 && nz <= 16383;
    if (exists) {
      const unsigned long long key = stein_key(static_cast<uint32_t>(nx), static_cast<uint32_t>(ny), static_cast<uint32_t>(nz));
      unsigned long long sl = mix64(key) & tmask;
      for (;;) {
        const unsigned long long cur = p.table[sl];
        if (cur == key) {
          my_listed = p.listed[sl];
          my_count = p.count[sl];
          my_start = p.incl[sl] - my_listed;
          break;
        }
        if (cur == kEmptySlot) break;
        sl = (sl + 1ull) & tmask;
      }
    }
  }
  // the bins that list somebody, one after the other (wave-uniform); the lanes stride over a bin's records
  for (unsigned long long todo = __ballot(my_listed != 0u); todo != 0ull; todo &= todo - 1ull) {
    const int src = __ffsll(static_cast<long long>(todo)) - 1;
    const uint32_t n_listed = __shfl(my_listed, src, 64);
    const float w_bin = static_cast<float>(__shfl(my_count, src, 64)) / static_cast<float>(n_listed);
    const unsigned long long start = __shfl(my_start, src, 64);
    for (uint32_t r = lane; r < n_listed; r += 64u) {
      const uint4* rec = reinterpret_cast<const uint4*>(p.records + static_cast<size_t>(kSteinRecordWords) * (start + r));
      const uint4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
      if (r0.w == pi) continue;
      const float drive_j[6] = {__uint_as_float(r2.x), __uint_as_float(r2.y), __uint_as_float(r2.z), __uint_as_float(r2.w),
                                __uint_as_float(r3.x), __uint_as_float(r3.y)};
      float e[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      float s = 0.0f;
      if (mask & 1u) { e[0] = (__uint_as_float(r0.x) - pose.t.x) / h_trans; s = s + e[0] * e[0]; }
      if (mask & 2u) { e[1] = (__uint_as_float(r0.y) - pose.t.y) / h_trans; s = s + e[1] * e[1]; }
      if (mask & 4u) { e[2] = (__uint_as_float(r0.z) - pose.t.z) / h_trans; s = s + e[2] * e[2]; }
      if (mask & 0x38u) {
        const quat qj = {__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z), __uint_as_float(r1.w)};
        const quat dq = qmul(qj, qi_conj);
        float rho[3] = {2.0f * dq.x, 2.0f * dq.y, 2.0f * dq.z};
        if (dq.w < 0.0f) { rho[0] = -rho[0]; rho[1] = -rho[1]; rho[2] = -rho[2]; }
        if (mask & 8u) { e[3] = rho[0] / h_rot; s = s + e[3] * e[3]; }
        if (mask & 16u) { e[4] = rho[1] / h_rot; s = s + e[4] * e[4]; }
        if (mask & 32u) { e[5] = rho[2] / h_rot; s = s + e[5] * e[5]; }
      }
      if (s < 1.0f) {
        const float u = 1.0f - s;
        const float kk = u * u;
        const float a = w_bin * kk;
        const float wu = w_bin * u;
        W += stein_q(a);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          if ((mask >> k) & 1u) {
            D[k] += stein_q(a * drive_j[k]);
            R[k] += stein_q(wu * e[k]);
          }
        }
        ++n_nb;
      }
    }
  }
  if (lane == 0u) {   // the self term
    const float* d = p.drive + static_cast<size_t>(kSteinDriveStride) * pi;
    W += 4294967296ll;
#pragma unroll
    for (int k = 0; k < 6; ++k)
      if ((mask >> k) & 1u) D[k] += stein_q(d[k]);
  }
  W = stein_wave_sum(W);
#pragma unroll
  for (int k = 0; k < 6; ++k) { D[k] = stein_wave_sum(D[k]); R[k] = stein_wave_sum(R[k]); }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) n_nb += __shfl_xor(n_nb, s, 64);
  // the move, in double: the kernel-weighted mean of the drives, minus repulsion * 4 * h_k * the mean of w u e_k
  double phi[6];
  const double Wd = static_cast<double>(W);
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double c = (static_cast<double>(p.repulsion) * 4.0) * static_cast<double>(k < 3 ? h_trans : h_rot);
    phi[k] = ((mask >> k) & 1u) ? (static_cast<double>(D[k]) - c * static_cast<double>(R[k])) / Wd : 0.0;
  }
  refine_limit(phi, p.r.max_step_trans, p.r.max_step_rot);
  const xform moved = refine_candidate(pose, phi, mask);
  if (lane != 0u) return;
  p.r.poses[pi] = moved;
  if (row != nullptr) {
    row[2] = n_nb;
    row[3] = __float_as_uint(static_cast<float>(Wd * (1.0 / 4294967296.0)));
  }
}

inline uint32_t blocks_of(uint32_t n, uint32_t per_block) { return static_cast<uint32_t>((static_cast<uint64_t>(n) + per_block - 1u) / per_block); }

}  // namespace

hipError_t launch_stein_iteration(const SteinKernelParams& p, hipStream_t s, hipEvent_t* events) {
  const uint32_t n = p.r.n_particles;
  if (n == 0u) return hipSuccess;
  if (n > kSteinMaxParticles || p.r.n_beams == 0u || p.r.n_beams > kRefineMaxBeams || p.max_per_bin == 0u) return hipErrorInvalidValue;
  // a power of two >= 2 n: the probe loops' guarantee of an empty word
  if (p.table_words < 2ull * n || (p.table_words & (p.table_words - 1ull)) != 0ull || p.table_words > (1ull << 27)) return hipErrorInvalidValue;
  const unsigned long long tmask = p.table_words - 1ull;
  const uint32_t words = static_cast<uint32_t>(p.table_words);
  hipError_t e = hipMemsetAsync(p.counters, 0, kSteinCounters * sizeof(uint32_t), s);
  if (e == hipSuccess && events) e = hipEventRecord(events[0], s);
  if (e != hipSuccess) return e;
  if (p.r.fv.lat != nullptr) hipLaunchKernelGGL(k_stein_drive<false>, dim3(blocks_of(n, 4u)), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(k_stein_drive<true>, dim3(blocks_of(n, 4u)), dim3(256), 0, s, p);   // a banded field
  if (events) e = hipEventRecord(events[1], s);
  if (e == hipSuccess) e = hipMemsetAsync(p.table, 0xFF, p.table_words * sizeof(unsigned long long), s);
  if (e == hipSuccess) e = hipMemsetAsync(p.count, 0, p.table_words * sizeof(uint32_t), s);
  if (e == hipSuccess) e = hipMemsetAsync(p.listed, 0, p.table_words * sizeof(uint32_t), s);
  if (e == hipSuccess) e = hipMemsetAsync(p.cursor, 0, p.table_words * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_stein_insert, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, s, p, tmask);
  hipLaunchKernelGGL(k_stein_decide, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, s, p);
  e = launch_scan_counts(p.listed, words, p.incl, p.block_tot, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_stein_scatter, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, s, p);
  if (events) e = hipEventRecord(events[2], s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_stein_pair, dim3(blocks_of(n, 4u)), dim3(256), 0, s, p, tmask);
  if (events) e = hipEventRecord(events[3], s);
  if (e != hipSuccess) return e;
  return hipGetLastError();
}

}  // namespace rmclhip

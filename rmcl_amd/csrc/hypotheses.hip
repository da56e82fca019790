// hypotheses.hip -- pose hypotheses: the connected components of the cloud's occupied bins, weighed and ranked on the device
// (include/rmclhip.h, POSE HYPOTHESES, states the rules; tests/hypotheses_ref.py restates them in numpy).  Input: the table of occupied
// bins k_kld_count_bins left (adaptive.hip), read with the one key rule of kld_bins.hip.h.  A bin is named by the index of its table
// word; `parent` is a union-find forest over those indices.
//
//   k_hyp_init        parent[s] = s, rank[s] = none, the per-word sums and the counters zeroed
//   k_hyp_link        one lane per occupied word: the keys of its neighbours (only the active fields are enumerated) are looked up
//                     read-only and the two sets united lock-free (compare-and-swap on a root's own word; the root of the smaller key
//                     wins, so parent pointers lead to strictly smaller keys and a finished component's root carries key_min)
//   k_hyp_flatten     every occupied word walks to its root and stores it (pointer jumping: afterwards parent[s] IS the root); bins per
//                     root and the number of roots
//   k_hyp_accumulate  one lane per particle: its bin's root; integer weight and count are combined within the wave per distinct root
//                     and added with one vector atomic per root and wave (a converged cloud puts thousands of particles on one root:
//                     11.4 ms against 0.43 ms for queuing on one word, profiles/adaptive_resample_time.txt)
//   k_hyp_compact     the roots' records {key_min, weight, bins, particles, root} as a dense list (order irrelevant: the ranking is total)
//   k_hyp_rank        one workgroup, max_hypotheses rounds of "the best record strictly after the previous winner": no marking, and
//                     the same winners whatever the order of the list
//   k_hyp_labels      particle -> rank of its root (0xFFFFFFFF beyond the cut and for uncounted particles)
// Integer atomics only: every sum is exact and independent of the schedule.  The moments of one hypothesis are k_pose_moments
// (kernels.hip) with these labels as its filter.
#include "kernels.h"
#include "kld_bins.hip.h"

namespace rmclhip {
namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kNone = 0xFFFFFFFFu;

// field f of a key: x y z roll pitch yaw
__device__ __forceinline__ constexpr uint32_t f_shift(int f) { return f == 0 ? 0u : f == 1 ? 14u : f == 2 ? 28u : f == 3 ? 42u : f == 4 ? 49u : 56u; }
__device__ __forceinline__ constexpr int32_t f_max(int f) { return f < 3 ? 16383 : 126; }
__device__ __forceinline__ constexpr bool f_wraps(int f) { return f == 3 || f == 5; }

__global__ void __launch_bounds__(kBlock) k_hyp_init(uint32_t* __restrict__ parent, uint32_t* __restrict__ rank, uint32_t* __restrict__ n_bins,
                                                     uint32_t* __restrict__ n_part, unsigned long long* __restrict__ weight, unsigned long long words,
                                                     unsigned long long* __restrict__ counters) {
  const unsigned long long s = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (s < kHypCounters) counters[s] = 0ull;
  if (s >= words) return;
  parent[s] = static_cast<uint32_t>(s);
  rank[s] = kNone;
  n_bins[s] = 0u;
  n_part[s] = 0u;
  weight[s] = 0ull;
}

// The forest's invariant: a word that is not its own parent points to a word with a strictly smaller key (k_hyp_link hooks the root
// of the larger key under the root of the smaller one; halving replaces a pointer by one further up the same path), and a word that
// has left the roots never returns to them.  Keys are distinct, so every walk along parent pointers ends at a root after fewer steps
// than there are bins -- whatever the other lanes store meanwhile.
__device__ __forceinline__ uint32_t uf_find_halving(uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = __atomic_load_n(&parent[x], __ATOMIC_RELAXED);
    if (p == x) return x;
    const uint32_t g = __atomic_load_n(&parent[p], __ATOMIC_RELAXED);
    if (g == p) return p;
    __atomic_store_n(&parent[x], g, __ATOMIC_RELAXED);   // x is not a root (never compared-and-swapped again): a plain shortcut
    x = g;
  }
}

// Lock-free union.  A compare-and-swap fails only because another lane hooked that very root in between, and a root is hooked once:
// at most (bins - 1) hooks ever happen, so this loop runs at most that many times more than once -- no lane waits for another's progress.
__device__ __forceinline__ void uf_unite(uint32_t* parent, const unsigned long long* __restrict__ table, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find_halving(parent, a);
    b = uf_find_halving(parent, b);
    if (a == b) return;
    if (table[a] > table[b]) { const uint32_t t = a; a = b; b = t; }   // a: the smaller key wins
    const uint32_t old = atomicCAS(&parent[b], b, a);
    if (old == b) return;
    b = old;                                                           // b has a parent now: go on from there
  }
}

struct HypBins { float bin_xyz[3], bin_rpy[3]; };

// candidate `c` of a field whose own index is i: c < 3: i - 1 + c; a field that wraps adds, at index 0, {last - 1, last} and, at
// indices >= last - 1, {0}.  (Candidates may repeat or name the bin itself: uniting twice, or with itself, changes nothing.)
__device__ __forceinline__ uint32_t f_count(bool active, bool wraps, int32_t i, int32_t last) {
  if (!active) return 1u;
  if (!wraps) return 3u;
  return (i == 0) ? 5u : (i >= last - 1 ? 4u : 3u);
}
__device__ __forceinline__ int32_t f_candidate(bool active, int32_t i, uint32_t c, int32_t last) {
  if (!active) return i;
  if (c < 3u) return i - 1 + static_cast<int32_t>(c);
  if (c == 3u) return (i == 0) ? last - 1 : 0;
  return last;
}

__global__ void __launch_bounds__(kBlock) k_hyp_link(const unsigned long long* __restrict__ table, unsigned long long mask, HypBins hb,
                                                     uint32_t* __restrict__ parent) {
  const unsigned long long s = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (s > mask) return;
  const unsigned long long key = table[s];
  if (key == kEmptySlot) return;
  int32_t idx[6], last[6];
  uint32_t cnt[6];
  bool active[6];
  uint32_t total = 1u;
#pragma unroll
  for (int f = 0; f < 6; ++f) {
    const float width = f < 3 ? hb.bin_xyz[f] : hb.bin_rpy[f - 3];
    active[f] = width != 0.0f;
    idx[f] = static_cast<int32_t>((key >> f_shift(f)) & static_cast<unsigned long long>(f < 3 ? 0x3FFF : 0x7F));
    last[f] = f_wraps(f) ? static_cast<int32_t>(bin_ang(3.14159265f, width)) : 0;
    cnt[f] = f_count(active[f], f_wraps(f), idx[f], last[f]);
    total *= cnt[f];                                        // <= 3^4 * 5^2
  }
  // `total` combinations, each with one look-up that ends at the key or at an empty word (the table is not written here and at least
  // half of it is empty) and one union (see uf_unite): the loop ends by construction.  Only neighbours with a LARGER key are looked
  // up: the pair is found from its smaller side.
  for (uint32_t e = 0u; e < total; ++e) {
    uint32_t rem = e;
    unsigned long long nk = 0ull;
    bool valid = true;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
      const uint32_t c = rem % cnt[f];
      rem /= cnt[f];
      const int32_t v = f_candidate(active[f], idx[f], c, last[f]);
      valid = valid && v >= 0 && v <= f_max(f);
      nk |= static_cast<unsigned long long>(static_cast<uint32_t>(v)) << f_shift(f);
    }
    if (!valid || nk <= key) continue;
    unsigned long long slot = mix64(nk) & mask;
    for (;;) {
      const unsigned long long cur = table[slot];
      if (cur == nk) { uf_unite(parent, table, static_cast<uint32_t>(s), static_cast<uint32_t>(slot)); break; }
      if (cur == kEmptySlot) break;
      slot = (slot + 1ull) & mask;
    }
  }
}

// Called by all 64 lanes of a wave together.  Every round serves the root of the lowest lane still waiting and clears at least that
// lane's bit: at most 64 rounds.  The lanes of that root sum their values across the wave and the lowest of them issues the atomics.
template <bool kWeights>
__device__ __forceinline__ void wave_add_by_root(bool active, uint32_t root, unsigned long long w, uint32_t c, unsigned long long* __restrict__ weight,
                                                 uint32_t* __restrict__ count) {
  const uint32_t lane = threadIdx.x & 63u;
  unsigned long long todo = __ballot(active);
  while (todo != 0ull) {
    const uint32_t leader = static_cast<uint32_t>(__ffsll(static_cast<long long>(todo)) - 1);
    const uint32_t r = __builtin_amdgcn_readfirstlane(__shfl(root, static_cast<int>(leader), 64));
    const bool mine = active && root == r;
    const unsigned long long m = __ballot(mine);
    unsigned long long sw = mine ? w : 0ull;
    uint32_t sc = mine ? c : 0u;
    if ((m & (m - 1ull)) != 0ull) {                 // (wave-uniform) more than one lane on this root
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        sc += __shfl_xor(sc, off, 64);
        if (kWeights) sw += __shfl_xor(sw, off, 64);
      }
    }
    if (lane == leader) {
      atomicAdd(&count[r], sc);
      if (kWeights) atomicAdd(&weight[r], sw);
    }
    todo &= ~m;
  }
}

// counters[0] = roots.  No lane leaves before the ballots: every wave of the launch reaches them whole.
__global__ void __launch_bounds__(kBlock) k_hyp_flatten(const unsigned long long* __restrict__ table, unsigned long long mask,
                                                        uint32_t* __restrict__ parent, uint32_t* __restrict__ n_bins,
                                                        unsigned long long* __restrict__ counters) {
  const unsigned long long s = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  const bool occupied = s <= mask && table[s] != kEmptySlot;
  uint32_t root = kNone;
  if (occupied) {
    // the link pass is complete: the roots are final.  The walk follows strictly decreasing keys (see uf_find_halving) and other
    // lanes only replace a pointer by the root of the same tree: it ends at that root.
    uint32_t x = static_cast<uint32_t>(s);
    for (;;) {
      const uint32_t p = __atomic_load_n(&parent[x], __ATOMIC_RELAXED);
      if (p == x) break;
      x = p;
    }
    root = x;
    if (root != static_cast<uint32_t>(s)) __atomic_store_n(&parent[s], root, __ATOMIC_RELAXED);
  }
  wave_add_by_root<false>(occupied, root, 0ull, 1u, nullptr, n_bins);
  const unsigned long long m_root = __ballot(occupied && root == static_cast<uint32_t>(s));
  if ((threadIdx.x & 63u) == 0u && m_root) atomicAdd(&counters[0], static_cast<unsigned long long>(__popcll(m_root)));
}

// labels[i] = the table word of particle i's root (kNone: not counted); counters[1] = the total weight.  Whole waves reach the ballots.
__global__ void __launch_bounds__(kBlock) k_hyp_accumulate(const xform* __restrict__ poses, const pattr36* __restrict__ attrs, uint32_t n, KldBins b,
                                                           double max_l, const unsigned long long* __restrict__ table, unsigned long long mask,
                                                           const uint32_t* __restrict__ parent, unsigned long long* __restrict__ weight,
                                                           uint32_t* __restrict__ n_part, unsigned long long* __restrict__ counters,
                                                           uint32_t* __restrict__ labels) {
  const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  bool active = false;
  uint32_t root = kNone;
  unsigned long long w = 0ull;
  if (i < n) {
    const xform T = poses[i];
    const float L = attrs[i].mean;
    unsigned long long key = 0ull;
    if (kld_particle_key(T, L, b, key)) {
      // the key was stored by k_kld_count_bins; the probe ends at it (or, were it missing, at an empty word: the table is half empty)
      unsigned long long slot = mix64(key) & mask;
      for (;;) {
        const unsigned long long cur = table[slot];
        if (cur == key) { root = parent[slot]; active = true; break; }
        if (cur == kEmptySlot) break;
        slot = (slot + 1ull) & mask;
      }
      if (active) w = sys_weight(L, max_l);
    }
    labels[i] = root;
  }
  wave_add_by_root<true>(active, root, w, 1u, weight, n_part);
  unsigned long long tw = w;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) tw += __shfl_xor(tw, off, 64);
  if ((threadIdx.x & 63u) == 0u && tw != 0ull) atomicAdd(&counters[1], tw);
}

// records[0 .. roots): counters[2] hands out the positions, one atomic per wave.  Whole waves reach the ballot.
__global__ void __launch_bounds__(kBlock) k_hyp_compact(const unsigned long long* __restrict__ table, unsigned long long mask,
                                                        const uint32_t* __restrict__ parent, const unsigned long long* __restrict__ weight,
                                                        const uint32_t* __restrict__ n_bins, const uint32_t* __restrict__ n_part,
                                                        unsigned long long* __restrict__ counters, HypRecord* __restrict__ records, uint32_t capacity) {
  const unsigned long long s = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long key = s <= mask ? table[s] : kEmptySlot;
  const bool is_root = key != kEmptySlot && parent[s] == static_cast<uint32_t>(s);
  const unsigned long long m = __ballot(is_root);
  unsigned long long base = 0ull;
  if (lane == 0u && m) base = atomicAdd(&counters[2], static_cast<unsigned long long>(__popcll(m)));
  base = __shfl(base, 0, 64);
  if (is_root) {
    const unsigned long long pos = base + static_cast<unsigned long long>(__popcll(m & ((1ull << lane) - 1ull)));
    if (pos < capacity) {                                   // (roots <= occupied bins = capacity)
      HypRecord r;
      r.key_min = key; r.weight = weight[s]; r.n_bins = n_bins[s]; r.n_particles = n_part[s]; r.root = static_cast<uint32_t>(s); r.pad = 0u;
      records[pos] = r;
    }
  }
}

// "a ranks before b": weight descending, then key ascending
__device__ __forceinline__ bool hyp_before(unsigned long long wa, unsigned long long ka, unsigned long long wb, unsigned long long kb) {
  return wa > wb || (wa == wb && ka < kb);
}

// One workgroup.  Round r: the best record that ranks strictly after round r - 1's winner -- `rounds` rounds over n_rec records each.
__global__ void __launch_bounds__(kBlock) k_hyp_rank(const HypRecord* __restrict__ records, const unsigned long long* __restrict__ counters,
                                                     uint32_t capacity, uint32_t max_hypotheses, HypRecord* __restrict__ hyps,
                                                     uint32_t* __restrict__ rank) {
  __shared__ unsigned long long s_w[4], s_k[4];
  __shared__ uint32_t s_i[4];
  __shared__ unsigned long long s_prev_w, s_prev_k;
  const uint32_t n_rec = static_cast<uint32_t>(counters[0] < capacity ? counters[0] : capacity);
  const uint32_t rounds = n_rec < max_hypotheses ? n_rec : max_hypotheses;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long prev_w = 0ull, prev_k = 0ull;
  for (uint32_t r = 0; r < rounds; ++r) {
    unsigned long long bw = 0ull, bk = 0ull;
    uint32_t bi = kNone;
    for (uint32_t i = threadIdx.x; i < n_rec; i += kBlock) {
      const unsigned long long w = records[i].weight, k = records[i].key_min;
      if (r != 0u && !hyp_before(prev_w, prev_k, w, k)) continue;
      if (bi == kNone || hyp_before(w, k, bw, bk)) { bw = w; bk = k; bi = i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long ow = __shfl_xor(bw, off, 64), ok = __shfl_xor(bk, off, 64);
      const uint32_t oi = __shfl_xor(bi, off, 64);
      if (oi != kNone && (bi == kNone || hyp_before(ow, ok, bw, bk))) { bw = ow; bk = ok; bi = oi; }
    }
    if (lane == 0u) { s_w[wave] = bw; s_k[wave] = bk; s_i[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0u) {
      for (uint32_t q = 1; q < 4u; ++q)
        if (s_i[q] != kNone && (bi == kNone || hyp_before(s_w[q], s_k[q], bw, bk))) { bw = s_w[q]; bk = s_k[q]; bi = s_i[q]; }
      // (rounds <= records and the order is total: every round has a winner)
      if (bi != kNone) {
        const HypRecord win = records[bi];
        hyps[r] = win;
        rank[win.root] = r;
      }
      s_prev_w = bw; s_prev_k = bk;
    }
    __syncthreads();
    prev_w = s_prev_w; prev_k = s_prev_k;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kBlock) k_hyp_labels(uint32_t* __restrict__ labels, uint32_t n, const uint32_t* __restrict__ rank) {
  const unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t root = labels[i];
  labels[i] = (root == kNone) ? kNone : rank[root];
}

}  // namespace

hipError_t launch_hypotheses(const xform* poses, const void* attrs, uint32_t n, const float* bin_xyz, const float* bin_rpy, float floor_l,
                             double max_l, const unsigned long long* table, uint64_t table_words, uint32_t k_bins, uint32_t max_hypotheses,
                             const HypScratch& sc, uint32_t* labels, hipStream_t s) {
  if (n == 0 || k_bins == 0) return hipSuccess;
  // the table count_bins filled (a power of two >= 2 n); word indices are 32 bits with 0xFFFFFFFF kept for "none"
  if (table_words < 2ull * n || (table_words & (table_words - 1ull)) != 0ull || table_words > (1ull << 31) || k_bins > n ||
      max_hypotheses == 0 || max_hypotheses > kMaxHypotheses)
    return hipErrorInvalidValue;
  KldBins b;
  HypBins hb;
  for (int d = 0; d < 3; ++d) { b.bin_xyz[d] = hb.bin_xyz[d] = bin_xyz[d]; b.bin_rpy[d] = hb.bin_rpy[d] = bin_rpy[d]; }
  b.floor_l = floor_l;
  const unsigned long long mask = static_cast<unsigned long long>(table_words - 1ull);
  const dim3 g_words(static_cast<uint32_t>((table_words + kBlock - 1u) / kBlock)), g_n(static_cast<uint32_t>((static_cast<uint64_t>(n) + kBlock - 1u) / kBlock));
  HypRecord* records = reinterpret_cast<HypRecord*>(sc.records);
  hipLaunchKernelGGL(k_hyp_init, g_words, dim3(kBlock), 0, s, sc.parent, sc.rank, sc.n_bins, sc.n_part, sc.weight,
                     static_cast<unsigned long long>(table_words), sc.counters);
  hipLaunchKernelGGL(k_hyp_link, g_words, dim3(kBlock), 0, s, table, mask, hb, sc.parent);
  hipLaunchKernelGGL(k_hyp_flatten, g_words, dim3(kBlock), 0, s, table, mask, sc.parent, sc.n_bins, sc.counters);
  hipLaunchKernelGGL(k_hyp_accumulate, g_n, dim3(kBlock), 0, s, poses, static_cast<const pattr36*>(attrs), n, b, max_l, table, mask, sc.parent,
                     sc.weight, sc.n_part, sc.counters, labels);
  hipLaunchKernelGGL(k_hyp_compact, g_words, dim3(kBlock), 0, s, table, mask, sc.parent, sc.weight, sc.n_bins, sc.n_part, sc.counters, records, k_bins);
  hipLaunchKernelGGL(k_hyp_rank, dim3(1), dim3(kBlock), 0, s, records, sc.counters, k_bins, max_hypotheses, sc.hyps, sc.rank);
  hipLaunchKernelGGL(k_hyp_labels, g_n, dim3(kBlock), 0, s, labels, n, sc.rank);
  return hipGetLastError();
}

}  // namespace rmclhip

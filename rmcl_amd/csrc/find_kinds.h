// find_kinds.h -- THE catalogue of k_find's traversal kinds: what the number means, once, for the kernel (find_kernel.hip.h), its
// launchers (kernels.hip, kernels_lab.hip) and the C ABI (capi_*.cpp; no device headers needed).  Adding a kind = one row here and one
// `case` in kernels_lab.hip lab_find_kind.
#pragma once
#include <cstdint>

namespace rmclhip {

enum class FindStep { kPacket, kQuad, kWw, kWwTail, kBf, kBfTail };   // trace_packet, trace_quad, trace_lane_ww, _ww_tail, _bf, _bf_tail
// where a ray starts when the tile has its plane table (without one, and for OnDn, always the root): frontier_start<16, 0>,
// frontier_start<kFindBfRows, 1>, frontier_descent_start, frontier_start's quad form (traverse.hip.h)
enum class FindStart { kRoot, kFrontierWw, kFrontierBf, kDescent, kFrontierQuad };

struct FindKind {
  bool exists = true;
  FindStep step = FindStep::kWw;
  FindStart start = FindStart::kRoot;
  // the step function's template arguments, under the callee's parameter names
  bool leaf_batch = false;   // one-round-trip leaves
  int leaf_trigger = 0;      // leave the node phase when <= leaf_trigger / 10 of the round's rays still descend
  bool quant = false;        // reads the 64-B quantised nodes (FindParams::qnodes) instead of the full ones
  bool pre = false;          // requests the best record's last 16 B during the traversal
  bool pipe = false;         // software-pipelined node step
  int sort_steps = 5;        // ordering steps of the node step
  bool tail = false;         // the tail of every wave is finished by quads (their stacks and hand-over rows follow the lane stacks in LDS)
  int top = 0;               // nodes of the top of the tree copied to LDS
  bool vote = false;         // leaf vote of the while-while step
  bool uniform = false;      // wave-uniform nodes through the scalar cache
  bool coop = false;         // frontier_descent_start's kCoop: one bit per final leaf and ray, the wave tests those leaves together
  bool by_start = false;     // trace_lane_ww takes k_find's ray slab and start by reference (kinds 4 and 11, older, build their own at the root)
  // what the host needs beyond that
  bool filter_tree = false;  // walks the particle filter's tree (leaves <= 2) and its frontier table
  bool in_product = false;   // built into librmclhip.so (the others: librmclhip_lab.so only)
  bool moments = false;      // has the MICP moment epilogue (launch_find_moments); lab_moments: it compiles, nothing launches it
  bool lab_moments = false;
  bool clock_start = false;  // a clocked launch reports the start's cycles and the visit counts in word 2 instead of the realtime clock

  constexpr bool packet() const { return step == FindStep::kPacket; }     // one ray stream per wave: 8 x 8 tiles by default, not 16 x 4
  constexpr bool quad() const { return step == FindStep::kQuad; }         // four lanes per ray
  constexpr bool frontier() const { return start != FindStart::kRoot; }
  constexpr bool descent() const { return start == FindStart::kDescent; }
  // tiles (64 rays) per workgroup = mask words of the moment epilogue per workgroup = group of the world order
  constexpr uint32_t tiles_per_block() const { return quad() ? 1u : 4u; }
  // dwords per wave of a clocked launch: 8, + the descent's 16 phase stamps
  constexpr uint32_t clock_words() const { return descent() ? 24u : 8u; }
};

constexpr FindKind find_kind(int kind) {
  FindKind k;
  switch (kind) {
    case 0: k.step = FindStep::kPacket; break;                             // wave packet (needs the map's stack_need <= 64)
    case 1: k.step = FindStep::kBf; break;                                 // one lane per ray, branch-free node step
    case 2: k.step = FindStep::kQuad; break;                               // four lanes per ray (quad-cooperative)
    case 4: k.quant = true; break;                                         // one lane per ray, while-while on the quantised nodes
    case 5: k.step = FindStep::kWwTail; k.tail = true; break;              // while-while, the tail of every wave handed to quads
    case 6: k = find_kind(5); k.top = 85; break;                           // 5 + top of the tree in LDS (levels 0-3 of a full BVH4)
    case 7: k = find_kind(5); k.top = 341; break;                          // 5 + levels 0-4
    case 8: k = find_kind(5); k.leaf_batch = true; break;                  // 5 + one-round-trip leaves
    case 9: k = find_kind(6); k.leaf_batch = true; break;                  // 6 + 8
    case 10: k = find_kind(7); k.leaf_batch = true; break;                 // 7 + 8
    case 11: break;                                                        // the branchy while-while step on the full nodes
    case 12: k = find_kind(1); k.leaf_batch = true; break;                 // 1 + one-round-trip leaves
    case 13: k = find_kind(1); k.uniform = true; break;                    // 1 with wave-uniform nodes through the scalar cache
    case 14: k = find_kind(12); k.uniform = true; break;                   // 12 + 13
    case 16: k.step = FindStep::kBfTail; k.tail = true; break;             // branch-free step + quad-finished tails
    case 17: k = find_kind(16); k.leaf_batch = true; break;                // 16 + one-round-trip leaves
    case 19: k = find_kind(17); k.leaf_trigger = 10; break;                // 17 + leaf trigger
    case 20: k = find_kind(16); k.leaf_trigger = 10; break;                // 16 + leaf trigger
    case 21: k = find_kind(5); k.vote = true; break;                       // 5 + leaf vote
    case 22: k = find_kind(4); k.vote = k.by_start = k.filter_tree = true; break;   // 4 + leaf vote, on the filter's tree
    case 23: k = find_kind(19); k.start = FindStart::kFrontierBf; break;   // 19 + frontier start
    case 24: k = find_kind(22); k.start = FindStart::kFrontierWw; break;   // 22 + frontier start
    case 25: k = find_kind(2); k.start = FindStart::kFrontierQuad; break;  // 2 + frontier start
    case 26: k = find_kind(23); k.quant = true; break;                     // 23 on the quantised nodes
    case 27: k = find_kind(23); k.pre = true; break;                       // 23 + prefetch of the hit record's normal
    case 28: k = find_kind(23); k.pipe = true; break;                      // 23 with the software-pipelined node step
    case 29: k = find_kind(23); k.sort_steps = 4; break;                   // 23, the middle two children unordered
    case 30: k = find_kind(23); k.sort_steps = 3; break;                   // 23, only the nearest child found
    case 31: k = find_kind(23); k.start = FindStart::kDescent; k.tail = false; break;   // 23 + cooperative descent (its lists take the tail's LDS), sorted hand-over
    case 32: k = find_kind(31); k.coop = true; break;                      // 31 with one bit per final leaf and ray
    default: k.exists = false; break;                                      // (3, 18, 33 ...; 15 is the automatic rule's number)
  }
  // what a row does not inherit from the kind it builds on
  k.in_product = kind == 0 || kind == 2 || kind == 23 || kind == 24 || kind == 32;
  k.moments = kind == 2 || kind == 23 || kind == 32;
  k.lab_moments = kind == 31;
  k.clock_start = kind == 23 || kind == 31 || kind == 32;
  return k;
}

}  // namespace rmclhip

// frontier_groups_sanitize.cpp -- the group boxes of the frontier tables (rmcl_amd/csrc/bvh_build.cpp frontier_groups_of) under
// AddressSanitizer + UBSan, without a GPU: the tables of a real build (both trees) and every length 0 ... 300 of a cut or repeated
// table -- empty, one entry, short last groups, exactly full, and longer than the 256 entries a table can have.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -Irmcl_amd/csrc \
//       rmcl_amd/csrc/bvh_build.cpp tools/ubench/frontier_groups_sanitize.cpp -o /tmp/frontier_groups_asan -lpthread && /tmp/frontier_groups_asan
#include <algorithm>
#include <cstdio>
#include <random>

#include "bvh_build.h"

using rmclhip::Node4C;

static int check(const std::vector<Node4C::Child>& table, const std::vector<Node4C::Child>& groups, const char* what) {
  if (table.empty()) return groups.empty() ? 0 : (std::printf("%s: groups of an empty table\n", what), 1);
  if (groups.size() != rmclhip::kFrontierGroups) return std::printf("%s: %zu groups\n", what, groups.size()), 1;
  const size_t n = std::min<size_t>(table.size(), rmclhip::kFrontierGroups * rmclhip::kFrontierGroupSize);
  for (size_t g = 0; g < groups.size(); ++g) {
    const size_t lo = g * rmclhip::kFrontierGroupSize, hi = std::min(lo + rmclhip::kFrontierGroupSize, n);
    const size_t count = hi > lo ? hi - lo : 0;
    if (groups[g].ref != count) return std::printf("%s: group %zu covers %zu entries, says %u\n", what, g, count, groups[g].ref), 1;
    if (count == 0) {
      if (groups[g].lo[0] != rmclhip::kFarPoint[0] || groups[g].hiz != rmclhip::kFarPoint[2]) return std::printf("%s: empty group %zu is not the far point\n", what, g), 1;
      continue;
    }
    for (size_t i = lo; i < hi; ++i) {
      const Node4C::Child& e = table[i];
      const Node4C::Child& b = groups[g];
      if (b.lo[0] > e.lo[0] || b.lo[1] > e.lo[1] || b.lo[2] > e.lo[2] || b.hix < e.hix || b.hiy < e.hiy || b.hiz < e.hiz)
        return std::printf("%s: group %zu does not contain entry %zu\n", what, g, i), 1;
    }
  }
  return 0;
}

int main() {
  std::vector<float> v;
  std::vector<uint32_t> f;
  std::mt19937 rng(11);
  std::uniform_real_distribution<float> U(-10.f, 10.f), S(-0.2f, 0.2f);
  int bad = 0;
  for (int n : {1, 4, 40, 300, 20000}) {
    v.clear(); f.clear();
    for (int i = 0; i < n; ++i) {
      const float o[3] = {U(rng), U(rng), U(rng)};
      const uint32_t base = static_cast<uint32_t>(v.size() / 3);
      for (int c = 0; c < 3; ++c) for (int k = 0; k < 3; ++k) v.push_back(o[k] + S(rng));
      f.push_back(base); f.push_back(base + 1); f.push_back(base + 2);
    }
    rmclhip::BvhHost out;
    const std::string err = rmclhip::build_bvh(v.data(), static_cast<uint32_t>(v.size() / 3), f.data(), static_cast<uint32_t>(f.size() / 3), out);
    if (!err.empty()) return std::printf("build of %d triangles: %s\n", n, err.c_str()), 1;
    bad += check(out.frontier, out.frontier_groups, "map tree") + check(out.frontier_pf, out.frontier_groups_pf, "filter tree");
    std::printf("%d triangles: tables of %zu and %zu entries\n", n, out.frontier.size(), out.frontier_pf.size());
    if (n == 20000) {
      for (size_t len = 0; len <= 300; ++len) {
        std::vector<Node4C::Child> cut, groups;
        for (size_t i = 0; i < len; ++i) cut.push_back(out.frontier[i % out.frontier.size()]);
        rmclhip::frontier_groups_of(cut, groups);
        bad += check(cut, groups, "cut table");
      }
    }
  }
  std::printf(bad ? "FAILED\n" : "frontier groups: ok\n");
  return bad ? 1 : 0;
}

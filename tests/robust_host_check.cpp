// Stand-alone check of the host side of ROBUST MICP (rmcl_amd/csrc/robust_host.h): the weight, the default parameters and the
// parameter check, compiled by tests/test_robust_cpu.py with -fsanitize=address,undefined and run on the CPU.  Exit status 0 and no
// sanitizer report: every weight lies in [0, 1], r = 0 gives 1, the defaults pass the check, every doctored field is refused by name.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "robust_host.h"

using namespace rmclhip;

static int failures = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  std::vector<float> cs = {1e-30f, 1e-3f, 0.05f, 0.3f, 1.0f, 7.5f, 3e38f};
  std::vector<float> rs = {0.0f, -0.0f, 1e-45f, -1e-40f, 1e-30f, 1e-3f, -0.05f, 0.3f, 1.0f, -7.5f, 1e19f, -3e38f};
  for (float c : cs) {
    rs.push_back(c);
    rs.push_back(std::nextafter(c, 0.0f));
    rs.push_back(-std::nextafter(c, inf));
  }
  for (int kernel = RMCLHIP_ROBUST_NONE; kernel <= RMCLHIP_ROBUST_GEMAN_MCCLURE; ++kernel) {
    rmclhip_robust_params p;
    std::memset(&p, 0xAB, sizeof(p));
    robust_params_default(kernel, &p);
    EXPECT(p.kernel == kernel && p.scale_mode == RMCLHIP_ROBUST_SCALE_MAD && p.scale_min == 1e-3f && p.reserved == 0u);
    EXPECT(robust_params_error(&p) == nullptr);
    for (float c : cs) {
      EXPECT(robust_weight(kernel, c, 0.0f) == 1.0f && robust_weight(kernel, c, -0.0f) == 1.0f);
      for (float r : rs) {
        const float w = robust_weight(kernel, c, r);
        EXPECT(w >= 0.0f && w <= 1.0f);
        EXPECT(robust_weight(kernel, c, -r) == w);
      }
    }
    // every field the check names
    rmclhip_robust_params q = p;
    q.kernel = 5;
    EXPECT(robust_params_error(&q) != nullptr && std::strstr(robust_params_error(&q), "kernel") != nullptr);
    q = p; q.kernel = -1;
    EXPECT(robust_params_error(&q) != nullptr);
    q = p; q.scale_mode = 2;
    EXPECT(robust_params_error(&q) != nullptr && std::strstr(robust_params_error(&q), "scale_mode") != nullptr);
    const float bad[] = {0.0f, -1.0f, inf, -inf, std::numeric_limits<float>::quiet_NaN()};
    for (float b : bad) {
      q = p; q.tuning = b;
      EXPECT(robust_params_error(&q) != nullptr && std::strstr(robust_params_error(&q), "tuning") != nullptr);
      q = p; q.scale_min = b;
      EXPECT(robust_params_error(&q) != nullptr && std::strstr(robust_params_error(&q), "scale_min") != nullptr);
      q = p; q.scale = b;
      EXPECT(robust_params_error(&q) == nullptr);   // MAD mode does not use it
      q.scale_mode = RMCLHIP_ROBUST_SCALE_FIXED;
      EXPECT(robust_params_error(&q) != nullptr && std::strstr(robust_params_error(&q), "scale") != nullptr);
      q = p; q.scale_mode = RMCLHIP_ROBUST_SCALE_FIXED; q.scale = 0.1f; q.tuning = b; q.scale_min = b;
      EXPECT(robust_params_error(&q) == nullptr);   // FIXED mode uses neither
    }
  }
  rmclhip_robust_params u;
  robust_params_default(99, &u);
  EXPECT(u.kernel == RMCLHIP_ROBUST_NONE);
  EXPECT(robust_mad_scale(1.345f, 0.0f, 1e-3f) == 1e-3f && robust_mad_scale(1.0f, 1.0f, 1e-3f) == static_cast<float>(1.4826));
  std::printf("%s\n", failures == 0 ? "robust host check: OK" : "robust host check: FAILED");
  return failures == 0 ? 0 : 1;
}

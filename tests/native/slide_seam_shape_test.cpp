// Host test of the sliding ring round's seam launch rule (federated_amd/csrc/cfa_slide_shape.h,
// slide_takes_seam and the seam kernel's LDS budget), built without HIP by
// tests/test_slide_seam_shape.py. Prints "OK" and returns 0 when every check holds.
#include <cstdio>
#include <initializer_list>

#include "cfa_slide_shape.h"

static int failures = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      ++failures;                         \
      std::printf("FAIL %s: ", #cond);    \
      std::printf(__VA_ARGS__);           \
      std::printf("\n");                  \
    }                                     \
  } while (0)

int main() {
  // a full ring in one segment with a window, at a width that has a seam kernel
  for (int hl = 0; hl <= 4; ++hl)
    for (int hr = 0; hr <= 4; ++hr)
      for (int rows = hl + hr + 1; rows <= hl + hr + 24; ++rows)
        for (int u : {1, 2, 4}) {
          const bool want = hl + hr >= 1 && u != 1;
          CHECK(slide_takes_seam(rows, rows, 1, hl, hr, u) == want, "rows %d %d/%d u %d", rows, hl, hr, u);
          // more than one segment: every segment re-reads its own halo, there is no seam
          for (int segments : {2, 3, rows})
            CHECK(!slide_takes_seam(rows, rows, segments, hl, hr, u), "rows %d segments %d", rows, segments);
          // a partial run ends on rows it never began with
          for (int count = 1; count < rows; ++count)
            CHECK(!slide_takes_seam(rows, count, 1, hl, hr, u), "rows %d count %d", rows, count);
        }
  // hl + hr = 0 retains nothing
  CHECK(!slide_takes_seam(128, 128, 1, 0, 0, 4) && !slide_takes_seam(128, 128, 1, 0, 0, 2), "empty window");
  // the bench's shape takes the seam kernel at the tuned width ...
  const long long bench = 25000000 / 4;
  const int ub = slide_pick_u(bench, kSlideDefault.u, 256, kSlideDefault.wg_per_cu);
  CHECK(slide_takes_seam(128, 128, kSlideDefault.segments, 4, 4, ub), "bench shape, u %d", ub);
  // ... and follows the step-down of a short row: two float4 per lane still has a seam kernel, one
  // float4 per lane takes the plain kernel
  const long long need = 256LL * kSlideDefault.wg_per_cu;
  const long long two = need * kSlideBlock * 2, one = (need - 1) * kSlideBlock * 2;
  CHECK(slide_pick_u(two, 4, 256, kSlideDefault.wg_per_cu) == 2, "step-down to 2");
  CHECK(slide_takes_seam(16, 16, 1, 4, 4, slide_pick_u(two, 4, 256, kSlideDefault.wg_per_cu)), "seam at 2");
  CHECK(slide_pick_u(one, 4, 256, kSlideDefault.wg_per_cu) == 1, "step-down to 1");
  CHECK(!slide_takes_seam(16, 16, 1, 4, 4, slide_pick_u(one, 4, 256, kSlideDefault.wg_per_cu)), "plain at 1");
  // the LDS budget: at most kSlideSeamLdsRows rows, never more than retained, and the workgroups
  // the kernel is held to (one per SIMD wave: slide_seam_waves) share a CU's 160 KB
  for (int k = 1; k <= 8; ++k)
    for (int u : {2, 4}) {
      CHECK(slide_seam_lds_rows(k) <= k && slide_seam_lds_rows(k) <= kSlideSeamLdsRows, "k %d", k);
      CHECK(slide_seam_lds_bytes(k, u) == slide_seam_lds_rows(k) * u * kSlideBlock * 16, "k %d u %d", k, u);
      CHECK((long long)slide_seam_lds_bytes(k, u) * slide_seam_waves(u) <= 160 * 1024, "k %d u %d: %d bytes x %d",
            k, u, slide_seam_lds_bytes(k, u), slide_seam_waves(u));
      // the resident tile width per CU of the plain kernel's tuned shapes: 32 KB
      CHECK(slide_seam_waves(u) * u * kSlideBlock * 16 == 32 * 1024, "u %d", u);
    }
  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}

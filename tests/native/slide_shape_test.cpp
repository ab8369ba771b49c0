// Host test of the sliding ring round's tile-width rule (federated_amd/csrc/cfa_slide_shape.h),
// built without HIP by tests/test_slide_shape.py. Prints "OK" and returns 0 when every check holds.
#include <cstdio>

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
  const int widths[] = {1, 2, 4};
  const int cus_list[] = {1, 64, 256, 304};
  const int wg_list[] = {1, 2, 4, 8, 16};
  // every row length around the thresholds tiles(u) == cus * wg of each width, and the small ones
  for (int cus : cus_list)
    for (int wg : wg_list)
      for (int want : widths) {
        const long long need = (long long)cus * wg;
        auto check = [&](long long nvec) {
          if (nvec < 1) return;
          const int u = slide_pick_u(nvec, want, cus, wg);
          CHECK(u == 1 || u == 2 || u == 4, "u %d", u);
          CHECK(u <= want, "u %d above the tuned %d", u, want);
          for (int v : widths) {
            // never a starved width while a narrower one would fill the device
            if (v < u)
              CHECK(!(slide_tiles(nvec, u) < need && slide_tiles(nvec, v) >= need),
                    "nvec %lld cus %d wg %d want %d: u %d starves, %d would not", nvec, cus, wg, want, u, v);
            // and never narrower than needed: a wider width up to the tuned one would starve
            if (v > u && v <= want)
              CHECK(slide_tiles(nvec, v) < need, "nvec %lld cus %d wg %d want %d: u %d, %d also fills", nvec, cus, wg,
                    want, u, v);
          }
          // a width above 1 always fills the device
          if (u > 1) CHECK(slide_tiles(nvec, u) >= need, "nvec %lld cus %d wg %d: u %d starves", nvec, cus, wg, u);
        };
        for (long long nvec = 1; nvec <= 2100; ++nvec) check(nvec);
        for (int v : widths)
          for (long long d = -3; d <= 3; ++d) {
            check(need * kSlideBlock * v + d);
            check((need - 1) * kSlideBlock * v + d);
          }
      }
  // the bench's shape: 25M fp32 per row on the MI355X's 256 CUs keeps the tuned default
  CHECK(slide_pick_u(25000000 / 4, kSlideDefault.u, 256, kSlideDefault.wg_per_cu) == kSlideDefault.u,
        "bench shape: %d", slide_pick_u(25000000 / 4, kSlideDefault.u, 256, kSlideDefault.wg_per_cu));
  // less than one narrow tile: one float4 per lane, whatever is asked for
  for (long long nvec = 1; nvec < kSlideBlock; ++nvec)
    for (int want : widths)
      CHECK(slide_pick_u(nvec, want, 256, kSlideDefault.wg_per_cu) == 1, "nvec %lld want %d", nvec, want);
  // the tile count rounds up
  CHECK(slide_tiles(1, 4) == 1 && slide_tiles(1024, 4) == 1 && slide_tiles(1025, 4) == 2 && slide_tiles(257, 1) == 2,
        "slide_tiles");
  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}

// Host test of the streaming mixes' host-only launch rules (federated_amd/csrc/cfa_mix_shape.h):
// the bucket split, the passes of a wide fan-in, the compression-range shift and the launch-shape
// bands. Built without HIP by tests/test_mix_shape.py. Prints "OK" and returns 0 when every check
// holds.
#include <cstdio>
#include <vector>

#include "cfa_mix_shape.h"

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

static void check_split() {
  // three pointers (out, local, one neighbour) at every byte misalignment, every P in 0..40
  const uintptr_t base = 0x7f0000001000ULL;  // 16-byte aligned
  for (unsigned a = 0; a < 16; ++a)
    for (unsigned b = 0; b < 16; ++b)
      for (unsigned c = 0; c < 16; ++c)
        for (size_t P = 0; P <= 40; ++P) {
          const uintptr_t ptrs[3] = {base + a, base + 4096 + b, base + 8192 + c};
          const BucketSplit s = bucket_split(3, [&](int k) { return ptrs[k]; }, P);
          const size_t tail = P - s.tail_begin;
          CHECK(s.head <= P, "a %u b %u c %u P %zu: head %zu", a, b, c, P, s.head);
          CHECK(s.tail_begin == s.head + 4 * s.nvec && s.head + 4 * s.nvec + tail == P && tail <= P,
                "a %u b %u c %u P %zu: head %zu nvec %zu tail_begin %zu", a, b, c, P, s.head, s.nvec, s.tail_begin);
          const bool vector_ok = a == b && b == c && a % 4 == 0;
          if (!vector_ok) {
            CHECK(s.head == P && s.nvec == 0 && s.tail_begin == P, "a %u b %u c %u P %zu: not all scalar", a, b, c, P);
            continue;
          }
          CHECK(tail < 4, "a %u P %zu: tail %zu", a, P, tail);
          CHECK(s.head < 4, "a %u P %zu: head %zu", a, P, s.head);
          if (s.nvec > 0)
            for (unsigned m : {a, b, c})
              CHECK((base + m + 4 * s.head) % 16 == 0, "a %u P %zu: body at head %zu not 16-byte aligned", a, P, s.head);
          // the body is as long as the bucket allows
          if (P >= s.head + 4) CHECK(s.nvec == (P - s.head) / 4 && s.nvec > 0, "a %u P %zu: nvec %zu", a, P, s.nvec);
          const BucketSplit t = all_scalar(P);
          CHECK(t.head == P && t.nvec == 0 && t.tail_begin == P, "all_scalar");
        }
}

static void check_passes() {
  for (int n = 0; n <= 3 * CFA_MAX_FANIN + 1; ++n)
    for (int empty_pass = 0; empty_pass < 2; ++empty_pass) {
      int next = 0, passes = 0, lasts = 0;
      bool last_is_final = false;
      const int rc = for_each_pass(n, [&](int done, int m, bool last) {
        CHECK(done == next, "n %d: pass %d starts at %d, expected %d", n, passes, done, next);
        CHECK(m >= (n ? 1 : 0) && m <= CFA_MAX_FANIN, "n %d: pass of %d", n, m);
        next = done + m;
        ++passes;
        lasts += last ? 1 : 0;
        last_is_final = last;
        return 0;
      }, empty_pass != 0);
      CHECK(rc == 0, "n %d: rc %d", n, rc);
      CHECK(next == n, "n %d: passes cover [0, %d)", n, next);
      const int want = n ? (n + CFA_MAX_FANIN - 1) / CFA_MAX_FANIN : empty_pass;
      CHECK(passes == want, "n %d empty_pass %d: %d passes, expected %d", n, empty_pass, passes, want);
      if (passes) CHECK(lasts == 1 && last_is_final, "n %d: last set on %d passes", n, lasts);
    }
  // a failing pass stops the walk and hands its code back
  int calls = 0;
  CHECK(for_each_pass(3 * CFA_MAX_FANIN, [&](int, int, bool) { return ++calls == 2 ? -7 : 0; }) == -7 && calls == 2,
        "early stop: %d calls", calls);
}

static void check_shift() {
  CompressParams cp{3, 0.5, 0.25, 10, 30, nullptr};
  const CompressParams s = shifted(cp, 12);
  CHECK(s.cbegin == -2 && s.cend == 18 && s.mode == 3 && s.thr == 0.5 && s.rep == 0.25 && s.kept == nullptr, "shifted");
  CHECK(cp.cbegin == 10 && cp.cend == 30, "shifted changed its argument");
}

static void check_shape() {
  // Both sides of each band edge (512K, 1.5M, 3M and 8M elements), for a narrow fan-in (n = 8) and
  // a wide one (n = 12). The expected {workgroups per CU, float4 per lane} were evaluated from the
  // function as it stood in cfa_internal.h before it moved here.
  struct Want { long long elems; int n, bpc, vec; };
  const long long K512 = 1LL << 19, M1_5 = 3LL << 19, M3 = 3LL << 20, M8 = 8LL << 20;
  const Want want[] = {
      {K512 - 4, 8, 1, 2}, {K512, 8, 4, 1}, {M1_5 - 4, 8, 4, 1}, {M1_5, 8, 4, 4},
      {M3 - 4, 8, 4, 4},   {M3, 8, 4, 4},   {M8 - 4, 8, 4, 4},   {M8, 8, 1, 2},
      {K512 - 4, 12, 1, 2}, {K512, 12, 4, 1}, {M1_5 - 4, 12, 4, 1}, {M1_5, 12, 4, 2},
      {M3 - 4, 12, 4, 2},   {M3, 12, 1, 2},   {M8 - 4, 12, 1, 2},   {M8, 12, 1, 2},
  };
  for (const Want& w : want) {
    int bpc = -1, vec = -1;
    mix_auto_shape(w.n, w.elems / 4, bpc, vec);
    CHECK(bpc == w.bpc && vec == w.vec, "n %d elems %lld: %d x %d, expected %d x %d", w.n, w.elems, bpc, vec, w.bpc, w.vec);
  }
  // the widths the bands rest on
  CHECK(norm_vec(0) == 0 && norm_vec(1) == 1 && norm_vec(3) == 2 && norm_vec(4) == 4 && norm_vec(9) == 4 && norm_vec(-1) == 0,
        "norm_vec");
  CHECK(auto_vec(9) == 4 && auto_vec(10) == 2 && auto_vec(19) == 2 && auto_vec(20) == 1, "auto_vec");
  CHECK(mix_auto_vec(2) == 2 && mix_auto_vec(3) == 1 && mix_auto_vec(5) == 1 && mix_auto_vec(6) == 2 && mix_auto_vec(16) == 2,
        "mix_auto_vec");
}

int main() {
  check_split();
  check_passes();
  check_shift();
  check_shape();
  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}

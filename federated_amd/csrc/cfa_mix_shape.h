// cfa_mix_shape.h — host-only rules of the streaming mixes' launches (cfa_mix.hip, cfa_tf1.hip,
// cfa_mewma.hip): the launch-shape bands, the split of a bucket into a scalar head, a 16-byte
// vector body and a scalar tail, the passes of a fan-in above CFA_MAX_FANIN, and the shift of a
// compression range to a piece of its bucket. No HIP in here: tests/native/mix_shape_test.cpp
// builds it with a plain C++ compiler.
#pragma once
#include <cstddef>
#include <cstdint>

#include "cfa_engine.h"

namespace {

inline int norm_vec(int v) { return v >= 4 ? 4 : (v >= 2 ? 2 : (v == 1 ? 1 : 0)); }
inline int auto_vec(int n) { return (n + 1) * 4 <= 40 ? 4 : ((n + 1) * 2 <= 40 ? 2 : 1); }
// The streaming mix's own default (round 2, tools/probe/tune_placed.py on placement-calibrated
// stacks, profiles/r02_tune_placed.jsonl: every shape of 1-4 workgroups per CU x 1/2/4 float4 per
// lane at K = 2/4/8/12 on two boxes): one workgroup per CU (one wave per SIMD) at every fan-in,
// two float4 per lane except for 3-5 neighbours, where one is best. Sequential rule only.
inline int mix_auto_vec(int n) { return (n >= 3 && n <= 5) ? 1 : ((n + 1) * 2 <= 40 ? 2 : 1); }
// ... for buckets of 8M elements and more. Shorter mixes need more loads in flight than one
// wave per SIMD issues (round 3, tools/probe/slice_shape.py on placement-calibrated populations,
// P = 0.5M-25M; profiles/r03_slice_shape_k{4,8}.jsonl for the sweep, r03_ab_shape.jsonl for two
// rounds of A/B against the one-workgroup shape at K = 2/4/8/16). Four workgroups per CU:
//   - with one float4 per lane from 512K to 1.5M elements (1M: +2-13% in 3 of 4 A/B pairs);
//   - with four float4 from 1.5M to 8M (3.125M, the N = 8 bench rank's slice: +6-13% on ring
//     windows, +7% on rows no two consecutive mixes share; 6.25M: +1-5%);
//   - with two for 10-16 neighbours from 1.5M to 3M (+3-5%; neutral to -2% above).
// Below 512K elements (e.g. the drop-in pipeline's 128K chunks read over PCIe; at 500K the A/B
// pairs split both ways at K = 4 and 16) the shape is unchanged.
inline void mix_auto_shape(int n, long long nvec, int& blocks_per_cu, int& vec) {
  const long long elems = nvec * 4;
  const bool narrow = (n + 1) * 4 <= 40;
  blocks_per_cu = 4;
  if (elems >= (1LL << 19) && elems < (3LL << 19)) {
    vec = 1;
  } else if (elems >= (3LL << 19) && elems < (8LL << 20) && narrow) {
    vec = 4;
  } else if (elems >= (3LL << 19) && elems < (3LL << 20) && !narrow) {
    vec = 2;
  } else {
    blocks_per_cu = 1;
    vec = mix_auto_vec(n);
  }
}

// The split of a bucket of P fp32 elements: scalar elements [0, head) until every pointer is
// 16-byte aligned, nvec float4 from there, scalar elements [tail_begin, P). The pointers must
// share one misalignment (address & 15), a multiple of 4; otherwise the bucket is all scalar
// (all_scalar: head = P). address(k), k < count, is the k-th pointer of the bucket as an integer.
struct BucketSplit {
  size_t head, nvec, tail_begin;
};
inline BucketSplit all_scalar(size_t P) { return {P, 0, P}; }
template <typename A>
inline BucketSplit bucket_split(int count, A&& address, size_t P) {
  const unsigned mis = (unsigned)(address(0) & 15);
  for (int k = 1; k < count; ++k)
    if ((unsigned)(address(k) & 15) != mis) return all_scalar(P);
  if (mis & 3) return all_scalar(P);
  size_t head = mis ? (16 - mis) / 4 : 0;
  if (head > P) head = P;
  const size_t nvec = (P - head) / 4;
  return {head, nvec, head + nvec * 4};
}

// The passes of a fan-in of n: fn(done, m, last) for each pass of m <= CFA_MAX_FANIN neighbours
// after `done` earlier ones (pass k > 0 continues from the previous pass's output); stops at the
// first non-zero return and hands it back. n == 0 runs no pass, or with `empty_pass` one pass of
// no neighbours (the mixes then copy local, and apply the epilogue).
template <typename F>
inline int for_each_pass(int n, F&& fn, bool empty_pass = false) {
  if (n <= 0 && !empty_pass) return 0;
  int done = 0;
  do {
    const int m = (n - done) > CFA_MAX_FANIN ? CFA_MAX_FANIN : (n - done);
    if (int rc = fn(done, m, done + m == n)) return rc;
    done += m;
  } while (done < n);
  return 0;
}

// Compression epilogue of a launch: the mode's thresholds, the element range [cbegin, cend) it
// applies to, relative to the launch's first element, and the device counter of kept elements.
struct CompressParams {
  int mode;
  double thr, rep;
  long long cbegin, cend;
  unsigned long long* kept;
};
// The same range as seen by a launch that starts at element b of the bucket.
inline CompressParams shifted(CompressParams cp, long long b) {
  cp.cbegin -= b;
  cp.cend -= b;
  return cp;
}

}  // namespace

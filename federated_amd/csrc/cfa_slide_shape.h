// cfa_slide_shape.h — host-only launch-shape rules of the sliding ring round
// (cfa_mix_ring_slide_f32, cfa_ring.hip). No HIP in here: tests/native/slide_shape_test.cpp
// builds it with a plain C++ compiler.
#pragma once

constexpr int kSlideBlock = 256;  // lanes of a workgroup, one float4 per lane and stripe

// Launch shape of the sliding ring round: segments of the run (grid.y), workgroups per CU over
// all segments, rows prefetched ahead of the fold (1 or 2), sc1 write-through instead of nontemporal
// stores, and u float4 per lane and row (1, 2, 4; a workgroup's tile is kSlideBlock * u float4).
struct SlideTune {
  int segments, wg_per_cu, pf, sc1, u;
};
constexpr SlideTune kSlideDefault{1, 4, 2, 0, 4};  // tools/probe/ring_slide.py sweep, profiles/r09_slide_tile_sweep.jsonl

// Column tiles of nvec float4 at u float4 per lane.
inline long long slide_tiles(long long nvec, int u) {
  const long long tile = (long long)kSlideBlock * u;
  return (nvec + tile - 1) / tile;
}

// The tile width of a launch whose tuned width is `want`: the widest u of 4, 2, 1 not above
// `want` that still leaves every wanted workgroup (cus * wg_per_cu) a tile of its own. A short row
// (a small fused P, a rank's slice) steps down to a narrower tile, so it spreads over the device
// as it did at one float4 per lane; 1 when even that leaves workgroups without a tile.
inline int slide_pick_u(long long nvec, int want, int cus, int wg_per_cu) {
  int u = want >= 4 ? 4 : (want >= 2 ? 2 : 1);
  while (u > 1 && slide_tiles(nvec, u) < (long long)cus * wg_per_cu) u >>= 1;
  return u;
}

// Seam rows once: a full ring walked in one segment ends with the hl + hr rows it began with, and
// the seam kernel keeps a lane's copy of them (registers and LDS) instead of loading them again.
// Of the k = hl + hr retained rows at most kSlideSeamLdsRows sit in LDS, the others in registers:
// 5 rows of a u = 4 tile are 80 KB, so two workgroups share a CU's 160 KB (four at u = 2), the
// resident tile width of the plain kernel's tuned shapes.
constexpr int kSlideSeamDefault = 1;  // tools/probe/ring_slide.py sweep, profiles/r13_slide_seam_sweep.jsonl
constexpr int kSlideSeamLdsRows = 5;
constexpr int slide_seam_lds_rows(int k) { return k < kSlideSeamLdsRows ? k : kSlideSeamLdsRows; }
constexpr int slide_seam_lds_bytes(int k, int u) { return slide_seam_lds_rows(k) * u * kSlideBlock * 16; }
constexpr int slide_seam_waves(int u) { return u >= 4 ? 2 : 4;  }  // waves per SIMD the kernel is held to

// Whether a call of `count` devices of a ring of `rows`, in `segments` segments at u float4 per
// lane (after slide_pick_u's step-down), takes the seam kernel: a full ring in one segment with a
// window to retain, at a tile width that has a seam instantiation (2, 4).
inline bool slide_takes_seam(int rows, int count, int segments, int hl, int hr, int u) {
  return count == rows && segments == 1 && hl + hr >= 1 && (u == 2 || u == 4);
}

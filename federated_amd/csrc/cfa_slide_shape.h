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

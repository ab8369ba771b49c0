// cfa_optim_shape.h — host-only shape rules of the population optimizer step
// (cfa_optim_step_f32, cfa_optim.hip). No HIP in here; cfa_optim_tile() and
// cfa_optim_workspace_bytes() hand them to callers and tests.
#pragma once

constexpr int kOptimBlock = 256;  // lanes of a workgroup
constexpr int kOptimGroups = 4;   // groups of 4 elements (one float4 where the row is aligned) per lane and tile

// A row is cut into tiles of kOptimTile elements counted from its first element, whatever its
// layers: tile k is [k * kOptimTile, (k + 1) * kOptimTile). The sum of squares of layer l is kept
// as one fp64 partial per tile the layer meets, in slot k + l of the device's part of the
// workspace: layers and tiles both ascend along the row, so k + l names each (tile, layer) pair
// that meets once, and a layer's partials lie next to each other in tile order.
constexpr int kOptimTile = kOptimBlock * kOptimGroups * 4;

inline long long optim_tiles(long long P) { return (P + kOptimTile - 1) / kOptimTile; }
inline long long optim_slots(long long P, int n_layers) { return optim_tiles(P) + n_layers; }

// Workgroups per CU over all devices of a launch (not measured against other values).
constexpr int kOptimWgPerCu = 4;

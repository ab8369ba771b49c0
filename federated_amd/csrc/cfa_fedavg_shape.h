// cfa_fedavg_shape.h — host-only launch-shape rules of the FedAvg population round
// (cfa_fedavg_population_round_f32, cfa_fedavg.hip). No HIP in here; the tests read the
// constants below to place their sizes on the kernel's tile and batch boundaries.
#pragma once

constexpr int kFedavgBlock = 256;  // lanes of a workgroup

// Launch shape: u float4 per lane and row (a workgroup's tile is kFedavgBlock * u float4) below /
// from kFedavgLongRow elements, the rows whose loads are issued together ahead of their folds, and
// the workgroups per CU. tools/probe/fedavg_round.py --sweep, profiles/r11_fedavg_round.jsonl
// (128 x 25M, C = 16, one process: u = 4 moves 0.605-0.617 of peak at either batch depth and 1-8
// workgroups per CU, u = 2 0.590-0.621, u = 1 0.45-0.60 and only at 8 workgroups per CU; the batch
// depth and the workgroup count change little from u = 2 up. Short rows keep u = 2, whose tiles
// spread them over more CUs.)
struct FedavgTune {
  int u, u_long, batch, wg_per_cu;
};
constexpr FedavgTune kFedavgDefault{2, 4, 4, 4};

// The size at which the streaming mix changes its shape and its store policy (mix_auto_shape in
// cfa_mix_shape.h, launch_vec_chunk): client rows of P >= this are stored nontemporally.
constexpr long long kFedavgLongRow = 8LL << 20;

inline int fedavg_u(long long P, const FedavgTune& t) { return P >= kFedavgLongRow ? t.u_long : t.u; }
inline bool fedavg_nt_store(long long P) { return P >= kFedavgLongRow; }

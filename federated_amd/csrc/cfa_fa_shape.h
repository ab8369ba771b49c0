// cfa_fa_shape.h — host-only launch-shape rules of the TF1 CFA-FA server epoch
// (cfa_fa_population_round_f32, cfa_fa.hip). No HIP in here; cfa_fa_round_tile() reports the tile
// so that the tests can place their sizes on its boundaries.
#pragma once

constexpr int kFaBlock = 256;  // lanes of a workgroup

// Launch shape: u column elements (float4 on aligned rows, float otherwise) per lane and row below /
// from kFaLongRow elements, the rows whose loads are issued together ahead of their folds (4 or 8),
// and the workgroups per CU. tools/cfa_fa_round.py, profiles/cfa_fa_round.jsonl (8 x 25M, one
// process, GB/s of the algorithmic 2 D P 4 + 16 P bytes): u = 2 / batch 8 6151, u = 4 / batch 8
// 6001, u = 4 / batch 4 5093, u = 2 / batch 4 4999. A batch that holds all D rows keeps them in
// registers for the client step; a smaller one reads them twice, which is what the batch of 4
// pays at D = 8. The fp64 chain doubles a column's registers, so u = 2 (198 VGPRs at batch 8)
// stays ahead of u = 4 (350, 94 of them AGPRs) on long rows too.
struct FaTune {
  int u, u_long, batch, wg_per_cu;
};
constexpr FaTune kFaDefault{2, 2, 8, 4};

// Rows of P >= this take the long-row shape and are stored nontemporally, as the FedAvg round's.
constexpr long long kFaLongRow = 8LL << 20;

inline int fa_u(long long P, const FaTune& t) { return P >= kFaLongRow ? t.u_long : t.u; }
inline bool fa_nt_store(long long P) { return P >= kFaLongRow; }

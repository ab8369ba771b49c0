// cfa_fedavg.hip — the FedAvg parameter-server round of a device-resident population
// (cfa_fedavg_population_round_f32). The steps are div_step / seq_step, the schedule lookup and
// the scan for the first flagged device sched_slot / first_flagged, all of cfa_internal.h.
#include <type_traits>

#include "cfa_internal.h"
#include "cfa_fedavg_shape.h"

// ------------------------------------------------------------------------------------------
// FedAvg parameter-server round (cfa_fedavg_population_round_f32): the server's fold of the
// round's active rows into the global model (parameter_server_v2.py:146-161) and every device's
// take of the published model (federated_learning_keras_PS_MNIST.py:307-309,
// learner_consensus.py:151-152) in one launch on a [D, pitch] stack. A lane owns its columns for
// the whole round: it loads params, streams the active rows and folds them in list order (the
// chain is sequential in p, the row loads are not: B rows' loads of U float4 each are issued
// ahead of their folds), writes params, then walks the D rows for the client rule. No other lane
// reads or writes those elements of params or of any row, so everything is in place. The steps
// are div_step / seq_step of cfa_internal.h; a lane whose fold produced a subnormal quotient
// (div4_rn) walks its column again with the IEEE division, re-reading the rows (C is a run-time
// count: the rows are not kept in registers as fold<N, SEQUENTIAL_DIV> keeps them).
// ------------------------------------------------------------------------------------------
namespace {

struct FedAvgArgs {
  float* models;           // [D, pitch]
  float* params;           // [P]
  const int32_t* act_ptr;  // [T + 1] absolute offsets into act_idx
  const int32_t* act_idx;  // device ids in fold order
  const float* act_div;    // [T] C of each list
  const double* act_rdiv;  // [T] RN_64(1 / C)
  const int32_t* ended;    // [D] flags, or null
  long long pitch;
  int D, client;
  float u, u_c, d_c;
  double rd_c;
};

// The round's list [e0, e1), its divisor, and the row of the transfer-learning step (-1: none).
struct FedAvgRound {
  int e0, e1, ended_row;
  float d;
  double rd;
};

// One chain of uniform loads (round -> sched -> the list's bounds and divisor), then the scan of
// the list for its first flagged entry. Called by every lane of the workgroup (the scan
// synchronises).
__device__ __forceinline__ FedAvgRound fedavg_round_lookup(const FedAvgArgs& a, const SchedArgs& sc) {
  const int t = sched_slot(sc);
  FedAvgRound fr{a.act_ptr[t], a.act_ptr[t + 1], -1, a.act_div[t], a.act_rdiv[t]};
  if (a.ended) {
    const int first = first_flagged(a.ended, a.act_idx, fr.e0, fr.e1);
    if (first < fr.e1) fr.ended_row = a.act_idx[first];
  }
  return fr;
}

// A lane's column element: a float4 (index in float4 units) or, in the scalar tail, a float.
template <typename T, bool NT>
__device__ __forceinline__ T ld_col(const float* row, long long i) {
  if constexpr (std::is_same_v<T, f4>) return ld4<NT>(row, i);
  else return row[i];
}
template <typename T, bool NT>
__device__ __forceinline__ void st_col(float* row, long long i, T v) {
  if constexpr (std::is_same_v<T, f4>) st4<NT>(row, i, v);
  else row[i] = v;
}

// The server's fold of the list into p (the lane's U elements at i0 + u * kBlock), B rows' loads
// in flight. The row ids are wave-uniform: scalar registers.
template <typename T, int U, int B, bool IEEE>
__device__ __forceinline__ void fedavg_fold(T (&p)[U], const FedAvgArgs& a, const FedAvgRound& fr, long long i0,
                                            bool& subnormal) {
  for (int e = fr.e0; e < fr.e1; e += B) {
    T x[B][U];
#pragma unroll
    for (int b = 0; b < B; ++b)
      if (e + b < fr.e1) {
        const float* row = a.models + (long long)__builtin_amdgcn_readfirstlane(a.act_idx[e + b]) * a.pitch;
#pragma unroll
        for (int u = 0; u < U; ++u) x[b][u] = ld_col<T, true>(row, i0 + (long long)u * kBlock);
      }
#pragma unroll
    for (int b = 0; b < B; ++b)
      if (e + b < fr.e1) {
#pragma unroll
        for (int u = 0; u < U; ++u) p[u] = div_step<IEEE>(p[u], x[b][u], a.u, fr.d, fr.rd, subnormal);
      }
  }
}

// One step of the divisor rule on a float4 with the redo of a subnormal quotient; IEEE on a float.
template <typename T>
__device__ __forceinline__ T div_step_exact(T w, T x, float c, float d, double rd) {
  bool subnormal = false;
  if constexpr (std::is_same_v<T, f4>) {
    const T y = div_step<false>(w, x, c, d, rd, subnormal);
    if (__builtin_expect(!subnormal, 1)) return y;
  }
  return div_step<true>(w, x, c, d, rd, subnormal);
}

// The whole round on the lane's U column elements at i0 + u * kBlock.
template <typename T, int U, int B, bool NT>
__device__ __forceinline__ void fedavg_columns(const FedAvgArgs& a, const FedAvgRound& fr, long long i0) {
  T p[U];
#pragma unroll
  for (int u = 0; u < U; ++u) p[u] = ld_col<T, false>(a.params, i0 + (long long)u * kBlock);
  if (fr.ended_row >= 0) {  // transfer learning: one step on the first ended device, no division
    const float* row = a.models + (long long)fr.ended_row * a.pitch;
#pragma unroll
    for (int u = 0; u < U; ++u) p[u] = seq_step(p[u], ld_col<T, true>(row, i0 + (long long)u * kBlock), a.u);
  } else if constexpr (std::is_same_v<T, f4>) {
    T p0[U];
#pragma unroll
    for (int u = 0; u < U; ++u) p0[u] = p[u];
    bool subnormal = false;
    fedavg_fold<T, U, B, false>(p, a, fr, i0, subnormal);
    // a subnormal quotient may be an exact tie: the column again with the IEEE division
    if (__builtin_expect(subnormal, 0)) {
#pragma unroll
      for (int u = 0; u < U; ++u) p[u] = p0[u];
      fedavg_fold<T, U, B, true>(p, a, fr, i0, subnormal);
    }
  } else {
    bool unused = false;
    fedavg_fold<T, U, B, true>(p, a, fr, i0, unused);
  }
  if (fr.e1 > fr.e0) {
#pragma unroll
    for (int u = 0; u < U; ++u) st_col<T, false>(a.params, i0 + (long long)u * kBlock, p[u]);
  }
  if (a.client == CFA_CLIENT_COPY) {
    float* row = a.models;
    for (int d = 0; d < a.D; ++d, row += a.pitch) {
#pragma unroll
      for (int u = 0; u < U; ++u) st_col<T, NT>(row, i0 + (long long)u * kBlock, p[u]);
    }
  } else if (a.client == CFA_CLIENT_MIX) {
    for (int d0 = 0; d0 < a.D; d0 += B) {
      float* const row0 = a.models + (long long)d0 * a.pitch;
      T w[B][U];
#pragma unroll
      for (int b = 0; b < B; ++b)
        if (d0 + b < a.D) {
#pragma unroll
          for (int u = 0; u < U; ++u) w[b][u] = ld_col<T, true>(row0 + b * a.pitch, i0 + (long long)u * kBlock);
        }
#pragma unroll
      for (int b = 0; b < B; ++b)
        if (d0 + b < a.D) {
#pragma unroll
          for (int u = 0; u < U; ++u)
            st_col<T, NT>(row0 + b * a.pitch, i0 + (long long)u * kBlock,
                          div_step_exact(w[b][u], p[u], a.u_c, a.d_c, a.rd_c));
        }
    }
  }
}

template <int U, int B, bool NT>
__global__ __launch_bounds__(kBlock) void fedavg_round_kernel(FedAvgArgs a, SchedArgs sc, long long nvec,
                                                              long long P) {
  const FedAvgRound fr = fedavg_round_lookup(a, sc);
  const TileWalk<U> tw(nvec);
  for (const long long base : tw.full_tiles()) fedavg_columns<f4, U, B, NT>(a, fr, base);
  if (tw.owns_partial())
    for (const long long i : tw.partial_tile()) fedavg_columns<f4, 1, B, NT>(a, fr, i);
  // the < 4-element tail, in the same launch: the scalar form of the same operations
  if (blockIdx.x == 0 && nvec * 4 + threadIdx.x < P) fedavg_columns<float, 1, B, false>(a, fr, nvec * 4 + threadIdx.x);
}

// Launch shape: FedavgTune of cfa_fedavg_shape.h; the environment overrides are read at each
// launch, so one process can compare shapes on the same buffers (tools/probe/fedavg_round.py);
// results are identical for every shape.
static_assert(kFedavgBlock == kBlock, "cfa_fedavg_shape.h counts tiles of kBlock lanes");
static FedavgTune fedavg_tune() {
  const FedavgTune d = kFedavgDefault;
  FedavgTune t{env_int("CFA_FEDAVG_U", d.u), env_int("CFA_FEDAVG_U", d.u_long), env_int("CFA_FEDAVG_BATCH", d.batch),
               env_int("CFA_FEDAVG_WG_PER_CU", d.wg_per_cu)};
  if (t.u != 1 && t.u != 2 && t.u != 4) t.u = d.u, t.u_long = d.u_long;
  if (t.batch != 4 && t.batch != 8) t.batch = d.batch;
  if (t.wg_per_cu <= 0) t.wg_per_cu = d.wg_per_cu;
  return t;
}
template <int U, int B>
void launch_fedavg_ub(const FedAvgArgs& a, const SchedArgs& sc, unsigned grid, bool nt, long long nvec, long long P,
                      hipStream_t st) {
  if (nt) fedavg_round_kernel<U, B, true><<<grid, kBlock, 0, st>>>(a, sc, nvec, P);
  else fedavg_round_kernel<U, B, false><<<grid, kBlock, 0, st>>>(a, sc, nvec, P);
}
template <int U>
void launch_fedavg_u(const FedAvgArgs& a, const SchedArgs& sc, const FedavgTune& t, long long nvec, long long P,
                     hipStream_t st) {
  const long long tile = (long long)kBlock * U;
  cfa_launch_t lc = tune();
  lc.blocks_per_cu = t.wg_per_cu;
  const unsigned grid = grid_for((nvec + tile - 1) / tile, lc);
  if (t.batch == 8) launch_fedavg_ub<U, 8>(a, sc, grid, fedavg_nt_store(P), nvec, P, st);
  else launch_fedavg_ub<U, 4>(a, sc, grid, fedavg_nt_store(P), nvec, P, st);
}

}  // namespace

extern "C" int cfa_fedavg_population_round_f32(float* models, size_t pitch, float* params,
                                               const int32_t* act_ptr, const int32_t* act_idx,
                                               const float* act_div, const double* act_rdiv, float u,
                                               const int32_t* sched, int S, int T,
                                               unsigned long long* round, const int32_t* ended,
                                               int client, float u_c, float d_c, double rd_c, int D,
                                               size_t P, void* stream) {
  SchedArgs sc{};
  if (int rc = sched_args(sched, S, T, round, sc)) return rc;
  if (D < 0) return fail(CFA_E_INVALID, "negative device count");
  if (client != CFA_CLIENT_NONE && client != CFA_CLIENT_COPY && client != CFA_CLIENT_MIX)
    return fail(CFA_E_INVALID, "unknown client rule %d", client);
  if (client == CFA_CLIENT_MIX && d_c == 0.0f) return fail(CFA_E_INVALID, "client divisor d_c is 0");
  if (!act_ptr || !act_idx || !act_div || !act_rdiv) return fail(CFA_E_INVALID, "null active table");
  if (pitch < P) return fail(CFA_E_INVALID, "pitch %zu below P %zu", pitch, P);
  if (P == 0) return CFA_OK;
  if (!params || (D > 0 && !models)) return fail(CFA_E_INVALID, "null models or params");
  if ((addr(models) & 15) || (addr(params) & 15) || (pitch % 4))
    return fail(CFA_E_UNSUPPORTED, "FedAvg round needs 16-byte aligned rows (bases aligned, pitch a multiple of 4)");
  const FedAvgArgs a{models, params, act_ptr, act_idx, act_div, act_rdiv, ended, (long long)pitch,
                     D, client, u, u_c, d_c, rd_c};
  const FedavgTune t = fedavg_tune();
  const long long nvec = (long long)P / 4;
  hipStream_t st = (hipStream_t)stream;
  switch (fedavg_u((long long)P, t)) {
    case 4: launch_fedavg_u<4>(a, sc, t, nvec, (long long)P, st); break;
    case 2: launch_fedavg_u<2>(a, sc, t, nvec, (long long)P, st); break;
    default: launch_fedavg_u<1>(a, sc, t, nvec, (long long)P, st); break;
  }
  if (int rc = check_launch("fedavg_round")) return rc;
  return advance_round(sc, st);
}

// cfa_population.hip — the CSR rounds of a whole population in one launch: cfa_mix_population_f32
// (_sched_f32 with a table per round; _ended_f32 with the training_end rule on device-resident
// flags; _tf1_f32 / _sched_tf1_f32 with the TF1 numerics), the CFA-GE population step, and the
// round counter's advance. The ring family is in cfa_ring.hip, the FedAvg round in
// cfa_fedavg.hip. Every rule's step (seq_step, lin_step, tf1_first / tf1_step, mewma_step,
// split_sum) is the one definition of cfa_internal.h, as are the schedule lookup (sched_slot) and
// the scan for the first flagged neighbour (first_flagged).
#include "cfa_internal.h"

// Resident workgroups per CU across a whole population launch (all devices together). 8 by
// default; CFA_POP_WG_PER_CU overrides it per call (read at each launch, so one process can
// compare values: tools/probe/pop_shape.py).
static int pop_wg_per_cu() {
  const int v = env_int("CFA_POP_WG_PER_CU", 8);
  return v > 0 ? v : 8;
}

namespace {

// ------------------------------------------------------------------------------------------
// Population round: grid.y = device, grid.x = tiles. CSR lists each device's sources.
// ------------------------------------------------------------------------------------------
// The fold of CSR entries [e0, e1) into `out` by the workgroups of one device (blockIdx.x over
// the tiles): entry e0 is the row the fold starts from, every later entry e one step with
// csr_coef[e], or with `eps` for all of them when use_eps (the training_end round's recomputed
// coefficient). e1 == e0 + 1 loads and stores row e0 with no arithmetic in between: a bit copy.
template <int RULE>
__device__ __forceinline__ void population_fold(float* out, const float* const* src_ptrs, const int32_t* csr_idx,
                                                const float* csr_coef, int e0, int e1, bool use_eps, float eps,
                                                long long nvec, long long P) {
  constexpr int U = 2;
  constexpr long long kTile = (long long)kBlock * U;
  for (long long t = blockIdx.x; t * kTile < nvec; t += gridDim.x) {
    long long idx[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      idx[u] = t * kTile + (long long)u * kBlock + threadIdx.x;
      ok[u] = idx[u] < nvec;
    }
    f4 w[U];
    const float* s0 = src_ptrs[csr_idx[e0]];
    const float c0 = csr_coef[e0];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      w[u] = ok[u] ? ld4<true>(s0, idx[u]) : f4{0.f, 0.f, 0.f, 0.f};
      if constexpr (RULE == CFA_RULE_LINEAR) w[u] = c0 * w[u];
    }
    for (int e = e0 + 1; e < e1; ++e) {
      const float* s = src_ptrs[csr_idx[e]];
      const float c = use_eps ? eps : csr_coef[e];
      f4 x[U];
#pragma unroll
      for (int u = 0; u < U; ++u) x[u] = ok[u] ? ld4<true>(s, idx[u]) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if constexpr (RULE == CFA_RULE_SEQUENTIAL) w[u] = seq_step(w[u], x[u], c);
        else w[u] = lin_step(w[u], x[u], c);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (ok[u]) st4<true>(out, idx[u], w[u]);
  }
  // the < 4-element tail, in the same launch (one kernel boundary fewer per round): the
  // scalar form of the same operations, so every element rounds as in the float4 body
  if (blockIdx.x == 0 && nvec * 4 + threadIdx.x < P) {
    const long long i = nvec * 4 + threadIdx.x;
    float w = src_ptrs[csr_idx[e0]][i];
    if constexpr (RULE == CFA_RULE_LINEAR) w = csr_coef[e0] * w;
    for (int e = e0 + 1; e < e1; ++e) {
      const float x = src_ptrs[csr_idx[e]][i];
      const float c = use_eps ? eps : csr_coef[e];
      if constexpr (RULE == CFA_RULE_SEQUENTIAL) w = seq_step(w, x, c);
      else w = lin_step(w, x, c);
    }
    out[i] = w;
  }
}

// The round's table, D + 1 row offsets into csr_idx / csr_coef: csr_ptr itself, or under a
// topology schedule (SCHED: cfa_mix_population_sched_f32 / _sched_tf1_f32 / _ended_f32) table
// sched[r mod S] of the T tables that lie back to back in csr_ptr, their offsets absolute in the
// shared csr_idx / csr_coef. The lookup is one chain of uniform loads (round -> sched -> the
// table's base) ahead of the tile loop; a static round does not read `sc`.
template <bool SCHED>
__device__ __forceinline__ const int32_t* round_table(const int32_t* csr_ptr, const SchedArgs& sc) {
  if constexpr (SCHED) return csr_ptr + (long long)sched_slot(sc) * ((long long)gridDim.y + 1);  // grid.y = D
  else return csr_ptr;
}

template <int RULE, bool SCHED>
__global__ __launch_bounds__(kBlock) void population_kernel(float* const* out_ptrs,
                                                            const float* const* src_ptrs,
                                                            const int32_t* csr_ptr,
                                                            const int32_t* csr_idx,
                                                            const float* csr_coef, SchedArgs sc,
                                                            long long nvec, long long P) {
  const int32_t* ptr = round_table<SCHED>(csr_ptr, sc);
  const int d = blockIdx.y;
  population_fold<RULE>(out_ptrs[d], src_ptrs, csr_idx, csr_coef, ptr[d], ptr[d + 1], false, 0.f, nvec, P);
}

__global__ void round_advance_kernel(unsigned long long* round) { *round += 1; }

// training_end round (cfa_mix_population_ended_f32): the population round with the TF2 protocol's
// training_end rule (consensus_v3.py:139-152, :233; consensus_v4.py:191-210, :234-248). A device
// that has ended keeps its row; any other collects its list up to and including the first
// neighbour flagged in `ended` and, by ended_rule, takes that neighbour's row as it is (COPY),
// folds the collected prefix with the table's coefficients (TRUNCATE), or folds it with
// 1 / (prefix length + 1) (TRUNCATE_EPS, also with no flagged neighbour: the whole list). Each
// case is a range of CSR entries handed to population_fold. Every workgroup of a device reaches
// the same range from `ended` alone: ended_next and saw are written by this launch (one lane of
// the device's first workgroup) and never read by it.
struct EndedArgs {
  const int32_t* ended;  // [D] the round's input flags
  int32_t* ended_next;   // [D] ended | saw, or null
  int32_t* saw;          // [D] a flagged neighbour was collected, or null
  int rule;
};

template <bool SCHED>
__global__ __launch_bounds__(kBlock) void population_ended_kernel(float* const* out_ptrs,
                                                                  const float* const* src_ptrs,
                                                                  const int32_t* csr_ptr,
                                                                  const int32_t* csr_idx,
                                                                  const float* csr_coef, SchedArgs sc,
                                                                  EndedArgs ea, long long nvec, long long P) {
  const int32_t* ptr = round_table<SCHED>(csr_ptr, sc);
  const int d = blockIdx.y;
  int e0 = ptr[d], e1 = ptr[d + 1];
  const bool self = ea.ended[d] != 0;  // uniform over the device's workgroups, as everything below
  int f = e1;
  if (!self) f = first_flagged(ea.ended, csr_idx, e0 + 1, e1);
  const bool found = f < e1;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (ea.saw) ea.saw[d] = found;
    if (ea.ended_next) ea.ended_next[d] = self || found;
  }
  if (self) {
    e1 = e0 + 1;  // the device has left its loop: its own row
  } else if (found) {
    if (ea.rule == CFA_ENDED_COPY) e0 = f;  // that neighbour's row and nothing else
    e1 = f + 1;
  }
  // numpy's Python float 1 / (len + 1) on fp32 arrays: one fp64 division, one rounding to fp32
  const bool use_eps = !self && ea.rule == CFA_ENDED_TRUNCATE_EPS;
  const float eps = use_eps ? (float)(1.0 / (double)(e1 - e0)) : 0.f;
  population_fold<CFA_RULE_SEQUENTIAL>(out_ptrs[d], src_ptrs, csr_idx, csr_coef, e0, e1, use_eps, eps, nvec, P);
}

// TF1 population round (cfa_mix_population_tf1_f32): per device the numpy-2 chain of the TF1
// modules (cfa.py:66-76): the first subtraction x_1 - w of two fp32 arrays is fp32, every later
// operation fp64 with the fp64 coefficients eps * wf_j, one rounding to fp32 at the end. A TF1
// driver assigns the returned fp64 arrays into its fp32 TF variables, so fp32 buckets mixed this
// way follow the reference run's trajectory exactly. Same operations as cfa_mix_tf1_f32.
__device__ __forceinline__ void population_tf1_body(float* const* out_ptrs, const float* const* src_ptrs,
                                                    const int32_t* csr_ptr, const int32_t* csr_idx,
                                                    const double* csr_coef, long long nvec, long long P,
                                                    const CompressParams& cp) {
  const int d = blockIdx.y;
  const int e0 = csr_ptr[d], e1 = csr_ptr[d + 1];
  float* out = out_ptrs[d];
  const float* l = src_ptrs[csr_idx[e0]];
  unsigned kept = 0;
  // the compression epilogue (cfa_ongraphs.py:225-273) on [cbegin, cend): fp64 against the
  // pre-mix local after a mix, fp32 on the local itself for a device without neighbours (the
  // reference then compresses the caller's fp32 array in place, numpy-2 fp32 thresholds)
  auto epi = [&](double w, float lv, long long e) -> float {
    if (cp.mode && e >= cp.cbegin && e < cp.cend) return (float)compress_one_d(w, (double)lv, cp, kept);
    return (float)w;
  };
  auto epi0 = [&](float lv, long long e) -> float {
    if (cp.mode && e >= cp.cbegin && e < cp.cend) return compress_one(lv, lv, cp, kept);
    return lv;
  };
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < nvec; i += (long long)gridDim.x * kBlock) {
    const f4 lv = ld4<true>(l, i);
    f4 y;
    if (e1 - e0 <= 1) {
#pragma unroll
      for (int c = 0; c < 4; ++c) y[c] = epi0(lv[c], 4 * i + c);
    } else {
      const f4 x1 = ld4<true>(src_ptrs[csr_idx[e0 + 1]], i);
      double w[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) w[c] = tf1_first(lv[c], x1[c], csr_coef[e0 + 1]);  // fp64 from here on
      for (int e = e0 + 2; e < e1; ++e) {
        const f4 x = ld4<true>(src_ptrs[csr_idx[e]], i);
        const double a = csr_coef[e];
#pragma unroll
        for (int c = 0; c < 4; ++c) w[c] = tf1_step(w[c], x[c], a);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) y[c] = epi(w[c], lv[c], 4 * i + c);
    }
    st4<true>(out, i, y);
  }
  if (blockIdx.x == 0) {  // the < 4-element tail
    for (long long i = nvec * 4 + threadIdx.x; i < P; i += kBlock) {
      const float lv = l[i];
      float y;
      if (e1 - e0 <= 1) {
        y = epi0(lv, i);
      } else {
        double w = tf1_first(lv, src_ptrs[csr_idx[e0 + 1]][i], csr_coef[e0 + 1]);
        for (int e = e0 + 2; e < e1; ++e) w = tf1_step(w, src_ptrs[csr_idx[e]][i], csr_coef[e]);
        y = epi(w, lv, i);
      }
      out[i] = y;
    }
  }
  if (cp.mode) block_add_count(kept, cp.kept + d);
}

template <bool SCHED>
__global__ __launch_bounds__(kBlock) void population_tf1_kernel(float* const* out_ptrs,
                                                                const float* const* src_ptrs,
                                                                const int32_t* csr_ptr,
                                                                const int32_t* csr_idx,
                                                                const double* csr_coef, SchedArgs sc,
                                                                long long nvec, long long P,
                                                                CompressParams cp) {
  population_tf1_body(out_ptrs, src_ptrs, round_table<SCHED>(csr_ptr, sc), csr_idx, csr_coef, nvec, P, cp);
}

}  // namespace

// The round is over: the next launch on the stream reads the counter one higher.
int advance_counter(unsigned long long* counter, hipStream_t st) {
  round_advance_kernel<<<1, 1, 0, st>>>(counter);
  return check_launch("round_advance");
}

// The common part of the CSR round entries: the shared argument checks, the grid from the
// kernel's tile of kBlock * tile_vec float4, the launch of `fixed`, or under a schedule
// (sc.sched) of `sched` and then the counter's advance. `own` is the result of the entry's own
// checks: a failure there is reported after a negative D and before an empty population returns
// CFA_OK (a negative D's message replaces the one `own` left). launch(kernel, grid, st, nvec)
// starts the kernel with the entry's arguments; both instances take the same ones.
template <typename K, typename Coef, typename Launch>
static int launch_population(K fixed, K sched, const char* name, const char* sched_name, int tile_vec,
                             float* const* out_ptrs, const float* const* src_ptrs, const int32_t* csr_ptr,
                             const int32_t* csr_idx, const Coef* csr_coef, const SchedArgs& sc, int D, int own,
                             size_t P, void* stream, Launch&& launch) {
  if (D < 0) return fail(CFA_E_INVALID, "negative device count");
  if (own) return own;
  if (D == 0 || P == 0) return CFA_OK;
  if (!out_ptrs || !src_ptrs || !csr_ptr || !csr_idx || !csr_coef)
    return fail(CFA_E_INVALID, "null population table");
  if (D > 65535) return fail(CFA_E_INVALID, "D=%d exceeds grid.y limit", D);
  // Buckets in a population are expected 16-byte aligned (allocator contract, checked by the
  // host layer); the body runs on float4, the <4-element tail in the first tile column.
  const long long nvec = (long long)P / 4, tile = (long long)kBlock * tile_vec;
  const dim3 grid(shared_grid_x((nvec + tile - 1) / tile, pop_wg_per_cu(), D), (unsigned)D);
  hipStream_t st = (hipStream_t)stream;
  launch(sc.sched ? sched : fixed, grid, st, nvec);
  if (int rc = check_launch(sc.sched ? sched_name : name)) return rc;
  return sc.sched ? advance_round(sc, st) : CFA_OK;
}

static int population_tf1(float* const* out_ptrs, const float* const* src_ptrs, const int32_t* csr_ptr,
                          const int32_t* csr_idx, const double* csr_coef, const SchedArgs& sc, int D,
                          size_t P, int mode, size_t cbegin, size_t cend, unsigned long long* kept_counts,
                          void* stream) {
  CompressParams cp{};
  int own = compress_params(mode, cp);
  if (!own && mode && (!kept_counts || cbegin > cend || cend > P))
    own = fail(CFA_E_INVALID, "compression needs per-device counters and a segment within the bucket");
  cp.cbegin = (long long)cbegin;
  cp.cend = (long long)cend;
  cp.kept = kept_counts;
  return launch_population(population_tf1_kernel<false>, population_tf1_kernel<true>, "population_tf1",
                           "population_tf1_sched", 1, out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, sc, D, own, P,
                           stream, [&](auto kernel, dim3 grid, hipStream_t st, long long nvec) {
                             kernel<<<grid, kBlock, 0, st>>>(out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, sc, nvec,
                                                             (long long)P, cp);
                           });
}

extern "C" int cfa_mix_population_tf1_f32(float* const* out_ptrs, const float* const* src_ptrs,
                                          const int32_t* csr_ptr, const int32_t* csr_idx,
                                          const double* csr_coef, int D, size_t P, int mode,
                                          size_t cbegin, size_t cend, unsigned long long* kept_counts,
                                          void* stream) {
  return population_tf1(out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, SchedArgs{}, D, P, mode, cbegin, cend,
                        kept_counts, stream);
}

extern "C" int cfa_mix_population_sched_tf1_f32(float* const* out_ptrs, const float* const* src_ptrs,
                                                const int32_t* csr_ptr, const int32_t* csr_idx,
                                                const double* csr_coef, const int32_t* sched, int S, int T,
                                                unsigned long long* round, int D, size_t P, int mode,
                                                size_t cbegin, size_t cend, unsigned long long* kept_counts,
                                                void* stream) {
  SchedArgs sc{};
  if (int rc = sched_args(sched, S, T, round, sc)) return rc;
  return population_tf1(out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, sc, D, P, mode, cbegin, cend,
                        kept_counts, stream);
}

static int population_f32(float* const* out_ptrs, const float* const* src_ptrs, const int32_t* csr_ptr,
                          const int32_t* csr_idx, const float* csr_coef, const SchedArgs& sc, int D, int rule,
                          size_t P, void* stream) {
  int own = CFA_OK;
  if (rule != CFA_RULE_SEQUENTIAL && rule != CFA_RULE_LINEAR) own = fail(CFA_E_INVALID, "unknown rule %d", rule);
  const bool lin = rule == CFA_RULE_LINEAR;
  return launch_population(lin ? population_kernel<CFA_RULE_LINEAR, false> : population_kernel<CFA_RULE_SEQUENTIAL, false>,
                           lin ? population_kernel<CFA_RULE_LINEAR, true> : population_kernel<CFA_RULE_SEQUENTIAL, true>,
                           "population", "population_sched", 2, out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, sc, D,
                           own, P, stream, [&](auto kernel, dim3 grid, hipStream_t st, long long nvec) {
                             kernel<<<grid, kBlock, 0, st>>>(out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, sc, nvec,
                                                             (long long)P);
                           });
}

extern "C" int cfa_mix_population_f32(float* const* out_ptrs, const float* const* src_ptrs,
                                      const int32_t* csr_ptr, const int32_t* csr_idx,
                                      const float* csr_coef, int D, int rule, size_t P,
                                      void* stream) {
  return population_f32(out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, SchedArgs{}, D, rule, P, stream);
}

extern "C" int cfa_mix_population_sched_f32(float* const* out_ptrs, const float* const* src_ptrs,
                                            const int32_t* csr_ptr, const int32_t* csr_idx,
                                            const float* csr_coef, const int32_t* sched, int S, int T,
                                            unsigned long long* round, int D, int rule, size_t P,
                                            void* stream) {
  SchedArgs sc{};
  if (int rc = sched_args(sched, S, T, round, sc)) return rc;
  return population_f32(out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, sc, D, rule, P, stream);
}

// [a, a + n) and [b, b + n) share an element.
static bool flags_overlap(const int32_t* a, const int32_t* b, int n) {
  return b && addr(a) < addr(b + n) && addr(b) < addr(a + n);
}

extern "C" int cfa_mix_population_ended_f32(float* const* out_ptrs, const float* const* src_ptrs,
                                            const int32_t* csr_ptr, const int32_t* csr_idx,
                                            const float* csr_coef, const int32_t* sched, int S, int T,
                                            unsigned long long* round, const int32_t* ended,
                                            int32_t* ended_next, int32_t* saw, int ended_rule, int D,
                                            size_t P, void* stream) {
  SchedArgs sc{};
  if (sched || round)
    if (int rc = sched_args(sched, S, T, round, sc)) return rc;
  int own = CFA_OK;
  if (ended_rule != CFA_ENDED_COPY && ended_rule != CFA_ENDED_TRUNCATE && ended_rule != CFA_ENDED_TRUNCATE_EPS)
    own = fail(CFA_E_INVALID, "unknown ended rule %d", ended_rule);
  else if (!ended)
    own = fail(CFA_E_INVALID, "null ended flags");
  // every workgroup of the round reads `ended` while one lane per device writes the other two
  else if (flags_overlap(ended, ended_next, D > 0 ? D : 1) || flags_overlap(ended, saw, D > 0 ? D : 1))
    own = fail(CFA_E_INVALID, "ended_next or saw aliases ended");
  // buckets 16-byte aligned and the tile of two float4 per lane, as cfa_mix_population_f32
  return launch_population(population_ended_kernel<false>, population_ended_kernel<true>, "population_ended",
                           "population_ended_sched", 2, out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, sc, D, own,
                           P, stream, [&](auto kernel, dim3 grid, hipStream_t st, long long nvec) {
                             const EndedArgs ea{ended, ended_next, saw, ended_rule};
                             kernel<<<grid, kBlock, 0, st>>>(out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, sc, ea,
                                                             nvec, (long long)P);
                           });
}

// ------------------------------------------------------------------------------------------
// CFA-GE population step (cfa_ge_population_step_f32): stage-1 mix and the neighbours' gradient
// step of every device in one launch (cfa_ge_2stage.py:446-466 then :591-621). The operations
// and their order are those of cfa_mix_population_f32 followed by cfa_mewma_update_f32, so the
// result is identical to the two launches, minus one write and one read of every mixed model.
// ------------------------------------------------------------------------------------------
namespace {

struct GeStepArgs {
  float* const* out;
  const float* const* src;
  float* const* state;
  const float* const* grad;
  const int32_t* ptr;
  const int32_t* idx;
  const float* coef;
  float rho, one_minus_rho, lr1, lr2;
  long long split;
  int filtered;
  // optional second job of the same launch: sum rsp partial buckets of rM gradient evaluations
  // (rws [rM][rsp][P], written by a partials-only cfa_ge_grad_*_rows_f32) into rout [rM][P]
  const float* rws;
  float* rout;
  int rM, rsp;
};

__device__ __forceinline__ float ge_lr(const GeStepArgs& a, long long i) { return i < a.split ? a.lr1 : a.lr2; }

__global__ __launch_bounds__(kBlock) void ge_step_kernel(GeStepArgs a, long long nvec, long long P) {
  const int d = blockIdx.y;
  if (d >= (int)gridDim.y - a.rM) {  // reduction rows: the split sum in split order (deterministic)
    const long long m = d - ((int)gridDim.y - a.rM);
    const float* w = a.rws + m * a.rsp * P;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long long)gridDim.x * kBlock)
      a.rout[m * P + i] = split_sum(w + i, a.rsp, P);
    return;
  }
  const int e0 = a.ptr[d], e1 = a.ptr[d + 1];
  float* out = a.out[d];
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < nvec; i += (long long)gridDim.x * kBlock) {
    f4 w = ld4<false>(a.src[a.idx[e0]], i);
    for (int e = e0 + 1; e < e1; ++e) {  // stage 1: sequential rule
      const f4 x = ld4<false>(a.src[a.idx[e]], i);
      w = seq_step(w, x, a.coef[e]);
    }
    f4 lr;
#pragma unroll
    for (int c = 0; c < 4; ++c) lr[c] = ge_lr(a, i * 4 + c);
    for (int e = e0 + 1; e < e1; ++e) {  // gradient step: MEWMA filter + SGD
      const float* gp = a.grad[e];
      const f4 g = gp ? ld4<false>(gp, i) : f4{0.f, 0.f, 0.f, 0.f};
      const f4 s_old = ld4<false>(a.state[e], i);
      st4<false>(a.state[e], i, mewma_step(w, g, s_old, a.rho, a.one_minus_rho, lr, false, a.filtered));
    }
    st4<false>(out, i, w);
  }
  if (blockIdx.x == 0) {  // the < 4-element tail
    for (long long i = nvec * 4 + threadIdx.x; i < P; i += kBlock) {
      float w = a.src[a.idx[e0]][i];
      for (int e = e0 + 1; e < e1; ++e) w = seq_step(w, a.src[a.idx[e]][i], a.coef[e]);
      const float lr = ge_lr(a, i);
      for (int e = e0 + 1; e < e1; ++e) {
        const float g = a.grad[e] ? a.grad[e][i] : 0.f;
        a.state[e][i] = mewma_step(w, g, a.state[e][i], a.rho, a.one_minus_rho, lr, false, a.filtered);
      }
      out[i] = w;
    }
  }
}

}  // namespace

extern "C" int cfa_ge_population_step_f32(float* const* out_ptrs, const float* const* src_ptrs,
                                          float* const* state_ptrs, const float* const* grad_ptrs,
                                          const int32_t* csr_ptr, const int32_t* csr_idx,
                                          const float* csr_coef, int D, double rho, float lr1,
                                          float lr2, size_t lr_split, int use_filtered, size_t P,
                                          const float* reduce_ws, float* reduce_out, int reduce_M,
                                          int reduce_splits, void* stream) {
  if (D < 0) return fail(CFA_E_INVALID, "negative device count");
  if (!reduce_ws) reduce_M = 0;
  if (reduce_M < 0 || (reduce_M > 0 && (!reduce_out || reduce_splits < 1)))
    return fail(CFA_E_INVALID, "bad split reduction (M %d, splits %d)", reduce_M, reduce_splits);
  if ((D == 0 && reduce_M == 0) || P == 0) return CFA_OK;
  if (D > 0 && (!out_ptrs || !src_ptrs || !state_ptrs || !grad_ptrs || !csr_ptr || !csr_idx || !csr_coef))
    return fail(CFA_E_INVALID, "null population table");
  if ((long long)D + reduce_M > 65535) return fail(CFA_E_INVALID, "D + M = %d exceeds grid.y limit", D + reduce_M);
  GeStepArgs a{out_ptrs, src_ptrs, state_ptrs, grad_ptrs, csr_ptr, csr_idx, csr_coef,
               (float)rho, (float)(1.0 - rho), lr1, lr2, (long long)lr_split, use_filtered ? 1 : 0,
               reduce_ws, reduce_out, reduce_M, reduce_splits};
  // buckets are 16-byte aligned (allocator contract, checked by the host layer)
  const long long nvec = (long long)P / 4;
  dim3 grid(shared_grid_x((nvec + kBlock - 1) / kBlock, pop_wg_per_cu(), D + reduce_M), (unsigned)(D + reduce_M));
  ge_step_kernel<<<grid, kBlock, 0, static_cast<hipStream_t>(stream)>>>(a, nvec, (long long)P);
  return check_launch("ge_step_kernel");
}

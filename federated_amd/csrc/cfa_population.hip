// cfa_population.hip — whole-population rounds: the CSR one-launch kernel
// (cfa_mix_population_f32; _sched_f32 with a table per round; _ended_f32 with the training_end
// rule on device-resident flags) and the sliding-window passes (cfa_mix_window_f32) that load each
// row of a ring window once for up to 8 consecutive devices, and the sliding ring round
// (cfa_mix_ring_slide_f32) that reads every row of a run of ring devices once, the FedAvg
// parameter-server round (cfa_fedavg_population_round_f32), and the CFA-GE population step. Every
// rule's step (seq_step, div_step, lin_step, tf1_first / tf1_step, mewma_step, split_sum) is the
// one definition of cfa_internal.h.
#include <type_traits>

#include "cfa_internal.h"
#include "cfa_fedavg_shape.h"
#include "cfa_slide_shape.h"

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

// csr_ptr is the round's table: D + 1 row offsets into csr_idx / csr_coef.
template <int RULE>
__device__ __forceinline__ void population_body(float* const* out_ptrs, const float* const* src_ptrs,
                                                const int32_t* csr_ptr, const int32_t* csr_idx,
                                                const float* csr_coef, long long nvec, long long P) {
  const int d = blockIdx.y;
  population_fold<RULE>(out_ptrs[d], src_ptrs, csr_idx, csr_coef, csr_ptr[d], csr_ptr[d + 1], false, 0.f, nvec, P);
}

template <int RULE>
__global__ __launch_bounds__(kBlock) void population_kernel(float* const* out_ptrs,
                                                            const float* const* src_ptrs,
                                                            const int32_t* csr_ptr,
                                                            const int32_t* csr_idx,
                                                            const float* csr_coef,
                                                            long long nvec, long long P) {
  population_body<RULE>(out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, nvec, P);
}

// Topology schedule (cfa_mix_population_sched_f32 / _sched_tf1_f32): T tables of D + 1 row offsets
// lie back to back in csr_ptr, their offsets absolute in the shared csr_idx / csr_coef, and round r
// mixes with table sched[r mod S]. The round counter is a device word, so a captured period of
// rounds replays with another table each time. Every workgroup of a round reads the same counter:
// round_advance_kernel raises it after the mix, in stream order. The lookup is one chain of
// uniform loads (round -> sched -> the table's base) ahead of the tile loop.
struct SchedArgs {
  const int32_t* sched;       // [S] table index of each slot
  unsigned long long* round;  // the round counter
  unsigned S;
};

__device__ __forceinline__ const int32_t* sched_table(const int32_t* csr_ptr, const SchedArgs& sc) {
  const unsigned long long r = *static_cast<const unsigned long long*>(sc.round);
  const int t = sc.sched[r % sc.S];
  return csr_ptr + (long long)t * ((long long)gridDim.y + 1);  // grid.y = D
}

template <int RULE>
__global__ __launch_bounds__(kBlock) void population_sched_kernel(float* const* out_ptrs,
                                                                  const float* const* src_ptrs,
                                                                  const int32_t* csr_ptr,
                                                                  const int32_t* csr_idx,
                                                                  const float* csr_coef, SchedArgs sc,
                                                                  long long nvec, long long P) {
  population_body<RULE>(out_ptrs, src_ptrs, sched_table(csr_ptr, sc), csr_idx, csr_coef, nvec, P);
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

// The first entry of [b, e) whose device is flagged, e when there is none: the workgroup's lanes
// take one entry each per pass and keep the smallest flagged position (as fedavg_round_lookup).
// Called by every lane of the workgroup (it synchronises).
__device__ __forceinline__ int first_ended(const int32_t* ended, const int32_t* csr_idx, int b, int e) {
  __shared__ int first;
  if (threadIdx.x == 0) first = e;
  __syncthreads();
  for (int k = b + (int)threadIdx.x; k < e; k += kBlock)
    if (ended[csr_idx[k]]) {
      atomicMin(&first, k);
      break;
    }
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(first);
}

template <bool SCHED>
__global__ __launch_bounds__(kBlock) void population_ended_kernel(float* const* out_ptrs,
                                                                  const float* const* src_ptrs,
                                                                  const int32_t* csr_ptr,
                                                                  const int32_t* csr_idx,
                                                                  const float* csr_coef, SchedArgs sc,
                                                                  EndedArgs ea, long long nvec, long long P) {
  const int32_t* ptr = csr_ptr;
  if constexpr (SCHED) ptr = sched_table(csr_ptr, sc);
  const int d = blockIdx.y;
  int e0 = ptr[d], e1 = ptr[d + 1];
  const bool self = ea.ended[d] != 0;  // uniform over the device's workgroups, as everything below
  int f = e1;
  if (!self) f = first_ended(ea.ended, csr_idx, e0 + 1, e1);
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

__global__ __launch_bounds__(kBlock) void population_tf1_kernel(float* const* out_ptrs,
                                                                const float* const* src_ptrs,
                                                                const int32_t* csr_ptr,
                                                                const int32_t* csr_idx,
                                                                const double* csr_coef,
                                                                long long nvec, long long P,
                                                                CompressParams cp) {
  population_tf1_body(out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, nvec, P, cp);
}

__global__ __launch_bounds__(kBlock) void population_tf1_sched_kernel(float* const* out_ptrs,
                                                                      const float* const* src_ptrs,
                                                                      const int32_t* csr_ptr,
                                                                      const int32_t* csr_idx,
                                                                      const double* csr_coef, SchedArgs sc,
                                                                      long long nvec, long long P,
                                                                      CompressParams cp) {
  population_tf1_body(out_ptrs, src_ptrs, sched_table(csr_ptr, sc), csr_idx, csr_coef, nvec, P, cp);
}

// ------------------------------------------------------------------------------------------
// Sliding-window population pass (cfa_mix_window_f32): nb <= 8 consecutive devices of a ring
// window (hl below, hr above) share their rows, so each row of the window is loaded ONCE per
// element for all nb devices: (nb + hl + hr) reads + nb writes instead of nb * (hl + hr + 2).
// Device b's local row is rows[b + hl]; its neighbours, in the reference window's order
// (g-hl .. g-1, g+1 .. g+hr), are rows[b .. b+hl-1], rows[b+hl+1 .. b+hl+hr].
// ------------------------------------------------------------------------------------------
constexpr int kWinMaxDev = 8;
struct WindowArgs {
  const float* rows[kWinMaxDev + 8];
  float* out[kWinMaxDev];
  float a[kWinMaxDev];  // one coefficient per device, used for each of its steps
  int nb;
};

// The fold of one ring device over its window's HL + HR + 1 rows, row(j) = the j-th row of the
// window (the local row is row(HL)): the local row, then the rows below in ascending order, then
// the rows above, as the reference window's order.
template <int HL, int HR, typename Row>
__device__ __forceinline__ f4 ring_fold(Row row, float a) {
  f4 acc = row(HL);
#pragma unroll
  for (int j = 0; j < HL; ++j) acc = seq_step(acc, row(j), a);
#pragma unroll
  for (int j = 0; j < HR; ++j) acc = seq_step(acc, row(HL + 1 + j), a);
  return acc;
}

template <int HL, int HR, int U, bool SC1>
__device__ __forceinline__ void window_body(const WindowArgs& w, long long nvec) {
  constexpr int R = kWinMaxDev + HL + HR;
  constexpr long long kTile = (long long)kBlock * U;
  const int nr = w.nb + HL + HR;
  for (long long t = blockIdx.x; t * kTile < nvec; t += gridDim.x) {
    const long long base = t * kTile + threadIdx.x;
    f4 r[U][R];
#pragma unroll
    for (int k = 0; k < R; ++k)
      if (k < nr)
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const long long i = base + (long long)u * kBlock;
          if (i < nvec) r[u][k] = ld4<true>(w.rows[k], i);
        }
#pragma unroll
    for (int b = 0; b < kWinMaxDev; ++b)
      if (b < w.nb) {
        // (unused and removed by the compiler when !SC1) write-through streaming store
        const __amdgpu_buffer_rsrc_t o = out_rsrc(w.out[b], (unsigned)(nvec * 16));
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const long long i = base + (long long)u * kBlock;
          if (i < nvec) {
            const f4 y = ring_fold<HL, HR>([&](int j) { return r[u][b + j]; }, w.a[b]);
            if constexpr (SC1)
              st16_buf<kStoreSc1>(o, i, y);
            else
              st4<true>(w.out[b], i, y);
          }
        }
      }
  }
}

template <int HL, int HR, int U, bool SC1>
__global__ __launch_bounds__(kBlock) void window_vec_kernel(WindowArgs w, long long nvec) {
  window_body<HL, HR, U, SC1>(w, nvec);
}

// A whole ring-window round of a stacked population in ONE launch (cfa_mix_ring_round_f32):
// grid.y = pass p over devices [8p, 8p + nb); each block derives its pass's rows from the stack
// base and pitch (row g of the window = in + ((8p - HL + g) mod D) * pitch), then runs the
// window pass body. Same operations as one cfa_mix_window_f32 launch per pass.
struct RingArgs {
  const float* in;
  float* out;
  const float* alphas;  // [D] device array, one coefficient per device
  long long pitch;      // floats between consecutive devices' rows
  long long off;        // element offset of this launch's chunk
  int D;
};

template <int HL, int HR, int U, bool SC1>
__global__ __launch_bounds__(kBlock) void ring_round_kernel(RingArgs ra, long long nvec) {
  const int p = blockIdx.y;
  WindowArgs w;
  w.nb = min(kWinMaxDev, ra.D - p * kWinMaxDev);
#pragma unroll
  for (int k = 0; k < kWinMaxDev + HL + HR; ++k) {
    const int g = ((p * kWinMaxDev - HL + k) % ra.D + ra.D) % ra.D;
    w.rows[k] = ra.in + (long long)g * ra.pitch + ra.off;
  }
#pragma unroll
  for (int b = 0; b < kWinMaxDev; ++b) {
    const int d = min(p * kWinMaxDev + b, ra.D - 1);
    w.out[b] = ra.out + (long long)d * ra.pitch + ra.off;
    w.a[b] = ra.alphas[d];
  }
  window_body<HL, HR, U, SC1>(w, nvec);
}

// ------------------------------------------------------------------------------------------
// Sliding ring round (cfa_mix_ring_slide_f32): every row of a run of consecutive ring devices is
// read ONCE and every output written once. A workgroup owns a column tile of kBlock * U float4
// (lane x holds vectors base + v * kBlock, v < U, so each wave instruction is a contiguous 1 KB)
// and a segment (blockIdx.y) of `seg` consecutive devices. It walks the segment's row stream
// (rows d0-HL .. d0+len-1+HR, mod `rows`) through a ring of W + PF register slots of U float4,
// W = HL+HR+1: device m of the segment folds stream rows m .. m+W-1 (its local row is m+HL) while
// the loads of rows m+W .. m+W-1+PF are in flight. The device loop is unrolled W + PF times, so
// stream row q always sits in slot q mod (W + PF) and every register index is static. A segment
// re-reads HL+HR halo rows: a call reads count + segments * (HL+HR) rows. The fold is the window
// pass's (ring_fold), on the slots the window's rows sit in, per vector.
// ------------------------------------------------------------------------------------------
struct SlideArgs {
  const float* in;
  float* out;
  const float* alphas;             // [count] device array, one coefficient per device of the run
  long long in_pitch, out_pitch;   // floats between consecutive rows
  long long off;                   // element offset of this launch's chunk
  int rows, first, count, seg;     // seg: devices per segment
};

template <int HL, int HR, int PF, int U, bool SC1>
__global__ __launch_bounds__(kBlock) void ring_slide_kernel(SlideArgs sa, long long nvec) {
  constexpr int W = HL + HR + 1;
  constexpr int RS = W + PF;
  constexpr long long kTile = (long long)kBlock * U;
  const int n0 = (int)blockIdx.y * sa.seg;  // first device of the segment, relative to sa.first
  const int len = min(sa.seg, sa.count - n0);
  const int total = len + HL + HR;  // rows of the segment's stream
  const int d0 = sa.first + n0;
  int g0 = (d0 - HL) % sa.rows;
  if (g0 < 0) g0 += sa.rows;
  const int o0 = d0 >= sa.rows ? d0 - sa.rows : d0;
  const float* const in = sa.in + sa.off;
  float* const out = sa.out + sa.off;
  const float* const in_end = in + (long long)sa.rows * sa.in_pitch;
  float* const out_end = out + (long long)sa.rows * sa.out_pitch;
  for (long long t = blockIdx.x; t * kTile < nvec; t += gridDim.x) {
    const long long i = t * kTile + threadIdx.x;
    if (i >= nvec) continue;  // the stripes ascend: a lane without its first vector has none
    // Byte offsets of the lane's vectors (a chunk is at most kMaxChunkVec float4: below 2^31). In
    // the last tile a stripe may lie partly or wholly past nvec: such a vector loads the lane's
    // first vector again (in bounds, so the loads need no branch) and is never stored.
    bool ok[U];
    unsigned voff[U];
#pragma unroll
    for (int v = 0; v < U; ++v) {
      ok[v] = i + (long long)v * kBlock < nvec;
      voff[v] = (unsigned)((ok[v] ? i + (long long)v * kBlock : i) * 16);
    }
    const float* rp = in + (long long)g0 * sa.in_pitch;  // next row of the stream to load
    float* op = out + (long long)o0 * sa.out_pitch;      // next output row
    f4 r[RS][U];
    auto load_row = [&](f4(&slot)[U]) {  // all U loads of the stream's next row
#pragma unroll
      for (int v = 0; v < U; ++v)
        slot[v] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(reinterpret_cast<const char*>(rp) + voff[v]));
      rp += sa.in_pitch;
      if (rp == in_end) rp = in;
    };
#pragma unroll
    for (int q = 0; q < RS - 1; ++q)
      if (q < total) load_row(r[q]);
    for (int n = 0; n < len; n += RS) {
#pragma unroll
      for (int u = 0; u < RS; ++u) {
        const int m = n + u;
        if (m < len) {
          // stream row m+W-1+PF: into the slot row m-1 has left
          if (m + RS - 1 < total) load_row(r[(u + RS - 1) % RS]);
          const float a = sa.alphas[n0 + m];
          f4 acc[U];
#pragma unroll
          for (int v = 0; v < U; ++v) acc[v] = ring_fold<HL, HR>([&](int j) { return r[(u + j) % RS][v]; }, a);
#pragma unroll
          for (int v = 0; v < U; ++v)
            if (ok[v]) {
              if constexpr (SC1)
                st16_buf<kStoreSc1>(out_rsrc(op, (unsigned)(nvec * 16)), i + (long long)v * kBlock, acc[v]);
              else
                __builtin_nontemporal_store(acc[v], reinterpret_cast<f4*>(reinterpret_cast<char*>(op) + voff[v]));
            }
          op += sa.out_pitch;
          if (op == out_end) op = out;
        }
      }
    }
  }
}

// Scalar window pass (misaligned rows, the < 4-element tail): runtime hl / hr.
__global__ __launch_bounds__(kBlock) void window_scalar_kernel(WindowArgs w, int hl, int hr,
                                                               long long begin, long long P) {
  for (long long i = begin + (long long)blockIdx.x * kBlock + threadIdx.x; i < P;
       i += (long long)gridDim.x * kBlock) {
    for (int b = 0; b < w.nb; ++b) {
      float acc = w.rows[b + hl][i];
      for (int j = 0; j < hl; ++j) acc = seq_step(acc, w.rows[b + j][i], w.a[b]);
      for (int j = 0; j < hr; ++j) acc = seq_step(acc, w.rows[b + hl + 1 + j][i], w.a[b]);
      w.out[b][i] = acc;
    }
  }
}

}  // namespace

namespace {
struct WindowTune {
  int vec, sc1, blocks_per_cu;
};
static WindowTune window_tune() {  // env overrides for tools/tune_window.py; results identical
  WindowTune t{1, 0, 6};  // tools/tune_window.py, profiles/r01_tune_window.jsonl
  t.vec = env_int("CFA_WINDOW_VEC", t.vec) == 1 ? 1 : 2;
  t.sc1 = env_int("CFA_WINDOW_SC1", t.sc1) ? 1 : 0;
  t.blocks_per_cu = env_int("CFA_WINDOW_BLOCKS_PER_CU", t.blocks_per_cu);
  if (t.blocks_per_cu <= 0) t.blocks_per_cu = 2;  // kept as it is: not the default 6
  return t;
}
static long long window_tiles(long long m, const WindowTune& t) {
  return (m + (long long)kBlock * t.vec - 1) / ((long long)kBlock * t.vec);
}
// The run-time (vec, sc1) of a window launch as the kernels' <U, SC1>: fn(U, SC1) gets them as
// std::integral_constant values.
template <typename F>
void for_vec_sc1(const WindowTune& t, F&& fn) {
  using One = std::integral_constant<int, 1>;
  using Two = std::integral_constant<int, 2>;
  if (t.vec == 1) {
    if (t.sc1) fn(One{}, std::true_type{});
    else fn(One{}, std::false_type{});
  } else {
    if (t.sc1) fn(Two{}, std::true_type{});
    else fn(Two{}, std::false_type{});
  }
}
template <int HL, int HR>
void launch_window(const WindowArgs& w, long long nvec, hipStream_t st) {
  const WindowTune t = window_tune();
  const cfa_launch_t lc{t.blocks_per_cu, t.vec, 1};
  for_each_chunk(nvec, [&](long long done, long long m) {
    WindowArgs c = w;
    for (int k = 0; k < w.nb + HL + HR; ++k) c.rows[k] = w.rows[k] + done * 4;
    for (int b = 0; b < w.nb; ++b) c.out[b] = w.out[b] + done * 4;
    const unsigned grid = grid_for(window_tiles(m, t), lc);
    for_vec_sc1(t, [&](auto u, auto sc1) {
      window_vec_kernel<HL, HR, decltype(u)::value, decltype(sc1)::value><<<grid, kBlock, 0, st>>>(c, m);
    });
  });
}
template <int HL, int HR>
void launch_ring_round(const RingArgs& ra, long long nvec, hipStream_t st) {
  const WindowTune t = window_tune();
  const cfa_launch_t lc{t.blocks_per_cu, t.vec, 1};
  const unsigned passes = (unsigned)((ra.D + kWinMaxDev - 1) / kWinMaxDev);
  for_each_chunk(nvec, [&](long long done, long long m) {
    RingArgs c = ra;
    c.off = ra.off + done * 4;
    const long long tiles = window_tiles(m, t);
    // the launch's blocks over all passes: about blocks_per_cu per CU in all. Not shared_grid_x:
    // the tiles are capped before the division by the passes (10 tiles over 16 passes give 1, not 10)
    long long gx = (grid_for(tiles, lc) + passes - 1) / passes;
    if (gx < 1) gx = 1;
    if (gx > tiles) gx = tiles;
    const dim3 grid((unsigned)gx, passes);
    for_vec_sc1(t, [&](auto u, auto sc1) {
      ring_round_kernel<HL, HR, decltype(u)::value, decltype(sc1)::value><<<grid, kBlock, 0, st>>>(c, m);
    });
  });
}

// Launch shape of the sliding ring round. The environment overrides are read at each launch, so
// one process can compare shapes on the same buffers (tools/probe/ring_slide.py); results are
// identical for every shape. SlideTune and its default are in cfa_slide_shape.h; here u = 0 stands
// for the tuned width, stepped down where a short row would leave workgroups without a tile
// (slide_pick_u), and CFA_SLIDE_U = 1, 2 or 4 for exactly that width.
static_assert(kSlideBlock == kBlock, "cfa_slide_shape.h counts tiles of kBlock lanes");
static SlideTune slide_tune() {
  const SlideTune d = kSlideDefault;
  SlideTune t{env_int("CFA_SLIDE_SEGMENTS", d.segments), env_int("CFA_SLIDE_WG_PER_CU", d.wg_per_cu),
              env_int("CFA_SLIDE_PF", d.pf), env_int("CFA_SLIDE_SC1", d.sc1) ? 1 : 0, env_int("CFA_SLIDE_U", 0)};
  if (t.segments <= 0) t.segments = d.segments;
  if (t.wg_per_cu <= 0) t.wg_per_cu = d.wg_per_cu;
  if (t.pf < 1 || t.pf > 2) t.pf = d.pf;
  if (t.u != 1 && t.u != 2 && t.u != 4) t.u = 0;
  return t;
}
template <int HL, int HR, int PF, int U>
void launch_slide_shape(const SlideArgs& c, long long m, dim3 grid, bool sc1, hipStream_t st) {
  if (sc1) ring_slide_kernel<HL, HR, PF, U, true><<<grid, kBlock, 0, st>>>(c, m);
  else ring_slide_kernel<HL, HR, PF, U, false><<<grid, kBlock, 0, st>>>(c, m);
}
template <int HL, int HR, int U>
void launch_slide_u(const SlideArgs& c, long long m, dim3 grid, const SlideTune& t, hipStream_t st) {
  switch (t.pf) {
    case 1: launch_slide_shape<HL, HR, 1, U>(c, m, grid, t.sc1, st); break;
    default: launch_slide_shape<HL, HR, 2, U>(c, m, grid, t.sc1, st); break;
  }
}
template <int HL, int HR>
void launch_ring_slide(const SlideArgs& sa, long long nvec, hipStream_t st) {
  const SlideTune t = slide_tune();
  int segments = t.segments < sa.count ? t.segments : sa.count;
  if (segments > 65535) segments = 65535;
  SlideArgs c = sa;
  c.seg = (sa.count + segments - 1) / segments;
  const unsigned gy = (unsigned)((sa.count + c.seg - 1) / c.seg);  // no empty segment
  for_each_chunk(nvec, [&](long long done, long long m) {
    c.off = done * 4;
    const int u = t.u ? t.u : slide_pick_u(m, kSlideDefault.u, device_cus(), t.wg_per_cu);
    // the launch's workgroups over all segments: about wg_per_cu per CU in all
    const dim3 grid(shared_grid_x(slide_tiles(m, u), t.wg_per_cu, gy), gy);
    switch (u) {
      case 4: launch_slide_u<HL, HR, 4>(c, m, grid, t, st); break;
      case 2: launch_slide_u<HL, HR, 2>(c, m, grid, t, st); break;
      default: launch_slide_u<HL, HR, 1>(c, m, grid, t, st); break;
    }
  });
}

// The launchers by (hl, hr), each 0..4: the one definition of the 5x5 table.
#define CFA_HLHR_ROW(F, L) {&F<L, 0>, &F<L, 1>, &F<L, 2>, &F<L, 3>, &F<L, 4>}
#define CFA_HLHR_TABLE(F) \
  {CFA_HLHR_ROW(F, 0), CFA_HLHR_ROW(F, 1), CFA_HLHR_ROW(F, 2), CFA_HLHR_ROW(F, 3), CFA_HLHR_ROW(F, 4)}
void (*const kWindowLaunch[5][5])(const WindowArgs&, long long, hipStream_t) = CFA_HLHR_TABLE(launch_window);
void (*const kRingLaunch[5][5])(const RingArgs&, long long, hipStream_t) = CFA_HLHR_TABLE(launch_ring_round);
void (*const kSlideLaunch[5][5])(const SlideArgs&, long long, hipStream_t) = CFA_HLHR_TABLE(launch_ring_slide);
#undef CFA_HLHR_TABLE
#undef CFA_HLHR_ROW
}  // namespace

extern "C" int cfa_mix_window_f32(float* const* out, const float* const* rows, const float* alphas,
                                  int nb, int hl, int hr, size_t P, void* stream) {
  if (nb < 1 || nb > kWinMaxDev) return fail(CFA_E_INVALID, "nb %d outside 1..%d", nb, kWinMaxDev);
  if (hl < 0 || hr < 0 || hl > 4 || hr > 4) return fail(CFA_E_INVALID, "window %d/%d outside 0..4", hl, hr);
  if (!out || !rows || !alphas) return fail(CFA_E_INVALID, "null table");
  if (P == 0) return CFA_OK;
  WindowArgs w{};
  w.nb = nb;
  const int nr = nb + hl + hr;
  bool aligned = true;
  for (int k = 0; k < nr; ++k) {
    if (!rows[k]) return fail(CFA_E_INVALID, "null row %d", k);
    w.rows[k] = rows[k];
    aligned = aligned && (addr(rows[k]) & 15) == 0;
  }
  for (int b = 0; b < nb; ++b) {
    if (!out[b]) return fail(CFA_E_INVALID, "null output %d", b);
    for (int k = 0; k < nr; ++k)
      if (out[b] == rows[k]) return fail(CFA_E_INVALID, "output %d aliases row %d", b, k);
    w.out[b] = out[b];
    aligned = aligned && (addr(out[b]) & 15) == 0;
    w.a[b] = alphas[b];
  }
  hipStream_t st = (hipStream_t)stream;
  const long long nvec = aligned ? (long long)(P / 4) : 0;
  if (nvec > 0) {
    kWindowLaunch[hl][hr](w, nvec, st);
    if (int rc = check_launch("window_vec")) return rc;
  }
  const long long begin = nvec * 4;
  if (begin < (long long)P) {
    const long long len = (long long)P - begin;
    window_scalar_kernel<<<grid_for((len + kBlock - 1) / kBlock), kBlock, 0, st>>>(w, hl, hr, begin, (long long)P);
    if (int rc = check_launch("window_scalar")) return rc;
  }
  return CFA_OK;
}

extern "C" int cfa_mix_ring_round_f32(float* out, const float* in, size_t pitch, const float* alphas, int D,
                                      int hl, int hr, size_t P, void* stream) {
  if (D < 1) return fail(CFA_E_INVALID, "device count %d", D);
  if (hl < 0 || hr < 0 || hl > 4 || hr > 4) return fail(CFA_E_INVALID, "window %d/%d outside 0..4", hl, hr);
  if (hl + hr >= D) return fail(CFA_E_INVALID, "window %d/%d wider than %d devices", hl, hr, D);
  if (!out || !in || !alphas) return fail(CFA_E_INVALID, "null buffer");
  if (pitch < P) return fail(CFA_E_INVALID, "pitch %zu below P %zu", pitch, P);
  if (P == 0) return CFA_OK;
  if ((addr(out) & 15) || (addr(in) & 15) || (pitch % 4) || (P % 4))
    return fail(CFA_E_UNSUPPORTED, "ring round needs 16-byte aligned rows (pitch and P multiples of 4)");
  const long long outb = (long long)addr(out), inb = (long long)addr(in), span = (long long)D * (long long)pitch * 4;
  if (outb < inb + span && inb < outb + span) return fail(CFA_E_INVALID, "out overlaps in");
  if ((long long)(D + kWinMaxDev - 1) / kWinMaxDev > 65535) return fail(CFA_E_INVALID, "D=%d exceeds grid.y", D);
  RingArgs ra{in, out, alphas, (long long)pitch, 0, D};
  kRingLaunch[hl][hr](ra, (long long)(P / 4), (hipStream_t)stream);
  return check_launch("ring_round");
}

extern "C" int cfa_mix_ring_slide_f32(float* out, size_t out_pitch, const float* in, size_t in_pitch,
                                      const float* alphas, int rows, int first, int count, int hl, int hr,
                                      size_t P, void* stream) {
  if (!out || !in || !alphas) return fail(CFA_E_INVALID, "null buffer");
  if (rows < 1 || count < 1) return fail(CFA_E_INVALID, "rows %d / count %d below 1", rows, count);
  if (first < 0 || first >= rows || count > rows || (count != rows && first > rows - count))
    return fail(CFA_E_INVALID, "devices %d..%d outside a ring of %d rows", first, first + count - 1, rows);
  if (hl < 0 || hr < 0 || hl > 4 || hr > 4) return fail(CFA_E_INVALID, "window %d/%d outside 0..4", hl, hr);
  if (hl + hr >= rows) return fail(CFA_E_INVALID, "window %d/%d wider than %d rows", hl, hr, rows);
  if (in_pitch < P || out_pitch < P)
    return fail(CFA_E_INVALID, "pitch %zu/%zu below P %zu", out_pitch, in_pitch, P);
  if (P == 0) return CFA_OK;
  const unsigned long long outb = addr(out), inb = addr(in);
  const unsigned long long out_span = ((unsigned long long)(rows - 1) * out_pitch + P) * 4;
  const unsigned long long in_span = ((unsigned long long)(rows - 1) * in_pitch + P) * 4;
  if (outb < inb + in_span && inb < outb + out_span) return fail(CFA_E_INVALID, "out overlaps in");
  if ((outb & 15) || (inb & 15) || (out_pitch % 4) || (in_pitch % 4) || (P % 4))
    return fail(CFA_E_UNSUPPORTED, "ring slide needs 16-byte aligned rows (pitches and P multiples of 4)");
  SlideArgs sa{in, out, alphas, (long long)in_pitch, (long long)out_pitch, 0, rows, first, count, count};
  kSlideLaunch[hl][hr](sa, (long long)(P / 4), (hipStream_t)stream);
  return check_launch("ring_slide");
}

// A scheduled entry's own arguments, checked before anything else; sc.sched == nullptr below
// stands for the static entry points' one table.
static int sched_args(const int32_t* sched, int S, int T, unsigned long long* round, SchedArgs& sc) {
  if (S <= 0 || T <= 0) return fail(CFA_E_INVALID, "schedule of %d slots over %d tables", S, T);
  if (!sched || !round) return fail(CFA_E_INVALID, "null schedule or round counter");
  sc = SchedArgs{sched, round, (unsigned)S};
  return CFA_OK;
}
// The round is over: the next launch on the stream reads the counter one higher.
int advance_counter(unsigned long long* counter, hipStream_t st) {
  round_advance_kernel<<<1, 1, 0, st>>>(counter);
  return check_launch("round_advance");
}
static int advance_round(const SchedArgs& sc, hipStream_t st) { return advance_counter(sc.round, st); }

static int population_tf1(float* const* out_ptrs, const float* const* src_ptrs, const int32_t* csr_ptr,
                          const int32_t* csr_idx, const double* csr_coef, const SchedArgs& sc, int D,
                          size_t P, int mode, size_t cbegin, size_t cend, unsigned long long* kept_counts,
                          void* stream) {
  if (D < 0) return fail(CFA_E_INVALID, "negative device count");
  CompressParams cp{};
  if (int rc = compress_params(mode, cp)) return rc;
  if (mode && (!kept_counts || cbegin > cend || cend > P))
    return fail(CFA_E_INVALID, "compression needs per-device counters and a segment within the bucket");
  cp.cbegin = (long long)cbegin;
  cp.cend = (long long)cend;
  cp.kept = kept_counts;
  if (D == 0 || P == 0) return CFA_OK;
  if (!out_ptrs || !src_ptrs || !csr_ptr || !csr_idx || !csr_coef)
    return fail(CFA_E_INVALID, "null population table");
  if (D > 65535) return fail(CFA_E_INVALID, "D=%d exceeds grid.y limit", D);
  const long long nvec = (long long)P / 4;
  const unsigned gx = shared_grid_x((nvec + kBlock - 1) / kBlock, pop_wg_per_cu(), D);
  hipStream_t st = (hipStream_t)stream;
  if (!sc.sched) {
    population_tf1_kernel<<<dim3(gx, (unsigned)D), kBlock, 0, st>>>(
        out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, nvec, (long long)P, cp);
    return check_launch("population_tf1");
  }
  population_tf1_sched_kernel<<<dim3(gx, (unsigned)D), kBlock, 0, st>>>(
      out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, sc, nvec, (long long)P, cp);
  if (int rc = check_launch("population_tf1_sched")) return rc;
  return advance_round(sc, st);
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
  if (D < 0) return fail(CFA_E_INVALID, "negative device count");
  if (rule != CFA_RULE_SEQUENTIAL && rule != CFA_RULE_LINEAR)
    return fail(CFA_E_INVALID, "unknown rule %d", rule);
  if (D == 0 || P == 0) return CFA_OK;
  if (!out_ptrs || !src_ptrs || !csr_ptr || !csr_idx || !csr_coef)
    return fail(CFA_E_INVALID, "null population table");
  if (D > 65535) return fail(CFA_E_INVALID, "D=%d exceeds grid.y limit", D);
  hipStream_t st = (hipStream_t)stream;
  // Buckets in a population are expected 16-byte aligned (allocator contract, checked by the
  // host layer); the body runs on float4, the <4-element tail in the first tile column.
  const long long nvec = (long long)P / 4;
  dim3 grid(shared_grid_x((nvec + 2LL * kBlock - 1) / (2LL * kBlock), pop_wg_per_cu(), D), (unsigned)D);
  if (!sc.sched) {
    if (rule == CFA_RULE_SEQUENTIAL)
      population_kernel<CFA_RULE_SEQUENTIAL><<<grid, kBlock, 0, st>>>(out_ptrs, src_ptrs, csr_ptr,
                                                                      csr_idx, csr_coef, nvec, (long long)P);
    else
      population_kernel<CFA_RULE_LINEAR><<<grid, kBlock, 0, st>>>(out_ptrs, src_ptrs, csr_ptr,
                                                                  csr_idx, csr_coef, nvec, (long long)P);
    return check_launch("population");
  }
  if (rule == CFA_RULE_SEQUENTIAL)
    population_sched_kernel<CFA_RULE_SEQUENTIAL><<<grid, kBlock, 0, st>>>(out_ptrs, src_ptrs, csr_ptr, csr_idx,
                                                                          csr_coef, sc, nvec, (long long)P);
  else
    population_sched_kernel<CFA_RULE_LINEAR><<<grid, kBlock, 0, st>>>(out_ptrs, src_ptrs, csr_ptr, csr_idx,
                                                                      csr_coef, sc, nvec, (long long)P);
  if (int rc = check_launch("population_sched")) return rc;
  return advance_round(sc, st);
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
  if (D < 0) return fail(CFA_E_INVALID, "negative device count");
  if (ended_rule != CFA_ENDED_COPY && ended_rule != CFA_ENDED_TRUNCATE && ended_rule != CFA_ENDED_TRUNCATE_EPS)
    return fail(CFA_E_INVALID, "unknown ended rule %d", ended_rule);
  if (!ended) return fail(CFA_E_INVALID, "null ended flags");
  // every workgroup of the round reads `ended` while one lane per device writes the other two
  if (flags_overlap(ended, ended_next, D > 0 ? D : 1) || flags_overlap(ended, saw, D > 0 ? D : 1))
    return fail(CFA_E_INVALID, "ended_next or saw aliases ended");
  if (D == 0 || P == 0) return CFA_OK;
  if (!out_ptrs || !src_ptrs || !csr_ptr || !csr_idx || !csr_coef)
    return fail(CFA_E_INVALID, "null population table");
  if (D > 65535) return fail(CFA_E_INVALID, "D=%d exceeds grid.y limit", D);
  hipStream_t st = (hipStream_t)stream;
  const EndedArgs ea{ended, ended_next, saw, ended_rule};
  const long long nvec = (long long)P / 4;  // buckets 16-byte aligned, as cfa_mix_population_f32
  dim3 grid(shared_grid_x((nvec + 2LL * kBlock - 1) / (2LL * kBlock), pop_wg_per_cu(), D), (unsigned)D);
  if (!sc.sched) {
    population_ended_kernel<false><<<grid, kBlock, 0, st>>>(out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, sc, ea,
                                                            nvec, (long long)P);
    return check_launch("population_ended");
  }
  population_ended_kernel<true><<<grid, kBlock, 0, st>>>(out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, sc, ea,
                                                         nvec, (long long)P);
  if (int rc = check_launch("population_ended_sched")) return rc;
  return advance_round(sc, st);
}

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
// the list for its first flagged entry: the workgroup's lanes take one entry each per pass and
// keep the smallest flagged position. Called by every lane of the workgroup (it synchronises).
__device__ __forceinline__ FedAvgRound fedavg_round_lookup(const FedAvgArgs& a, const SchedArgs& sc) {
  const unsigned long long r = *static_cast<const unsigned long long*>(sc.round);
  const int t = sc.sched[r % sc.S];
  FedAvgRound fr{a.act_ptr[t], a.act_ptr[t + 1], -1, a.act_div[t], a.act_rdiv[t]};
  if (a.ended) {
    __shared__ int first;
    if (threadIdx.x == 0) first = fr.e1;
    __syncthreads();
    for (int e = fr.e0 + (int)threadIdx.x; e < fr.e1; e += kBlock)
      if (a.ended[a.act_idx[e]]) {
        atomicMin(&first, e);
        break;
      }
    __syncthreads();
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

// cfa_grad.hip — CFA-GE neighbour-gradient evaluation: the gradient of a device's
// own cost at each neighbour's model, for the two TF1 graphs of cfa_ge_2stage.py, batched over
// the neighbour models in one launch (one workgroup per model).
//
// The reference builds the graph once per call (TF1/consensus/cfa_ge_2stage.py:391-433) and runs
// one Session per neighbour model (:512-528); cfa_ge_4stage.py:391-433 is the same graph. The
// graphs, their TF conventions and every phase of them (with its summation order) are in
// cfa_tf1_graph.h, shared with the local SGD epoch of cfa_local_sgd.hip. What is this file's own:
// the staging of the model with the first chunk, the chunks of a batch larger than the LDS, the
// batch split over grid.y, and the sink that accumulates a parameter's sum in its gradient bucket.
//
// These are tiny latency-bound graphs (P = 1 488 and 16 680 parameters, 24 samples per device):
// each workgroup keeps its model and every activation in LDS and runs forward and backward with
// barriers between the phases.
#include <algorithm>

#include "cfa_tf1_graph.h"

namespace {

// Phase timestamps for tools/probe/grad_phases.hip (compiled out of the library).
#ifdef CFA_GRAD_PHASES
// Stamps go to LDS and are copied out at the last phase (8 / 17), so no phase waits on the
// previous stamp's global store.
__device__ unsigned long long g_phase[32];
__device__ unsigned long long g_wg[4096][2];  // per workgroup: first and last stamp
__device__ __forceinline__ unsigned long long* phase_lds() {
  __shared__ unsigned long long s[32];  // one array per kernel, shared by every PHASE site
  return s;
}
#define PHASE(k) \
  do {           \
    unsigned long long* s_ts_ = phase_lds(); \
    __syncthreads(); \
    if (threadIdx.x == 0) { \
      s_ts_[k] = wall_clock64(); \
      if ((k) == 8 || (k) == 17) { \
        const unsigned wg_ = blockIdx.y * gridDim.x + blockIdx.x; \
        const int k0_ = (k) == 8 ? 0 : 10; \
        if (blockIdx.x == 0 && blockIdx.y == 0) \
          for (int j_ = k0_; j_ <= (k); ++j_) g_phase[j_] = s_ts_[j_]; \
        if (wg_ < 4096) g_wg[wg_][0] = s_ts_[k0_], g_wg[wg_][1] = s_ts_[k]; \
      } \
    } \
  } while (0)
#else
#define PHASE(k) \
  do {           \
  } while (0)
#endif

// stage() of three segments with all their loads in flight together.
__device__ __forceinline__ void stage3(float* d0, const float* s0, int n0, float* d1, const float* s1, int n1,
                                       float* d2, const float* s2, int n2, int tid, int T) {
  constexpr int U = 4;
  const int n = max(n0, max(n1, n2));
  for (int i = tid; i < n; i += U * T) {
    float v0[U], v1[U], v2[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = i + u * T;
      v0[u] = j < n0 ? s0[j] : 0.f;
      v1[u] = j < n1 ? s1[j] : 0.f;
      v2[u] = j < n2 ? s2[j] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = i + u * T;
      if (j < n0) d0[j] = v0[u];
      if (j < n1) d1[j] = v1[u];
      if (j < n2) d2[j] = v2[u];
    }
  }
}

// What belongs to a launch, not to the graph: B samples per evaluation, Bc per LDS-resident chunk,
// Bs per workgroup (grid.y splits the batch; partial sums go to a workspace).
struct GradBatch {
  int B, Bc, Bs;
};

// Per-sample LDS floats of the CNN kernel: x row, pooled / argmax / d pooled, logits, and the
// per-sample partial sums of the conv-layer gradients.
inline long long cnn_lds_per_sample(const CnnGeom& d) {
  const long long LN = (long long)d.L2 * d.NC;
  return d.L + 3 * LN + 2LL * d.C + (long long)d.F * d.NC + d.NC;
}
inline long long cnn_lds_fixed(const CnnGeom& d) {
  const long long LN = (long long)d.L2 * d.NC;
  return (long long)d.F * d.NC + d.NC + LN * d.C + d.C;
}

// Gradient sums run over all B samples; samples go through LDS in chunks of Bc. Every output
// element is owned by one thread for the whole launch (the same index loop in every chunk), so
// the per-chunk sums accumulate in the output bucket without atomics, in a fixed order (GradSink).
// FT, ST: conv_pool_forward's.
template <int FT, int ST>
__global__ __launch_bounds__(kGradBlock) void grad_cnn_kernel(const float* __restrict__ x,
                                                              const float* __restrict__ y,
                                                              const float* __restrict__ models,
                                                              const int* __restrict__ mrow,
                                                              const int* __restrict__ drow,
                                                              float* __restrict__ grads, CnnGeom d, GradBatch bt) {
  extern __shared__ float lds[];
  const int LN = d.L2 * d.NC;
  const int nW1 = d.F * d.NC, nW2 = LN * d.C, nG1 = nW1 + d.NC;
  float* W1 = lds;                        // [F][NC]
  float* b1 = W1 + nW1;                   // [NC]
  float* W2 = b1 + d.NC;                  // [LN][C]
  float* b2 = W2 + nW2;                   // [C]
  float* xs = b2 + d.C;                   // [Bc][L]
  float* pooled = xs + bt.Bc * d.L;       // [Bc][L2][NC]
  int* arg = reinterpret_cast<int*>(pooled + bt.Bc * LN);  // conv position of each window's max
  float* dfc = reinterpret_cast<float*>(arg + bt.Bc * LN); // [Bc][LN]
  float* zl = dfc + bt.Bc * LN;           // [Bc][C]: logits, then d logits
  float* ys = zl + bt.Bc * d.C;           // [Bc][C] labels
  float* part = ys + bt.Bc * d.C;         // [Bc][nG1]: per-sample conv-gradient sums
  // model and data rows of this workgroup's evaluation (population form), else model blockIdx.x
  // on the one data set
  const float* m = models + (long long)(mrow ? mrow[blockIdx.x] : (int)blockIdx.x) * d.P;
  const long long dr = drow ? drow[blockIdx.x] : 0;
  x += dr * bt.B * d.L;
  y += dr * bt.B * d.C;
  // grid.y splits the batch: this workgroup sums samples [bb, be) into its own partial bucket
  // (gridDim.y == 1: the model's gradient bucket itself)
  float* g = grads + ((long long)blockIdx.x * gridDim.y + blockIdx.y) * d.P;
  const int bb = blockIdx.y * bt.Bs, be = min(bt.B, bb + bt.Bs);
  const int tid = threadIdx.x, T = blockDim.x;
  float* gW2 = g + nG1;
  float* gb2 = gW2 + nW2;
  const float invB = 1.0f / (float)bt.B;

  PHASE(0);
  // the model bucket (W1 b1 W2 b2) and the first chunk's samples and labels, all in flight
  // together: one global round trip before the first barrier
  stage3(W1, m, nG1 + nW2 + d.C, xs, x + (long long)bb * d.L, bb < be ? min(bt.Bc, be - bb) * d.L : 0, ys,
         y + (long long)bb * d.C, bb < be ? min(bt.Bc, be - bb) * d.C : 0, tid, T);
  __syncthreads();
  PHASE(1);
  const bool taps_in_regs = cnn_taps_in_regs(d, T);
  float wreg[kMaxTaps];
  load_taps<FT>(wreg, W1, d, taps_in_regs, tid);
  if (bb >= be) {  // no sample left for this split: a zero partial
    for (long long i = threadIdx.x; i < d.P; i += blockDim.x) g[i] = 0.f;
    return;
  }
  for (int b0 = bb; b0 < be; b0 += bt.Bc) {
    const int nb = min(bt.Bc, be - b0);
    const GradSink sink{b0 == bb};
    if (!sink.first) {  // the first chunk was staged with the model
      stage(xs, x + (long long)b0 * d.L, nb * d.L, tid, T);
      stage(ys, y + (long long)b0 * d.C, nb * d.C, tid, T);
      __syncthreads();
    }
    PHASE(2);
    conv_pool_forward<FT, ST>(pooled, arg, xs, W1, b1, wreg, taps_in_regs, nb, d, tid, T);
    __syncthreads();
    PHASE(3);
    cnn_logits(zl, pooled, W2, b2, nb, LN, d.C, tid, T);
    __syncthreads();
    PHASE(4);
    softmax_xent<false>(zl, ys, nullptr, nb, d.C, d.SW, invB, true, tid, T);
    __syncthreads();
    PHASE(5);
    // dense layer gradients and the gradient flowing into the pooled features
    weight_sums<8>(gW2, nW2, d.C, pooled, LN, zl, nb, sink, tid, T);
    column_sums(gb2, d.C, zl, nb, sink, tid, T);
    relu_layer_backward(dfc, pooled, zl, W2, nb, LN, d.C, tid, T);
    __syncthreads();
    PHASE(6);
    conv_grad_partials(part, xs, arg, dfc, nb, d, tid, T);
    __syncthreads();
    PHASE(7);
    column_sums(g, nG1, part, nb, sink, tid, T);  // W1 and b1 are contiguous
    __syncthreads();  // the chunk's LDS is reused by the next one
    PHASE(8);
  }
}


inline long long nn_lds_per_sample(const NnGeom& d) { return d.L + 2LL * d.H + 2LL * d.C + (long long)d.G * d.H; }
inline long long nn_lds_fixed(const NnGeom& d) { return d.H + (long long)d.H * d.C + d.C; }

__global__ __launch_bounds__(kGradBlock) void grad_2nn_kernel(const float* __restrict__ x,
                                                              const float* __restrict__ y,
                                                              const float* __restrict__ models,
                                                              const int* __restrict__ mrow,
                                                              const int* __restrict__ drow,
                                                              float* __restrict__ grads, NnGeom d, GradBatch bt) {
  extern __shared__ float lds[];
  float* b1 = lds;                 // [H]
  float* W2 = b1 + d.H;            // [H][C]
  float* b2 = W2 + d.H * d.C;      // [C]
  float* xs = b2 + d.C;            // [Bc][L]
  float* act = xs + bt.Bc * d.L;   // [Bc][H] relu(x W1 + b1)
  float* dz = act + bt.Bc * d.H;   // [Bc][H]
  float* zl = dz + bt.Bc * d.H;    // [Bc][C]
  float* ys = zl + bt.Bc * d.C;    // [Bc][C]
  float* zpart = ys + bt.Bc * d.C; // [G][Bc][H]
  const long long nW1 = (long long)d.L * d.H;
  const float* m = models + (long long)(mrow ? mrow[blockIdx.x] : (int)blockIdx.x) * d.P;
  const long long dr = drow ? drow[blockIdx.x] : 0;
  x += dr * bt.B * d.L;
  y += dr * bt.B * d.C;
  const float* W1 = m;             // [L][H], read from global once per launch (kept in registers)
  // grid.y splits the batch: this workgroup sums samples [bb, be) into its own partial bucket
  // (gridDim.y == 1: the model's gradient bucket itself)
  float* g = grads + ((long long)blockIdx.x * gridDim.y + blockIdx.y) * d.P;
  const int bb = blockIdx.y * bt.Bs, be = min(bt.B, bb + bt.Bs);
  float* gW1 = g;
  float* gb1 = gW1 + nW1;
  float* gW2 = gb1 + d.H;
  float* gb2 = gW2 + d.H * d.C;
  const int tid = threadIdx.x, T = blockDim.x;
  const float invB = 1.0f / (float)bt.B;
  const int H4 = (d.H % 4 == 0 && (reinterpret_cast<uintptr_t>(dz) & 15) == 0) ? d.H / 4 : 0;

  PHASE(10);
  // W1 slice of this thread's (slice, h) pairs: with G * H <= T every thread owns one pair and
  // loads its kSpan weights once, for the whole launch (W1 is never staged in LDS). These loads,
  // the rest of the model (b1 W2 b2) and the first chunk's samples and labels are all in flight
  // together: one global round trip.
  const bool w_in_regs = d.G * d.H <= T;
  float wreg[kSpan];
  {
    const int h = tid % d.H, grp = tid / d.H, i0 = grp * kSpan;
#pragma unroll
    for (int u = 0; u < kSpan; ++u)
      wreg[u] = (w_in_regs && grp < d.G && i0 + u < d.L) ? W1[(long long)(i0 + u) * d.H + h] : 0.f;
  }
  stage3(b1, m + nW1, d.H + d.H * d.C + d.C, xs, x + (long long)bb * d.L, bb < be ? min(bt.Bc, be - bb) * d.L : 0,
         ys, y + (long long)bb * d.C, bb < be ? min(bt.Bc, be - bb) * d.C : 0, tid, T);
  if (bb >= be) {  // no sample left for this split: a zero partial
    for (long long i = threadIdx.x; i < d.P; i += blockDim.x) g[i] = 0.f;
    return;
  }
  for (int b0 = bb; b0 < be; b0 += bt.Bc) {
    const int nb = min(bt.Bc, be - b0);
    const GradSink sink{b0 == bb};
    if (!sink.first) {  // the first chunk was staged with the model
      stage(xs, x + (long long)b0 * d.L, nb * d.L, tid, T);
      stage(ys, y + (long long)b0 * d.C, nb * d.C, tid, T);
    }
    __syncthreads();
    PHASE(11);
    if (w_in_regs) {
      if (tid / d.H < d.G) nn_slice_partials<true>(zpart, bt.Bc, xs, wreg, tid / d.H, tid % d.H, nb, d);
    } else {
      nn_partials_from_memory(zpart, bt.Bc, xs, W1, nb, d, tid, T);
    }
    __syncthreads();
    PHASE(12);
    hidden_from_partials(act, zpart, bt.Bc, b1, nb, d, tid, T);
    __syncthreads();
    PHASE(13);
    nn_logits(zl, act, W2, b2, nb, d, tid, T);
    __syncthreads();
    PHASE(14);
    softmax_xent<false>(zl, ys, nullptr, nb, d.C, d.SW, invB, true, tid, T);
    __syncthreads();
    PHASE(15);
    weight_sums<0>(gW2, d.H * d.C, d.C, act, d.H, zl, nb, sink, tid, T);
    column_sums(gb2, d.C, zl, nb, sink, tid, T);
    relu_layer_backward(dz, act, zl, W2, nb, d.H, d.C, tid, T);
    __syncthreads();
    PHASE(16);
    if (H4) {  // gW1 = x^T dz, four h per thread: one x read feeds four FMAs
      const f4* dz4 = reinterpret_cast<const f4*>(dz);
      f4* gW14 = reinterpret_cast<f4*>(gW1);
      const bool aligned = (reinterpret_cast<uintptr_t>(gW1) & 15) == 0;
      for (long long idx = tid; idx < nW1 / 4; idx += T) {
        const int i = (int)(idx / H4), hq = (int)(idx % H4);
        f4 s;
        if (sink.first) {
          s = f4{0.f, 0.f, 0.f, 0.f};
        } else if (aligned) {
          s = gW14[idx];
        } else {
          for (int c = 0; c < 4; ++c) s[c] = gW1[idx * 4 + c];
        }
#pragma unroll 8
        for (int b = 0; b < nb; ++b) {
          const float xv = xs[b * d.L + i];
          const f4 dv = dz4[b * H4 + hq];
          s.x = fmaf(xv, dv.x, s.x);
          s.y = fmaf(xv, dv.y, s.y);
          s.z = fmaf(xv, dv.z, s.z);
          s.w = fmaf(xv, dv.w, s.w);
        }
        if (aligned) gW14[idx] = s;
        else for (int c = 0; c < 4; ++c) gW1[idx * 4 + c] = s[c];
      }
    } else {
      weight_sums<0>(gW1, nW1, d.H, xs, d.L, dz, nb, sink, tid, T);
    }
    column_sums(gb1, d.H, dz, nb, sink, tid, T);
    __syncthreads();
    PHASE(17);
  }
}

// Samples per chunk for `fixed` + Bc * `per_sample` floats of LDS; sets *bytes. 0 if not even one fits.
int plan_chunk(const void* kernel, long long fixed, long long per_sample, int B, long long* bytes) {
  long long limit = device_lds_max();
  if (const char* cap = getenv("CFA_GRAD_LDS_CAP")) limit = std::min<long long>(limit, atoll(cap));  // measurement knob
  auto fit = [&](long long lim) { return (int)std::min<long long>(B, (lim / 4 - fixed) / per_sample); };
  int bc = fit(limit);
  if (4 * (fixed + per_sample * bc) > 65536 && !raise_lds_limit(kernel, (int)limit)) bc = fit(65536);
  *bytes = 4 * (fixed + per_sample * std::max(bc, 0));
  return std::max(bc, 0);
}

}  // namespace

// Current device: cache its LDS size and raise every gradient kernel's dynamic-LDS limit to it
// now, so later launches (e.g. under hipGraph capture) need no attribute call.
int grad_prepare_device() {
  const int lim = device_lds_max();
  if (lim <= 65536) return CFA_OK;
  const void* kernels[] = {(const void*)grad_cnn_kernel<16, 5>, (const void*)grad_cnn_kernel<0, 0>,
                           (const void*)grad_2nn_kernel};
  for (const void* k : kernels) (void)raise_lds_limit(k, lim);  // refused: launches stay within 64 KiB
  return CFA_OK;
}

namespace {

// Sum of the Sp partial buckets of each evaluation, in split order (deterministic).
__global__ __launch_bounds__(kBlock) void reduce_splits_kernel(const float* __restrict__ ws,
                                                               float* __restrict__ grads, int Sp,
                                                               long long P) {
  const long long m = blockIdx.y;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < P; i += (long long)gridDim.x * kBlock)
    grads[m * P + i] = split_sum(ws + (m * Sp) * P + i, Sp, P);
}

int launch_reduce_splits(const float* ws, float* grads, int M, int Sp, long long P, hipStream_t st) {
  reduce_splits_kernel<<<dim3((unsigned)std::min<long long>((P + kBlock - 1) / kBlock, 64), (unsigned)M), kBlock, 0,
                         st>>>(ws, grads, Sp, P);
  return check_launch("reduce_splits_kernel");
}

// Batch split for M evaluations of B samples of P-parameter models: about two workgroups per CU
// in all, at most 8 per evaluation, and fewer for larger models, whose partial buckets (written
// and re-read by the reduction) and per-workgroup weight staging grow with P. Measured at the
// CFA-GE shapes (tools/probe/grad_split_sweep.sh, 32 evaluations of 24 samples): CNN (P = 1 488)
// 41.5 -> 17.0 us at 8 splits, 2NN (P = 16 680) 28.5 -> 21.3 us at 3, both slower past that.
int batch_split(int M, int B, long long P) {
  if (M <= 0 || B <= 1) return 1;
  int want = (2 * device_cus() + M - 1) / M;
  want = std::min<long long>(want, std::min<long long>(8, std::max<long long>(1, 65536 / std::max<long long>(P, 1))));
  if (const char* e = getenv("CFA_GRAD_SPLIT")) want = std::max(1, atoi(e));  // measurement knob
  int sp = std::max(1, std::min(B, want));
  const int bs = (B + sp - 1) / sp;
  return (B + bs - 1) / bs;
}

// Workspace of a split launch: the M * Sp partial buckets.
size_t split_workspace_elems(int M, int Sp, long long P) { return (size_t)M * Sp * (size_t)P; }

// What the two gradient launchers share once the graph's P and the batch B are known: the batch
// split (one workgroup per evaluation when no workspace holds the partials), the LDS chunk plan
// of a workgroup's samples, launch(grid, lds_bytes, part) of `kern` into the partial buckets, and
// the reduction of the splits into `grads`.
template <typename Launch>
int launch_grad_split(const char* fn, const char* what, const void* kern, long long P, GradBatch& bt,
                      long long lds_fixed, long long lds_per_sample, float* grads, float* ws, size_t ws_elems, int M,
                      hipStream_t st, Launch&& launch) {
  int Sp = batch_split(M, bt.B, P);
  if (!grads) {  // partials only: [M][Sp][P] into the workspace, summed by the caller
    if (ws_elems < split_workspace_elems(M, Sp, P))
      return fail(CFA_E_INVALID, "%s: partials-only launch needs %zu workspace floats", fn,
                  split_workspace_elems(M, Sp, P));
  } else if (!ws || ws_elems < split_workspace_elems(M, Sp, P)) {
    Sp = 1;
  }
  bt.Bs = (bt.B + Sp - 1) / Sp;
  // LDS for the samples one workgroup takes (its split), not the whole batch
  long long bytes = 0;
  bt.Bc = plan_chunk(kern, lds_fixed, lds_per_sample, bt.Bs, &bytes);
  if (bt.Bc < 1) return fail(CFA_E_UNSUPPORTED, "%s: one sample does not fit the workgroup's LDS", fn);
  launch(dim3((unsigned)M, (unsigned)Sp), (size_t)bytes, (Sp > 1 || !grads) ? ws : grads);
  if (int rc = check_launch(what)) return rc;
  return (Sp > 1 && grads) ? launch_reduce_splits(ws, grads, M, Sp, P, st) : CFA_OK;
}

// The launch's own arguments, after the graph's: M evaluations of B samples.
int grad_args(const char* fn, const float* x, const float* y, int B, const float* models, const float* grads,
              const float* ws, int M) {
  if (M < 0 || B < 1) return fail(CFA_E_INVALID, "%s: bad dimensions (B %d M %d)", fn, B, M);
  if (M > 0 && (!x || !y || !models || (!grads && !ws))) return fail(CFA_E_INVALID, "%s: null buffer", fn);
  return CFA_OK;
}

int launch_grad_cnn(const char* fn, const float* x, const float* y, int B, int L, int classes, int filter,
                    int number, int stride, const float* models, const int* mrow, const int* drow,
                    float* grads, float* ws, size_t ws_elems, int M, void* stream) {
  CnnGeom d;
  if (int rc = cnn_geom(fn, L, classes, filter, number, stride, d)) return rc;
  if (int rc = grad_args(fn, x, y, B, models, grads, ws, M)) return rc;
  if (M == 0) return CFA_OK;
  GradBatch bt{B, 0, 0};
  const bool fast = cnn_fast(d);
  const void* kern = fast ? (const void*)grad_cnn_kernel<16, 5> : (const void*)grad_cnn_kernel<0, 0>;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return launch_grad_split(fn, "grad_cnn_kernel", kern, d.P, bt, cnn_lds_fixed(d), cnn_lds_per_sample(d), grads, ws,
                           ws_elems, M, st, [&](dim3 grid, size_t bytes, float* part) {
    if (fast)
      grad_cnn_kernel<16, 5><<<grid, kGradBlock, bytes, st>>>(x, y, models, mrow, drow, part, d, bt);
    else
      grad_cnn_kernel<0, 0><<<grid, kGradBlock, bytes, st>>>(x, y, models, mrow, drow, part, d, bt);
  });
}

int launch_grad_2nn(const char* fn, const float* x, const float* y, int B, int L, int hidden, int classes,
                    const float* models, const int* mrow, const int* drow, float* grads, float* ws,
                    size_t ws_elems, int M, void* stream) {
  NnGeom d;
  if (int rc = nn_geom(fn, L, hidden, classes, d)) return rc;
  if (int rc = grad_args(fn, x, y, B, models, grads, ws, M)) return rc;
  if (M == 0) return CFA_OK;
  GradBatch bt{B, 0, 0};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return launch_grad_split(fn, "grad_2nn_kernel", (const void*)grad_2nn_kernel, d.P, bt, nn_lds_fixed(d),
                           nn_lds_per_sample(d), grads, ws, ws_elems, M, st,
                           [&](dim3 grid, size_t bytes, float* part) {
    grad_2nn_kernel<<<grid, kGradBlock, bytes, st>>>(x, y, models, mrow, drow, part, d, bt);
  });
}

}  // namespace

extern "C" int cfa_ge_grad_cnn_f32(const float* x, const float* y, int B, int L, int classes,
                                   int filter, int number, int stride, const float* models,
                                   float* grads, int M, void* stream) {
  return launch_grad_cnn("cfa_ge_grad_cnn_f32", x, y, B, L, classes, filter, number, stride, models, nullptr,
                         nullptr, grads, nullptr, 0, M, stream);
}

extern "C" int cfa_ge_grad_2nn_f32(const float* x, const float* y, int B, int L, int hidden,
                                   int classes, const float* models, float* grads, int M,
                                   void* stream) {
  return launch_grad_2nn("cfa_ge_grad_2nn_f32", x, y, B, L, hidden, classes, models, nullptr, nullptr, grads,
                         nullptr, 0, M, stream);
}

extern "C" int cfa_ge_grad_splits(int M, int B, size_t P) { return batch_split(M, B, (long long)P); }

extern "C" size_t cfa_ge_grad_workspace_elems(int M, int B, size_t P) {
  const int sp = batch_split(M, B, (long long)P);
  return sp > 1 ? split_workspace_elems(M, sp, (long long)P) : 0;
}

extern "C" int cfa_ge_grad_cnn_rows_f32(const float* x, const float* y, int B, int L, int classes,
                                        int filter, int number, int stride, const float* models,
                                        const int32_t* model_row, const int32_t* data_row,
                                        float* grads, float* workspace, size_t workspace_elems, int M,
                                        void* stream) {
  if (M > 0 && (!model_row || !data_row))
    return fail(CFA_E_INVALID, "cfa_ge_grad_cnn_rows_f32: null row table");
  return launch_grad_cnn("cfa_ge_grad_cnn_rows_f32", x, y, B, L, classes, filter, number, stride, models,
                         model_row, data_row, grads, workspace, workspace_elems, M, stream);
}

extern "C" int cfa_ge_grad_2nn_rows_f32(const float* x, const float* y, int B, int L, int hidden,
                                        int classes, const float* models, const int32_t* model_row,
                                        const int32_t* data_row, float* grads, float* workspace,
                                        size_t workspace_elems, int M, void* stream) {
  if (M > 0 && (!model_row || !data_row))
    return fail(CFA_E_INVALID, "cfa_ge_grad_2nn_rows_f32: null row table");
  return launch_grad_2nn("cfa_ge_grad_2nn_rows_f32", x, y, B, L, hidden, classes, models, model_row, data_row,
                         grads, workspace, workspace_elems, M, stream);
}

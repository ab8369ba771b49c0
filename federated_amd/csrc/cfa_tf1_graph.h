// cfa_tf1_graph.h — the two TF1 model graphs of cfa_ge_2stage.py:391-433, written once as phases
// for the kernels that evaluate them (cfa_grad.hip: the CFA-GE neighbour gradients;
// cfa_local_sgd.hip: the local SGD epoch), and the graphs' geometry on the host.
//   CNN (ML_model 1, :392-405): x[B,L] -> conv1d(W1[F,1,NC], stride S, SAME) + b1 -> relu ->
//       max_pooling1d(pool S, stride S, SAME) -> flatten NWC [B, L2*NC] -> softmax(. W2 + b2)
//   2NN (ML_model 2, :407-420): softmax(relu(x W1 + b1) W2 + b2)
//   cost = mean_b(-sum_c y * log(clip(pred, 1e-15, 0.99))) (:425-426); d cost / d{W1,b1,W2,b2} (:429-430)
// TF conventions kept: SAME padding (out = ceil(L/S), total pad max((out-1)S + k - L, 0), left =
// total/2, padded pooling entries never win), max-pool gradient to the first maximum of a window,
// relu gradient where the activation is > 0, clip gradient where 1e-15 <= pred <= 0.99.
//
// A phase is a __device__ __forceinline__ function over LDS pointers that every thread of the
// workgroup calls (tid of T); the caller puts the barriers between phases. A kernel keeps what is
// its own: staging and prefetch, chunking and the batch split, the cost, and through a sink where
// a parameter's gradient sum starts and where it goes. The order of every sum is fixed here, so
// the kernels agree bit for bit (tests/test_gpu_local_sgd_paths.py asserts it). fp32 throughout,
// like the reference's placeholders. Not installed, not an ABI.
#pragma once
#include "cfa_grad_common.h"

namespace {

constexpr int kSpan = 32;  // first-layer inputs of the 2NN per partial sum (a W1 slice held in registers)

// ---- geometry (host) ----------------------------------------------------------------------

struct CnnGeom {
  int L, C, F, NC, S;
  int SW;              // softmax lanes per sample (softmax_width(C))
  int L1, L2, pl, ql;  // conv / pool output lengths, left pads
  long long P;         // parameters per model: W1 b1 W2 b2
};

struct NnGeom {
  int L, H, C;
  int SW;  // softmax lanes per sample (softmax_width(C))
  int G;   // ceil(L / kSpan) slices of the input dimension for the first layer's partial sums
  long long P;
};

// The CNN's geometry from the caller's dimensions; refuses what no kernel of the graph takes.
inline int cnn_geom(const char* fn, int L, int classes, int filter, int number, int stride, CnnGeom& d) {
  if (L < 1 || classes < 1 || filter < 1 || number < 1 || stride < 1)
    return fail(CFA_E_INVALID, "%s: bad dimensions (L %d C %d F %d NC %d S %d)", fn, L, classes, filter, number,
                stride);
  if (classes > 64) return fail(CFA_E_UNSUPPORTED, "%s: more than 64 classes", fn);
  d.L = L, d.C = classes, d.F = filter, d.NC = number, d.S = stride;
  d.SW = softmax_width(classes);
  d.L1 = (L + stride - 1) / stride;
  d.L2 = (d.L1 + stride - 1) / stride;
  d.pl = same_left(L, filter, stride);
  d.ql = same_left(d.L1, stride, stride);
  d.P = (long long)filter * number + number + (long long)d.L2 * number * classes + classes;
  return CFA_OK;
}

// The CFA-GE CNN's geometry (filter 16, stride 5: federated_sample_CNN_CFA-GE.py:36-39) gets the
// kernels' <16, 5> instantiation, every other one <0, 0>.
inline bool cnn_fast(const CnnGeom& d) { return d.F == 16 && d.S == 5; }

inline int nn_geom(const char* fn, int L, int hidden, int classes, NnGeom& d) {
  if (L < 1 || hidden < 1 || classes < 1)
    return fail(CFA_E_INVALID, "%s: bad dimensions (L %d H %d C %d)", fn, L, hidden, classes);
  if (classes > 64) return fail(CFA_E_UNSUPPORTED, "%s: more than 64 classes", fn);
  d.L = L, d.H = hidden, d.C = classes;
  d.SW = softmax_width(classes);
  d.G = (L + kSpan - 1) / kSpan;
  d.P = (long long)L * hidden + hidden + (long long)hidden * classes + classes;
  return CFA_OK;
}

// ---- sinks: where a parameter's sum over the samples starts and where it goes ---------------

// cfa_grad.hip: the sum continues the bucket's (the first chunk starts it) and is stored there.
struct GradSink {
  bool first;
  __device__ __forceinline__ float start(const float* g) const { return first ? 0.f : *g; }
  __device__ __forceinline__ void put(float* g, float s) const { *g = s; }
};

// cfa_local_sgd.hip: the sum is the minibatch's gradient, applied to the parameter in LDS.
struct SgdSink {
  float lr;
  __device__ __forceinline__ float start(const float*) const { return 0.f; }
  __device__ __forceinline__ void put(float* w, float s) const { *w = *w - lr * s; }
};

// body(b) for the samples of a chunk in order; U > 0 is the kernel's own unroll count.
template <int U, typename Body>
__device__ __forceinline__ void for_samples(int nb, Body&& body) {
  if constexpr (U > 0) {
#pragma unroll U
    for (int b = 0; b < nb; ++b) body(b);
  } else {
    for (int b = 0; b < nb; ++b) body(b);
  }
}

// dst[i][k] (+)= sum_b a[b][i] * dl[b][k] for the n = rows * K elements of a weight matrix: W2 of
// both graphs (a: pooled or act) and W1 of the 2NN (a: x, dl: dz).
template <int U, typename Idx, typename Sink>
__device__ __forceinline__ void weight_sums(float* dst, Idx n, int K, const float* a, int a_stride, const float* dl,
                                            int nb, const Sink& sink, int tid, int T) {
  for (Idx idx = tid; idx < n; idx += T) {
    const int i = (int)(idx / K), k = (int)(idx % K);
    float s = sink.start(dst + idx);
    for_samples<U>(nb, [&](int b) { s = fmaf(a[b * a_stride + i], dl[b * K + k], s); });
    sink.put(dst + idx, s);
  }
}

// dst[k] (+)= sum_b v[b][k]: the biases (v: d logits, dz) and W1 b1 of the CNN (v: part).
template <typename Sink>
__device__ __forceinline__ void column_sums(float* dst, int n, const float* v, int nb, const Sink& sink, int tid,
                                            int T) {
  for (int k = tid; k < n; k += T) {
    float s = sink.start(dst + k);
    for (int b = 0; b < nb; ++b) s += v[b * n + k];
    sink.put(dst + k, s);
  }
}

// ---- both graphs ----------------------------------------------------------------------------

// Softmax and clipped cross-entropy of logits z[nb][C]. COST: cs[b] = -sum_c y_c log(clip(pred_c)).
// backward: z becomes d cost / d logits in place: d cost / d pred_c = -(y_c / clip(pred_c)) / B
// where the clip passes the gradient; then the softmax gradient (dp - sum(dp * p)) * p (TF
// SoftmaxGrad). One lane per class: a sample's W >= C lanes (W a power of two <= 64, so a group
// never straddles a wave) reduce max, sum, cost and dot with xor shuffles, and every value stays
// in registers.
template <bool COST>
__device__ __forceinline__ void softmax_xent(float* z, const float* y, float* cs, int nb, int C, int W, float invB,
                                             bool backward, int tid, int T) {
  for (int idx = tid; idx < nb * W; idx += T) {
    const int b = idx / W, c = idx % W;
    const bool valid = c < C;
    const float zc = valid ? z[b * C + c] : -INFINITY;
    const float yc = valid ? y[b * C + c] : 0.f;
    float mx = zc;
    for (int o = W >> 1; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, W));
    const float e = valid ? expf(zc - mx) : 0.f;
    float s = e;
    for (int o = W >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, W);
    const float p = e / s;  // pred
    const float pc = fminf(fmaxf(p, kClipLo), kClipHi);
    if constexpr (COST) {
      float l = valid ? yc * logf(pc) : 0.f;
      for (int o = W >> 1; o > 0; o >>= 1) l += __shfl_xor(l, o, W);
      if (c == 0) cs[b] = -l;
    }
    if (backward) {
      const bool pass = valid && p >= kClipLo && p <= kClipHi;
      const float dp = pass ? -(yc / pc) * invB : 0.f;
      float dot = dp * p;
      for (int o = W >> 1; o > 0; o >>= 1) dot += __shfl_xor(dot, o, W);
      if (valid) z[b * C + c] = (dp - dot) * p;
    }
  }
}

// The gradient flowing from d logits dl[nb][C] through W2[n][C] into a relu'd layer h[nb][n]
// (the CNN's pooled features: the relu gradient at the window's max; the 2NN's hidden layer).
__device__ __forceinline__ void relu_layer_backward(float* dh, const float* h, const float* dl, const float* W2,
                                                    int nb, int n, int C, int tid, int T) {
  for (int idx = tid; idx < nb * n; idx += T) {
    const int b = idx / n, i = idx % n;
    float s = 0.f;
    for (int k = 0; k < C; ++k) s = fmaf(dl[b * C + k], W2[i * C + k], s);
    dh[idx] = h[idx] > 0.f ? s : 0.f;
  }
}

// ---- CNN ------------------------------------------------------------------------------------

// The conv taps of this thread's channel in registers (T is a multiple of NC, so every item a
// thread takes in conv_pool_forward has the same channel c = tid % NC). One channel index and one
// uniform branch around every tap load (a per-tap predicate recomputed the modulo and branched 32
// times: 2.6 us at the config-3 shapes).
__device__ __forceinline__ bool cnn_taps_in_regs(const CnnGeom& d, int T) { return d.F <= kMaxTaps && T % d.NC == 0; }

template <int FT>
__device__ __forceinline__ void load_taps(float (&wreg)[kMaxTaps], const float* W1, const CnnGeom& d,
                                          bool taps_in_regs, int tid) {
  const int creg = tid % d.NC;
  constexpr int KT = FT > 0 ? FT : kMaxTaps;
#pragma unroll
  for (int k = 0; k < kMaxTaps; ++k) wreg[k] = 0.f;
  if (taps_in_regs) {
#pragma unroll
    for (int k = 0; k < KT; ++k)
      if (FT > 0 || k < d.F) wreg[k] = W1[k * d.NC + creg];
  }
}

// conv + bias + relu evaluated inside each pooling window; keeps the max (pooled[nb][L2][NC]) and
// its conv position (arg). FT, ST > 0: a filter of FT taps with stride (= pool size) ST at compile
// time: a pooling window's (ST - 1) * ST + FT input samples are loaded once, all in flight
// together, and its ST convolutions run from registers. FT = ST = 0: any geometry (runtime loops).
template <int FT, int ST>
__device__ __forceinline__ void conv_pool_forward(float* pooled, int* arg, const float* xs, const float* W1,
                                                  const float* b1, const float (&wreg)[kMaxTaps], bool taps_in_regs,
                                                  int nb, const CnnGeom& d, int tid, int T) {
  const int LN = d.L2 * d.NC;
  for (int idx = tid; idx < nb * LN; idx += T) {
    const int b = idx / LN, r = idx % LN, q = r / d.NC, c = r % d.NC;
    const float* xb = xs + b * d.L;
    float best = -INFINITY;
    int barg = -1;
    bool done = false;
    if constexpr (FT > 0 && ST > 0) {
      // Every window, boundary ones included, takes this branch-free path: samples outside
      // [0, L) read as 0 (a zero tap adds nothing: fma(0, w, z) == z) and positions outside
      // [0, L1) never win, so no lane of a wave waits on a divergent slow path.
      constexpr int NX = (ST - 1) * ST + FT;
      const int p0 = q * ST - d.ql, t0 = p0 * ST - d.pl;
      if (taps_in_regs) {
        float xv[NX];
#pragma unroll
        for (int u = 0; u < NX; ++u) {
          const int t = t0 + u;
          const bool in = t >= 0 && t < d.L;
          const float v = xb[in ? t : 0];
          xv[u] = in ? v : 0.f;
        }
#pragma unroll
        for (int j = 0; j < ST; ++j) {
          float z = 0.f;
#pragma unroll
          for (int k = 0; k < FT; ++k) z = fmaf(xv[j * ST + k], wreg[k], z);
          z += b1[c];
          const float h = z > 0.f ? z : 0.f;
          const int p = p0 + j;
          if (p >= 0 && p < d.L1 && h > best) {
            best = h;
            barg = p;
          }
        }
        done = true;
      }
    }
    for (int j = 0; j < d.S && !done; ++j) {
      const int p = q * d.S - d.ql + j;
      if (p < 0 || p >= d.L1) continue;
      const int t0 = p * d.S - d.pl;
      float z = 0.f;
      for (int k = 0; k < d.F; ++k) {
        const int t = t0 + k;
        if (t >= 0 && t < d.L) z = fmaf(xb[t], W1[k * d.NC + c], z);
      }
      z += b1[c];
      const float h = z > 0.f ? z : 0.f;
      if (h > best) {
        best = h;
        barg = p;
      }
    }
    pooled[idx] = best;
    arg[idx] = barg;
  }
}

// logits zl[nb][C] = pooled W2 + b2: 8 lanes per (sample, class), strided partial sums,
// xor-shuffle reduction
__device__ __forceinline__ void cnn_logits(float* zl, const float* pooled, const float* W2, const float* b2, int nb,
                                           int LN, int C, int tid, int T) {
  for (int idx = tid; idx < nb * C * 8; idx += T) {
    const int o = idx >> 3, lane = idx & 7;
    const int b = o / C, k = o % C;
    float z = 0.f;
    for (int i = lane; i < LN; i += 8) z = fmaf(pooled[b * LN + i], W2[i * C + k], z);
    z += __shfl_xor(z, 1, 8);
    z += __shfl_xor(z, 2, 8);
    z += __shfl_xor(z, 4, 8);
    if (lane == 0) zl[o] = z + b2[k];
  }
}

// conv gradients per (weight, sample), part[nb][F * NC + NC] (W1 then b1): only each window's max
// position receives gradient
__device__ __forceinline__ void conv_grad_partials(float* part, const float* xs, const int* arg, const float* dfc,
                                                   int nb, const CnnGeom& d, int tid, int T) {
  const int LN = d.L2 * d.NC, nW1 = d.F * d.NC, nG1 = nW1 + d.NC;
  for (int idx = tid; idx < nG1 * nb; idx += T) {  // e fastest: lanes read neighbouring channels
    const int e = idx % nG1, b = idx / nG1;
    float s = 0.f;
    if (e < nW1) {
      const int k = e / d.NC, c = e % d.NC;
#pragma unroll 7
      for (int q = 0; q < d.L2; ++q) {  // select, not branch: the loads stay in flight together
        const int f = b * LN + q * d.NC + c;
        const int t = arg[f] * d.S + k - d.pl;
        const bool in = t >= 0 && t < d.L;
        const float xv = xs[b * d.L + (in ? t : 0)];
        s = fmaf(dfc[f], in ? xv : 0.f, s);
      }
    } else {
      const int c = e - nW1;
#pragma unroll 7
      for (int q = 0; q < d.L2; ++q) s += dfc[b * LN + q * d.NC + c];
    }
    part[b * nG1 + e] = s;
  }
}

// ---- 2NN ------------------------------------------------------------------------------------

// The first layer as G partial sums over kSpan-wide slices of the input dimension, zpart[G][zs][H]
// (zs: the sample stride the caller's LDS plan gives a slice). One (slice grp, unit h) pair from
// its weights w in registers, for every sample of the chunk. PRELOAD: a full slice's inputs are
// all loaded before the FMA chain; the chain is the same either way.
template <bool PRELOAD>
__device__ __forceinline__ void nn_slice_partials(float* zpart, int zs, const float* xs, const float (&w)[kSpan],
                                                  int grp, int h, int nb, const NnGeom& d) {
  const int i0 = grp * kSpan, n = min(kSpan, d.L - i0);
  for (int b = 0; b < nb; ++b) {
    const float* xb = xs + b * d.L + i0;
    float z = 0.f;
    if (PRELOAD && n == kSpan) {
      float xv[kSpan];
#pragma unroll
      for (int u = 0; u < kSpan; ++u) xv[u] = xb[u];
#pragma unroll
      for (int u = 0; u < kSpan; ++u) z = fmaf(xv[u], w[u], z);
    } else {
#pragma unroll
      for (int u = 0; u < kSpan; ++u)
        if (u < n) z = fmaf(xb[u], w[u], z);
    }
    zpart[(grp * zs + b) * d.H + h] = z;
  }
}

// The same partial sums with W1[L][H] read from memory, one (slice, sample, unit) per item.
__device__ __forceinline__ void nn_partials_from_memory(float* zpart, int zs, const float* xs, const float* W1,
                                                        int nb, const NnGeom& d, int tid, int T) {
  for (int idx = tid; idx < d.G * nb * d.H; idx += T) {
    const int h = idx % d.H, r = idx / d.H, b = r % nb, grp = r / nb;
    const int i0 = grp * kSpan, i1 = min(d.L, i0 + kSpan);
    float z = 0.f;
    for (int i = i0; i < i1; ++i) z = fmaf(xs[b * d.L + i], W1[(long long)i * d.H + h], z);
    zpart[(grp * zs + b) * d.H + h] = z;
  }
}

// act[nb][H] = relu(sum of the slices in order + b1)
__device__ __forceinline__ void hidden_from_partials(float* act, const float* zpart, int zs, const float* b1, int nb,
                                                     const NnGeom& d, int tid, int T) {
  for (int idx = tid; idx < nb * d.H; idx += T) {
    const int b = idx / d.H, h = idx % d.H;
    float z = 0.f;
    for (int grp = 0; grp < d.G; ++grp) z += zpart[(grp * zs + b) * d.H + h];
    z += b1[h];
    act[idx] = z > 0.f ? z : 0.f;
  }
}

// logits zl[nb][C] = act W2 + b2
__device__ __forceinline__ void nn_logits(float* zl, const float* act, const float* W2, const float* b2, int nb,
                                          const NnGeom& d, int tid, int T) {
  for (int idx = tid; idx < nb * d.C; idx += T) {
    const int b = idx / d.C, k = idx % d.C;
    float z = 0.f;
    for (int h = 0; h < d.H; ++h) z = fmaf(act[b * d.H + h], W2[h * d.C + k], z);
    zl[idx] = z + b2[k];
  }
}

}  // namespace

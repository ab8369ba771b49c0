// cfa_local_sgd.hip — one local epoch of plain minibatch SGD for every device of a TF1 population
// in ONE launch (tensorflow1_implementations/federated_sample_CNN_CFA-GE.py:137-173 and
// federated_sample_2NN_CFA.py:97-101: per minibatch W <- W_ext - learning_rate * grad, :114-118,
// then the validation cost :163-172), on the two model graphs of cfa_grad.hip.
//
// One workgroup owns one device for the whole launch: its model is read from global memory once,
// stays in LDS for all `steps` minibatches and is stepped there, and is written back once. The
// graph of a minibatch is the graph of cfa_grad.hip (same phases, same summation orders); what
// differs is that the gradient of a parameter is not stored but applied to the LDS copy by the
// thread that owns it, after every read of the pre-update value (the hidden-layer gradient reads
// the pre-update W2; a barrier separates it from W2's step). The next minibatch's samples are
// loaded into registers before the current one's first phase and stored to the other half of a
// double buffer after its last, so their global round trip hides behind the compute.
//
// update = 0 is the validation pass: forward only, models untouched. The mean minibatch cost of
// the launch is accumulated in fp64 (the driver's Python float `avg_cost += c / total_batch`).
// Every output is owned by one thread and every sum runs in a fixed order: a launch is
// deterministic.
#include "cfa_grad_common.h"

namespace {

struct SgdArgs {
  const float* x;        // [D][Ns][L]
  const float* y;        // [D][Ns][C]
  float* models;         // [D][pitch]
  long long pitch;
  int Ns, bstride, nb, steps;  // minibatch i = rows [i * bstride, i * bstride + nb)
  float lr;
  int update;
  double* cost;                     // [D] or null
  double* cost_log;                 // [log_cap][D] or null
  int log_cap;
  const unsigned long long* epoch;  // row of cost_log (clamped), or null
};

// The next minibatch on its way from global memory to LDS: the first kPreX * T floats of its
// samples and kPreY * T of its labels wait in registers between load() and store(); what a larger
// minibatch has beyond that is copied by store() itself.
constexpr int kPreX = 8, kPreY = 2;
struct Prefetch {
  float x[kPreX], y[kPreY];
  __device__ __forceinline__ void load(const float* xs, int nx, const float* ys, int ny, int tid, int T) {
#pragma unroll
    for (int u = 0; u < kPreX; ++u) x[u] = tid + u * T < nx ? xs[tid + u * T] : 0.f;
#pragma unroll
    for (int u = 0; u < kPreY; ++u) y[u] = tid + u * T < ny ? ys[tid + u * T] : 0.f;
  }
  __device__ __forceinline__ void store(float* dx, const float* xs, int nx, float* dy, const float* ys, int ny,
                                        int tid, int T) const {
#pragma unroll
    for (int u = 0; u < kPreX; ++u)
      if (tid + u * T < nx) dx[tid + u * T] = x[u];
#pragma unroll
    for (int u = 0; u < kPreY; ++u)
      if (tid + u * T < ny) dy[tid + u * T] = y[u];
    for (int j = tid + kPreX * T; j < nx; j += T) dx[j] = xs[j];
    for (int j = tid + kPreY * T; j < ny; j += T) dy[j] = ys[j];
  }
};

// Softmax and clipped cross-entropy of logits z[nb][C]: cs[b] = -sum_c y_c log(clip(pred_c)), and
// with `backward` z becomes d cost / d logits in place, as softmax_xent_backward of cfa_grad.hip
// leaves it (the same operations in the same order). One lane per class, W >= C lanes per sample.
__device__ void softmax_xent_cost(float* z, const float* y, float* cs, int nb, int C, int W, float invB,
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
    float l = valid ? yc * logf(pc) : 0.f;
    for (int o = W >> 1; o > 0; o >>= 1) l += __shfl_xor(l, o, W);
    if (c == 0) cs[b] = -l;
    if (backward) {
      const bool pass = valid && p >= kClipLo && p <= kClipHi;
      const float dp = pass ? -(yc / pc) * invB : 0.f;
      float dot = dp * p;
      for (int o = W >> 1; o > 0; o >>= 1) dot += __shfl_xor(dot, o, W);
      if (valid) z[b * C + c] = (dp - dot) * p;
    }
  }
}

// Thread 0 after the cost phase's barrier: the minibatch's mean cost in fp32 (reduce_mean), added
// to the launch's mean in fp64.
__device__ __forceinline__ void add_cost(double& acc, const float* cs, int nb, int steps) {
  float c = 0.f;
  for (int b = 0; b < nb; ++b) c += cs[b];
  c = c / (float)nb;
  acc += (double)c / (double)steps;
}

// Thread 0 at the end of the launch: the device's mean cost, and its entry of the cost log.
__device__ __forceinline__ void put_cost(const SgdArgs& a, int dv, int D, double acc) {
  if (a.cost) a.cost[dv] = acc;
  if (a.cost_log) {
    const unsigned long long e = *a.epoch, last = (unsigned long long)(a.log_cap - 1);
    a.cost_log[(long long)(e < last ? e : last) * D + dv] = acc;
  }
}

struct CnnGeom {
  int L, C, F, NC, S;
  int SW;              // softmax lanes per sample
  int L1, L2, pl, ql;  // conv / pool output lengths, left pads
  int P;
};

// LDS floats of the CNN kernel: the model, two minibatches of samples and labels, and per sample
// pooled / argmax / d pooled, logits, the conv-gradient partial sums and the cost.
inline long long cnn_sgd_lds(const CnnGeom& d, int nb) {
  const long long LN = (long long)d.L2 * d.NC;
  return d.P + (long long)nb * (2LL * (d.L + d.C) + 3 * LN + d.C + (long long)d.F * d.NC + d.NC + 1);
}

// FT, ST as grad_cnn_kernel of cfa_grad.hip: the CFA-GE geometry unrolled, or runtime loops.
template <int FT, int ST>
__global__ __launch_bounds__(kGradBlock) void local_sgd_cnn_kernel(SgdArgs a, CnnGeom d) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int nb = a.nb, LN = d.L2 * d.NC;
  const int nW1 = d.F * d.NC, nW2 = LN * d.C, nG1 = nW1 + d.NC;
  float* W1 = lds;                        // [F][NC]
  float* b1 = W1 + nW1;                   // [NC]
  float* W2 = b1 + d.NC;                  // [LN][C]
  float* b2 = W2 + nW2;                   // [C]
  float* xs0 = b2 + d.C;                  // [2][nb][L]
  float* ys0 = xs0 + 2 * nb * d.L;        // [2][nb][C]
  float* pooled = ys0 + 2 * nb * d.C;     // [nb][L2][NC]
  int* arg = reinterpret_cast<int*>(pooled + nb * LN);   // conv position of each window's max
  float* dfc = reinterpret_cast<float*>(arg + nb * LN);  // [nb][LN]
  float* zl = dfc + nb * LN;              // [nb][C]: logits, then d logits
  float* part = zl + nb * d.C;            // [nb][nG1]: per-sample conv-gradient sums
  float* cs = part + nb * nG1;            // [nb]: per-sample cost
  const int dv = blockIdx.x, D = gridDim.x;
  const int tid = threadIdx.x, T = blockDim.x;
  float* m = a.models + (long long)dv * a.pitch;
  const float* xd = a.x + (long long)dv * a.Ns * d.L;
  const float* yd = a.y + (long long)dv * a.Ns * d.C;
  const int nx = nb * d.L, ny = nb * d.C;
  const float invB = 1.0f / (float)nb;
  const float lr = a.lr;

  // the first minibatch and the model, all in flight together: one global round trip
  Prefetch pf;
  pf.load(xd, nx, yd, ny, tid, T);
  stage(W1, m, d.P, tid, T);
  pf.store(xs0, xd, nx, ys0, yd, ny, tid, T);
  __syncthreads();
  const bool taps_in_regs = d.F <= kMaxTaps && T % d.NC == 0;
  double acc = 0.0;
  for (int i = 0; i < a.steps; ++i) {
    const float* xs = xs0 + (i & 1) * nx;
    const float* ys = ys0 + (i & 1) * ny;
    // the next minibatch leaves global memory now and lands in the other buffer after the step
    const bool more = i + 1 < a.steps;
    const float* xn = xd + (long long)(more ? i + 1 : i) * a.bstride * d.L;
    const float* yn = yd + (long long)(more ? i + 1 : i) * a.bstride * d.C;
    pf.load(xn, more ? nx : 0, yn, more ? ny : 0, tid, T);
    // the conv taps of this thread's channel (T is a multiple of NC, so every item a thread takes
    // below has the same channel c = tid % NC), reloaded from the stepped W1
    float wreg[kMaxTaps];
    {
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
    // conv + bias + relu evaluated inside each pooling window; keep the max and its position
    for (int idx = tid; idx < nb * LN; idx += T) {
      const int b = idx / LN, r = idx % LN, q = r / d.NC, c = r % d.NC;
      const float* xb = xs + b * d.L;
      float best = -INFINITY;
      int barg = -1;
      bool done = false;
      if constexpr (FT > 0 && ST > 0) {
        // branch-free: samples outside [0, L) read as 0, positions outside [0, L1) never win
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
    __syncthreads();
    // logits: 8 lanes per (sample, class), strided partial sums, xor-shuffle reduction
    for (int idx = tid; idx < nb * d.C * 8; idx += T) {
      const int o = idx >> 3, lane = idx & 7;
      const int b = o / d.C, k = o % d.C;
      float z = 0.f;
      for (int j = lane; j < LN; j += 8) z = fmaf(pooled[b * LN + j], W2[j * d.C + k], z);
      z += __shfl_xor(z, 1, 8);
      z += __shfl_xor(z, 2, 8);
      z += __shfl_xor(z, 4, 8);
      if (lane == 0) zl[o] = z + b2[k];
    }
    __syncthreads();
    softmax_xent_cost(zl, ys, cs, nb, d.C, d.SW, invB, a.update != 0, tid, T);
    __syncthreads();
    if (tid == 0) add_cost(acc, cs, nb, a.steps);
    if (a.update) {
      // the gradient flowing into the pooled features, through the pre-update W2
      for (int idx = tid; idx < nb * LN; idx += T) {
        const int b = idx / LN, j = idx % LN;
        float s = 0.f;
        for (int k = 0; k < d.C; ++k) s = fmaf(zl[b * d.C + k], W2[j * d.C + k], s);
        dfc[idx] = pooled[idx] > 0.f ? s : 0.f;  // relu gradient at the window's max
      }
      __syncthreads();
      // the dense layer's step, each element by the thread that owns it
      for (int idx = tid; idx < nW2; idx += T) {
        const int j = idx / d.C, k = idx % d.C;
        float s = 0.f;
#pragma unroll 4
        for (int b = 0; b < nb; ++b) s = fmaf(pooled[b * LN + j], zl[b * d.C + k], s);
        W2[idx] = W2[idx] - lr * s;
      }
      for (int k = tid; k < d.C; k += T) {
        float s = 0.f;
        for (int b = 0; b < nb; ++b) s += zl[b * d.C + k];
        b2[k] = b2[k] - lr * s;
      }
      // conv gradients per (weight, sample): only each window's max position receives gradient
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
      __syncthreads();
      for (int e = tid; e < nG1; e += T) {  // W1 and b1 are contiguous: sum over the samples in order
        float s = 0.f;
        for (int b = 0; b < nb; ++b) s += part[b * nG1 + e];
        W1[e] = W1[e] - lr * s;
      }
    }
    pf.store(xs0 + ((i + 1) & 1) * nx, xn, more ? nx : 0, ys0 + ((i + 1) & 1) * ny, yn, more ? ny : 0, tid, T);
    __syncthreads();
  }
  if (a.update)
    for (int j = tid; j < d.P; j += T) m[j] = W1[j];
  if (tid == 0) put_cost(a, dv, D, acc);
}

constexpr int kSpan = 32;  // first-layer inputs per partial sum, as cfa_grad.hip

struct NnGeom {
  int L, H, C;
  int SW;  // softmax lanes per sample
  int G;   // ceil(L / kSpan) slices of the input dimension for the first layer's partial sums
  int P;
};

inline long long nn_sgd_lds(const NnGeom& d, int nb) {
  return d.P + (long long)nb * (2LL * (d.L + d.C) + 2LL * d.H + d.C + (long long)d.G * d.H + 1);
}

__global__ __launch_bounds__(kGradBlock) void local_sgd_2nn_kernel(SgdArgs a, NnGeom d) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int nb = a.nb, nW1 = d.L * d.H;
  float* W1 = lds;                     // [L][H]
  float* b1 = W1 + nW1;                // [H]
  float* W2 = b1 + d.H;                // [H][C]
  float* b2 = W2 + d.H * d.C;          // [C]
  float* xs0 = b2 + d.C;               // [2][nb][L]
  float* ys0 = xs0 + 2 * nb * d.L;     // [2][nb][C]
  float* act = ys0 + 2 * nb * d.C;     // [nb][H] relu(x W1 + b1)
  float* dz = act + nb * d.H;          // [nb][H]
  float* zl = dz + nb * d.H;           // [nb][C]
  float* zpart = zl + nb * d.C;        // [G][nb][H]
  float* cs = zpart + d.G * nb * d.H;  // [nb]
  const int dv = blockIdx.x, D = gridDim.x;
  const int tid = threadIdx.x, T = blockDim.x;
  float* m = a.models + (long long)dv * a.pitch;
  const float* xd = a.x + (long long)dv * a.Ns * d.L;
  const float* yd = a.y + (long long)dv * a.Ns * d.C;
  const int nx = nb * d.L, ny = nb * d.C;
  const float invB = 1.0f / (float)nb;
  const float lr = a.lr;

  Prefetch pf;
  pf.load(xd, nx, yd, ny, tid, T);
  stage(W1, m, d.P, tid, T);
  pf.store(xs0, xd, nx, ys0, yd, ny, tid, T);
  __syncthreads();
  double acc = 0.0;
  for (int i = 0; i < a.steps; ++i) {
    const float* xs = xs0 + (i & 1) * nx;
    const float* ys = ys0 + (i & 1) * ny;
    const bool more = i + 1 < a.steps;
    const float* xn = xd + (long long)(more ? i + 1 : i) * a.bstride * d.L;
    const float* yn = yd + (long long)(more ? i + 1 : i) * a.bstride * d.C;
    pf.load(xn, more ? nx : 0, yn, more ? ny : 0, tid, T);
    // first layer as G partial sums over kSpan-wide slices of the input dimension; a (slice, h)
    // pair's weights are read once and serve every sample
    for (int idx = tid; idx < d.G * d.H; idx += T) {
      const int h = idx % d.H, grp = idx / d.H, i0 = grp * kSpan, n = min(kSpan, d.L - i0);
      float w[kSpan];
#pragma unroll
      for (int u = 0; u < kSpan; ++u) w[u] = W1[(i0 + (u < n ? u : 0)) * d.H + h];
      for (int b = 0; b < nb; ++b) {
        const float* xb = xs + b * d.L + i0;
        float z = 0.f;
#pragma unroll
        for (int u = 0; u < kSpan; ++u)
          if (u < n) z = fmaf(xb[u], w[u], z);
        zpart[(grp * nb + b) * d.H + h] = z;
      }
    }
    __syncthreads();
    for (int idx = tid; idx < nb * d.H; idx += T) {
      const int b = idx / d.H, h = idx % d.H;
      float z = 0.f;
      for (int grp = 0; grp < d.G; ++grp) z += zpart[(grp * nb + b) * d.H + h];
      z += b1[h];
      act[idx] = z > 0.f ? z : 0.f;
    }
    __syncthreads();
    for (int idx = tid; idx < nb * d.C; idx += T) {
      const int b = idx / d.C, k = idx % d.C;
      float z = 0.f;
      for (int h = 0; h < d.H; ++h) z = fmaf(act[b * d.H + h], W2[h * d.C + k], z);
      zl[idx] = z + b2[k];
    }
    __syncthreads();
    softmax_xent_cost(zl, ys, cs, nb, d.C, d.SW, invB, a.update != 0, tid, T);
    __syncthreads();
    if (tid == 0) add_cost(acc, cs, nb, a.steps);
    if (a.update) {
      // the hidden layer's gradient, through the pre-update W2
      for (int idx = tid; idx < nb * d.H; idx += T) {
        const int b = idx / d.H, h = idx % d.H;
        float s = 0.f;
        for (int k = 0; k < d.C; ++k) s = fmaf(zl[b * d.C + k], W2[h * d.C + k], s);
        dz[idx] = act[idx] > 0.f ? s : 0.f;
      }
      __syncthreads();
      // every parameter's step by the thread that owns it
      for (int idx = tid; idx < d.H * d.C; idx += T) {
        const int h = idx / d.C, k = idx % d.C;
        float s = 0.f;
        for (int b = 0; b < nb; ++b) s = fmaf(act[b * d.H + h], zl[b * d.C + k], s);
        W2[idx] = W2[idx] - lr * s;
      }
      for (int k = tid; k < d.C; k += T) {
        float s = 0.f;
        for (int b = 0; b < nb; ++b) s += zl[b * d.C + k];
        b2[k] = b2[k] - lr * s;
      }
      for (int idx = tid; idx < nW1; idx += T) {  // W1 -= lr * x^T dz
        const int j = idx / d.H, h = idx % d.H;
        float s = 0.f;
#pragma unroll 4
        for (int b = 0; b < nb; ++b) s = fmaf(xs[b * d.L + j], dz[b * d.H + h], s);
        W1[idx] = W1[idx] - lr * s;
      }
      for (int h = tid; h < d.H; h += T) {
        float s = 0.f;
        for (int b = 0; b < nb; ++b) s += dz[b * d.H + h];
        b1[h] = b1[h] - lr * s;
      }
    }
    pf.store(xs0 + ((i + 1) & 1) * nx, xn, more ? nx : 0, ys0 + ((i + 1) & 1) * ny, yn, more ? ny : 0, tid, T);
    __syncthreads();
  }
  if (a.update)
    for (int j = tid; j < d.P; j += T) m[j] = W1[j];
  if (tid == 0) put_cost(a, dv, D, acc);
}

// The arguments every entry shares, checked before any device work.
int sgd_args(const char* fn, const float* x, const float* y, int Ns, float* models, size_t pitch, int D,
             int batch_stride, int batch_rows, int steps, float lr, int update, double* cost, double* cost_log,
             int log_cap, unsigned long long* epoch, long long P, SgdArgs& a) {
  if (D < 0 || Ns < 1) return fail(CFA_E_INVALID, "%s: bad dimensions (D %d Ns %d)", fn, D, Ns);
  if (steps < 1 || batch_rows < 1 || batch_stride < 1)
    return fail(CFA_E_INVALID, "%s: steps %d, batch_rows %d and batch_stride %d must be >= 1", fn, steps,
                batch_rows, batch_stride);
  if ((long long)(steps - 1) * batch_stride + batch_rows > Ns)
    return fail(CFA_E_INVALID, "%s: minibatch %d ends at row %lld of %d", fn, steps - 1,
                (long long)(steps - 1) * batch_stride + batch_rows, Ns);
  if ((long long)pitch < P) return fail(CFA_E_INVALID, "%s: pitch %zu below the model's %lld parameters", fn, pitch, P);
  // an empty population has no buffers: D == 0 returns before anything is read
  if (D > 0 && (!x || !y || !models)) return fail(CFA_E_INVALID, "%s: null buffer", fn);
  if ((cost_log == nullptr) != (epoch == nullptr))
    return fail(CFA_E_INVALID, "%s: cost_log and epoch are given together or not at all", fn);
  if (cost_log && log_cap < 1) return fail(CFA_E_INVALID, "%s: log_cap %d must be >= 1", fn, log_cap);
  a = SgdArgs{x, y, models, (long long)pitch, Ns, batch_stride, batch_rows, steps, lr, update != 0, cost, cost_log,
              log_cap, epoch};
  return CFA_OK;
}

// LDS of a launch: within the default 64 KiB, or the kernel's limit raised to the device's.
int sgd_lds(const char* fn, const void* kern, long long floats, size_t& bytes) {
  const long long need = 4 * floats, limit = device_lds_max();
  if (need > limit || (need > 65536 && !raise_lds_limit(kern, (int)limit)))
    return fail(CFA_E_UNSUPPORTED, "%s: model, two minibatches and activations need %lld bytes of LDS", fn, need);
  bytes = (size_t)need;
  return CFA_OK;
}

// After the launch: the cost log's epoch counter one higher, in stream order.
int sgd_finish(const char* what, const SgdArgs& a, unsigned long long* epoch, hipStream_t st) {
  if (int rc = check_launch(what)) return rc;
  return a.cost_log ? advance_counter(epoch, st) : CFA_OK;
}

}  // namespace

// Current device: raise every local-SGD kernel's dynamic-LDS limit now (cfa_device_prepare), so
// later launches (e.g. under hipGraph capture) need no attribute call.
int local_sgd_prepare_device() {
  const int lim = device_lds_max();
  if (lim <= 65536) return CFA_OK;
  const void* kernels[] = {(const void*)local_sgd_cnn_kernel<16, 5>, (const void*)local_sgd_cnn_kernel<0, 0>,
                           (const void*)local_sgd_2nn_kernel};
  for (const void* k : kernels) (void)raise_lds_limit(k, lim);  // refused: launches stay within 64 KiB
  return CFA_OK;
}

extern "C" int cfa_local_sgd_cnn_f32(const float* x, const float* y, int Ns, int L, int classes, int filter,
                                     int number, int stride, float* models, size_t pitch, int D,
                                     int batch_stride, int batch_rows, int steps, float lr, int update,
                                     double* cost, double* cost_log, int log_cap, unsigned long long* epoch,
                                     void* stream) {
  const char* fn = "cfa_local_sgd_cnn_f32";
  if (L < 1 || classes < 1 || filter < 1 || number < 1 || stride < 1)
    return fail(CFA_E_INVALID, "%s: bad dimensions (L %d C %d F %d NC %d S %d)", fn, L, classes, filter, number,
                stride);
  CnnGeom d;
  d.L = L, d.C = classes, d.F = filter, d.NC = number, d.S = stride;
  d.L1 = (L + stride - 1) / stride;
  d.L2 = (d.L1 + stride - 1) / stride;
  d.pl = same_left(L, filter, stride);
  d.ql = same_left(d.L1, stride, stride);
  const long long P = (long long)filter * number + number + (long long)d.L2 * number * classes + classes;
  SgdArgs a;
  if (int rc = sgd_args(fn, x, y, Ns, models, pitch, D, batch_stride, batch_rows, steps, lr, update, cost, cost_log,
                        log_cap, epoch, P, a))
    return rc;
  if (D == 0) return CFA_OK;
  if (classes > 64) return fail(CFA_E_UNSUPPORTED, "%s: more than 64 classes", fn);
  if (P > (1 << 20)) return fail(CFA_E_UNSUPPORTED, "%s: a model of %lld parameters does not fit the LDS", fn, P);
  d.P = (int)P;
  d.SW = softmax_width(classes);
  const bool fast = filter == 16 && stride == 5;  // the CFA-GE CNN's geometry: the unrolled kernel
  const void* kern = fast ? (const void*)local_sgd_cnn_kernel<16, 5> : (const void*)local_sgd_cnn_kernel<0, 0>;
  size_t bytes = 0;
  if (int rc = sgd_lds(fn, kern, cnn_sgd_lds(d, batch_rows), bytes)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (fast)
    local_sgd_cnn_kernel<16, 5><<<(unsigned)D, kGradBlock, bytes, st>>>(a, d);
  else
    local_sgd_cnn_kernel<0, 0><<<(unsigned)D, kGradBlock, bytes, st>>>(a, d);
  return sgd_finish("local_sgd_cnn_kernel", a, epoch, st);
}

extern "C" int cfa_local_sgd_2nn_f32(const float* x, const float* y, int Ns, int L, int hidden, int classes,
                                     float* models, size_t pitch, int D, int batch_stride, int batch_rows,
                                     int steps, float lr, int update, double* cost, double* cost_log,
                                     int log_cap, unsigned long long* epoch, void* stream) {
  const char* fn = "cfa_local_sgd_2nn_f32";
  if (L < 1 || hidden < 1 || classes < 1)
    return fail(CFA_E_INVALID, "%s: bad dimensions (L %d H %d C %d)", fn, L, hidden, classes);
  NnGeom d;
  d.L = L, d.H = hidden, d.C = classes;
  d.G = (L + kSpan - 1) / kSpan;
  const long long P = (long long)L * hidden + hidden + (long long)hidden * classes + classes;
  SgdArgs a;
  if (int rc = sgd_args(fn, x, y, Ns, models, pitch, D, batch_stride, batch_rows, steps, lr, update, cost, cost_log,
                        log_cap, epoch, P, a))
    return rc;
  if (D == 0) return CFA_OK;
  if (classes > 64) return fail(CFA_E_UNSUPPORTED, "%s: more than 64 classes", fn);
  if (P > (1 << 20)) return fail(CFA_E_UNSUPPORTED, "%s: a model of %lld parameters does not fit the LDS", fn, P);
  d.P = (int)P;
  d.SW = softmax_width(classes);
  size_t bytes = 0;
  if (int rc = sgd_lds(fn, (const void*)local_sgd_2nn_kernel, nn_sgd_lds(d, batch_rows), bytes)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  local_sgd_2nn_kernel<<<(unsigned)D, kGradBlock, bytes, st>>>(a, d);
  return sgd_finish("local_sgd_2nn_kernel", a, epoch, st);
}

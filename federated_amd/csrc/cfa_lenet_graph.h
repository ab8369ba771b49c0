// cfa_lenet_graph.h — the forward and backward pass of the TF2 drivers' "LeNet-1 family"
// (create_q_model, condition 0,
// federated_learning_keras_consensus_FL_threads_MNIST_crossentropy_gradients_exchange.py:158-194),
// written once as phases for the kernels that evaluate it (cfa_lenet.hip: the validation cost;
// cfa_lenet_grad.hip: a minibatch's gradient on the same forward phases), and the family's geometry
// on the host.
//   x [side, side, 1] -> Conv2D(c1, k x k, valid) + b1 -> relu -> AveragePooling2D(2 x 2, stride 2)
//     -> Conv2D(c2, k x k, valid) + b2 -> relu -> AveragePooling2D(2 x 2) -> Flatten -> Dense(classes)
//   loss = -log softmax(z)[label], evaluated as -(z_l - max - log(sum exp(z - max))), or the Huber
//   drivers' Huber(label, softmax(z)[label]) (lenet_huber); a kernel is instantiated for one of the two (lenet_loss)
// Keras conventions kept: Conv2D is a cross-correlation with the kernel tensor (kh, kw, in, out);
// activations are NHWC, so Flatten gives index (h * w + x) * c2 + c; "valid" pooling drops an odd
// last row and column. A model row is get_weights() order, C-order: K1 b1 K2 b2 Wd bd.
//
// The reference takes log of the softmax output (:442). The two forms agree to rounding wherever
// no class probability underflows in fp32; where one does the reference yields inf / nan and
// this form a finite cost (a deliberate difference: the cost stays comparable to a target).
//
// A phase is a __device__ __forceinline__ function over LDS pointers that every thread of the
// workgroup calls (tid of T); the caller puts the barriers between phases. Every sample's
// arithmetic is its own and every sum has a fixed order, so a sample's loss does not depend on
// which chunk, workgroup or device evaluates it. fp32 throughout. Not installed, not an ABI.
//
// Backward (per sample; the 1 / batch factor belongs to the caller's finishing step):
//   dz[c] = exp(z_c - max) / sum - (c == l), with the forward's own max and sum (lenet_huber: its own)
//   dWd[i][c] = flat[i] dz[c], dbd[c] = dz[c], dflat[i] = sum_c Wd[i][c] dz[c]
//   pool: each of a window's four positions receives 0.25 d(pooled); a dropped row or column none
//   relu: the forward's own test z > 0 (z == 0 passes nothing, as TF's ReluGrad)
//   conv: dK[ky][kx][ci][co] = sum_{y,x} in[y+ky][x+kx][ci] dzc[y][x][co], db[co] = sum_{y,x} dzc[y][x][co],
//         stage 2 also din[y][x][ci] = sum over the taps that reach (y, x) of K[ky][kx][ci][co] dzc[y-ky][x-kx][co]
// The gates are STORED, as bits: the forward phase's optional output is one byte per pooled
// element whose bit 2 dy + dx is the test of window position (dy, dx), so a gate costs a quarter
// of a byte where a float mask would cost four. A gated gradient is (bit ? 0.25 : 0) * d(pooled)
// (LenetGated), a product, so that a NaN upstream (a label out of range) reaches every element.
// Stage 2's is written out once (it is read k * k * c1 times by the input gradient), stage 1's
// is formed where it is read. LDS of the gradient kernel, in floats, for a chunk of n samples and a
// group of g: 2 P (model, gradient sums) + n (side^2 + 2 p1^2 c1 + 2 flat + 2 C + 4 p2^2 c2) + g + n
// + ceil(n (p1^2 c1 + flat) / 4) (lenet_grad_lds in cfa_lenet_grad.hip; LeNet-1 at n = 2, g = 4: 39.9 KiB).
// A weight gradient is summed in a fixed order: the rows (sample, y) of a chunk are dealt to L
// lanes (L a power of two from the geometry alone), each lane sums its rows in order, x in order,
// from 0, the lanes are folded by xor-shuffles, and the chunk's sum is added to the running one.
#pragma once
#include "cfa_grad_common.h"

namespace {

// ---- geometry (host) ----------------------------------------------------------------------

// One geometry for every kernel of the family. With an input of `cin` channels and a hidden dense
// layer (cfa_lenet_hidden.hip: the CIFAR drivers' -modelselection 1) the graph is
//   x [side, side, cin] -> Conv2D(c1) -> relu -> pool -> Conv2D(c2) -> relu -> pool
//     -> Flatten -> Dense(H, relu) -> Dense(classes)
// and a model row K1 (k, k, cin, c1) b1 K2 (k, k, c1, c2) b2 Wh (flat, H) bh Wd (H, classes) bd.
// Without a hidden layer H = 0, Wh and bh are empty (oWh = obh = oWd) and Wd is (flat, classes).
struct LenetGeom {
  int side, cin, k, c1, c2, H, C;
  int s1, p1, s2, p2;  // conv / pool output sides of the two stages
  int flat;            // p2 * p2 * c2
  int oK1, ob1, oK2, ob2, oWh, obh, oWd, obd;  // offsets of the tensors in a model row
  long long P;
};

// The geometry from the caller's seven numbers; with_hidden: whether the family has a hidden layer
// (`hidden` counts only then). false for a geometry that has no model: a dimension < 1 (hidden
// included where there is one), a kernel larger than its input, an empty pooled map. Offsets are
// valid only while P fits an int; a kernel's entry refuses a model that large before any launch.
inline bool lenet_geom(int side, int channels, int kernel, int c1, int c2, int hidden, int classes, bool with_hidden,
                       LenetGeom& g) {
  if (side < 1 || channels < 1 || kernel < 1 || c1 < 1 || c2 < 1 || (with_hidden && hidden < 1) || classes < 1)
    return false;
  g.side = side, g.cin = channels, g.k = kernel, g.c1 = c1, g.c2 = c2, g.H = with_hidden ? hidden : 0, g.C = classes;
  g.s1 = side - kernel + 1;
  g.p1 = g.s1 > 0 ? g.s1 / 2 : 0;
  g.s2 = g.p1 - kernel + 1;
  g.p2 = g.s2 > 0 ? g.s2 / 2 : 0;
  if (g.p2 < 1) return false;
  const long long kk = (long long)kernel * kernel, flat = (long long)g.p2 * g.p2 * c2;
  const long long nK1 = kk * channels * c1, nK2 = kk * c1 * c2, nWh = flat * g.H;
  const long long nWd = (with_hidden ? (long long)g.H : flat) * classes;
  g.P = nK1 + c1 + nK2 + c2 + nWh + g.H + nWd + classes;
  if (g.P > 0x7fffffffLL) {
    g.flat = g.oK1 = g.ob1 = g.oK2 = g.ob2 = g.oWh = g.obh = g.oWd = g.obd = 0;
    return true;
  }
  g.flat = (int)flat;
  g.oK1 = 0;
  g.ob1 = (int)nK1;
  g.oK2 = g.ob1 + c1;
  g.ob2 = g.oK2 + (int)nK2;
  g.oWh = g.ob2 + c2;
  g.obh = g.oWh + (int)nWh;
  g.oWd = g.obh + g.H;
  g.obd = g.oWd + (int)nWd;
  return true;
}

// The five-number spelling: one channel, no hidden layer.
inline bool lenet_geom(int side, int kernel, int c1, int c2, int classes, LenetGeom& g) {
  return lenet_geom(side, 1, kernel, c1, c2, 0, classes, false, g);
}

// LDS floats one sample's forward pass needs: the image, the two pooled maps, h and the logits.
inline long long lenet_sample_floats(const LenetGeom& g) {
  return (long long)g.side * g.side * g.cin + (long long)g.p1 * g.p1 * g.c1 + g.flat + g.H + g.C;
}

// The hidden layer's forward plan for a workgroup of T threads, from H and T alone: a pass covers
// W = min(H, T) neighbouring columns j, and S slices (a power of two, at most 16, S W <= T) share
// a column's sum over i, slice q taking i = q, q + S, ...
__host__ __device__ inline int lenet_hidden_cols(int H, int T) { return H < T ? H : T; }
__host__ __device__ inline int lenet_hidden_slices(int H, int T) {
  const int W = lenet_hidden_cols(H, T);
  int S = 1;
  while (S < 16 && 2 * S * W <= T) S *= 2;
  return S;
}
// LDS floats of lenet_hidden_forward's partial sums for a chunk of n samples.
inline long long lenet_hidden_part_floats(int H, int T, int n) {
  return (long long)lenet_hidden_slices(H, T) * n * lenet_hidden_cols(H, T);
}

// ---- phases ---------------------------------------------------------------------------------

// AveragePooling2D of a window's relu(z): summed (0,0) (0,1) (1,0) (1,1) and scaled by 0.25 (exact);
// bits: bit 2 dy + dx is the test z > 0 of window position (dy, dx).
struct LenetAvgPool {
  static __device__ __forceinline__ float pool(float z00, float z01, float z10, float z11, uint8_t& bits) {
    const float h00 = z00 > 0.f ? z00 : 0.f, h01 = z01 > 0.f ? z01 : 0.f;
    const float h10 = z10 > 0.f ? z10 : 0.f, h11 = z11 > 0.f ? z11 : 0.f;
    bits = (uint8_t)((z00 > 0.f ? 1 : 0) | (z01 > 0.f ? 2 : 0) | (z10 > 0.f ? 4 : 0) | (z11 > 0.f ? 8 : 0));
    return (((h00 + h01) + h10) + h11) * 0.25f;
  }
};

// MaxPooling2D of a window's relu(z), and the decision TF's MaxPoolGrad takes again: the FIRST
// largest relu(z) in window order (0,0) (0,1) (1,0) (1,1) (a later position wins only where it is
// strictly larger). bits: the position 2 dy + dx in bits 0-1 and its test z > 0 in bit 2; a
// window without a positive z keeps position 0 with the test clear, so it passes nothing.
struct LenetMaxPool {
  static __device__ __forceinline__ float pool(float z00, float z01, float z10, float z11, uint8_t& bits) {
    const float h00 = z00 > 0.f ? z00 : 0.f, h01 = z01 > 0.f ? z01 : 0.f;
    const float h10 = z10 > 0.f ? z10 : 0.f, h11 = z11 > 0.f ? z11 : 0.f;
    float m = h00;
    int at = 0;
    if (h01 > m) m = h01, at = 1;
    if (h10 > m) m = h10, at = 2;
    if (h11 > m) m = h11, at = 3;
    bits = (uint8_t)(at | (m > 0.f ? 4 : 0));
    return m;
  }
};

// One stage of the family for ns samples: out[s][py][px][co] = mean over the 2 x 2 window of
// relu(conv(in)[2py + dy][2px + dx][co] + b[co]), in [ns][sin][sin][cin] and out
// [ns][pout][pout][cout] both NHWC, W (k, k, cin, cout). The four convolutions of a window run
// side by side from one weight load per tap; each sums its taps in (ci, ky, kx) order from 0 and
// adds the bias last, and the window is summed (0,0) (0,1) (1,0) (1,1) and scaled by 0.25 (exact).
// K > 0: the kernel side at compile time (the tap loops unroll, and the window's (K + 1)^2 inputs
// are loaded once); K = 0: any side. The arithmetic and its order are the same either way.
// gate (or null): [ns][pout][pout][cout] bytes, bit 2 dy + dx set where z[2py + dy][2px + dx] > 0.
// Pool: what a window's four pre-activations become (LenetAvgPool above, or LenetMaxPool, whose
// pooled value is the window's largest relu(z) and whose byte is LenetMaxGated's); everything up
// to the bias is the same code for both.
template <int K, class Pool = LenetAvgPool>
__device__ __forceinline__ void lenet_conv_pool(float* __restrict__ out, const float* __restrict__ in,
                                                const float* __restrict__ W, const float* __restrict__ b, int ns,
                                                int sin, int cin, int cout, int kside, int pout, int tid, int T,
                                                uint8_t* __restrict__ gate = nullptr) {
  const int k = K > 0 ? K : kside;
  const int per = pout * pout * cout, row = sin * cin;
  for (int idx = tid; idx < ns * per; idx += T) {
    const int s = idx / per, r = idx % per;
    const int co = r % cout, px = (r / cout) % pout, py = r / (cout * pout);
    const float* base = in + (s * sin + 2 * py) * row + 2 * px * cin;
    float z00 = 0.f, z01 = 0.f, z10 = 0.f, z11 = 0.f;
    const auto tap = [&](int ky, int kx, int ci) {
      const float w = W[((ky * k + kx) * cin + ci) * cout + co];
      const float* p = base + ky * row + kx * cin + ci;
      z00 = fmaf(p[0], w, z00);
      z01 = fmaf(p[cin], w, z01);
      z10 = fmaf(p[row], w, z10);
      z11 = fmaf(p[row + cin], w, z11);
    };
    for (int ci = 0; ci < cin; ++ci) {
      if constexpr (K > 0) {
#pragma unroll
        for (int ky = 0; ky < K; ++ky)
#pragma unroll
          for (int kx = 0; kx < K; ++kx) tap(ky, kx, ci);
      } else {
        for (int ky = 0; ky < k; ++ky)
          for (int kx = 0; kx < k; ++kx) tap(ky, kx, ci);
      }
    }
    const float bias = b[co];
    z00 += bias, z01 += bias, z10 += bias, z11 += bias;
    uint8_t bits;
    out[idx] = Pool::pool(z00, z01, z10, z11, bits);
    if (gate) gate[idx] = bits;
  }
}

// logits zl[ns][C] = flat Wd + bd: 8 lanes per (sample, class), strided partial sums, xor-shuffle
// reduction (T is a multiple of 8, so a group of 8 items is 8 neighbouring lanes of one wave).
__device__ __forceinline__ void lenet_logits(float* zl, const float* flat, const float* Wd, const float* bd, int ns,
                                             int F, int C, int tid, int T) {
  for (int idx = tid; idx < ns * C * 8; idx += T) {
    const int o = idx >> 3, lane = idx & 7;
    const int s = o / C, c = o % C;
    float z = 0.f;
    for (int i = lane; i < F; i += 8) z = fmaf(flat[s * F + i], Wd[i * C + c], z);
    z += __shfl_xor(z, 1, 8);
    z += __shfl_xor(z, 2, 8);
    z += __shfl_xor(z, 4, 8);
    if (lane == 0) zl[o] = z + bd[c];
  }
}

// loss[s] = -(z_l - max - log(sum_c exp(z_c - max))) for sample s's label l, one thread per
// sample, classes in order. A label outside [0, C) reads nothing and gives NaN. dz (or null):
// [ns][C], the loss's gradient at the logits, exp(z_c - max) / sum - (c == l); all NaN for such a label.
__device__ __forceinline__ void lenet_xent(float* loss, const float* zl, const int32_t* labels, int ns, int C,
                                           int tid, int T, float* dz = nullptr) {
  for (int s = tid; s < ns; s += T) {
    const float* z = zl + s * C;
    float mx = z[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, z[c]);
    float sum = 0.f;
    for (int c = 0; c < C; ++c) sum += expf(z[c] - mx);
    const int l = labels[s];
    loss[s] = (unsigned)l < (unsigned)C ? -((z[l] - mx) - logf(sum)) : NAN;
    if (dz) {
      const bool ok = (unsigned)l < (unsigned)C;
      for (int c = 0; c < C; ++c) dz[s * C + c] = ok ? expf(z[c] - mx) / sum - (c == l ? 1.f : 0.f) : NAN;
    }
  }
}

// The Huber drivers' objective (federated_learning_keras_consensus_FL_MNIST.py:369-377, validation
// :481-483): keras.losses.Huber() (delta = 1) between the integer label itself, cast to float, and
// the softmax probability of the true class. loss[s] = 0.5 e^2 where |e| <= 1, else |e| - 0.5, with
// e = p - (float)l and p = exp(z_l - max) / sum, lenet_xent's own max, sum and quotient. Same
// shape: one thread per sample, classes in order; a label outside [0, C) reads nothing and gives
// NaN. dz (or null): [ns][C], (g p) ((c == l) - exp(z_c - max) / sum) with g = e on the quadratic
// branch and sign(e) on the linear one; all NaN for such a label. With 0 < p < 1 the label alone
// picks the branch (0: quadratic in p; 1: quadratic in 1 - p; 2 and above: linear); where p
// rounds to exactly 0 or 1 in fp32, e of label 0 or 2 lands on a branch's edge, and <= keeps the
// quadratic branch there, as Keras does.
__device__ __forceinline__ void lenet_huber(float* loss, const float* zl, const int32_t* labels, int ns, int C,
                                            int tid, int T, float* dz = nullptr) {
  for (int s = tid; s < ns; s += T) {
    const float* z = zl + s * C;
    float mx = z[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, z[c]);
    float sum = 0.f;
    for (int c = 0; c < C; ++c) sum += expf(z[c] - mx);
    const int l = labels[s];
    const bool ok = (unsigned)l < (unsigned)C;
    const float p = ok ? expf(z[l] - mx) / sum : NAN;
    const float e = p - (float)l, ae = fabsf(e);
    const bool quad = ae <= 1.f;  // false for NaN: the linear branch keeps it NaN
    loss[s] = quad ? 0.5f * e * e : ae - 0.5f;
    if (dz) {
      const float gp = (quad ? e : e > 0.f ? 1.f : -1.f) * p;
      for (int c = 0; c < C; ++c) dz[s * C + c] = ok ? gp * ((c == l ? 1.f : 0.f) - expf(z[c] - mx) / sum) : NAN;
    }
  }
}

// The loss phase of a kernel instantiated for the objective LOSS (CFA_LENET_LOSS_XENT or
// CFA_LENET_LOSS_HUBER; the entry points refuse any other): the cross-entropy kernels hold
// lenet_xent alone, as they did before there was a second objective.
template <int LOSS>
__device__ __forceinline__ void lenet_loss(float* loss, const float* zl, const int32_t* labels, int ns, int C,
                                           int tid, int T, float* dz = nullptr) {
  if constexpr (LOSS == CFA_LENET_LOSS_HUBER)
    lenet_huber(loss, zl, labels, ns, C, tid, T, dz);
  else
    lenet_xent(loss, zl, labels, ns, C, tid, T, dz);
}

// ---- backward phases --------------------------------------------------------------------------

// The dense layer's backward for ns samples: gWd[i][c] += sum_s flat[s][i] dz[s][c] and
// gbd[c] += sum_s dz[s][c] (one thread per element, samples in order, onto the running sum), and
// dflat[s][i] = sum_c Wd[i][c] dz[s][c], classes in order from 0.
__device__ __forceinline__ void lenet_dense_backward(float* gWd, float* gbd, float* dflat, const float* flat,
                                                     const float* dz, const float* Wd, int ns, int F, int C, int tid,
                                                     int T) {
  for (int e = tid; e < F * C; e += T) {
    const int i = e / C, c = e % C;
    float a = gWd[e];
    for (int s = 0; s < ns; ++s) a = fmaf(flat[s * F + i], dz[s * C + c], a);
    gWd[e] = a;
  }
  for (int c = tid; c < C; c += T) {
    float a = gbd[c];
    for (int s = 0; s < ns; ++s) a += dz[s * C + c];
    gbd[c] = a;
  }
  for (int idx = tid; idx < ns * F; idx += T) {
    const int s = idx / F, i = idx % F;
    float a = 0.f;
    for (int c = 0; c < C; ++c) a = fmaf(Wd[i * C + c], dz[s * C + c], a);
    dflat[idx] = a;
  }
}

// dzc[s][y][x][co] of a stage, y and x below 2 pout (what the pool kept), from the stage's gate
// bytes and the gradient dp [ns][pout][pout][cout] of its pooled map.
struct LenetGated {
  const uint8_t* gate;
  const float* dp;
  int pout, cout;
  __device__ __forceinline__ float operator()(int s, int y, int x, int co) const {
    const int i = ((s * pout + (y >> 1)) * pout + (x >> 1)) * cout + co;
    return ((gate[i] >> (2 * (y & 1) + (x & 1))) & 1 ? 0.25f : 0.f) * dp[i];
  }
};

// The max pool's: the whole of d(pooled) to the window's selected position where its z > 0, as a
// product with 1 or 0 (a NaN upstream reaches every element); gate holds LenetMaxPool's bytes.
struct LenetMaxGated {
  const uint8_t* gate;
  const float* dp;
  int pout, cout;
  __device__ __forceinline__ float operator()(int s, int y, int x, int co) const {
    const int i = ((s * pout + (y >> 1)) * pout + (x >> 1)) * cout + co;
    const int b = gate[i];
    return ((b >> 2) & 1 && (b & 3) == 2 * (y & 1) + (x & 1) ? 1.f : 0.f) * dp[i];
  }
};

// The same values written out: v [ns][side][side][cout], side = 2 pout.
struct LenetStored {
  const float* v;
  int side, cout;
  __device__ __forceinline__ float operator()(int s, int y, int x, int co) const {
    return v[((s * side + y) * side + x) * cout + co];
  }
};

template <class Gated>
__device__ __forceinline__ void lenet_store_gated(float* v, const Gated& g, int ns, int tid, int T) {
  const int side = 2 * g.pout;
  for (int idx = tid; idx < ns * side * side * g.cout; idx += T) {
    const int co = idx % g.cout, x = (idx / g.cout) % side, y = (idx / (g.cout * side)) % side;
    v[idx] = g(idx / (g.cout * side * side), y, x, co);
  }
}

// Lanes that share one sum of `items` sums among T threads: the largest power of two L <= 64
// with items * L <= T (1 when there are more sums than threads). T is a multiple of 64, so the L
// lanes of a sum are neighbours in one wave.
__device__ __forceinline__ int lenet_lanes(int items, int T) {
  int L = 1;
  while (L < 64 && 2 * L * items <= T) L *= 2;
  return L;
}

__device__ __forceinline__ float lenet_fold(float v, int L) {
  for (int m = 1; m < L; m <<= 1) v += __shfl_xor(v, m, L);
  return v;
}

// gK[ky][kx][ci][co] += sum_{s,y,x} in[s][y+ky][x+kx][ci] dz(s, y, x, co) over the chunk's ns
// samples, in [ns][sin][sin][cin]. An item is (ky, ci, co) with all its kx; its rows (s, y) are
// dealt to L lanes, row r to lane r % L. K > 0: the k inputs under a row's taps slide through
// registers (one input and one dz read per x for k multiply-adds); K = 0: any side, one sum at
// a time. Every sum runs over its lane's rows in order and x in order from 0, either way.
template <int K, class Dz>
__device__ __forceinline__ void lenet_conv_wgrad(float* gK, const float* in, const Dz& dz, int ns, int sin, int cin,
                                                 int cout, int kside, int pout, int tid, int T) {
  const int k = K > 0 ? K : kside;
  const int items = k * cin * cout, L = lenet_lanes(items, T);
  const int side = 2 * pout, rows = ns * side;
  for (int idx = tid; idx < items * L; idx += T) {
    const int it = idx / L, lane = idx % L;
    const int co = it % cout, ci = (it / cout) % cin, ky = it / (cout * cin);
    float* out = gK + (ky * k * cin + ci) * cout + co;  // + kx * cin * cout
    if constexpr (K > 0) {
      float acc[K];
#pragma unroll
      for (int j = 0; j < K; ++j) acc[j] = 0.f;
      for (int r = lane; r < rows; r += L) {
        const int s = r / side, y = r % side;
        const float* p = in + ((s * sin + y + ky) * sin) * cin + ci;
        float w[K];  // w[j] = in[.][x + j][ci] once x's input has been shifted in
#pragma unroll
        for (int j = 1; j < K; ++j) w[j] = p[(j - 1) * cin];
        for (int x = 0; x < side; ++x) {
#pragma unroll
          for (int j = 0; j + 1 < K; ++j) w[j] = w[j + 1];
          w[K - 1] = p[(x + K - 1) * cin];
          const float d = dz(s, y, x, co);
#pragma unroll
          for (int j = 0; j < K; ++j) acc[j] = fmaf(w[j], d, acc[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const float v = lenet_fold(acc[j], L);
        if (lane == 0) out[j * cin * cout] += v;
      }
    } else {
      for (int kx = 0; kx < k; ++kx) {
        float acc = 0.f;
        for (int r = lane; r < rows; r += L) {
          const int s = r / side, y = r % side;
          const float* p = in + ((s * sin + y + ky) * sin + kx) * cin + ci;
          for (int x = 0; x < side; ++x) acc = fmaf(p[x * cin], dz(s, y, x, co), acc);
        }
        const float v = lenet_fold(acc, L);
        if (lane == 0) out[kx * cin * cout] += v;
      }
    }
  }
}

// gb[co] += sum_{s,y,x} dz(s, y, x, co): the chunk's ns * (2 pout)^2 terms of a channel dealt to
// L lanes, term t to lane t % L, each lane in order from 0.
template <class Dz>
__device__ __forceinline__ void lenet_conv_bgrad(float* gb, const Dz& dz, int ns, int cout, int pout, int tid, int T) {
  const int L = lenet_lanes(cout, T), side = 2 * pout, terms = ns * side * side;
  for (int idx = tid; idx < cout * L; idx += T) {
    const int co = idx / L, lane = idx % L;
    float acc = 0.f;
    for (int t = lane; t < terms; t += L) acc += dz(t / (side * side), (t / side) % side, t % side, co);
    const float v = lenet_fold(acc, L);
    if (lane == 0) gb[co] += v;
  }
}

// din[s][y][x][ci] = sum over the taps (ky, kx) with y - ky and x - kx in [0, 2 pout), in order,
// and co in order, of W[ky][kx][ci][co] dzc[s][y-ky][x-kx][co]; din [ns][sin][sin][cin], dzc
// [ns][2 pout][2 pout][cout]. An input no kept output reads receives 0.
__device__ __forceinline__ void lenet_conv_igrad(float* din, const float* dzc, const float* W, int ns, int sin,
                                                 int cin, int cout, int k, int pout, int tid, int T) {
  const int side = 2 * pout;
  for (int idx = tid; idx < ns * sin * sin * cin; idx += T) {
    const int ci = idx % cin, x = (idx / cin) % sin, y = (idx / (cin * sin)) % sin, s = idx / (cin * sin * sin);
    const int ky0 = max(0, y - side + 1), ky1 = min(k - 1, y), kx0 = max(0, x - side + 1), kx1 = min(k - 1, x);
    float acc = 0.f;
    for (int ky = ky0; ky <= ky1; ++ky)
      for (int kx = kx0; kx <= kx1; ++kx) {
        const float* w = W + ((ky * k + kx) * cin + ci) * cout;
        const float* d = dzc + ((s * side + y - ky) * side + x - kx) * cout;
        for (int co = 0; co < cout; ++co) acc = fmaf(w[co], d[co], acc);
      }
    din[idx] = acc;
  }
}

// lenet_conv_igrad for weights that are NOT in LDS (W in global memory), bit for bit the same
// sums: tap by tap in (ky, kx) order the tap's [cin][cout] slice is copied (coalesced) into `tile`
// [cin][cout + 1] floats of LDS (the pad keeps the cin rows a wave reads on different banks), every
// thread continues the sums it owns over co in order, and keeps them in din between taps (an fp32
// store and load is exact, so the chain of fmas is lenet_conv_igrad's). One copy of a tap serves
// all ns samples. Every thread of the workgroup calls it: it holds barriers, two per tap; the
// caller puts one after it.
__device__ __forceinline__ void lenet_conv_igrad_tiled(float* din, const float* dzc, const float* W, float* tile,
                                                       int ns, int sin, int cin, int cout, int k, int pout, int tid,
                                                       int T) {
  const int side = 2 * pout, tp = cout + 1, n = ns * sin * sin * cin;
  for (int idx = tid; idx < n; idx += T) din[idx] = 0.f;
  for (int ky = 0; ky < k; ++ky)
    for (int kx = 0; kx < k; ++kx) {
      __syncthreads();  // the previous tap's readers of the tile
      const float* w = W + (ky * k + kx) * cin * cout;
      for (int i = tid; i < cin * cout; i += T) tile[(i / cout) * tp + i % cout] = w[i];
      __syncthreads();
      for (int idx = tid; idx < n; idx += T) {
        const int ci = idx % cin, x = (idx / cin) % sin, y = (idx / (cin * sin)) % sin, s = idx / (cin * sin * sin);
        const int oy = y - ky, ox = x - kx;
        if ((unsigned)oy >= (unsigned)side || (unsigned)ox >= (unsigned)side) continue;
        const float* wt = tile + ci * tp;
        const float* d = dzc + ((s * side + oy) * side + ox) * cout;
        float acc = din[idx];
        for (int co = 0; co < cout; ++co) acc = fmaf(wt[co], d[co], acc);
        din[idx] = acc;
      }
    }
}

// ---- the hidden dense layer (cfa_lenet_hidden.hip) ---------------------------------------------

// h[s][j] = relu(sum_i flat[s][i] Wh[i][j] + bh[j]) for a chunk of ns <= MAXN samples, Wh (F, H)
// with j innermost (global memory or LDS): neighbouring threads take neighbouring j, so a weight
// load is a coalesced line, and one load serves every sample of the chunk. The plan is
// lenet_hidden_cols / lenet_hidden_slices: thread (q, j) sums i = q, q + S, ... in order from 0
// into `part` [S][ns][W] (LDS), and the column's owner adds the slices 0 .. S - 1 in order, then
// the bias. The order depends on (F, H, T) alone and a sample's arithmetic is its own, so the
// chunk moves no bit. The gate is NOT stored: h > 0 exactly where z > 0, and the backward phase
// tests the stored h again. Every thread of the workgroup calls it: it holds two barriers a pass
// and ends on one.
template <int MAXN>
__device__ __forceinline__ void lenet_hidden_forward(float* __restrict__ h, const float* __restrict__ flat,
                                                     const float* __restrict__ Wh, const float* __restrict__ bh,
                                                     float* __restrict__ part, int ns, int F, int H, int tid, int T) {
  const int W = lenet_hidden_cols(H, T), S = lenet_hidden_slices(H, T);
  const int q = tid / W, jj = tid % W;
  for (int j0 = 0; j0 < H; j0 += W) {
    const int j = j0 + jj;
    if (q < S && j < H) {
      float acc[MAXN];
#pragma unroll
      for (int s = 0; s < MAXN; ++s) acc[s] = 0.f;
      for (int i = q; i < F; i += S) {
        const float w = Wh[i * H + j];
#pragma unroll
        for (int s = 0; s < MAXN; ++s)
          if (s < ns) acc[s] = fmaf(flat[s * F + i], w, acc[s]);
      }
#pragma unroll
      for (int s = 0; s < MAXN; ++s)
        if (s < ns) part[(q * ns + s) * W + jj] = acc[s];
    }
    __syncthreads();
    for (int idx = tid; idx < ns * W; idx += T) {
      const int s = idx / W, c = idx % W;
      if (j0 + c >= H) continue;
      float z = part[s * W + c];
      for (int r = 1; r < S; ++r) z += part[(r * ns + s) * W + c];
      z += bh[j0 + c];
      h[s * H + j0 + c] = z > 0.f ? z : 0.f;
    }
    __syncthreads();  // the next pass writes part again; the caller reads h
  }
}

// Lanes that share one dflat sum over j: the power of two >= min(H, 64), from H alone.
__device__ __forceinline__ int lenet_hidden_lanes(int H) {
  int L = 1;
  while (L < 64 && L < H) L *= 2;
  return L;
}

// The hidden layer's backward for a chunk of ns <= MAXN samples. dh [ns][H] arrives as the output
// dense layer's input gradient (lenet_dense_backward with F = H) and is gated in place first, by
// the forward's own test read from the stored h (a product with 1 or 0, so a NaN upstream reaches
// every element). Then gWh[i][j] += sum_s flat[s][i] dh[s][j] and gbh[j] += sum_s dh[s][j], one
// thread per element (neighbouring threads neighbouring j), samples in order onto the running sum;
// and dflat[s][i] = sum_j Wh[i][j] dh[s][j]: the L lanes of a row i (lenet_hidden_lanes) take
// j = lane, lane + L, ... in order from 0 and fold by xor-shuffles, one weight load serving every
// sample. Every thread of the workgroup calls it: it holds one barrier; the caller puts one after it.
template <int MAXN>
__device__ __forceinline__ void lenet_hidden_backward(float* __restrict__ gWh, float* __restrict__ gbh,
                                                      float* __restrict__ dflat, float* __restrict__ dh,
                                                      const float* __restrict__ h, const float* __restrict__ flat,
                                                      const float* __restrict__ Wh, int ns, int F, int H, int tid,
                                                      int T) {
  for (int idx = tid; idx < ns * H; idx += T) dh[idx] = (h[idx] > 0.f ? 1.f : 0.f) * dh[idx];
  __syncthreads();
  for (int e = tid; e < F * H; e += T) {
    const int i = e / H, j = e % H;
    float a = gWh[e];
    for (int s = 0; s < ns; ++s) a = fmaf(flat[s * F + i], dh[s * H + j], a);
    gWh[e] = a;
  }
  for (int j = tid; j < H; j += T) {
    float a = gbh[j];
    for (int s = 0; s < ns; ++s) a += dh[s * H + j];
    gbh[j] = a;
  }
  const int L = lenet_hidden_lanes(H);
  for (int idx = tid; idx < F * L; idx += T) {  // T is a multiple of 64: a row's L lanes enter together
    const int i = idx / L, lane = idx % L;
    float acc[MAXN];
#pragma unroll
    for (int s = 0; s < MAXN; ++s) acc[s] = 0.f;
    for (int j = lane; j < H; j += L) {
      const float w = Wh[i * H + j];
#pragma unroll
      for (int s = 0; s < MAXN; ++s)
        if (s < ns) acc[s] = fmaf(w, dh[s * H + j], acc[s]);
    }
#pragma unroll
    for (int s = 0; s < MAXN; ++s)
      if (s < ns) {
        const float v = lenet_fold(acc[s], L);
        if (lane == 0) dflat[s * F + i] = v;
      }
  }
}

// ---- what the average-pool and the max-pool kernels share around the phases ------------------

constexpr int kLenetFinishBlock = 256;  // the workgroup of both finishing kernels

// The arguments of an evaluation kernel (cfa_lenet.hip, cfa_lenet_global.h).
struct LenetArgs {
  const float* x;         // [Nt][side][side][cin], or [D][Nt][side][side][cin] with x_stride
  const int32_t* labels;  // [Nt], or [D][Nt] with label_stride
  long long x_stride, label_stride;
  const float* models;    // [D][pitch]
  long long pitch;
  int batch, batches;
  const int32_t* skip;    // [D] or null
  float* ws;              // [D][batches] batch losses
};

struct LenetFinish {
  const float* ws;
  int D, batches;
  const int32_t* skip;
  double target;
  int32_t* ended;  // or null
  double* cost;
  double* cost_log;  // or null
  int log_cap;
  unsigned long long* epoch;  // or null, with cost_log
};

// One workgroup. Thread d % T owns device d: its cost, its flag (read before it is written, so
// skip and ended may be one array) and its log entry.
__global__ __launch_bounds__(kLenetFinishBlock) void lenet_finish_kernel(LenetFinish f) {
  unsigned long long row = 0;
  if (f.cost_log) {
    const unsigned long long e = *f.epoch, last = (unsigned long long)(f.log_cap - 1);
    row = e < last ? e : last;
  }
  for (int d = threadIdx.x; d < f.D; d += blockDim.x) {
    double c;
    if (f.skip && f.skip[d]) {
      c = f.cost[d];
    } else {
      double acc = 0.0;
      for (int b = 0; b < f.batches; ++b) acc += (double)f.ws[(long long)d * f.batches + b];
      c = acc / (double)f.batches;
      f.cost[d] = c;
      if (f.ended) f.ended[d] = f.ended[d] | (c < f.target ? 1 : 0);
    }
    if (f.cost_log) f.cost_log[row * (unsigned long long)f.D + d] = c;
  }
  if (f.cost_log) {
    __syncthreads();  // every thread has read the counter
    if (threadIdx.x == 0) *f.epoch = *f.epoch + 1;
  }
}

// The arguments of a gradient kernel (cfa_lenet_grad.hip, cfa_lenet_global.h).
struct LenetGradArgs {
  const float* x;         // [Nt][side][side][cin], or [D][Nt][side][side][cin] with x_stride
  const int32_t* labels;  // [Nt], or [D][Nt] with label_stride
  long long x_stride, label_stride;
  const float* models;    // [D][pitch]
  long long pitch;
  const int32_t* src;      // [D] or null: the row of models device d evaluates
  const long long* first;  // [D] or null: the first sample of device d's batch
  const int32_t* skip;     // [D] or null
  int Nt, batch, D, groups;
  float* ws;  // [D][groups][P + GROUP]: a group's gradient sums, then its samples' losses
};

struct LenetGradFinish {
  const float* ws;
  int P, groups, batch;
  const int32_t* skip;
  float* grads;  // [D][gpitch]
  long long gpitch;
  float* loss;  // [D] or null
};

// Grid (ceil((P + 1) / block), D): element e < P of device d's row, or e == P, its loss. GROUP:
// the samples of a sample group of the gradient kernel that filled ws.
template <int GROUP>
__global__ __launch_bounds__(kLenetFinishBlock) void lenet_grad_finish_kernel(LenetGradFinish f) {
  const int dv = blockIdx.y;
  if (f.skip && f.skip[dv]) return;
  const int e = blockIdx.x * blockDim.x + threadIdx.x, stride = f.P + GROUP;
  const float* base = f.ws + (long long)dv * f.groups * stride;
  if (e < f.P) {
    float acc = base[e];
    for (int gi = 1; gi < f.groups; ++gi) acc += base[(long long)gi * stride + e];
    f.grads[(long long)dv * f.gpitch + e] = acc / (float)f.batch;
  } else if (e == f.P && f.loss) {  // reduce_mean over the batch, fp32, in sample order
    float c = 0.f;
    for (int s = 0; s < f.batch; ++s) c += base[(long long)(s / GROUP) * stride + f.P + s % GROUP];
    f.loss[dv] = c / (float)f.batch;
  }
}

// The host checks of an evaluation entry, in the order every entry of the family keeps: the
// objective first, then CFA_E_INVALID for the arguments (ws_need: the entry's workspace bytes),
// then CFA_E_UNSUPPORTED for classes and D. What fits LDS is the entry's own check, after these.
// The entry's family gives the geometry's verdict: whether it has a model (geom_ok), its numbers
// and rule as text for the refusal (geom_text), the model's parameters P and an image's floats.
inline int lenet_eval_checks_for(const char* fn, const void* x, const void* labels, size_t x_dev_stride,
                                 size_t label_dev_stride, int Nt, bool geom_ok, const char* geom_text, long long P,
                                 long long image, int classes, const void* models, size_t pitch, int D, int batch,
                                 int batches, double target, const void* ended, const void* cost,
                                 const void* cost_log, int log_cap, const void* epoch, const void* workspace,
                                 size_t workspace_bytes, size_t ws_need, int loss) {
  if (loss != CFA_LENET_LOSS_XENT && loss != CFA_LENET_LOSS_HUBER)
    return fail(CFA_E_INVALID, "%s: unknown loss kind %d (CFA_LENET_LOSS_XENT or CFA_LENET_LOSS_HUBER)", fn, loss);
  if (!x || !labels || !models || !cost || !workspace) return fail(CFA_E_INVALID, "%s: null buffer", fn);
  if (D < 1 || batch < 1 || batches < 1 || Nt < 1)
    return fail(CFA_E_INVALID, "%s: D %d, batch %d, batches %d and Nt %d must be >= 1", fn, D, batch, batches, Nt);
  if (!geom_ok) return fail(CFA_E_INVALID, "%s: bad geometry %s", fn, geom_text);
  if ((long long)batch * batches > Nt)
    return fail(CFA_E_INVALID, "%s: %d batches of %d samples do not fit the %d of the test set", fn, batches, batch,
                Nt);
  if ((long long)pitch < P)
    return fail(CFA_E_INVALID, "%s: pitch %zu below the model's %lld parameters", fn, pitch, P);
  const long long set = (long long)Nt * image;
  if ((x_dev_stride != 0 && (long long)x_dev_stride < set) || (label_dev_stride != 0 && (long long)label_dev_stride < Nt))
    return fail(CFA_E_INVALID, "%s: device strides %zu / %zu below one device's set (%lld / %d)", fn, x_dev_stride,
                label_dev_stride, set, Nt);
  if ((cost_log == nullptr) != (epoch == nullptr))
    return fail(CFA_E_INVALID, "%s: cost_log and epoch are given together or not at all", fn);
  if (cost_log && log_cap < 1) return fail(CFA_E_INVALID, "%s: log_cap %d must be >= 1", fn, log_cap);
  if (workspace_bytes < ws_need)
    return fail(CFA_E_INVALID, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, ws_need);
  if (ended && !std::isfinite(target)) return fail(CFA_E_INVALID, "%s: target must be finite", fn);
  if (classes > 64) return fail(CFA_E_UNSUPPORTED, "%s: more than 64 classes", fn);
  if (D > 65535) return fail(CFA_E_UNSUPPORTED, "%s: more than 65535 devices", fn);
  return CFA_OK;
}

// The five-number family's verdict text.
inline void lenet_geom_text(char (&text)[192], int side, int kernel, int c1, int c2, int classes) {
  snprintf(text, sizeof text, "(side %d kernel %d c1 %d c2 %d classes %d): every dimension >= 1 and a second pooled "
           "map of at least 1 x 1", side, kernel, c1, c2, classes);
}

inline int lenet_eval_checks(const char* fn, const void* x, const void* labels, size_t x_dev_stride,
                             size_t label_dev_stride, int Nt, int side, int kernel, int c1, int c2, int classes,
                             const void* models, size_t pitch, int D, int batch, int batches, double target,
                             const void* ended, const void* cost, const void* cost_log, int log_cap,
                             const void* epoch, const void* workspace, size_t workspace_bytes, size_t ws_need,
                             int loss, LenetGeom& g) {
  char text[192];
  lenet_geom_text(text, side, kernel, c1, c2, classes);
  const bool ok = lenet_geom(side, kernel, c1, c2, classes, g);
  return lenet_eval_checks_for(fn, x, labels, x_dev_stride, label_dev_stride, Nt, ok, text, ok ? g.P : 0,
                               (long long)side * side, classes, models, pitch, D, batch, batches, target, ended, cost,
                               cost_log, log_cap, epoch, workspace, workspace_bytes, ws_need, loss);
}

// The same for a gradient entry. Its workspace is checked by the entry after what fits LDS, as
// cfa_lenet_grad_loss_f32 always has.
inline int lenet_grad_checks_for(const char* fn, const void* x, const void* labels, size_t x_dev_stride,
                                 size_t label_dev_stride, int Nt, bool geom_ok, const char* geom_text, long long P,
                                 long long image, int classes, const void* models, size_t pitch, int D, int batch,
                                 const void* grads, size_t gpitch, const void* workspace, int loss_kind) {
  if (loss_kind != CFA_LENET_LOSS_XENT && loss_kind != CFA_LENET_LOSS_HUBER)
    return fail(CFA_E_INVALID, "%s: unknown loss kind %d (CFA_LENET_LOSS_XENT or CFA_LENET_LOSS_HUBER)", fn,
                loss_kind);
  if (!x || !labels || !models || !grads || !workspace) return fail(CFA_E_INVALID, "%s: null buffer", fn);
  if (D < 1 || batch < 1 || Nt < 1)
    return fail(CFA_E_INVALID, "%s: D %d, batch %d and Nt %d must be >= 1", fn, D, batch, Nt);
  if (!geom_ok) return fail(CFA_E_INVALID, "%s: bad geometry %s", fn, geom_text);
  if (batch > Nt)
    return fail(CFA_E_INVALID, "%s: a batch of %d samples does not fit the %d of the training set", fn, batch, Nt);
  if ((long long)pitch < P)
    return fail(CFA_E_INVALID, "%s: pitch %zu below the model's %lld parameters", fn, pitch, P);
  if ((long long)gpitch < P)
    return fail(CFA_E_INVALID, "%s: gpitch %zu below the model's %lld parameters", fn, gpitch, P);
  const long long set = (long long)Nt * image;
  if ((x_dev_stride != 0 && (long long)x_dev_stride < set) || (label_dev_stride != 0 && (long long)label_dev_stride < Nt))
    return fail(CFA_E_INVALID, "%s: device strides %zu / %zu below one device's set (%lld / %d)", fn, x_dev_stride,
                label_dev_stride, set, Nt);
  if (classes > 64) return fail(CFA_E_UNSUPPORTED, "%s: more than 64 classes", fn);
  if (D > 65535) return fail(CFA_E_UNSUPPORTED, "%s: more than 65535 devices", fn);
  return CFA_OK;
}

inline int lenet_grad_checks(const char* fn, const void* x, const void* labels, size_t x_dev_stride,
                             size_t label_dev_stride, int Nt, int side, int kernel, int c1, int c2, int classes,
                             const void* models, size_t pitch, int D, int batch, const void* grads, size_t gpitch,
                             const void* workspace, int loss_kind, LenetGeom& g) {
  char text[192];
  lenet_geom_text(text, side, kernel, c1, c2, classes);
  const bool ok = lenet_geom(side, kernel, c1, c2, classes, g);
  return lenet_grad_checks_for(fn, x, labels, x_dev_stride, label_dev_stride, Nt, ok, text, ok ? g.P : 0,
                               (long long)side * side, classes, models, pitch, D, batch, grads, gpitch, workspace,
                               loss_kind);
}

}  // namespace

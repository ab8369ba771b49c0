// cfa_lenet_graph.h — the forward pass of the TF2 drivers' "LeNet-1 family" (create_q_model,
// condition 0, federated_learning_keras_consensus_FL_threads_MNIST_crossentropy_gradients_exchange.py
// :158-194), written once as phases for the kernels that evaluate it (cfa_lenet.hip: the validation
// cost; a gradient kernel would run the same forward phases), and the family's geometry on the host.
//   x [side, side, 1] -> Conv2D(c1, k x k, valid) + b1 -> relu -> AveragePooling2D(2 x 2, stride 2)
//     -> Conv2D(c2, k x k, valid) + b2 -> relu -> AveragePooling2D(2 x 2) -> Flatten -> Dense(classes)
//   loss = -log softmax(z)[label], evaluated as -(z_l - max - log(sum exp(z - max)))
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
#pragma once
#include "cfa_grad_common.h"

namespace {

// ---- geometry (host) ----------------------------------------------------------------------

struct LenetGeom {
  int side, k, c1, c2, C;
  int s1, p1, s2, p2;  // conv / pool output sides of the two stages
  int flat;            // p2 * p2 * c2
  int oK1, ob1, oK2, ob2, oWd, obd;  // offsets of the six tensors in a model row
  long long P;
};

// The family's geometry from the caller's five numbers; false for a geometry that has no model
// (a dimension < 1, a kernel larger than its input, an empty pooled map). Offsets are valid only
// while P fits an int; a kernel's entry refuses a model that large before any launch.
inline bool lenet_geom(int side, int kernel, int c1, int c2, int classes, LenetGeom& g) {
  if (side < 1 || kernel < 1 || c1 < 1 || c2 < 1 || classes < 1) return false;
  g.side = side, g.k = kernel, g.c1 = c1, g.c2 = c2, g.C = classes;
  g.s1 = side - kernel + 1;
  g.p1 = g.s1 > 0 ? g.s1 / 2 : 0;
  g.s2 = g.p1 - kernel + 1;
  g.p2 = g.s2 > 0 ? g.s2 / 2 : 0;
  if (g.p2 < 1) return false;
  const long long kk = (long long)kernel * kernel, flat = (long long)g.p2 * g.p2 * c2;
  const long long nK1 = kk * c1, nK2 = kk * c1 * c2, nWd = flat * classes;
  g.P = nK1 + c1 + nK2 + c2 + nWd + classes;
  if (g.P > 0x7fffffffLL) {
    g.flat = g.oK1 = g.ob1 = g.oK2 = g.ob2 = g.oWd = g.obd = 0;
    return true;
  }
  g.flat = (int)flat;
  g.oK1 = 0;
  g.ob1 = (int)nK1;
  g.oK2 = g.ob1 + c1;
  g.ob2 = g.oK2 + (int)nK2;
  g.oWd = g.ob2 + c2;
  g.obd = g.oWd + (int)nWd;
  return true;
}

// LDS floats one sample's forward pass needs: the image, the two pooled maps and the logits.
inline long long lenet_sample_floats(const LenetGeom& g) {
  return (long long)g.side * g.side + (long long)g.p1 * g.p1 * g.c1 + g.flat + g.C;
}

// ---- phases ---------------------------------------------------------------------------------

// One stage of the family for ns samples: out[s][py][px][co] = mean over the 2 x 2 window of
// relu(conv(in)[2py + dy][2px + dx][co] + b[co]), in [ns][sin][sin][cin] and out
// [ns][pout][pout][cout] both NHWC, W (k, k, cin, cout). The four convolutions of a window run
// side by side from one weight load per tap; each sums its taps in (ci, ky, kx) order from 0 and
// adds the bias last, and the window is summed (0,0) (0,1) (1,0) (1,1) and scaled by 0.25 (exact).
// K > 0: the kernel side at compile time (the tap loops unroll, and the window's (K + 1)^2 inputs
// are loaded once); K = 0: any side. The arithmetic and its order are the same either way.
template <int K>
__device__ __forceinline__ void lenet_conv_pool(float* __restrict__ out, const float* __restrict__ in,
                                                const float* __restrict__ W, const float* __restrict__ b, int ns,
                                                int sin, int cin, int cout, int kside, int pout, int tid, int T) {
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
    const float h00 = z00 > 0.f ? z00 : 0.f, h01 = z01 > 0.f ? z01 : 0.f;
    const float h10 = z10 > 0.f ? z10 : 0.f, h11 = z11 > 0.f ? z11 : 0.f;
    out[idx] = (((h00 + h01) + h10) + h11) * 0.25f;
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
// sample, classes in order. A label outside [0, C) reads nothing and gives NaN.
__device__ __forceinline__ void lenet_xent(float* loss, const float* zl, const int32_t* labels, int ns, int C,
                                           int tid, int T) {
  for (int s = tid; s < ns; s += T) {
    const float* z = zl + s * C;
    float mx = z[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, z[c]);
    float sum = 0.f;
    for (int c = 0; c < C; ++c) sum += expf(z[c] - mx);
    const int l = labels[s];
    loss[s] = (unsigned)l < (unsigned)C ? -((z[l] - mx) - logf(sum)) : NAN;
  }
}

}  // namespace

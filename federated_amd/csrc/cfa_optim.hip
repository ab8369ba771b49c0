// cfa_optim.hip — the local optimizer step of a device-resident TF2 population
// (cfa_optim_step_f32): plain SGD, Keras momentum SGD and Keras Adam with tf.clip_by_norm per
// layer, for every device of a [D, pitch] stack at once. The shape rules (tile, workspace slots)
// are in cfa_optim_shape.h.
#include "cfa_internal.h"
#include "cfa_optim_shape.h"

// ------------------------------------------------------------------------------------------
// A workgroup takes tiles of kOptimTile elements of one device's row (blockIdx.y), grid-stride
// along the row. A tile is cut at the layer boundaries that fall into it; each piece [lo, hi) is
// one layer's, so it has one clip scale and one trainable flag. Lane i owns the groups
// i, i + kBlock, ... of four consecutive elements of the tile, counted from the row's first
// element: a group that lies inside the piece is one 16-byte access when the row starts 16-byte
// aligned, and element by element otherwise (a piece's head and tail, a misaligned row). Which
// lane adds which element, and in which order, is therefore the same for every alignment.
//
// Adam with the clip is two launches. optim_sumsq_kernel leaves one fp64 partial sum of g * g per
// (tile, layer) pair in slot k + l; optim_update_kernel adds a layer's partials (lanes take them
// in index order at a stride of kBlock, then the fixed tree of block_sum) before it steps the
// layer's elements. No atomics: the same inputs give the same bits. A last small launch leaves
// the step counters and the running powers of the stepped devices one step on.
// ------------------------------------------------------------------------------------------
namespace {

static_assert(kOptimBlock == kBlock, "cfa_optim_shape.h counts tiles of kBlock lanes");
constexpr int kT = kOptimTile;

struct OptimArgs {
  float* w;                  // [D, w_pitch]
  const float* g;            // [D, g_pitch]
  float* m;                  // [D, s_pitch] (momentum: the accumulator)
  float* v;                  // [D, s_pitch]
  const int32_t* layer_ptr;  // [n + 1]
  const int32_t* trainable;  // [n]
  const int32_t* skip;       // [D] or null
  const double* pw;          // [D, 2] running beta_1^t, beta_2^t before this step
  double* ws;                // [D, slots] partial sums of squares
  long long w_pitch, g_pitch, s_pitch, slots;
  int n, P;
  bool clip;
  float lr, momentum, omb1, omb2, eps;
  double beta1, beta2, clipnorm;
};

// What an element's step needs besides its own values.
struct Coef {
  float lr, momentum, omb1, omb2, eps, lr_t, scale;
};

// The largest l in [0, n) with layer_ptr[l] <= e (uniform: every lane walks the same loads).
__device__ __forceinline__ int layer_of(const int32_t* lp, int n, int e) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (lp[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Sum of one value per lane, the same bits in every lane: a butterfly within the wave, then the
// waves' sums in wave order. Called by every lane of the workgroup (it synchronises).
__device__ __forceinline__ double block_sum(double x) {
  __shared__ double red[kBlock / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  __syncthreads();  // the previous call's readers are done
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int i = 1; i < kBlock / 64; ++i) s += red[i];
  return s;
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// One element's step. Every operation is rounded to fp32 on its own (-ffp-contract=off).
template <int RULE>
__device__ __forceinline__ void step1(float& w, float g, float& m, float& v, const Coef& c) {
  if constexpr (RULE == CFA_OPTIM_SGD) {
    const float t = c.lr * g;
    w = w - t;
  } else if constexpr (RULE == CFA_OPTIM_MOMENTUM) {
    const float t1 = c.momentum * m;
    const float t2 = c.lr * g;
    m = t1 - t2;
    w = w + m;
  } else {
    const float gs = g * c.scale;  // scale is exactly 1 without the clip and below the norm
    float t = gs - m;
    t = t * c.omb1;
    m = m + t;
    t = gs * gs;
    t = t - v;
    t = t * c.omb2;
    v = v + t;
    t = c.lr_t * m;
    const float den = sqrtf(v) + c.eps;
    t = t / den;
    w = w - t;
  }
}
template <int RULE>
__device__ __forceinline__ void step4(f4& w, f4 g, f4& m, f4& v, const Coef& c) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // a vector's component does not bind to a reference
    float w1 = w[k], m1 = m[k], v1 = v[k];
    step1<RULE>(w1, g[k], m1, v1, c);
    w[k] = w1, m[k] = m1, v[k] = v1;
  }
}

// One device's rows.
struct Rows {
  float* w;
  const float* g;
  float* m;
  float* v;
};

// The group of four elements at e0 (a multiple of 4), as far as it lies in [lo, hi).
template <int RULE>
__device__ __forceinline__ void update_group(const Rows& r, int e0, int lo, int hi, bool vec, const Coef& c) {
  constexpr bool M = RULE != CFA_OPTIM_SGD, V = RULE == CFA_OPTIM_ADAM;
  if (vec && e0 >= lo && e0 + 4 <= hi) {
    const long long i = e0 >> 2;
    f4 w = ld4<false>(r.w, i), m = {}, v = {};
    const f4 g = ld4<true>(r.g, i);
    if constexpr (M) m = ld4<false>(r.m, i);
    if constexpr (V) v = ld4<false>(r.v, i);
    step4<RULE>(w, g, m, v, c);
    st4<false>(r.w, i, w);
    if constexpr (M) st4<false>(r.m, i, m);
    if constexpr (V) st4<false>(r.v, i, v);
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int e = e0 + k;
    if (e < lo || e >= hi) continue;
    float w = r.w[e], m = 0.0f, v = 0.0f;
    if constexpr (M) m = r.m[e];
    if constexpr (V) v = r.v[e];
    step1<RULE>(w, r.g[e], m, v, c);
    r.w[e] = w;
    if constexpr (M) r.m[e] = m;
    if constexpr (V) r.v[e] = v;
  }
}

// A whole tile inside one layer on an aligned row: every load of the lane issued ahead of the steps.
template <int RULE>
__device__ __forceinline__ void update_full_tile(const Rows& r, int ts, const Coef& c) {
  constexpr bool M = RULE != CFA_OPTIM_SGD, V = RULE == CFA_OPTIM_ADAM;
  constexpr int U = kOptimGroups;
  const long long i0 = (ts >> 2) + threadIdx.x;
  f4 w[U], g[U], m[U], v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long long i = i0 + u * kBlock;
    w[u] = ld4<false>(r.w, i);
    g[u] = ld4<true>(r.g, i);
    if constexpr (M) m[u] = ld4<false>(r.m, i);
    else m[u] = f4{};
    if constexpr (V) v[u] = ld4<false>(r.v, i);
    else v[u] = f4{};
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long long i = i0 + u * kBlock;
    step4<RULE>(w[u], g[u], m[u], v[u], c);
    st4<false>(r.w, i, w[u]);
    if constexpr (M) st4<false>(r.m, i, m[u]);
    if constexpr (V) st4<false>(r.v, i, v[u]);
  }
}

// Squares of the group at e0 as far as it lies in [lo, hi), added to acc in element order. The
// square of an fp32 value is exact in fp64.
__device__ __forceinline__ void sumsq_group(const float* g, int e0, int lo, int hi, bool vec, double& acc) {
  if (vec && e0 >= lo && e0 + 4 <= hi) {
    const f4 x = ld4<false>(g, e0 >> 2);  // read again by the update: not a streaming load
    acc += (double)x.x * (double)x.x;
    acc += (double)x.y * (double)x.y;
    acc += (double)x.z * (double)x.z;
    acc += (double)x.w * (double)x.w;
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int e = e0 + k;
    if (e < lo || e >= hi) continue;
    const double x = g[e];
    acc += x * x;
  }
}

__global__ __launch_bounds__(kBlock) void optim_sumsq_kernel(OptimArgs a) {
  const int d = blockIdx.y;
  if (a.skip && a.skip[d]) return;
  const float* g = a.g + d * a.g_pitch;
  const bool vec = aligned16(g);
  double* ws = a.ws + d * a.slots;
  const int ntiles = (a.P + kT - 1) / kT;
  for (int k = blockIdx.x; k < ntiles; k += gridDim.x) {
    const int ts = k * kT, te = min(ts + kT, a.P);
    for (int l = layer_of(a.layer_ptr, a.n, ts); l < a.n && a.layer_ptr[l] < te; ++l) {
      if (!a.trainable[l]) continue;
      const int lo = max(ts, a.layer_ptr[l]), hi = min(te, a.layer_ptr[l + 1]);
      double acc = 0.0;
#pragma unroll
      for (int u = 0; u < kOptimGroups; ++u) {
        const int e0 = ts + 4 * ((int)threadIdx.x + u * kBlock);
        if (e0 < hi && e0 + 4 > lo) sumsq_group(g, e0, lo, hi, vec, acc);
      }
      acc = block_sum(acc);
      if (threadIdx.x == 0) ws[k + l] = acc;
    }
  }
}

// The clip scale of layer l of the device whose partials are ws: clipnorm / max(norm, clipnorm),
// formed in fp64 and rounded once. Called by every lane of the workgroup.
__device__ __forceinline__ float layer_scale(const OptimArgs& a, const double* ws, int l, int ntiles) {
  int kf = a.layer_ptr[l] / kT, kl = (a.layer_ptr[l + 1] - 1) / kT;
  kf = max(kf, 0);  // a table the caller did not check must not lead outside the workspace
  kl = min(kl, ntiles - 1);
  double s = 0.0;
  for (int k = kf + (int)threadIdx.x; k <= kl; k += kBlock) s += ws[k + l];
  s = block_sum(s);
  return (float)(a.clipnorm / fmax(sqrt(s), a.clipnorm));
}

template <int RULE>
__global__ __launch_bounds__(kBlock) void optim_update_kernel(OptimArgs a) {
  constexpr bool M = RULE != CFA_OPTIM_SGD, V = RULE == CFA_OPTIM_ADAM;
  const int d = blockIdx.y;
  if (a.skip && a.skip[d]) return;
  const Rows r{a.w + d * a.w_pitch, a.g + d * a.g_pitch, M ? a.m + d * a.s_pitch : nullptr,
               V ? a.v + d * a.s_pitch : nullptr};
  const bool vec = aligned16(r.w) && aligned16(r.g) && (!M || aligned16(r.m)) && (!V || aligned16(r.v));
  Coef c{a.lr, a.momentum, a.omb1, a.omb2, a.eps, 0.0f, 1.0f};
  if constexpr (V) {
    const double b1p = a.pw[2 * d] * a.beta1, b2p = a.pw[2 * d + 1] * a.beta2;  // beta^t of this step
    c.lr_t = (float)((double)a.lr * sqrt(1.0 - b2p) / (1.0 - b1p));
  }
  const double* ws = a.ws + d * a.slots;
  const int ntiles = (a.P + kT - 1) / kT;
  int scaled = -1;  // the layer c.scale belongs to: a workgroup's tiles ascend, long layers repeat
  for (int k = blockIdx.x; k < ntiles; k += gridDim.x) {
    const int ts = k * kT, te = min(ts + kT, a.P);
    for (int l = layer_of(a.layer_ptr, a.n, ts); l < a.n && a.layer_ptr[l] < te; ++l) {
      if (!a.trainable[l]) continue;
      const int lo = max(ts, a.layer_ptr[l]), hi = min(te, a.layer_ptr[l + 1]);
      if (V && a.clip && l != scaled) {
        c.scale = layer_scale(a, ws, l, ntiles);
        scaled = l;
      }
      if (vec && lo == ts && hi == ts + kT) {
        update_full_tile<RULE>(r, ts, c);
        continue;
      }
#pragma unroll
      for (int u = 0; u < kOptimGroups; ++u) {
        const int e0 = ts + 4 * ((int)threadIdx.x + u * kBlock);
        if (e0 < hi && e0 + 4 > lo) update_group<RULE>(r, e0, lo, hi, vec, c);
      }
    }
  }
}

// The stepped devices' counters one higher and their running powers one factor on.
__global__ void optim_advance_kernel(const int32_t* skip, long long* t, double* pw, double beta1, double beta2, int D) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D || (skip && skip[d])) return;
  t[d] += 1;
  if (pw) {
    pw[2 * d] *= beta1;
    pw[2 * d + 1] *= beta2;
  }
}

constexpr int kMaxGridY = 65535;

}  // namespace

extern "C" int cfa_optim_tile(void) { return kOptimTile; }

extern "C" size_t cfa_optim_workspace_bytes(int D, size_t P, int n_layers) {
  if (D < 1 || P < 1 || n_layers < 1) return 0;
  return (size_t)D * (size_t)optim_slots((long long)P, n_layers) * sizeof(double);
}

extern "C" int cfa_optim_step_f32(float* models, size_t pitch, const float* grads, size_t grad_pitch, float* m,
                                  float* v, size_t state_pitch, const int32_t* layer_ptr,
                                  const int32_t* trainable, int n_layers, const int32_t* skip, long long* t,
                                  double* pow, int rule, float lr, float momentum, double beta_1, double beta_2,
                                  float epsilon, float clipnorm, void* workspace, size_t workspace_bytes, int D,
                                  size_t P, void* stream) {
  if (rule != CFA_OPTIM_SGD && rule != CFA_OPTIM_MOMENTUM && rule != CFA_OPTIM_ADAM)
    return fail(CFA_E_INVALID, "unknown optimizer rule %d", rule);
  const bool adam = rule == CFA_OPTIM_ADAM, clip = adam && clipnorm > 0.0f;
  if (D < 1 || P < 1 || n_layers < 1)
    return fail(CFA_E_INVALID, "optimizer step of %d devices, %zu parameters, %d layers: all must be >= 1", D, P,
                n_layers);
  if (!models || !grads || !layer_ptr || !trainable || !t)
    return fail(CFA_E_INVALID, "null models, grads, layer table, trainable flags or step counters");
  if (rule != CFA_OPTIM_SGD && !m) return fail(CFA_E_INVALID, "null state m");
  if (adam && (!v || !pow)) return fail(CFA_E_INVALID, "null state v or running powers");
  if (pitch < P || grad_pitch < P || (rule != CFA_OPTIM_SGD && state_pitch < P))
    return fail(CFA_E_INVALID, "pitch %zu / %zu / %zu below P %zu", pitch, grad_pitch, state_pitch, P);
  if (P > (size_t)0x7fffffff - kOptimTile)
    return fail(CFA_E_UNSUPPORTED, "P %zu does not fit the int32 layer table", P);
  if (D > kMaxGridY) return fail(CFA_E_UNSUPPORTED, "more than %d devices in one step", kMaxGridY);
  if (!std::isfinite(lr)) return fail(CFA_E_INVALID, "learning rate is not finite");
  if (rule == CFA_OPTIM_MOMENTUM && !std::isfinite(momentum)) return fail(CFA_E_INVALID, "momentum is not finite");
  if (adam && !(beta_1 >= 0.0 && beta_1 < 1.0 && beta_2 >= 0.0 && beta_2 < 1.0))
    return fail(CFA_E_INVALID, "beta_1 %g and beta_2 %g must lie in [0, 1)", beta_1, beta_2);
  if (adam && !(epsilon >= 0.0f)) return fail(CFA_E_INVALID, "epsilon %g is negative or NaN", (double)epsilon);
  // rows that start 16-byte aligned are streamed as float4, the others element by element
  if (((addr(models) | addr(grads) | addr(m) | addr(v)) & 3) || ((addr(t) | addr(pow) | addr(workspace)) & 7))
    return fail(CFA_E_UNSUPPORTED, "misaligned rows (fp32 arrays to 4 bytes, counters, powers and workspace to 8)");
  const size_t need = cfa_optim_workspace_bytes(D, P, n_layers);
  if (clip && (!workspace || workspace_bytes < need))
    return fail(CFA_E_INVALID, "the clip needs a workspace of %zu bytes (cfa_optim_workspace_bytes)", need);

  OptimArgs a{};
  a.w = models, a.g = grads, a.m = m, a.v = v;
  a.layer_ptr = layer_ptr, a.trainable = trainable, a.skip = skip;
  a.pw = pow, a.ws = (double*)workspace;
  a.w_pitch = (long long)pitch, a.g_pitch = (long long)grad_pitch, a.s_pitch = (long long)state_pitch;
  a.slots = optim_slots((long long)P, n_layers);
  a.n = n_layers, a.P = (int)P, a.clip = clip;
  a.lr = lr, a.momentum = momentum, a.eps = epsilon;
  a.omb1 = (float)(1.0 - beta_1), a.omb2 = (float)(1.0 - beta_2);
  a.beta1 = beta_1, a.beta2 = beta_2, a.clipnorm = (double)clipnorm;

  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(shared_grid_x(optim_tiles((long long)P), kOptimWgPerCu, D), (unsigned)D);
  if (clip) {
    optim_sumsq_kernel<<<grid, kBlock, 0, st>>>(a);
    if (int rc = check_launch("optim_sumsq")) return rc;
  }
  if (adam) optim_update_kernel<CFA_OPTIM_ADAM><<<grid, kBlock, 0, st>>>(a);
  else if (rule == CFA_OPTIM_MOMENTUM) optim_update_kernel<CFA_OPTIM_MOMENTUM><<<grid, kBlock, 0, st>>>(a);
  else optim_update_kernel<CFA_OPTIM_SGD><<<grid, kBlock, 0, st>>>(a);
  if (int rc = check_launch("optim_update")) return rc;
  optim_advance_kernel<<<(D + kBlock - 1) / kBlock, kBlock, 0, st>>>(skip, t, adam ? pow : nullptr, beta_1, beta_2, D);
  return check_launch("optim_advance");
}

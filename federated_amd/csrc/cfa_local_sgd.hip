// cfa_local_sgd.hip — one local epoch of plain minibatch SGD for every device of a TF1 population
// in ONE launch (tensorflow1_implementations/federated_sample_CNN_CFA-GE.py:137-173 and
// federated_sample_2NN_CFA.py:97-101: per minibatch W <- W_ext - learning_rate * grad, :114-118,
// then the validation cost :163-172), on the two model graphs of cfa_tf1_graph.h.
//
// One workgroup owns one device for the whole launch: its model is read from global memory once,
// stays in LDS for all `steps` minibatches and is stepped there, and is written back once. A
// minibatch runs the phases of cfa_tf1_graph.h, the functions cfa_grad.hip runs, so the gradient
// is that file's by construction; what differs is that the gradient of a parameter is not stored
// but applied to the LDS copy by the thread that owns it (SgdSink), after every read of the
// pre-update value (the hidden-layer gradient reads the pre-update W2; a barrier separates it
// from W2's step). The next minibatch's samples are loaded into registers before the current
// one's first phase and stored to the other half of a double buffer after its last, so their
// global round trip hides behind the compute.
//
// update = 0 is the validation pass: forward only, models untouched. The mean minibatch cost of
// the launch is accumulated in fp64 (the driver's Python float `avg_cost += c / total_batch`).
// Every output is owned by one thread and every sum runs in a fixed order: a launch is
// deterministic.
#include "cfa_tf1_graph.h"

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

// LDS floats of the CNN kernel: the model, two minibatches of samples and labels, and per sample
// pooled / argmax / d pooled, logits, the conv-gradient partial sums and the cost.
inline long long cnn_sgd_lds(const CnnGeom& d, int nb) {
  const long long LN = (long long)d.L2 * d.NC;
  return d.P + (long long)nb * (2LL * (d.L + d.C) + 3 * LN + d.C + (long long)d.F * d.NC + d.NC + 1);
}

// FT, ST: conv_pool_forward's.
template <int FT, int ST>
__global__ __launch_bounds__(kGradBlock) void local_sgd_cnn_kernel(SgdArgs a, CnnGeom d) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int nb = a.nb, LN = d.L2 * d.NC, P = (int)d.P;
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
  const SgdSink sink{a.lr};

  // the first minibatch and the model, all in flight together: one global round trip
  Prefetch pf;
  pf.load(xd, nx, yd, ny, tid, T);
  stage(W1, m, P, tid, T);
  pf.store(xs0, xd, nx, ys0, yd, ny, tid, T);
  __syncthreads();
  const bool taps_in_regs = cnn_taps_in_regs(d, T);
  double acc = 0.0;
  for (int i = 0; i < a.steps; ++i) {
    const float* xs = xs0 + (i & 1) * nx;
    const float* ys = ys0 + (i & 1) * ny;
    // the next minibatch leaves global memory now and lands in the other buffer after the step
    const bool more = i + 1 < a.steps;
    const float* xn = xd + (long long)(more ? i + 1 : i) * a.bstride * d.L;
    const float* yn = yd + (long long)(more ? i + 1 : i) * a.bstride * d.C;
    pf.load(xn, more ? nx : 0, yn, more ? ny : 0, tid, T);
    float wreg[kMaxTaps];
    load_taps<FT>(wreg, W1, d, taps_in_regs, tid);  // reloaded from the stepped W1
    conv_pool_forward<FT, ST>(pooled, arg, xs, W1, b1, wreg, taps_in_regs, nb, d, tid, T);
    __syncthreads();
    cnn_logits(zl, pooled, W2, b2, nb, LN, d.C, tid, T);
    __syncthreads();
    softmax_xent<true>(zl, ys, cs, nb, d.C, d.SW, invB, a.update != 0, tid, T);
    __syncthreads();
    if (tid == 0) add_cost(acc, cs, nb, a.steps);
    if (a.update) {
      // the gradient flowing into the pooled features, through the pre-update W2
      relu_layer_backward(dfc, pooled, zl, W2, nb, LN, d.C, tid, T);
      __syncthreads();
      // the dense layer's step, each element by the thread that owns it
      weight_sums<4>(W2, nW2, d.C, pooled, LN, zl, nb, sink, tid, T);
      column_sums(b2, d.C, zl, nb, sink, tid, T);
      conv_grad_partials(part, xs, arg, dfc, nb, d, tid, T);
      __syncthreads();
      column_sums(W1, nG1, part, nb, sink, tid, T);  // W1 and b1 are contiguous
    }
    pf.store(xs0 + ((i + 1) & 1) * nx, xn, more ? nx : 0, ys0 + ((i + 1) & 1) * ny, yn, more ? ny : 0, tid, T);
    __syncthreads();
  }
  if (a.update)
    for (int j = tid; j < P; j += T) m[j] = W1[j];
  if (tid == 0) put_cost(a, dv, D, acc);
}


inline long long nn_sgd_lds(const NnGeom& d, int nb) {
  return d.P + (long long)nb * (2LL * (d.L + d.C) + 2LL * d.H + d.C + (long long)d.G * d.H + 1);
}

__global__ __launch_bounds__(kGradBlock) void local_sgd_2nn_kernel(SgdArgs a, NnGeom d) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int nb = a.nb, nW1 = d.L * d.H, P = (int)d.P;
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
  const SgdSink sink{a.lr};

  Prefetch pf;
  pf.load(xd, nx, yd, ny, tid, T);
  stage(W1, m, P, tid, T);
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
    // a (slice, h) pair's weights are reloaded from the stepped W1 once per minibatch and serve
    // every sample
    for (int idx = tid; idx < d.G * d.H; idx += T) {
      const int h = idx % d.H, grp = idx / d.H, i0 = grp * kSpan, n = min(kSpan, d.L - i0);
      float w[kSpan];
#pragma unroll
      for (int u = 0; u < kSpan; ++u) w[u] = W1[(i0 + (u < n ? u : 0)) * d.H + h];
      nn_slice_partials<false>(zpart, nb, xs, w, grp, h, nb, d);
    }
    __syncthreads();
    hidden_from_partials(act, zpart, nb, b1, nb, d, tid, T);
    __syncthreads();
    nn_logits(zl, act, W2, b2, nb, d, tid, T);
    __syncthreads();
    softmax_xent<true>(zl, ys, cs, nb, d.C, d.SW, invB, a.update != 0, tid, T);
    __syncthreads();
    if (tid == 0) add_cost(acc, cs, nb, a.steps);
    if (a.update) {
      // the hidden layer's gradient, through the pre-update W2
      relu_layer_backward(dz, act, zl, W2, nb, d.H, d.C, tid, T);
      __syncthreads();
      // every parameter's step by the thread that owns it
      weight_sums<0>(W2, d.H * d.C, d.C, act, d.H, zl, nb, sink, tid, T);
      column_sums(b2, d.C, zl, nb, sink, tid, T);
      weight_sums<4>(W1, nW1, d.H, xs, d.L, dz, nb, sink, tid, T);  // W1 -= lr * x^T dz
      column_sums(b1, d.H, dz, nb, sink, tid, T);
    }
    pf.store(xs0 + ((i + 1) & 1) * nx, xn, more ? nx : 0, ys0 + ((i + 1) & 1) * ny, yn, more ? ny : 0, tid, T);
    __syncthreads();
  }
  if (a.update)
    for (int j = tid; j < P; j += T) m[j] = W1[j];
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

// LDS of a launch: within the default 64 KiB, or the kernel's limit raised to the device's. The
// kernels index the model's P parameters and the LDS with ints.
int sgd_lds(const char* fn, const void* kern, long long P, long long floats, size_t& bytes) {
  if (P > (1 << 20)) return fail(CFA_E_UNSUPPORTED, "%s: a model of %lld parameters does not fit the LDS", fn, P);
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
  CnnGeom d;
  if (int rc = cnn_geom(fn, L, classes, filter, number, stride, d)) return rc;
  SgdArgs a;
  if (int rc = sgd_args(fn, x, y, Ns, models, pitch, D, batch_stride, batch_rows, steps, lr, update, cost, cost_log,
                        log_cap, epoch, d.P, a))
    return rc;
  if (D == 0) return CFA_OK;
  const bool fast = cnn_fast(d);
  const void* kern = fast ? (const void*)local_sgd_cnn_kernel<16, 5> : (const void*)local_sgd_cnn_kernel<0, 0>;
  size_t bytes = 0;
  if (int rc = sgd_lds(fn, kern, d.P, cnn_sgd_lds(d, batch_rows), bytes)) return rc;
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
  NnGeom d;
  if (int rc = nn_geom(fn, L, hidden, classes, d)) return rc;
  SgdArgs a;
  if (int rc = sgd_args(fn, x, y, Ns, models, pitch, D, batch_stride, batch_rows, steps, lr, update, cost, cost_log,
                        log_cap, epoch, d.P, a))
    return rc;
  if (D == 0) return CFA_OK;
  size_t bytes = 0;
  if (int rc = sgd_lds(fn, (const void*)local_sgd_2nn_kernel, d.P, nn_sgd_lds(d, batch_rows), bytes)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  local_sgd_2nn_kernel<<<(unsigned)D, kGradBlock, bytes, st>>>(a, d);
  return sgd_finish("local_sgd_2nn_kernel", a, epoch, st);
}

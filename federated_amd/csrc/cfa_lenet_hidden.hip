// cfa_lenet_hidden.hip — the validation pass and the minibatch gradient of a TF2 population whose
// model is the CIFAR drivers' hidden-layer LeNet
// (federated_learning_keras_consensus_FL_threads_CIFAR_crossentropy.py:179-186, -modelselection 1:
// x [32, 32, 3] -> Conv2D(4, 5 x 5, relu) -> AveragePooling2D -> Conv2D(8, 5 x 5, relu) ->
// AveragePooling2D -> Flatten -> Dense(128, relu) -> Dense(10, softmax); 28 130 parameters), on the
// phases of cfa_lenet_graph.h: the conv / pool phases with cin = channels in stage 1, the hidden
// layer's lenet_hidden_forward / lenet_hidden_backward, and lenet_logits / lenet_dense_backward
// with F = hidden. Geometry (seven numbers), row layout (eight tensors), objectives, the order of
// the argument checks and both finishing kernels are the family's.
//
// The plan is cfa_lenet_max.hip's: the MODEL STAYS OUT OF LDS (28 130 parameters are 110 KiB, and
// with the gradient sums 220 KiB). A workgroup reads its device's weights from global memory,
// where a [D, P] stack of these rows stays in L2 / the Infinity Cache; co (the convolutions) and j
// (the hidden layer) are innermost, so a wave's weight load is a coalesced line. LDS holds a
// chunk's activations, their gradients, the gate bytes of both pools, the hidden layer's partial
// sums [S][chunk][W] and one [c1][c2 + 1] tile that carries stage 2's weights into the input
// gradient (lenet_conv_igrad_tiled). The hidden layer's gate is not stored: h > 0 is tested again.
//
// Validation, launch 1, grid (batch groups, D): a workgroup owns whole batches and thread 0 sums a
// batch's losses in sample order. The chunk is the most samples (up to 4) whose state fits 64 KiB
// beside the batch's losses, or 1 sample under the device's limit (the driver geometry: 3 samples,
// 56 872 bytes at batch 100). Launch 2: lenet_finish_kernel.
//
// Gradient, launch 1, grid (sample groups, D): group g owns samples [g * kHidGroup, ...) of the
// batch whatever D, the CU count, skip or src are; its slot workspace[d][g] (global memory) holds
// its gradient sums, each element added sample by sample in order by the one thread that owns it.
// The chunk is the most samples (up to 2) whose state fits 64 KiB, or 1 under the device's limit
// (the driver geometry: 2 samples, 55 176 bytes, which leaves room for two workgroups a CU). A
// sample's sums are its own, so the chunk moves no bit. Launch 2: lenet_grad_finish_kernel adds the
// groups in order. No atomics; a device's row has the same bits alone or in a population, and the
// gradient call's loss is the validation call's batch loss bit for bit (same phases, same block).
#include "cfa_lenet_graph.h"

namespace {

constexpr int kHidBlock = 512;     // 8 waves: the weights come from L2; the hidden layer's plan is for this T
constexpr int kHidEvalChunk = 4;   // most samples per pass through the forward phases
constexpr int kHidGradChunk = 2;   // most samples per pass through forward and backward
constexpr int kHidGroup = 8;       // samples per workgroup of the gradient kernel
constexpr long long kLdsDefault = 65536;

// LDS floats one sample's forward pass needs: the image, the two pooled maps, h and the logits.
inline long long lenet_hidden_sample_floats(const LenetHiddenGeom& g) {
  return (long long)g.side * g.side * g.cin + (long long)g.p1 * g.p1 * g.c1 + g.flat + g.H + g.C;
}

// LDS floats of the evaluation kernel for a chunk of n samples: their activations, the hidden
// layer's partial sums, a batch's losses.
inline long long lenet_hidden_eval_lds(const LenetHiddenGeom& g, int n, int batch) {
  return (long long)n * lenet_hidden_sample_floats(g) + lenet_hidden_part_floats(g.H, kHidBlock, n) + batch;
}

// The chunk of the evaluation kernel (0: one sample's state does not fit `limit` bytes).
inline int lenet_hidden_eval_chunk(const LenetHiddenGeom& g, int batch, long long limit) {
  for (int n = kHidEvalChunk; n >= 1; --n)
    if (4 * lenet_hidden_eval_lds(g, n, batch) <= kLdsDefault) return n;
  return 4 * lenet_hidden_eval_lds(g, 1, batch) <= limit ? 1 : 0;
}

// K: the kernel side at compile time, or 0; LOSS: the objective (CFA_LENET_LOSS_*).
template <int K, int LOSS>
__global__ __launch_bounds__(kHidBlock) void lenet_hidden_eval_kernel(LenetArgs a, LenetHiddenGeom g, int chunk) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int dv = blockIdx.y;
  if (a.skip && a.skip[dv]) return;  // the whole workgroup: the device has left its loop
  const int tid = threadIdx.x, T = blockDim.x;
  const int nx = g.side * g.side * g.cin, n1 = g.p1 * g.p1 * g.c1;
  float* xs = lds;                    // [chunk][side][side][cin]
  float* a1 = xs + chunk * nx;        // [chunk][p1][p1][c1]
  float* a2 = a1 + chunk * n1;        // [chunk][flat]
  float* hh = a2 + chunk * g.flat;    // [chunk][H]
  float* zl = hh + chunk * g.H;       // [chunk][C]
  float* part = zl + chunk * g.C;     // [S][chunk][W]
  float* loss = part + lenet_hidden_slices(g.H, T) * chunk * lenet_hidden_cols(g.H, T);  // [batch]
  const float* m = a.models + (long long)dv * a.pitch;  // global: read through L2
  const float* xd = a.x + (long long)dv * a.x_stride;
  const int32_t* ld = a.labels + (long long)dv * a.label_stride;
  for (int b = blockIdx.x; b < a.batches; b += gridDim.x) {
    const long long first = (long long)b * a.batch;
    for (int s0 = 0; s0 < a.batch; s0 += chunk) {
      const int ns = min(chunk, a.batch - s0);
      // the previous chunk's last read of xs was its first phase, several barriers ago
      stage(xs, xd + (first + s0) * nx, ns * nx, tid, T);
      __syncthreads();
      lenet_conv_pool<K>(a1, xs, m + g.oK1, m + g.ob1, ns, g.side, g.cin, g.c1, g.k, g.p1, tid, T);
      __syncthreads();
      lenet_conv_pool<K>(a2, a1, m + g.oK2, m + g.ob2, ns, g.p1, g.c1, g.c2, g.k, g.p2, tid, T);
      __syncthreads();
      lenet_hidden_forward<kHidEvalChunk>(hh, a2, m + g.oWh, m + g.obh, part, ns, g.flat, g.H, tid, T);
      lenet_logits(zl, hh, m + g.oWd, m + g.obd, ns, g.H, g.C, tid, T);
      __syncthreads();
      lenet_loss<LOSS>(loss + s0, zl, ld + first + s0, ns, g.C, tid, T);
    }
    __syncthreads();
    if (tid == 0) {  // reduce_mean over the batch, fp32, in sample order
      float c = 0.f;
      for (int s = 0; s < a.batch; ++s) c += loss[s];
      a.ws[(long long)dv * a.batches + b] = c / (float)a.batch;
    }
    // the next batch writes loss only after several more barriers
  }
}

// LDS floats of the gradient kernel for a chunk of n samples: image, both pooled maps and their
// gradients, h and its gradient, logits and theirs, stage 2's gated map; the hidden layer's
// partial sums; the weight tile; a group's losses; the chunk's labels; the gate bytes.
inline long long lenet_hidden_grad_lds(const LenetHiddenGeom& g, int n) {
  const long long n1 = (long long)g.p1 * g.p1 * g.c1, d2 = 4LL * g.p2 * g.p2 * g.c2;
  const long long sample = (long long)g.side * g.side * g.cin + 2 * n1 + 2 * g.flat + 2 * g.H + 2 * g.C + d2;
  return n * sample + lenet_hidden_part_floats(g.H, kHidBlock, n) + (long long)g.c1 * (g.c2 + 1) + kHidGroup + n +
         (n * (n1 + g.flat) + 3) / 4;
}

// The chunk of the gradient kernel (0: one sample's state does not fit `limit` bytes).
inline int lenet_hidden_grad_chunk(const LenetHiddenGeom& g, long long limit) {
  for (int n = kHidGradChunk; n >= 1; --n)
    if (4 * lenet_hidden_grad_lds(g, n) <= kLdsDefault) return n;
  return 4 * lenet_hidden_grad_lds(g, 1) <= limit ? 1 : 0;
}

template <int K, int LOSS>
__global__ __launch_bounds__(kHidBlock) void lenet_hidden_grad_kernel(LenetGradArgs a, LenetHiddenGeom g, int chunk) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int dv = blockIdx.y;
  if (a.skip && a.skip[dv]) return;  // the whole workgroup
  const int tid = threadIdx.x, T = blockDim.x;
  const int P = (int)g.P, nx = g.side * g.side * g.cin, n1 = g.p1 * g.p1 * g.c1, s2 = 2 * g.p2;
  const int nd2 = s2 * s2 * g.c2;
  float* xs = lds;                          // [chunk][side][side][cin]
  float* a1 = xs + chunk * nx;              // [chunk][p1][p1][c1]
  float* da1 = a1 + chunk * n1;             // [chunk][p1][p1][c1]
  float* a2 = da1 + chunk * n1;             // [chunk][flat]
  float* da2 = a2 + chunk * g.flat;         // [chunk][flat] = [chunk][p2][p2][c2]
  float* hh = da2 + chunk * g.flat;         // [chunk][H]
  float* dh = hh + chunk * g.H;             // [chunk][H]
  float* zl = dh + chunk * g.H;             // [chunk][C]
  float* dzl = zl + chunk * g.C;            // [chunk][C]
  float* dz2 = dzl + chunk * g.C;           // [chunk][2 p2][2 p2][c2]
  float* part = dz2 + chunk * nd2;          // [S][chunk][W]
  float* tile = part + lenet_hidden_slices(g.H, T) * chunk * lenet_hidden_cols(g.H, T);  // [c1][c2 + 1]
  float* loss = tile + g.c1 * (g.c2 + 1);   // [group]
  int32_t* lab = reinterpret_cast<int32_t*>(loss + kHidGroup);  // [chunk]
  uint8_t* g1 = reinterpret_cast<uint8_t*>(lab + chunk);        // [chunk][p1][p1][c1]
  uint8_t* g2 = g1 + chunk * n1;                                // [chunk][flat]
  const int grp = blockIdx.x, begin = grp * kHidGroup, count = min(kHidGroup, a.batch - begin);
  float* gs = a.ws + ((long long)dv * a.groups + grp) * (P + kHidGroup);  // [P] the group's sums, then its losses
  const int row = a.src ? a.src[dv] : dv;
  if ((unsigned)row >= (unsigned)a.D) {  // the caller's error: nothing is read, the row becomes NaN
    for (int i = tid; i < P + kHidGroup; i += T) gs[i] = NAN;
    return;
  }
  long long f0 = a.first ? a.first[dv] % a.Nt : 0;
  if (f0 < 0) f0 += a.Nt;
  const float* xd = a.x + (long long)dv * a.x_stride;
  const int32_t* ld = a.labels + (long long)dv * a.label_stride;
  const float* m = a.models + (long long)row * a.pitch;  // global: read through L2
  for (int i = tid; i < P; i += T) gs[i] = 0.f;
  for (int c0 = 0; c0 < count; c0 += chunk) {
    const int ns = min(chunk, count - c0);
    for (int j = 0; j < ns; ++j) {
      const long long sample = (f0 + begin + c0 + j) % a.Nt;  // a batch past the set's end wraps
      stage(xs + j * nx, xd + sample * nx, nx, tid, T);
      if (tid == 0) lab[j] = ld[sample];
    }
    __syncthreads();  // also the sums' zeros, the first time: their owners read them from here on
    lenet_conv_pool<K>(a1, xs, m + g.oK1, m + g.ob1, ns, g.side, g.cin, g.c1, g.k, g.p1, tid, T, g1);
    __syncthreads();
    lenet_conv_pool<K>(a2, a1, m + g.oK2, m + g.ob2, ns, g.p1, g.c1, g.c2, g.k, g.p2, tid, T, g2);
    __syncthreads();
    lenet_hidden_forward<kHidGradChunk>(hh, a2, m + g.oWh, m + g.obh, part, ns, g.flat, g.H, tid, T);
    lenet_logits(zl, hh, m + g.oWd, m + g.obd, ns, g.H, g.C, tid, T);
    __syncthreads();
    lenet_loss<LOSS>(loss + c0, zl, lab, ns, g.C, tid, T, dzl);
    __syncthreads();
    lenet_dense_backward(gs + g.oWd, gs + g.obd, dh, hh, dzl, m + g.oWd, ns, g.H, g.C, tid, T);
    __syncthreads();
    lenet_hidden_backward<kHidGradChunk>(gs + g.oWh, gs + g.obh, da2, dh, hh, a2, m + g.oWh, ns, g.flat, g.H, tid, T);
    __syncthreads();
    lenet_store_gated(dz2, LenetGated{g2, da2, g.p2, g.c2}, ns, tid, T);
    __syncthreads();
    for (int j = 0; j < ns; ++j) {  // a sample at a time: the sums do not depend on the chunk
      const LenetStored d2{dz2 + j * nd2, s2, g.c2};
      lenet_conv_wgrad<K>(gs + g.oK2, a1 + j * n1, d2, 1, g.p1, g.c1, g.c2, g.k, g.p2, tid, T);
      lenet_conv_bgrad(gs + g.ob2, d2, 1, g.c2, g.p2, tid, T);
    }
    lenet_conv_igrad_tiled(da1, dz2, m + g.oK2, tile, ns, g.p1, g.c1, g.c2, g.k, g.p2, tid, T);
    __syncthreads();
    for (int j = 0; j < ns; ++j) {  // stage 1 with cin channels; its input gradient is not needed
      const LenetGated d1{g1 + j * n1, da1 + j * n1, g.p1, g.c1};
      lenet_conv_wgrad<K>(gs + g.oK1, xs + j * nx, d1, 1, g.side, g.cin, g.c1, g.k, g.p1, tid, T);
      lenet_conv_bgrad(gs + g.ob1, d1, 1, g.c1, g.p1, tid, T);
    }
    __syncthreads();  // the next chunk's images replace the ones just read
  }
  for (int i = tid; i < kHidGroup; i += T) gs[P + i] = i < count ? loss[i] : 0.f;
}

inline int lenet_hidden_groups(int batch) { return (batch + kHidGroup - 1) / kHidGroup; }

using LenetHiddenEvalKernel = void (*)(LenetArgs, LenetHiddenGeom, int);
using LenetHiddenGradKernel = void (*)(LenetGradArgs, LenetHiddenGeom, int);

// The kernel table below: 2 passes x 2 kernel sides x 2 objectives. Every one needs a slot of
// raise_lds_limit, or a launch above 64 KiB would call the runtime under capture: another
// compile-time side or objective has to raise kLdsLimitSlots with it.
static_assert(2 * 2 * 2 <= kLdsLimitSlots, "every instantiated kernel needs a raise_lds_limit slot");

// The kernel side the kernels are instantiated for: the drivers' 5, every other one 0.
inline bool lenet_hidden_fast(const LenetHiddenGeom& g) { return g.k == 5; }

inline LenetHiddenEvalKernel lenet_hidden_eval_kernel_for(bool fast, int loss) {
  if (loss == CFA_LENET_LOSS_HUBER)
    return fast ? lenet_hidden_eval_kernel<5, CFA_LENET_LOSS_HUBER> : lenet_hidden_eval_kernel<0, CFA_LENET_LOSS_HUBER>;
  return fast ? lenet_hidden_eval_kernel<5, CFA_LENET_LOSS_XENT> : lenet_hidden_eval_kernel<0, CFA_LENET_LOSS_XENT>;
}

inline LenetHiddenGradKernel lenet_hidden_grad_kernel_for(bool fast, int loss) {
  if (loss == CFA_LENET_LOSS_HUBER)
    return fast ? lenet_hidden_grad_kernel<5, CFA_LENET_LOSS_HUBER> : lenet_hidden_grad_kernel<0, CFA_LENET_LOSS_HUBER>;
  return fast ? lenet_hidden_grad_kernel<5, CFA_LENET_LOSS_XENT> : lenet_hidden_grad_kernel<0, CFA_LENET_LOSS_XENT>;
}

// The seven-number family's verdict text for a refusal.
inline void lenet_hidden_geom_text(char (&text)[192], int side, int channels, int kernel, int c1, int c2, int hidden,
                                   int classes) {
  snprintf(text, sizeof text, "(side %d channels %d kernel %d c1 %d c2 %d hidden %d classes %d): every dimension >= 1 "
           "and a second pooled map of at least 1 x 1", side, channels, kernel, c1, c2, hidden, classes);
}

}  // namespace

// Current device: raise the hidden-layer kernels' dynamic-LDS limit now (lenet_prepare_device), so
// later launches (e.g. under hipGraph capture) need no attribute call.
int lenet_hidden_prepare_device() {
  const int lim = device_lds_max();
  if (lim <= kLdsDefault) return CFA_OK;
  for (int loss : {CFA_LENET_LOSS_XENT, CFA_LENET_LOSS_HUBER})
    for (bool fast : {true, false}) {  // refused: launches stay within 64 KiB
      (void)raise_lds_limit((const void*)lenet_hidden_eval_kernel_for(fast, loss), lim);
      (void)raise_lds_limit((const void*)lenet_hidden_grad_kernel_for(fast, loss), lim);
    }
  return CFA_OK;
}

extern "C" size_t cfa_lenet_hidden_params(int side, int channels, int kernel, int c1, int c2, int hidden,
                                          int classes) {
  LenetHiddenGeom g;
  return lenet_hidden_geom(side, channels, kernel, c1, c2, hidden, classes, g) ? (size_t)g.P : 0;
}

extern "C" size_t cfa_lenet_hidden_eval_workspace_bytes(int D, int batches) {
  return D < 1 || batches < 1 ? 0 : (size_t)D * (size_t)batches * sizeof(float);
}

extern "C" int cfa_lenet_hidden_eval_loss_f32(const float* x, size_t x_dev_stride, const int32_t* labels,
                                              size_t label_dev_stride, int Nt, int side, int channels, int kernel,
                                              int c1, int c2, int hidden, int classes, const float* models,
                                              size_t pitch, int D, int batch, int batches, const int32_t* skip,
                                              double target, int32_t* ended, double* cost, double* cost_log,
                                              int log_cap, unsigned long long* epoch, void* workspace,
                                              size_t workspace_bytes, int loss, void* stream) {
  const char* fn = "cfa_lenet_hidden_eval_loss_f32";
  LenetHiddenGeom g;
  char text[192];
  lenet_hidden_geom_text(text, side, channels, kernel, c1, c2, hidden, classes);
  const bool ok = lenet_hidden_geom(side, channels, kernel, c1, c2, hidden, classes, g);
  if (int rc = lenet_eval_checks_for(fn, x, labels, x_dev_stride, label_dev_stride, Nt, ok, text, ok ? g.P : 0,
                                     (long long)side * side * channels, classes, models, pitch, D, batch, batches,
                                     target, ended, cost, cost_log, log_cap, epoch, workspace, workspace_bytes,
                                     cfa_lenet_hidden_eval_workspace_bytes(D, batches), loss))
    return rc;
  // the kernel indexes the model and the LDS with ints
  const LenetHiddenEvalKernel kern = lenet_hidden_eval_kernel_for(lenet_hidden_fast(g), loss);
  const long long limit = device_lds_max();
  const int chunk = g.P > 0x7fffffffLL ? 0 : lenet_hidden_eval_chunk(g, batch, limit);
  const long long need = chunk ? 4 * lenet_hidden_eval_lds(g, chunk, batch) : -1;
  if (need < 0 || (need > kLdsDefault && !raise_lds_limit((const void*)kern, (int)limit)))
    return fail(CFA_E_UNSUPPORTED, "%s: one sample's activations (%lld floats) and a batch of %d losses do not fit "
                "one workgroup's LDS", fn, lenet_hidden_sample_floats(g), batch);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LenetArgs a{x, labels, (long long)x_dev_stride, (long long)label_dev_stride, models, (long long)pitch,
                    batch, batches, skip, static_cast<float*>(workspace)};
  // about two workgroups per CU over all devices (what a 64 KiB chunk leaves room for), and every
  // batch group the same number of batches (but the last)
  const int gx = (int)shared_grid_x(batches, 2, D), per = (batches + gx - 1) / gx;
  const dim3 grid((unsigned)((batches + per - 1) / per), (unsigned)D);
  kern<<<grid, kHidBlock, (size_t)need, st>>>(a, g, chunk);
  if (int rc = check_launch("lenet_hidden_eval_kernel")) return rc;
  const LenetFinish f{a.ws, D, batches, skip, target, ended, cost, cost_log, log_cap, epoch};
  lenet_finish_kernel<<<1, kLenetFinishBlock, 0, st>>>(f);
  return check_launch("lenet_finish_kernel");
}

extern "C" size_t cfa_lenet_hidden_grad_workspace_bytes(int D, int batch, int side, int channels, int kernel, int c1,
                                                        int c2, int hidden, int classes) {
  LenetHiddenGeom g;
  if (D < 1 || batch < 1 || !lenet_hidden_geom(side, channels, kernel, c1, c2, hidden, classes, g)) return 0;
  return (size_t)D * (size_t)lenet_hidden_groups(batch) * (size_t)(g.P + kHidGroup) * sizeof(float);
}

extern "C" int cfa_lenet_hidden_grad_loss_f32(const float* x, size_t x_dev_stride, const int32_t* labels,
                                              size_t label_dev_stride, int Nt, int side, int channels, int kernel,
                                              int c1, int c2, int hidden, int classes, const float* models,
                                              size_t pitch, int D, const int32_t* src, const long long* first,
                                              int batch, const int32_t* skip, float* grads, size_t gpitch,
                                              float* loss, void* workspace, size_t workspace_bytes, int loss_kind,
                                              void* stream) {
  const char* fn = "cfa_lenet_hidden_grad_loss_f32";
  LenetHiddenGeom g;
  char text[192];
  lenet_hidden_geom_text(text, side, channels, kernel, c1, c2, hidden, classes);
  const bool ok = lenet_hidden_geom(side, channels, kernel, c1, c2, hidden, classes, g);
  if (int rc = lenet_grad_checks_for(fn, x, labels, x_dev_stride, label_dev_stride, Nt, ok, text, ok ? g.P : 0,
                                     (long long)side * side * channels, classes, models, pitch, D, batch, grads,
                                     gpitch, workspace, loss_kind))
    return rc;
  // the kernel indexes the model and the LDS with ints
  const LenetHiddenGradKernel kern = lenet_hidden_grad_kernel_for(lenet_hidden_fast(g), loss_kind);
  const long long limit = device_lds_max();
  const int chunk = g.P > 0x7fffffffLL ? 0 : lenet_hidden_grad_chunk(g, limit);
  const long long need = chunk ? 4 * lenet_hidden_grad_lds(g, chunk) : -1;
  if (need < 0 || (need > kLdsDefault && !raise_lds_limit((const void*)kern, (int)limit)))
    return fail(CFA_E_UNSUPPORTED, "%s: one sample's activations and their gradients (%lld bytes) do not fit one "
                "workgroup's LDS", fn, g.P > 0x7fffffffLL ? -1LL : 4 * lenet_hidden_grad_lds(g, 1));
  const size_t ws_need =
      cfa_lenet_hidden_grad_workspace_bytes(D, batch, side, channels, kernel, c1, c2, hidden, classes);
  if (workspace_bytes < ws_need)
    return fail(CFA_E_INVALID, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, ws_need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int groups = lenet_hidden_groups(batch);
  const LenetGradArgs a{x, labels, (long long)x_dev_stride, (long long)label_dev_stride, models, (long long)pitch,
                        src, first, skip, Nt, batch, D, groups, static_cast<float*>(workspace)};
  const dim3 grid((unsigned)groups, (unsigned)D);
  kern<<<grid, kHidBlock, (size_t)need, st>>>(a, g, chunk);
  if (int rc = check_launch("lenet_hidden_grad_kernel")) return rc;
  const LenetGradFinish f{a.ws, (int)g.P, groups, batch, skip, grads, (long long)gpitch, loss};
  const dim3 fgrid((unsigned)((g.P + 1 + kLenetFinishBlock - 1) / kLenetFinishBlock), (unsigned)D);
  lenet_grad_finish_kernel<kHidGroup><<<fgrid, kLenetFinishBlock, 0, st>>>(f);
  return check_launch("lenet_grad_finish_kernel");
}

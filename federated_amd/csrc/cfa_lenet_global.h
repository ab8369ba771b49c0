// cfa_lenet_global.h — the plan with the MODEL IN GLOBAL MEMORY, written once for the families
// whose model does not fit LDS beside a sample's state (cfa_lenet_max.hip: the max-pool CNNs;
// cfa_lenet_hidden.hip: the CIFAR drivers' hidden-layer LeNet): the validation kernel, the gradient
// kernel, their LDS sizes, chunks and launches, on the phases of cfa_lenet_graph.h. A family is a
// struct of compile-time traits (see LenetMaxFamily); nothing here branches on it at run time.
//   Pool, Gated   the pool policy and its gated gradient (LenetAvgPool / LenetGated, LenetMaxPool / LenetMaxGated)
//   hidden        whether Dense(H, relu) stands between Flatten and the output layer
//   channels      whether stage 1 reads g.cin input channels (false: one, known at compile time)
//   side          the kernel side the fast kernels are instantiated for; every other side runs K = 0
//   grad_chunk_fills_device   the gradient chunk's rule, see lenet_global_grad_chunk
//   eval_name, grad_name      the kernels' names in a launch error
// One translation unit per family: each instantiates 2 passes x 2 sides x 2 objectives, and
// raise_lds_limit remembers kLdsLimitSlots kernels per translation unit.
//
// A workgroup reads its device's weights from global memory, where a [D, P] stack of these rows
// stays in L2 / the Infinity Cache; co (the convolutions) and j (the hidden layer) are innermost, so
// a wave's weight load is one coalesced line that serves the window's four positions (and, at a
// compile-time side, the inputs under a window are read once for all taps). LDS holds a chunk's
// activations, their gradients, the pool decisions (a byte per pooled element), the hidden layer's
// partial sums [S][chunk][W] where there is one, and one [c1][c2 + 1] tile that carries stage 2's
// weights, tap by tap, into the input gradient (lenet_conv_igrad_tiled), where they are read across
// ci. The hidden layer's gate is not stored: h > 0 is tested again.
//
// Validation, launch 1, grid (batch groups, D): as cfa_lenet.hip, a workgroup owns whole batches
// and thread 0 sums a batch's losses in sample order. The chunk is the most samples (up to 4)
// whose activations fit 64 KiB beside the batch's losses, or 1 sample under the device's limit; a
// sample's arithmetic is its own, so the chunk moves no bit. Launch 2: lenet_finish_kernel.
//
// Gradient, launch 1, grid (sample groups, D): group g owns samples [g * kGlobalGroup, ...) of the
// batch whatever D, the CU count, skip or src are, and its slot workspace[d][g] (global memory)
// holds its gradient sums: the slot starts at 0 and every sample adds its own sums to it, sample
// by sample in order, each element by the one thread that owns it. A sample's weight-gradient
// sums are lenet_conv_wgrad's and lenet_conv_bgrad's over that sample's rows alone, so the chunk
// (up to 2 samples) moves no bit either: it only lets samples share a phase, a barrier and a copy
// of a weight tile. Launch 2: lenet_grad_finish_kernel adds the groups in order. No atomics; a
// device's row has the same bits alone or in a population, and the gradient call's loss is the
// validation call's batch loss bit for bit (same phases, same block).
#pragma once
#include "cfa_lenet_graph.h"

namespace {

constexpr int kGlobalBlock = 512;     // 8 waves: the weights come from L2, and LDS leaves one or two workgroups a CU
constexpr int kGlobalEvalChunk = 4;   // most samples per pass through the forward phases
constexpr int kGlobalGradChunk = 2;   // most samples per pass through forward and backward
constexpr int kGlobalGroup = 8;       // samples per workgroup of the gradient kernel
constexpr long long kLdsDefault = 65536;

// A family's kernel table: 2 passes x 2 kernel sides x 2 objectives. Every one needs a slot of
// raise_lds_limit, or a launch above 64 KiB would call the runtime under capture: another
// compile-time side or objective has to raise kLdsLimitSlots with it.
static_assert(2 * 2 * 2 <= kLdsLimitSlots, "every instantiated kernel needs a raise_lds_limit slot");

// LDS floats of the evaluation kernel for a chunk of n samples: their activations, the hidden
// layer's partial sums, a batch's losses.
template <class Family>
inline long long lenet_global_eval_lds(const LenetGeom& g, int n, int batch) {
  const long long part = Family::hidden ? lenet_hidden_part_floats(g.H, kGlobalBlock, n) : 0;
  return (long long)n * lenet_sample_floats(g) + part + batch;
}

// The chunk of the evaluation kernel (0: one sample's state does not fit `limit` bytes).
template <class Family>
inline int lenet_global_eval_chunk(const LenetGeom& g, int batch, long long limit) {
  for (int n = kGlobalEvalChunk; n >= 1; --n)
    if (4 * lenet_global_eval_lds<Family>(g, n, batch) <= kLdsDefault) return n;
  return 4 * lenet_global_eval_lds<Family>(g, 1, batch) <= limit ? 1 : 0;
}

// K: the kernel side at compile time, or 0; LOSS: the objective (CFA_LENET_LOSS_*).
template <class Family, int K, int LOSS>
__global__ __launch_bounds__(kGlobalBlock) void lenet_global_eval_kernel(LenetArgs a, LenetGeom g, int chunk) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int dv = blockIdx.y;
  if (a.skip && a.skip[dv]) return;  // the whole workgroup: the device has left its loop
  const int tid = threadIdx.x, T = blockDim.x;
  const int cin = Family::channels ? g.cin : 1;
  const int nx = g.side * g.side * cin, n1 = g.p1 * g.p1 * g.c1;
  int nh = 0, npart = 0;  // a chunk's h and the hidden layer's partial sums: no floats without one
  if constexpr (Family::hidden) {
    nh = chunk * g.H;
    npart = lenet_hidden_slices(g.H, T) * chunk * lenet_hidden_cols(g.H, T);
  }
  float* xs = lds;                    // [chunk][side][side][cin]
  float* a1 = xs + chunk * nx;        // [chunk][p1][p1][c1]
  float* a2 = a1 + chunk * n1;        // [chunk][flat]
  float* hh = a2 + chunk * g.flat;    // [chunk][H]
  float* zl = hh + nh;                // [chunk][C]
  float* part = zl + chunk * g.C;     // [S][chunk][W]
  float* loss = part + npart;         // [batch]
  const float* m = a.models + (long long)dv * a.pitch;  // global: read through L2
  const float* xd = a.x + (long long)dv * a.x_stride;
  const int32_t* ld = a.labels + (long long)dv * a.label_stride;
  for (int b = blockIdx.x; b < a.batches; b += gridDim.x) {
    const long long first = (long long)b * a.batch;
    for (int s0 = 0; s0 < a.batch; s0 += chunk) {
      const int ns = min(chunk, a.batch - s0);
      // the previous chunk's last read of xs was its first phase, three barriers ago
      stage(xs, xd + (first + s0) * nx, ns * nx, tid, T);
      __syncthreads();
      lenet_conv_pool<K, typename Family::Pool>(a1, xs, m + g.oK1, m + g.ob1, ns, g.side, cin, g.c1, g.k, g.p1, tid, T);
      __syncthreads();
      lenet_conv_pool<K, typename Family::Pool>(a2, a1, m + g.oK2, m + g.ob2, ns, g.p1, g.c1, g.c2, g.k, g.p2, tid, T);
      __syncthreads();
      if constexpr (Family::hidden) {  // ends on a barrier of its own
        lenet_hidden_forward<kGlobalEvalChunk>(hh, a2, m + g.oWh, m + g.obh, part, ns, g.flat, g.H, tid, T);
        lenet_logits(zl, hh, m + g.oWd, m + g.obd, ns, g.H, g.C, tid, T);
      } else {
        lenet_logits(zl, a2, m + g.oWd, m + g.obd, ns, g.flat, g.C, tid, T);
      }
      __syncthreads();
      lenet_loss<LOSS>(loss + s0, zl, ld + first + s0, ns, g.C, tid, T);
    }
    __syncthreads();
    if (tid == 0) {  // reduce_mean over the batch, fp32, in sample order
      float c = 0.f;
      for (int s = 0; s < a.batch; ++s) c += loss[s];
      a.ws[(long long)dv * a.batches + b] = c / (float)a.batch;
    }
    // the next batch writes loss only after four more barriers
  }
}

// LDS floats of the gradient kernel for a chunk of n samples: image, both pooled maps and their
// gradients, h and its gradient, logits and theirs, stage 2's gated map; the hidden layer's
// partial sums; the weight tile; a group's losses; the chunk's labels; the decision bytes.
template <class Family>
inline long long lenet_global_grad_lds(const LenetGeom& g, int n) {
  const long long n1 = (long long)g.p1 * g.p1 * g.c1, d2 = 4LL * g.p2 * g.p2 * g.c2;
  const long long sample = (long long)g.side * g.side * g.cin + 2 * n1 + 2 * g.flat + 2 * g.H + 2 * g.C + d2;
  const long long part = Family::hidden ? lenet_hidden_part_floats(g.H, kGlobalBlock, n) : 0;
  return n * sample + part + (long long)g.c1 * (g.c2 + 1) + kGlobalGroup + n + (n * (n1 + g.flat) + 3) / 4;
}

// The chunk of the gradient kernel (0: one sample's state does not fit `limit` bytes). The two
// families' rules differ, and each keeps its own: where grad_chunk_fills_device, the most samples
// that fit the device's limit (the max-pool drivers' (28, 3, 14, 64, 10): 2 samples, about 121 KB,
// one workgroup a CU); otherwise the most that fit 64 KiB, which leaves room for two workgroups a
// CU, or 1 sample under the device's limit.
template <class Family>
inline int lenet_global_grad_chunk(const LenetGeom& g, long long limit) {
  const long long many = Family::grad_chunk_fills_device ? limit : kLdsDefault;
  for (int n = kGlobalGradChunk; n >= 1; --n)
    if (4 * lenet_global_grad_lds<Family>(g, n) <= many) return n;
  return 4 * lenet_global_grad_lds<Family>(g, 1) <= limit ? 1 : 0;
}

template <class Family, int K, int LOSS>
__global__ __launch_bounds__(kGlobalBlock) void lenet_global_grad_kernel(LenetGradArgs a, LenetGeom g, int chunk) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int dv = blockIdx.y;
  if (a.skip && a.skip[dv]) return;  // the whole workgroup
  const int tid = threadIdx.x, T = blockDim.x;
  const int cin = Family::channels ? g.cin : 1;
  const int P = (int)g.P, nx = g.side * g.side * cin, n1 = g.p1 * g.p1 * g.c1, s2 = 2 * g.p2;
  const int nd2 = s2 * s2 * g.c2;
  int nh = 0, npart = 0;  // a chunk's h and the hidden layer's partial sums: no floats without one
  if constexpr (Family::hidden) {
    nh = chunk * g.H;
    npart = lenet_hidden_slices(g.H, T) * chunk * lenet_hidden_cols(g.H, T);
  }
  float* xs = lds;                          // [chunk][side][side][cin]
  float* a1 = xs + chunk * nx;              // [chunk][p1][p1][c1]
  float* da1 = a1 + chunk * n1;             // [chunk][p1][p1][c1]
  float* a2 = da1 + chunk * n1;             // [chunk][flat]
  float* da2 = a2 + chunk * g.flat;         // [chunk][flat] = [chunk][p2][p2][c2]
  float* hh = da2 + chunk * g.flat;         // [chunk][H]
  float* dh = hh + nh;                      // [chunk][H]
  float* zl = dh + nh;                      // [chunk][C]
  float* dzl = zl + chunk * g.C;            // [chunk][C]
  float* dz2 = dzl + chunk * g.C;           // [chunk][2 p2][2 p2][c2]
  float* part = dz2 + chunk * nd2;          // [S][chunk][W]
  float* tile = part + npart;               // [c1][c2 + 1]
  float* loss = tile + g.c1 * (g.c2 + 1);   // [group]
  int32_t* lab = reinterpret_cast<int32_t*>(loss + kGlobalGroup);  // [chunk]
  uint8_t* g1 = reinterpret_cast<uint8_t*>(lab + chunk);           // [chunk][p1][p1][c1]
  uint8_t* g2 = g1 + chunk * n1;                                   // [chunk][flat]
  const int grp = blockIdx.x, begin = grp * kGlobalGroup, count = min(kGlobalGroup, a.batch - begin);
  float* gs = a.ws + ((long long)dv * a.groups + grp) * (P + kGlobalGroup);  // [P] the group's sums, then its losses
  const int row = a.src ? a.src[dv] : dv;
  if ((unsigned)row >= (unsigned)a.D) {  // the caller's error: nothing is read, the row becomes NaN
    for (int i = tid; i < P + kGlobalGroup; i += T) gs[i] = NAN;
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
    lenet_conv_pool<K, typename Family::Pool>(a1, xs, m + g.oK1, m + g.ob1, ns, g.side, cin, g.c1, g.k, g.p1, tid, T, g1);
    __syncthreads();
    lenet_conv_pool<K, typename Family::Pool>(a2, a1, m + g.oK2, m + g.ob2, ns, g.p1, g.c1, g.c2, g.k, g.p2, tid, T, g2);
    __syncthreads();
    if constexpr (Family::hidden) {  // ends on a barrier of its own
      lenet_hidden_forward<kGlobalGradChunk>(hh, a2, m + g.oWh, m + g.obh, part, ns, g.flat, g.H, tid, T);
      lenet_logits(zl, hh, m + g.oWd, m + g.obd, ns, g.H, g.C, tid, T);
    } else {
      lenet_logits(zl, a2, m + g.oWd, m + g.obd, ns, g.flat, g.C, tid, T);
    }
    __syncthreads();
    lenet_loss<LOSS>(loss + c0, zl, lab, ns, g.C, tid, T, dzl);
    __syncthreads();
    if constexpr (Family::hidden) {
      lenet_dense_backward(gs + g.oWd, gs + g.obd, dh, hh, dzl, m + g.oWd, ns, g.H, g.C, tid, T);
      __syncthreads();
      lenet_hidden_backward<kGlobalGradChunk>(gs + g.oWh, gs + g.obh, da2, dh, hh, a2, m + g.oWh, ns, g.flat, g.H, tid, T);
    } else {
      lenet_dense_backward(gs + g.oWd, gs + g.obd, da2, a2, dzl, m + g.oWd, ns, g.flat, g.C, tid, T);
    }
    __syncthreads();
    lenet_store_gated(dz2, typename Family::Gated{g2, da2, g.p2, g.c2}, ns, tid, T);
    __syncthreads();
    for (int j = 0; j < ns; ++j) {  // a sample at a time: the sums do not depend on the chunk
      const LenetStored d2{dz2 + j * nd2, s2, g.c2};
      lenet_conv_wgrad<K>(gs + g.oK2, a1 + j * n1, d2, 1, g.p1, g.c1, g.c2, g.k, g.p2, tid, T);
      lenet_conv_bgrad(gs + g.ob2, d2, 1, g.c2, g.p2, tid, T);
    }
    lenet_conv_igrad_tiled(da1, dz2, m + g.oK2, tile, ns, g.p1, g.c1, g.c2, g.k, g.p2, tid, T);
    __syncthreads();
    for (int j = 0; j < ns; ++j) {  // stage 1's input gradient is not needed
      const typename Family::Gated d1{g1 + j * n1, da1 + j * n1, g.p1, g.c1};
      lenet_conv_wgrad<K>(gs + g.oK1, xs + j * nx, d1, 1, g.side, cin, g.c1, g.k, g.p1, tid, T);
      lenet_conv_bgrad(gs + g.ob1, d1, 1, g.c1, g.p1, tid, T);
    }
    __syncthreads();  // the next chunk's images replace the ones just read
  }
  for (int i = tid; i < kGlobalGroup; i += T) gs[P + i] = i < count ? loss[i] : 0.f;
}

inline int lenet_global_groups(int batch) { return (batch + kGlobalGroup - 1) / kGlobalGroup; }

inline size_t lenet_global_eval_workspace_bytes(int D, int batches) {
  return D < 1 || batches < 1 ? 0 : (size_t)D * (size_t)batches * sizeof(float);
}

// D >= 1, batch >= 1 and a geometry with a model: the entries answer 0 for anything else.
inline size_t lenet_global_grad_workspace_bytes(const LenetGeom& g, int D, int batch) {
  return (size_t)D * (size_t)lenet_global_groups(batch) * (size_t)(g.P + kGlobalGroup) * sizeof(float);
}

using LenetGlobalEvalKernel = void (*)(LenetArgs, LenetGeom, int);
using LenetGlobalGradKernel = void (*)(LenetGradArgs, LenetGeom, int);

// The family's kernels are instantiated for its drivers' kernel side; every other one runs K = 0.
template <class Family>
inline LenetGlobalEvalKernel lenet_global_eval_kernel_for(bool fast, int loss) {
  constexpr int K = Family::side, X = CFA_LENET_LOSS_XENT, H = CFA_LENET_LOSS_HUBER;
  if (loss == H) return fast ? lenet_global_eval_kernel<Family, K, H> : lenet_global_eval_kernel<Family, 0, H>;
  return fast ? lenet_global_eval_kernel<Family, K, X> : lenet_global_eval_kernel<Family, 0, X>;
}

template <class Family>
inline LenetGlobalGradKernel lenet_global_grad_kernel_for(bool fast, int loss) {
  constexpr int K = Family::side, X = CFA_LENET_LOSS_XENT, H = CFA_LENET_LOSS_HUBER;
  if (loss == H) return fast ? lenet_global_grad_kernel<Family, K, H> : lenet_global_grad_kernel<Family, 0, H>;
  return fast ? lenet_global_grad_kernel<Family, K, X> : lenet_global_grad_kernel<Family, 0, X>;
}

// Current device: raise the family's kernels' dynamic-LDS limit now (lenet_prepare_device), so
// later launches (e.g. under hipGraph capture) need no attribute call.
template <class Family>
int lenet_global_prepare_device() {
  const int lim = device_lds_max();
  if (lim <= kLdsDefault) return CFA_OK;
  for (int loss : {CFA_LENET_LOSS_XENT, CFA_LENET_LOSS_HUBER})
    for (bool fast : {true, false}) {  // refused: launches stay within 64 KiB
      (void)raise_lds_limit((const void*)lenet_global_eval_kernel_for<Family>(fast, loss), lim);
      (void)raise_lds_limit((const void*)lenet_global_grad_kernel_for<Family>(fast, loss), lim);
    }
  return CFA_OK;
}

// An evaluation entry after its argument checks (lenet_eval_checks_for): what fits LDS, then both launches.
template <class Family>
int lenet_global_eval_launch(const char* fn, const LenetGeom& g, const float* x, size_t x_dev_stride,
                             const int32_t* labels, size_t label_dev_stride, const float* models, size_t pitch, int D,
                             int batch, int batches, const int32_t* skip, double target, int32_t* ended, double* cost,
                             double* cost_log, int log_cap, unsigned long long* epoch, void* workspace, int loss,
                             void* stream) {
  // the kernel indexes the model and the LDS with ints
  const LenetGlobalEvalKernel kern = lenet_global_eval_kernel_for<Family>(g.k == Family::side, loss);
  const long long limit = device_lds_max();
  const int chunk = g.P > 0x7fffffffLL ? 0 : lenet_global_eval_chunk<Family>(g, batch, limit);
  const long long need = chunk ? 4 * lenet_global_eval_lds<Family>(g, chunk, batch) : -1;
  if (need < 0 || (need > kLdsDefault && !raise_lds_limit((const void*)kern, (int)limit)))
    return fail(CFA_E_UNSUPPORTED, "%s: one sample's activations (%lld floats) and a batch of %d losses do not fit "
                "one workgroup's LDS", fn, lenet_sample_floats(g), batch);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LenetArgs a{x, labels, (long long)x_dev_stride, (long long)label_dev_stride, models, (long long)pitch,
                    batch, batches, skip, static_cast<float*>(workspace)};
  // about two workgroups per CU over all devices (what a 64 KiB chunk leaves room for), and every
  // batch group the same number of batches (but the last)
  const int gx = (int)shared_grid_x(batches, 2, D), per = (batches + gx - 1) / gx;
  const dim3 grid((unsigned)((batches + per - 1) / per), (unsigned)D);
  kern<<<grid, kGlobalBlock, (size_t)need, st>>>(a, g, chunk);
  if (int rc = check_launch(Family::eval_name)) return rc;
  const LenetFinish f{a.ws, D, batches, skip, target, ended, cost, cost_log, log_cap, epoch};
  lenet_finish_kernel<<<1, kLenetFinishBlock, 0, st>>>(f);
  return check_launch("lenet_finish_kernel");
}

// A gradient entry after its argument checks (lenet_grad_checks_for): what fits LDS, then the
// workspace, then both launches.
template <class Family>
int lenet_global_grad_launch(const char* fn, const LenetGeom& g, const float* x, size_t x_dev_stride,
                             const int32_t* labels, size_t label_dev_stride, int Nt, const float* models, size_t pitch,
                             int D, const int32_t* src, const long long* first, int batch, const int32_t* skip,
                             float* grads, size_t gpitch, float* loss, void* workspace, size_t workspace_bytes,
                             int loss_kind, void* stream) {
  // the kernel indexes the model and the LDS with ints
  const LenetGlobalGradKernel kern = lenet_global_grad_kernel_for<Family>(g.k == Family::side, loss_kind);
  const long long limit = device_lds_max();
  const int chunk = g.P > 0x7fffffffLL ? 0 : lenet_global_grad_chunk<Family>(g, limit);
  const long long need = chunk ? 4 * lenet_global_grad_lds<Family>(g, chunk) : -1;
  if (need < 0 || (need > kLdsDefault && !raise_lds_limit((const void*)kern, (int)limit)))
    return fail(CFA_E_UNSUPPORTED, "%s: one sample's activations and their gradients (%lld bytes) do not fit one "
                "workgroup's LDS", fn, g.P > 0x7fffffffLL ? -1LL : 4 * lenet_global_grad_lds<Family>(g, 1));
  const size_t ws_need = lenet_global_grad_workspace_bytes(g, D, batch);
  if (workspace_bytes < ws_need)
    return fail(CFA_E_INVALID, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, ws_need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int groups = lenet_global_groups(batch);
  const LenetGradArgs a{x, labels, (long long)x_dev_stride, (long long)label_dev_stride, models, (long long)pitch,
                        src, first, skip, Nt, batch, D, groups, static_cast<float*>(workspace)};
  const dim3 grid((unsigned)groups, (unsigned)D);
  kern<<<grid, kGlobalBlock, (size_t)need, st>>>(a, g, chunk);
  if (int rc = check_launch(Family::grad_name)) return rc;
  const LenetGradFinish f{a.ws, (int)g.P, groups, batch, skip, grads, (long long)gpitch, loss};
  const dim3 fgrid((unsigned)((g.P + 1 + kLenetFinishBlock - 1) / kLenetFinishBlock), (unsigned)D);
  lenet_grad_finish_kernel<kGlobalGroup><<<fgrid, kLenetFinishBlock, 0, st>>>(f);
  return check_launch("lenet_grad_finish_kernel");
}

}  // namespace

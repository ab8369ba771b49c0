// cfa_lenet_grad.hip — a minibatch's gradient for every device of a TF2 LeNet-1 population: the
// loss and tape.gradient of a local batch
// (federated_learning_keras_consensus_FL_threads_MNIST_crossentropy_gradients_exchange.py:321-337)
// and of a batch of a device's own data at a neighbour's model (:360-385), on the forward and
// backward phases of cfa_lenet_graph.h. The loss phase is the cross-entropy drivers' or the Huber
// drivers' (federated_learning_keras_consensus_FL_MNIST.py:369-377), a template parameter of the
// kernel; everything behind the gradient at the logits is shared.
//
// Launch 1, grid (sample groups, D): a batch's samples are cut into groups of kGradGroup, group g
// owning samples [g * kGradGroup, ...) of the batch whatever D, the CU count, skip or src are. A
// workgroup stages its model into LDS once and takes its group through forward and backward in
// chunks of kGradChunk samples, adding each chunk's sums to the group's gradient in LDS in a fixed
// order; it leaves the group's gradient and its samples' losses in workspace[d][g]. Launch 2, grid
// (elements, D): a thread per gradient element sums the groups in group order and divides by the
// batch; one more thread sums the losses in sample order and divides as the validation kernel
// does. No atomics; a call is deterministic, and a device's row has the same bits alone or in a
// population.
#include "cfa_lenet_graph.h"

namespace {

constexpr int kGradBlockL = 256;  // 4 waves; three workgroups of LeNet-1 share a CU
constexpr int kGradChunk = 2;     // samples per pass through the phases
constexpr int kGradGroup = 4;     // samples per workgroup: two chunks

// LDS floats of the gradient kernel (the sum is spelled out in cfa_lenet_graph.h).
inline long long lenet_grad_lds(const LenetGeom& g) {
  const long long n1 = (long long)g.p1 * g.p1 * g.c1, d2 = 4LL * g.p2 * g.p2 * g.c2;
  const long long sample = (long long)g.side * g.side + 2 * n1 + 2 * g.flat + 2 * g.C + d2;
  return 2 * g.P + kGradChunk * sample + kGradGroup + kGradChunk + (kGradChunk * (n1 + g.flat) + 3) / 4;
}

// K: the kernel side at compile time, or 0; LOSS: the objective (CFA_LENET_LOSS_*).
template <int K, int LOSS>
__global__ __launch_bounds__(kGradBlockL, 3) void lenet_grad_kernel(LenetGradArgs a, LenetGeom g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int dv = blockIdx.y;
  if (a.skip && a.skip[dv]) return;  // the whole workgroup
  const int tid = threadIdx.x, T = blockDim.x;
  const int P = (int)g.P, nx = g.side * g.side, n1 = g.p1 * g.p1 * g.c1, s2 = 2 * g.p2;
  const int nd2 = s2 * s2 * g.c2;
  float* m = lds;                          // [P]
  float* gs = m + P;                       // [P] the group's gradient sums
  float* xs = gs + P;                      // [chunk][side][side]
  float* a1 = xs + kGradChunk * nx;        // [chunk][p1][p1][c1]
  float* da1 = a1 + kGradChunk * n1;       // [chunk][p1][p1][c1]
  float* a2 = da1 + kGradChunk * n1;       // [chunk][flat]
  float* da2 = a2 + kGradChunk * g.flat;   // [chunk][flat] = [chunk][p2][p2][c2]
  float* zl = da2 + kGradChunk * g.flat;   // [chunk][C]
  float* dzl = zl + kGradChunk * g.C;      // [chunk][C]
  float* dz2 = dzl + kGradChunk * g.C;     // [chunk][2 p2][2 p2][c2]
  float* loss = dz2 + kGradChunk * nd2;    // [group]
  int32_t* lab = reinterpret_cast<int32_t*>(loss + kGradGroup);  // [chunk]
  uint8_t* g1 = reinterpret_cast<uint8_t*>(lab + kGradChunk);    // [chunk][p1][p1][c1]
  uint8_t* g2 = g1 + kGradChunk * n1;                            // [chunk][flat]
  const int grp = blockIdx.x, begin = grp * kGradGroup, count = min(kGradGroup, a.batch - begin);
  float* out = a.ws + ((long long)dv * a.groups + grp) * (P + kGradGroup);
  const int row = a.src ? a.src[dv] : dv;
  if ((unsigned)row >= (unsigned)a.D) {  // the caller's error: nothing is read, the row becomes NaN
    for (int i = tid; i < P + kGradGroup; i += T) out[i] = NAN;
    return;
  }
  long long f0 = a.first ? a.first[dv] % a.Nt : 0;
  if (f0 < 0) f0 += a.Nt;
  const float* xd = a.x + (long long)dv * a.x_stride;
  const int32_t* ld = a.labels + (long long)dv * a.label_stride;
  stage(m, a.models + (long long)row * a.pitch, P, tid, T);
  for (int i = tid; i < P; i += T) gs[i] = 0.f;
  for (int c0 = 0; c0 < count; c0 += kGradChunk) {
    const int ns = min(kGradChunk, count - c0);
    for (int j = 0; j < ns; ++j) {
      const long long sample = (f0 + begin + c0 + j) % a.Nt;  // a batch past the set's end wraps
      stage(xs + j * nx, xd + sample * nx, nx, tid, T);
      if (tid == 0) lab[j] = ld[sample];
    }
    __syncthreads();  // also the model's and the sums', the first time
    lenet_conv_pool<K>(a1, xs, m + g.oK1, m + g.ob1, ns, g.side, 1, g.c1, g.k, g.p1, tid, T, g1);
    __syncthreads();
    lenet_conv_pool<K>(a2, a1, m + g.oK2, m + g.ob2, ns, g.p1, g.c1, g.c2, g.k, g.p2, tid, T, g2);
    __syncthreads();
    lenet_logits(zl, a2, m + g.oWd, m + g.obd, ns, g.flat, g.C, tid, T);
    __syncthreads();
    lenet_loss<LOSS>(loss + c0, zl, lab, ns, g.C, tid, T, dzl);
    __syncthreads();
    lenet_dense_backward(gs + g.oWd, gs + g.obd, da2, a2, dzl, m + g.oWd, ns, g.flat, g.C, tid, T);
    __syncthreads();
    lenet_store_gated(dz2, LenetGated{g2, da2, g.p2, g.c2}, ns, tid, T);
    __syncthreads();
    const LenetStored d2{dz2, s2, g.c2};
    lenet_conv_wgrad<K>(gs + g.oK2, a1, d2, ns, g.p1, g.c1, g.c2, g.k, g.p2, tid, T);
    lenet_conv_bgrad(gs + g.ob2, d2, ns, g.c2, g.p2, tid, T);
    lenet_conv_igrad(da1, dz2, m + g.oK2, ns, g.p1, g.c1, g.c2, g.k, g.p2, tid, T);
    __syncthreads();
    const LenetGated d1{g1, da1, g.p1, g.c1};
    lenet_conv_wgrad<K>(gs + g.oK1, xs, d1, ns, g.side, 1, g.c1, g.k, g.p1, tid, T);
    lenet_conv_bgrad(gs + g.ob1, d1, ns, g.c1, g.p1, tid, T);
    __syncthreads();  // the next chunk's images replace the ones just read
  }
  for (int i = tid; i < P; i += T) out[i] = gs[i];
  for (int i = tid; i < kGradGroup; i += T) out[P + i] = i < count ? loss[i] : 0.f;
}

inline int lenet_grad_groups(int batch) { return (batch + kGradGroup - 1) / kGradGroup; }

using LenetGradKernel = void (*)(LenetGradArgs, LenetGeom);

// The instantiation for a geometry and an objective (a valid CFA_LENET_LOSS_*).
inline LenetGradKernel lenet_grad_kernel_for(bool fast, int loss) {
  if (loss == CFA_LENET_LOSS_HUBER)
    return fast ? lenet_grad_kernel<5, CFA_LENET_LOSS_HUBER> : lenet_grad_kernel<0, CFA_LENET_LOSS_HUBER>;
  return fast ? lenet_grad_kernel<5, CFA_LENET_LOSS_XENT> : lenet_grad_kernel<0, CFA_LENET_LOSS_XENT>;
}

}  // namespace

// Current device: raise the gradient kernels' dynamic-LDS limit now (lenet_prepare_device).
int lenet_grad_prepare_device() {
  const int lim = device_lds_max();
  if (lim <= 65536) return CFA_OK;
  for (int loss : {CFA_LENET_LOSS_XENT, CFA_LENET_LOSS_HUBER})
    for (bool fast : {true, false})  // refused: launches stay within 64 KiB
      (void)raise_lds_limit((const void*)lenet_grad_kernel_for(fast, loss), lim);
  return CFA_OK;
}

extern "C" size_t cfa_lenet_grad_workspace_bytes(int D, int batch, int side, int kernel, int c1, int c2, int classes) {
  LenetGeom g;
  if (D < 1 || batch < 1 || !lenet_geom(side, kernel, c1, c2, classes, g)) return 0;
  return (size_t)D * (size_t)lenet_grad_groups(batch) * (size_t)(g.P + kGradGroup) * sizeof(float);
}

extern "C" int cfa_lenet_grad_f32(const float* x, size_t x_dev_stride, const int32_t* labels, size_t label_dev_stride,
                                  int Nt, int side, int kernel, int c1, int c2, int classes, const float* models,
                                  size_t pitch, int D, const int32_t* src, const long long* first, int batch,
                                  const int32_t* skip, float* grads, size_t gpitch, float* loss, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  return cfa_lenet_grad_loss_f32(x, x_dev_stride, labels, label_dev_stride, Nt, side, kernel, c1, c2, classes, models,
                                 pitch, D, src, first, batch, skip, grads, gpitch, loss, workspace, workspace_bytes,
                                 CFA_LENET_LOSS_XENT, stream);
}

extern "C" int cfa_lenet_grad_loss_f32(const float* x, size_t x_dev_stride, const int32_t* labels,
                                       size_t label_dev_stride, int Nt, int side, int kernel, int c1, int c2,
                                       int classes, const float* models, size_t pitch, int D, const int32_t* src,
                                       const long long* first, int batch, const int32_t* skip, float* grads,
                                       size_t gpitch, float* loss, void* workspace, size_t workspace_bytes,
                                       int loss_kind, void* stream) {
  // the messages keep the name callers of either entry know
  const char* fn = loss_kind == CFA_LENET_LOSS_XENT ? "cfa_lenet_grad_f32" : "cfa_lenet_grad_loss_f32";
  LenetGeom g;
  if (int rc = lenet_grad_checks(fn, x, labels, x_dev_stride, label_dev_stride, Nt, side, kernel, c1, c2, classes, models,
                                 pitch, D, batch, grads, gpitch, workspace, loss_kind, g))
    return rc;
  // the kernel indexes the model and the LDS with ints
  const bool fast = g.k == 5;
  const LenetGradKernel kern = lenet_grad_kernel_for(fast, loss_kind);
  const long long need = g.P > (1 << 20) ? -1 : 4 * lenet_grad_lds(g), limit = device_lds_max();
  if (need < 0 || need > limit || (need > 65536 && !raise_lds_limit((const void*)kern, (int)limit)))
    return fail(CFA_E_UNSUPPORTED, "%s: a model of %lld parameters, its gradient and %d samples' activations do not "
                "fit one workgroup's LDS", fn, g.P, kGradChunk);
  const size_t ws_need = cfa_lenet_grad_workspace_bytes(D, batch, side, kernel, c1, c2, classes);
  if (workspace_bytes < ws_need)
    return fail(CFA_E_INVALID, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, ws_need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int groups = lenet_grad_groups(batch);
  const LenetGradArgs a{x, labels, (long long)x_dev_stride, (long long)label_dev_stride, models, (long long)pitch,
                        src, first, skip, Nt, batch, D, groups, static_cast<float*>(workspace)};
  const dim3 grid((unsigned)groups, (unsigned)D);
  kern<<<grid, kGradBlockL, (size_t)need, st>>>(a, g);
  if (int rc = check_launch("lenet_grad_kernel")) return rc;
  const LenetGradFinish f{a.ws, (int)g.P, groups, batch, skip, grads, (long long)gpitch, loss};
  const dim3 fgrid((unsigned)((g.P + 1 + kLenetFinishBlock - 1) / kLenetFinishBlock), (unsigned)D);
  lenet_grad_finish_kernel<kGradGroup><<<fgrid, kLenetFinishBlock, 0, st>>>(f);
  return check_launch("lenet_grad_finish_kernel");
}

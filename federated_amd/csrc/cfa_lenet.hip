// cfa_lenet.hip — the validation pass of a TF2 LeNet-1 population: every device's model run forward
// over the test set in batches, the mean batch loss and the training_end flag it raises
// (federated_learning_keras_consensus_FL_threads_MNIST_crossentropy_gradients_exchange.py:430-455,
// the model of :158-194), on the forward phases of cfa_lenet_graph.h. Forward only: the gradient is cfa_lenet_grad.hip.
// The loss phase is the cross-entropy drivers' or the Huber drivers'
// (federated_learning_keras_consensus_FL_MNIST.py:481-483), a template parameter of the kernel.
//
// Launch 1, grid (batch groups, D): a workgroup stages its device's model into LDS once and owns
// whole batches b = blockIdx.x, blockIdx.x + gridDim.x, ... A batch goes through the phases in
// chunks of kLenetChunk samples; each sample's loss lands in LDS and thread 0 sums the batch in
// sample order, so the fp32 batch loss workspace[d][b] has one owner and does not depend on the
// grid. A device flagged in `skip` does no work. Launch 2, one workgroup: a thread per device sums
// its batch losses in fp64 in batch order, writes cost, log entry and flag, and after every thread
// has read the log's epoch counter one thread leaves it one higher. No atomics; a call is
// deterministic.
#include "cfa_lenet_graph.h"

namespace {

constexpr int kLenetBlock = 256;  // 4 waves; several workgroups share a CU and overlap their barriers
constexpr int kLenetChunk = 4;    // samples per pass through the phases

// LDS floats of the evaluation kernel: the model, a chunk's activations, a batch's losses.
inline long long lenet_eval_lds(const LenetGeom& g, int batch) {
  return g.P + (long long)kLenetChunk * lenet_sample_floats(g) + batch;
}

// K: the kernel side at compile time, or 0; LOSS: the objective (CFA_LENET_LOSS_*).
template <int K, int LOSS>
__global__ __launch_bounds__(kLenetBlock) void lenet_eval_kernel(LenetArgs a, LenetGeom g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int dv = blockIdx.y;
  if (a.skip && a.skip[dv]) return;  // the whole workgroup: the device has left its loop
  const int tid = threadIdx.x, T = blockDim.x;
  const int nx = g.side * g.side, n1 = g.p1 * g.p1 * g.c1;
  float* m = lds;                        // [P]
  float* xs = m + (int)g.P;              // [chunk][side][side]
  float* a1 = xs + kLenetChunk * nx;     // [chunk][p1][p1][c1]
  float* a2 = a1 + kLenetChunk * n1;     // [chunk][flat]
  float* zl = a2 + kLenetChunk * g.flat; // [chunk][C]
  float* loss = zl + kLenetChunk * g.C;  // [batch]
  const float* xd = a.x + (long long)dv * a.x_stride;
  const int32_t* ld = a.labels + (long long)dv * a.label_stride;
  stage(m, a.models + (long long)dv * a.pitch, (int)g.P, tid, T);
  for (int b = blockIdx.x; b < a.batches; b += gridDim.x) {
    const long long first = (long long)b * a.batch;
    for (int s0 = 0; s0 < a.batch; s0 += kLenetChunk) {
      const int ns = min(kLenetChunk, a.batch - s0);
      // the previous chunk's last read of xs was its first phase, three barriers ago
      stage(xs, xd + (first + s0) * nx, ns * nx, tid, T);
      __syncthreads();  // also the model's, the first time
      lenet_conv_pool<K>(a1, xs, m + g.oK1, m + g.ob1, ns, g.side, 1, g.c1, g.k, g.p1, tid, T);
      __syncthreads();
      lenet_conv_pool<K>(a2, a1, m + g.oK2, m + g.ob2, ns, g.p1, g.c1, g.c2, g.k, g.p2, tid, T);
      __syncthreads();
      lenet_logits(zl, a2, m + g.oWd, m + g.obd, ns, g.flat, g.C, tid, T);
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

// The kernel side the evaluation kernel is instantiated for: LeNet-1's 5, every other one 0.
inline bool lenet_fast(const LenetGeom& g) { return g.k == 5; }

using LenetEvalKernel = void (*)(LenetArgs, LenetGeom);

// The instantiation for a geometry and an objective (a valid CFA_LENET_LOSS_*).
inline LenetEvalKernel lenet_eval_kernel_for(bool fast, int loss) {
  if (loss == CFA_LENET_LOSS_HUBER)
    return fast ? lenet_eval_kernel<5, CFA_LENET_LOSS_HUBER> : lenet_eval_kernel<0, CFA_LENET_LOSS_HUBER>;
  return fast ? lenet_eval_kernel<5, CFA_LENET_LOSS_XENT> : lenet_eval_kernel<0, CFA_LENET_LOSS_XENT>;
}

}  // namespace

// Current device: raise the evaluation kernels' dynamic-LDS limit now (cfa_device_prepare), so
// later launches (e.g. under hipGraph capture) need no attribute call.
int lenet_prepare_device() {
  const int lim = device_lds_max();
  if (lim <= 65536) return CFA_OK;  // nor would the gradient kernels' be raised
  for (int loss : {CFA_LENET_LOSS_XENT, CFA_LENET_LOSS_HUBER})
    for (bool fast : {true, false})  // refused: launches stay within 64 KiB
      (void)raise_lds_limit((const void*)lenet_eval_kernel_for(fast, loss), lim);
  if (int rc = lenet_grad_prepare_device()) return rc;
  if (int rc = lenet_max_prepare_device()) return rc;
  return lenet_hidden_prepare_device();
}

extern "C" size_t cfa_lenet_params(int side, int kernel, int c1, int c2, int classes) {
  LenetGeom g;
  return lenet_geom(side, kernel, c1, c2, classes, g) ? (size_t)g.P : 0;
}

extern "C" size_t cfa_lenet_eval_workspace_bytes(int D, int batches) {
  return D < 1 || batches < 1 ? 0 : (size_t)D * (size_t)batches * sizeof(float);
}

extern "C" int cfa_lenet_eval_f32(const float* x, size_t x_dev_stride, const int32_t* labels, size_t label_dev_stride,
                                  int Nt, int side, int kernel, int c1, int c2, int classes, const float* models,
                                  size_t pitch, int D, int batch, int batches, const int32_t* skip, double target,
                                  int32_t* ended, double* cost, double* cost_log, int log_cap,
                                  unsigned long long* epoch, void* workspace, size_t workspace_bytes, void* stream) {
  return cfa_lenet_eval_loss_f32(x, x_dev_stride, labels, label_dev_stride, Nt, side, kernel, c1, c2, classes, models,
                                 pitch, D, batch, batches, skip, target, ended, cost, cost_log, log_cap, epoch,
                                 workspace, workspace_bytes, CFA_LENET_LOSS_XENT, stream);
}

extern "C" int cfa_lenet_eval_loss_f32(const float* x, size_t x_dev_stride, const int32_t* labels,
                                       size_t label_dev_stride, int Nt, int side, int kernel, int c1, int c2,
                                       int classes, const float* models, size_t pitch, int D, int batch, int batches,
                                       const int32_t* skip, double target, int32_t* ended, double* cost,
                                       double* cost_log, int log_cap, unsigned long long* epoch, void* workspace,
                                       size_t workspace_bytes, int loss, void* stream) {
  // the messages keep the name callers of either entry know
  const char* fn = loss == CFA_LENET_LOSS_XENT ? "cfa_lenet_eval_f32" : "cfa_lenet_eval_loss_f32";
  LenetGeom g;
  if (int rc = lenet_eval_checks(fn, x, labels, x_dev_stride, label_dev_stride, Nt, side, kernel, c1, c2, classes,
                                 models, pitch, D, batch, batches, target, ended, cost, cost_log, log_cap, epoch,
                                 workspace, workspace_bytes, cfa_lenet_eval_workspace_bytes(D, batches), loss, g))
    return rc;
  // the kernel indexes the model and the LDS with ints
  const bool fast = lenet_fast(g);
  const LenetEvalKernel kern = lenet_eval_kernel_for(fast, loss);
  const long long need = g.P > (1 << 20) ? -1 : 4 * lenet_eval_lds(g, batch), limit = device_lds_max();
  if (need < 0 || need > limit || (need > 65536 && !raise_lds_limit((const void*)kern, (int)limit)))
    return fail(CFA_E_UNSUPPORTED, "%s: a model of %lld parameters, %d samples' activations and a batch of %d losses "
                "do not fit one workgroup's LDS", fn, g.P, kLenetChunk, batch);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LenetArgs a{x, labels, (long long)x_dev_stride, (long long)label_dev_stride, models, (long long)pitch,
                    batch, batches, skip, static_cast<float*>(workspace)};
  // about four workgroups per CU over all devices, and every batch group the same number of
  // batches (but the last)
  const int per = (batches + (int)shared_grid_x(batches, 4, D) - 1) / (int)shared_grid_x(batches, 4, D);
  const dim3 grid((unsigned)((batches + per - 1) / per), (unsigned)D);
  kern<<<grid, kLenetBlock, (size_t)need, st>>>(a, g);
  if (int rc = check_launch("lenet_eval_kernel")) return rc;
  const LenetFinish f{a.ws, D, batches, skip, target, ended, cost, cost_log, log_cap, epoch};
  lenet_finish_kernel<<<1, kLenetFinishBlock, 0, st>>>(f);
  return check_launch("lenet_finish_kernel");
}

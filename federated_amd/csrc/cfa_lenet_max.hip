// cfa_lenet_max.hip — the validation pass and the minibatch gradient of a TF2 population whose
// model is create_q_model's max-pool CNN
// (federated_learning_keras_consensus_FL_threads_MNIST_crossentropy_gradients_exchange.py:170-182,
// conditions 1 and 2: Conv2D(32 or 14, 3 x 3, relu) -> MaxPooling2D -> Conv2D(64, 3 x 3, relu) ->
// MaxPooling2D -> Flatten -> Dense(10, softmax); used at :321-337, :360-385 and :430-455), on the
// plan of cfa_lenet_global.h with LenetMaxPool / LenetMaxGated in the pool's place. Geometry (five
// numbers, one input channel), row layout, objectives, argument checks and both finishing kernels
// are the average-pool family's.
//
// The model stays out of LDS because 34 826 parameters (32 first-stage channels) are 136 KiB. At a
// batch of 100 the validation chunk is 2 samples (62 816 bytes) with 32 channels and 3 (57 520
// bytes) with 14; the gradient chunk is 1 sample (100 244 bytes) with 32 and 2 (132 700 bytes,
// beyond the default 64 KiB) with 14, as many as fit the device's LDS.
#include "cfa_lenet_global.h"

namespace {

struct LenetMaxFamily {
  using Pool = LenetMaxPool;
  using Gated = LenetMaxGated;
  static constexpr bool hidden = false;
  static constexpr bool channels = false;  // x [side, side, 1]
  static constexpr int side = 3;           // the drivers' kernel side
  static constexpr bool grad_chunk_fills_device = true;
  static constexpr const char* eval_name = "lenet_max_eval_kernel";
  static constexpr const char* grad_name = "lenet_max_grad_kernel";
};

}  // namespace

int lenet_max_prepare_device() { return lenet_global_prepare_device<LenetMaxFamily>(); }

extern "C" size_t cfa_lenet_max_eval_workspace_bytes(int D, int batches) {
  return lenet_global_eval_workspace_bytes(D, batches);
}

extern "C" int cfa_lenet_max_eval_loss_f32(const float* x, size_t x_dev_stride, const int32_t* labels,
                                           size_t label_dev_stride, int Nt, int side, int kernel, int c1, int c2,
                                           int classes, const float* models, size_t pitch, int D, int batch,
                                           int batches, const int32_t* skip, double target, int32_t* ended,
                                           double* cost, double* cost_log, int log_cap, unsigned long long* epoch,
                                           void* workspace, size_t workspace_bytes, int loss, void* stream) {
  const char* fn = "cfa_lenet_max_eval_loss_f32";
  LenetGeom g;
  if (int rc = lenet_eval_checks(fn, x, labels, x_dev_stride, label_dev_stride, Nt, side, kernel, c1, c2, classes,
                                 models, pitch, D, batch, batches, target, ended, cost, cost_log, log_cap, epoch,
                                 workspace, workspace_bytes, cfa_lenet_max_eval_workspace_bytes(D, batches), loss, g))
    return rc;
  return lenet_global_eval_launch<LenetMaxFamily>(fn, g, x, x_dev_stride, labels, label_dev_stride, models, pitch, D,
                                                  batch, batches, skip, target, ended, cost, cost_log, log_cap, epoch,
                                                  workspace, loss, stream);
}

extern "C" size_t cfa_lenet_max_grad_workspace_bytes(int D, int batch, int side, int kernel, int c1, int c2,
                                                     int classes) {
  LenetGeom g;
  if (D < 1 || batch < 1 || !lenet_geom(side, kernel, c1, c2, classes, g)) return 0;
  return lenet_global_grad_workspace_bytes(g, D, batch);
}

extern "C" int cfa_lenet_max_grad_loss_f32(const float* x, size_t x_dev_stride, const int32_t* labels,
                                           size_t label_dev_stride, int Nt, int side, int kernel, int c1, int c2,
                                           int classes, const float* models, size_t pitch, int D, const int32_t* src,
                                           const long long* first, int batch, const int32_t* skip, float* grads,
                                           size_t gpitch, float* loss, void* workspace, size_t workspace_bytes,
                                           int loss_kind, void* stream) {
  const char* fn = "cfa_lenet_max_grad_loss_f32";
  LenetGeom g;
  if (int rc = lenet_grad_checks(fn, x, labels, x_dev_stride, label_dev_stride, Nt, side, kernel, c1, c2, classes, models,
                                 pitch, D, batch, grads, gpitch, workspace, loss_kind, g))
    return rc;
  return lenet_global_grad_launch<LenetMaxFamily>(fn, g, x, x_dev_stride, labels, label_dev_stride, Nt, models, pitch, D,
                                                  src, first, batch, skip, grads, gpitch, loss, workspace,
                                                  workspace_bytes, loss_kind, stream);
}

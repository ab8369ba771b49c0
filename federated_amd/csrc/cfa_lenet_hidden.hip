// cfa_lenet_hidden.hip — the validation pass and the minibatch gradient of a TF2 population whose
// model is the CIFAR drivers' hidden-layer LeNet
// (federated_learning_keras_consensus_FL_threads_CIFAR_crossentropy.py:179-186, -modelselection 1:
// x [32, 32, 3] -> Conv2D(4, 5 x 5, relu) -> AveragePooling2D -> Conv2D(8, 5 x 5, relu) ->
// AveragePooling2D -> Flatten -> Dense(128, relu) -> Dense(10, softmax); 28 130 parameters), on the
// plan of cfa_lenet_global.h: the conv / pool phases with cin = channels in stage 1, the hidden
// layer's lenet_hidden_forward / lenet_hidden_backward, and lenet_logits / lenet_dense_backward
// with F = hidden. Geometry (seven numbers), row layout (eight tensors), objectives, the order of
// the argument checks and both finishing kernels are the family's.
//
// The model stays out of LDS because 28 130 parameters are 110 KiB, and with the gradient sums
// 220 KiB. At the driver geometry the validation chunk is 3 samples (56 872 bytes at batch 100) and
// the gradient chunk 2 samples (55 176 bytes): the most that fit 64 KiB, which leaves room for two
// workgroups a CU.
#include "cfa_lenet_global.h"

namespace {

struct LenetHiddenFamily {
  using Pool = LenetAvgPool;
  using Gated = LenetGated;
  static constexpr bool hidden = true;
  static constexpr bool channels = true;  // x [side, side, cin]
  static constexpr int side = 5;          // the drivers' kernel side
  static constexpr bool grad_chunk_fills_device = false;
  static constexpr const char* eval_name = "lenet_hidden_eval_kernel";
  static constexpr const char* grad_name = "lenet_hidden_grad_kernel";
};

// The seven-number family's geometry (false: no model) and its verdict text for a refusal.
inline bool lenet_hidden_verdict(char (&text)[192], int side, int channels, int kernel, int c1, int c2, int hidden,
                                 int classes, LenetGeom& g) {
  snprintf(text, sizeof text, "(side %d channels %d kernel %d c1 %d c2 %d hidden %d classes %d): every dimension >= 1 "
           "and a second pooled map of at least 1 x 1", side, channels, kernel, c1, c2, hidden, classes);
  return lenet_geom(side, channels, kernel, c1, c2, hidden, classes, LenetHiddenFamily::hidden, g);
}

}  // namespace

int lenet_hidden_prepare_device() { return lenet_global_prepare_device<LenetHiddenFamily>(); }

extern "C" size_t cfa_lenet_hidden_params(int side, int channels, int kernel, int c1, int c2, int hidden,
                                          int classes) {
  LenetGeom g;
  return lenet_geom(side, channels, kernel, c1, c2, hidden, classes, LenetHiddenFamily::hidden, g) ? (size_t)g.P : 0;
}

extern "C" size_t cfa_lenet_hidden_eval_workspace_bytes(int D, int batches) {
  return lenet_global_eval_workspace_bytes(D, batches);
}

extern "C" int cfa_lenet_hidden_eval_loss_f32(const float* x, size_t x_dev_stride, const int32_t* labels,
                                              size_t label_dev_stride, int Nt, int side, int channels, int kernel,
                                              int c1, int c2, int hidden, int classes, const float* models,
                                              size_t pitch, int D, int batch, int batches, const int32_t* skip,
                                              double target, int32_t* ended, double* cost, double* cost_log,
                                              int log_cap, unsigned long long* epoch, void* workspace,
                                              size_t workspace_bytes, int loss, void* stream) {
  const char* fn = "cfa_lenet_hidden_eval_loss_f32";
  LenetGeom g;
  char text[192];
  const bool ok = lenet_hidden_verdict(text, side, channels, kernel, c1, c2, hidden, classes, g);
  if (int rc = lenet_eval_checks_for(fn, x, labels, x_dev_stride, label_dev_stride, Nt, ok, text, ok ? g.P : 0,
                                     (long long)side * side * channels, classes, models, pitch, D, batch, batches,
                                     target, ended, cost, cost_log, log_cap, epoch, workspace, workspace_bytes,
                                     cfa_lenet_hidden_eval_workspace_bytes(D, batches), loss))
    return rc;
  return lenet_global_eval_launch<LenetHiddenFamily>(fn, g, x, x_dev_stride, labels, label_dev_stride, models, pitch,
                                                     D, batch, batches, skip, target, ended, cost, cost_log, log_cap,
                                                     epoch, workspace, loss, stream);
}

extern "C" size_t cfa_lenet_hidden_grad_workspace_bytes(int D, int batch, int side, int channels, int kernel, int c1,
                                                        int c2, int hidden, int classes) {
  LenetGeom g;
  if (D < 1 || batch < 1 || !lenet_geom(side, channels, kernel, c1, c2, hidden, classes, LenetHiddenFamily::hidden, g))
    return 0;
  return lenet_global_grad_workspace_bytes(g, D, batch);
}

extern "C" int cfa_lenet_hidden_grad_loss_f32(const float* x, size_t x_dev_stride, const int32_t* labels,
                                              size_t label_dev_stride, int Nt, int side, int channels, int kernel,
                                              int c1, int c2, int hidden, int classes, const float* models,
                                              size_t pitch, int D, const int32_t* src, const long long* first,
                                              int batch, const int32_t* skip, float* grads, size_t gpitch,
                                              float* loss, void* workspace, size_t workspace_bytes, int loss_kind,
                                              void* stream) {
  const char* fn = "cfa_lenet_hidden_grad_loss_f32";
  LenetGeom g;
  char text[192];
  const bool ok = lenet_hidden_verdict(text, side, channels, kernel, c1, c2, hidden, classes, g);
  if (int rc = lenet_grad_checks_for(fn, x, labels, x_dev_stride, label_dev_stride, Nt, ok, text, ok ? g.P : 0,
                                     (long long)side * side * channels, classes, models, pitch, D, batch, grads,
                                     gpitch, workspace, loss_kind))
    return rc;
  return lenet_global_grad_launch<LenetHiddenFamily>(fn, g, x, x_dev_stride, labels, label_dev_stride, Nt, models,
                                                     pitch, D, src, first, batch, skip, grads, gpitch, loss, workspace,
                                                     workspace_bytes, loss_kind, stream);
}

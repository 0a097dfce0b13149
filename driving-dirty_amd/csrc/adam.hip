// torch.optim.Adam on the device (autoencoder.py:119-120, roadmap_bce_v2.py:154-157):
//   dd_adam_step         over one flat buffer
//   dd_adam_step_multi   over a HOST table of small tensors, one launch per 48
//   *_dev                the same with the gradient scale read from device memory (what dd_clip_scale wrote earlier on the stream)
// The kernels and the host code around them are dd_adam.h's templates without the decay; csrc/adamw.hip instantiates the same text
// with it, adam_rankb.hip forms the gradient inside the pass.
#include "dd_adam.h"

namespace {

// dd_adam_step / dd_adam_step_dev: one host path
int adam_launch(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                int32_t step, float grad_scale, const float* gscale_dev, void* stream) {
  DD_REQUIRE(p && g && m && v && n > 0 && step >= 1, DD_ERR_BAD_ARG, "adam: bad argument");
  DD_REQUIRE(((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16 == 0, DD_ERR_BAD_ARG, "adam: buffers must be 16-byte aligned");
  return adam_stream_launch<false>("adam", p, g, m, v, n, lr, beta1, beta2, eps, step, grad_scale, gscale_dev, 1.f, stream);
}

int adam_multi_launch(const dd_adam_tensor* tensors, int32_t count, float lr, float beta1, float beta2, float eps, int32_t step,
                      float grad_scale, const float* gscale_dev, void* stream) {
  DD_REQUIRE(tensors && count > 0 && step >= 1, DD_ERR_BAD_ARG, "adam_multi: bad argument");
  return adam_table_launch<false>("adam_multi", tensors, nullptr, count, lr, beta1, beta2, eps, step, grad_scale, gscale_dev, stream,
                                  [](int32_t i, const dd_adam_tensor& t) {
                                    DD_REQUIRE(t.p && t.g && t.m && t.v && t.n > 0 && t.n < (1 << 30), DD_ERR_BAD_ARG,
                                               "adam_multi: tensor %d: NULL pointer or bad size", i);
                                    return 0;
                                  });
}

}  // namespace

extern "C" {

int dd_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                 int32_t step, float grad_scale, void* stream) {
  return adam_launch(p, g, m, v, n, lr, beta1, beta2, eps, step, grad_scale, nullptr, stream);
}

int dd_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                     int32_t step, const float* grad_scale_dev, void* stream) {
  DD_REQUIRE(grad_scale_dev && (uintptr_t)grad_scale_dev % 4 == 0, DD_ERR_BAD_ARG, "adam_dev: bad argument");
  return adam_launch(p, g, m, v, n, lr, beta1, beta2, eps, step, 0.f, grad_scale_dev, stream);
}

int dd_adam_step_multi(const dd_adam_tensor* tensors, int32_t count, float lr, float beta1, float beta2, float eps, int32_t step,
                       float grad_scale, void* stream) {
  return adam_multi_launch(tensors, count, lr, beta1, beta2, eps, step, grad_scale, nullptr, stream);
}

int dd_adam_step_multi_dev(const dd_adam_tensor* tensors, int32_t count, float lr, float beta1, float beta2, float eps, int32_t step,
                           const float* grad_scale_dev, void* stream) {
  DD_REQUIRE(grad_scale_dev && (uintptr_t)grad_scale_dev % 4 == 0, DD_ERR_BAD_ARG, "adam_multi_dev: bad argument");
  return adam_multi_launch(tensors, count, lr, beta1, beta2, eps, step, 0.f, grad_scale_dev, stream);
}

}  // extern "C"

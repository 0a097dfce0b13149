// Decoupled weight decay (include/dd_adamw.h; csrc/libdd_adamw.so, a library of its own):
//   dd_adamw_step         torch.optim.AdamW over one flat buffer: p1 = p * keep, then the Adam element of dd_adam.h
//   dd_adamw_step_multi   the same for a HOST table of small tensors with one keep per tensor
//   dd_decay              p *= keep: the pre-scale in front of dd_adam_step_rankb, whose kernels do not change
// The two step functions run dd_adam.h's kernel templates with DECAY: the text, the grid and the table of dd_adam_step* (adam.hip) with
// ONE rounded multiply in front of the element.  The by-value kernel has the 48 vector registers of the pass it is a mode of
// (tests/test_adamw_surface.py holds it there) and so fits beside the same conv kernels.
#include "dd_adam.h"

#include "../../include/dd_adamw.h"

#pragma clang fp contract(off)      // p * keep is ONE rounded multiply

namespace {

__global__ __launch_bounds__(256) void decay_kernel(float* __restrict__ p, long n, float keep) {
  const long n4 = n / 4, stride = (long)gridDim.x * blockDim.x;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  // four 16-byte loads in flight per lane, as the Adam pass has with p, g, m, v: with one per lane and one workgroup per CU the pass
  // waited on memory latency (3.5 TB/s on fc1's weight; the Adam pass reaches 5.9)
  for (; i + 3 * stride < n4; i += 4 * stride) {      // the last of the four is inside the whole vectors
    f32x4 pv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) pv[u] = __builtin_nontemporal_load((f32x4*)p + i + u * stride);
#pragma unroll
    for (int u = 0; u < 4; ++u) __builtin_nontemporal_store(pv[u] * keep, (f32x4*)p + i + u * stride);
  }
  for (; i < n4; i += stride) {
    const f32x4 pv = __builtin_nontemporal_load((f32x4*)p + i);
    __builtin_nontemporal_store(pv * keep, (f32x4*)p + i);
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4)) {
    const long i = 4 * n4 + threadIdx.x;
    p[i] = p[i] * keep;
  }
}

// 0, or the refusal: a NaN fails both comparisons
int check_keep(const char* who, const char* what, int index, float keep) {
  if (keep >= 0.f && keep <= 1.f) return 0;
  if (index < 0) return dd_fail(DD_ERR_BAD_ARG, "%s: %s = %g is outside [0, 1]", who, what, (double)keep);
  return dd_fail(DD_ERR_BAD_ARG, "%s: %s[%d] = %g is outside [0, 1]", who, what, index, (double)keep);
}

int check_scale_dev(const char* who, const float* gscale_dev) {
  DD_REQUIRE(!gscale_dev || (uintptr_t)gscale_dev % 4 == 0, DD_ERR_BAD_ARG, "%s: grad_scale_dev is not 4-byte aligned", who);
  return 0;
}

}  // namespace

extern "C" {

int dd_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, int32_t step,
                  float grad_scale, const float* grad_scale_dev, float keep, void* stream) {
  DD_REQUIRE(p, DD_ERR_BAD_ARG, "adamw_step: p is NULL");
  DD_REQUIRE(g, DD_ERR_BAD_ARG, "adamw_step: g is NULL");
  DD_REQUIRE(m, DD_ERR_BAD_ARG, "adamw_step: m is NULL");
  DD_REQUIRE(v, DD_ERR_BAD_ARG, "adamw_step: v is NULL");
  DD_REQUIRE(n > 0, DD_ERR_BAD_ARG, "adamw_step: n = %lld, at least one element is needed", (long long)n);
  DD_REQUIRE(step >= 1, DD_ERR_BAD_ARG, "adamw_step: step = %d, steps count from 1", step);
  DD_REQUIRE(((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16 == 0, DD_ERR_BAD_ARG,
             "adamw_step: buffers must be 16-byte aligned");
  if (int rc = check_scale_dev("adamw_step", grad_scale_dev)) return rc;
  if (int rc = check_keep("adamw_step", "keep", -1, keep)) return rc;
  return adam_stream_launch<true>("adamw_step", p, g, m, v, n, lr, beta1, beta2, eps, step, grad_scale, grad_scale_dev, keep, stream);
}

int dd_adamw_step_multi(const dd_adam_tensor* tensors, const float* keep, int32_t count, float lr, float beta1, float beta2, float eps,
                        int32_t step, float grad_scale, const float* grad_scale_dev, void* stream) {
  DD_REQUIRE(tensors, DD_ERR_BAD_ARG, "adamw_step_multi: tensors is NULL");
  DD_REQUIRE(keep, DD_ERR_BAD_ARG, "adamw_step_multi: keep is NULL");
  DD_REQUIRE(count > 0, DD_ERR_BAD_ARG, "adamw_step_multi: count = %d, at least one tensor is needed", count);
  DD_REQUIRE(step >= 1, DD_ERR_BAD_ARG, "adamw_step_multi: step = %d, steps count from 1", step);
  if (int rc = check_scale_dev("adamw_step_multi", grad_scale_dev)) return rc;
  return adam_table_launch<true>("adamw_step_multi", tensors, keep, count, lr, beta1, beta2, eps, step, grad_scale, grad_scale_dev, stream,
                                 [keep](int32_t i, const dd_adam_tensor& t) {
                                   DD_REQUIRE(t.p && t.g && t.m && t.v, DD_ERR_BAD_ARG, "adamw_step_multi: tensor %d: a NULL pointer", i);
                                   DD_REQUIRE(t.n > 0 && t.n < (1 << 30), DD_ERR_BAD_ARG, "adamw_step_multi: tensor %d: n = %lld is outside [1, 2^30)", i,
                                              (long long)t.n);
                                   return check_keep("adamw_step_multi", "keep", i, keep[i]);
                                 });
}

int dd_decay(float* p, int64_t n, float keep, void* stream) {
  DD_REQUIRE(p, DD_ERR_BAD_ARG, "decay: p is NULL");
  DD_REQUIRE(n > 0, DD_ERR_BAD_ARG, "decay: n = %lld, at least one element is needed", (long long)n);
  DD_REQUIRE((uintptr_t)p % 16 == 0, DD_ERR_BAD_ARG, "decay: p must be 16-byte aligned");
  if (int rc = check_keep("decay", "keep", -1, keep)) return rc;
  // four vectors per lane: a quarter of the Adam pass's workgroups, under the same cap less the spare compute units
  const int grid = adam_stream_grid((n + 3) / 4, std::max(DD_NUM_CU - dd_adam_spare_internal(), 1));
  hipLaunchKernelGGL(decay_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, (long)n, keep);
  DD_LAUNCH_CHECK("decay");
  return 0;
}

}  // extern "C"

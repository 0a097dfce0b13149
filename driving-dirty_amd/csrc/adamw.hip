// Decoupled weight decay (include/dd_adamw.h; csrc/libdd_adamw.so, a library of its own):
//   dd_adamw_step         torch.optim.AdamW over one flat buffer: p1 = p * keep, then the Adam element of dd_adam.h
//   dd_adamw_step_multi   the same for a HOST table of small tensors with one keep per tensor
//   dd_decay              p *= keep: the pre-scale in front of dd_adam_step_rankb, whose kernels do not change
// The kernels are dense.hip's adam_kernel / adam_dev_kernel / adam_multi_kernel / adam_multi_dev_kernel with ONE multiply in front of
// the element: the same loads and stores (non-temporal, 16 bytes per lane), the same grid (dd_adam_blocks_internal() persistent
// workgroups per CU), the same scalar tail by workgroup 0.  `keep` is a kernel argument and stays in a scalar register: the by-value
// kernel has adam_kernel's 48 vector registers (tests/test_adamw_surface.py holds it there) and so fits beside the same conv kernels.
// As in dense.hip the loop is written out in each of the two streaming kernels rather than shared: called as one function the
// by-value kernel came out of the compiler with another schedule.
#include <algorithm>
#include <math.h>

#include "dd_adam.h"

#include "../../include/dd_adamw.h"

#pragma clang fp contract(off)      // p * keep is ONE rounded multiply: never fused into the element's last multiply-add

namespace {

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, long n, float lr, float b1, float b2, float eps, float bc1,
                                                    float bc2_sqrt, float gscale, float keep) {
  const long n4 = n / 4;
  const float step_size = lr / bc1;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f32x4 pv = __builtin_nontemporal_load((f32x4*)p + i), mv = __builtin_nontemporal_load((f32x4*)m + i),
          vv = __builtin_nontemporal_load((f32x4*)v + i);
    const f32x4 gv = __builtin_nontemporal_load((const f32x4*)g + i);
    const float inv_bc2 = 1.f / bc2_sqrt;
    pv = pv * keep;
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
      f32x2 pe = {pv[k], pv[k + 1]}, me = {mv[k], mv[k + 1]}, ve = {vv[k], vv[k + 1]};
      adam_elem2(pe, me, ve, f32x2{gv[k], gv[k + 1]}, gscale, b1, b2, eps, step_size, inv_bc2);
      pv[k] = pe.x; pv[k + 1] = pe.y; mv[k] = me.x; mv[k + 1] = me.y; vv[k] = ve.x; vv[k + 1] = ve.y;
    }
    __builtin_nontemporal_store(pv, (f32x4*)p + i);
    __builtin_nontemporal_store(mv, (f32x4*)m + i);
    __builtin_nontemporal_store(vv, (f32x4*)v + i);
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4)) {      // i < n: the last n % 4 elements
    const long i = 4 * n4 + threadIdx.x;
    float pe = p[i] * keep, me = m[i], ve = v[i];
    adam_elem(pe, me, ve, g[i], gscale, b1, b2, eps, step_size, bc2_sqrt);
    p[i] = pe; m[i] = me; v[i] = ve;
  }
}

// the gradient scale read from device memory (one uniform load), as dense.hip's adam_dev_kernel
__global__ __launch_bounds__(256) void adamw_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, long n, float lr, float b1, float b2, float eps,
                                                        float bc1, float bc2_sqrt, const float* __restrict__ gscale_dev, float keep) {
  const float gscale = gscale_dev[0];
  const long n4 = n / 4;
  const float step_size = lr / bc1;
  const float inv_bc2 = 1.f / bc2_sqrt;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f32x4 pv = __builtin_nontemporal_load((f32x4*)p + i), mv = __builtin_nontemporal_load((f32x4*)m + i),
          vv = __builtin_nontemporal_load((f32x4*)v + i);
    const f32x4 gv = __builtin_nontemporal_load((const f32x4*)g + i);
    pv = pv * keep;
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
      f32x2 pe = {pv[k], pv[k + 1]}, me = {mv[k], mv[k + 1]}, ve = {vv[k], vv[k + 1]};
      adam_elem2(pe, me, ve, f32x2{gv[k], gv[k + 1]}, gscale, b1, b2, eps, step_size, inv_bc2);
      pv[k] = pe.x; pv[k + 1] = pe.y; mv[k] = me.x; mv[k + 1] = me.y; vv[k] = ve.x; vv[k + 1] = ve.y;
    }
    __builtin_nontemporal_store(pv, (f32x4*)p + i);
    __builtin_nontemporal_store(mv, (f32x4*)m + i);
    __builtin_nontemporal_store(vv, (f32x4*)v + i);
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4)) {
    const long i = 4 * n4 + threadIdx.x;
    float pe = p[i] * keep, me = m[i], ve = v[i];
    adam_elem(pe, me, ve, g[i], gscale, b1, b2, eps, step_size, bc2_sqrt);
    p[i] = pe; m[i] = me; v[i] = ve;
  }
}

// The small tensors in one launch: dense.hip's AdamTable with one keep per tensor.  Block b works on tensor t with
// first[t] <= b < first[t + 1]; a block past a tensor's last element of its last 256 leaves.
constexpr int kMultiMax = 48;
struct AdamWTable {
  float* p[kMultiMax];
  const float* g[kMultiMax];
  float* m[kMultiMax];
  float* v[kMultiMax];
  int n[kMultiMax];
  float keep[kMultiMax];
  int first[kMultiMax + 1];
  int count;
};

template <bool DEV>
__global__ __launch_bounds__(256) void adamw_multi_kernel(AdamWTable tab, float lr, float b1, float b2, float eps, float bc1,
                                                          float bc2_sqrt, float gscale, const float* __restrict__ gscale_dev) {
  int t = 0;
  while (t + 1 < tab.count && (int)blockIdx.x >= tab.first[t + 1]) ++t;
  float* __restrict__ p = tab.p[t];
  const float* __restrict__ g = tab.g[t];
  float* __restrict__ m = tab.m[t];
  float* __restrict__ v = tab.v[t];
  const int i = ((int)blockIdx.x - tab.first[t]) * 256 + threadIdx.x;
  if (i >= tab.n[t]) return;
  if constexpr (DEV) gscale = gscale_dev[0];
  const float step_size = lr / bc1;
  float pe = p[i] * tab.keep[t], me = m[i], ve = v[i];
  adam_elem(pe, me, ve, g[i], gscale, b1, b2, eps, step_size, bc2_sqrt);
  p[i] = pe; m[i] = me; v[i] = ve;
}

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

// workgroups of a streaming pass over n elements, 16 bytes per lane: the Adam pass's grid (dense.hip adam_launch) on `cus` compute units
int stream_grid(int64_t n, int cus) { return (int)std::min<long>((n / 4 + 255) / 256 + 1, (long)cus * dd_adam_blocks_internal()); }

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
  const double bc1 = 1.0 - pow((double)beta1, (double)step);      // as dense.hip's adam_launch: the same step gives the same bits
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const int grid = stream_grid(n, DD_NUM_CU);
  if (grad_scale_dev)
    hipLaunchKernelGGL(adamw_dev_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long)n, lr, beta1, beta2, eps,
                       (float)bc1, (float)sqrt(bc2), grad_scale_dev, keep);
  else
    hipLaunchKernelGGL(adamw_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long)n, lr, beta1, beta2, eps,
                       (float)bc1, (float)sqrt(bc2), grad_scale, keep);
  DD_LAUNCH_CHECK("adamw_step");
  return 0;
}

int dd_adamw_step_multi(const dd_adam_tensor* tensors, const float* keep, int32_t count, float lr, float beta1, float beta2, float eps,
                        int32_t step, float grad_scale, const float* grad_scale_dev, void* stream) {
  DD_REQUIRE(tensors, DD_ERR_BAD_ARG, "adamw_step_multi: tensors is NULL");
  DD_REQUIRE(keep, DD_ERR_BAD_ARG, "adamw_step_multi: keep is NULL");
  DD_REQUIRE(count > 0, DD_ERR_BAD_ARG, "adamw_step_multi: count = %d, at least one tensor is needed", count);
  DD_REQUIRE(step >= 1, DD_ERR_BAD_ARG, "adamw_step_multi: step = %d, steps count from 1", step);
  if (int rc = check_scale_dev("adamw_step_multi", grad_scale_dev)) return rc;
  for (int32_t i = 0; i < count; ++i) {      // the whole table before the first launch
    const dd_adam_tensor& t = tensors[i];
    DD_REQUIRE(t.p && t.g && t.m && t.v, DD_ERR_BAD_ARG, "adamw_step_multi: tensor %d: a NULL pointer", i);
    DD_REQUIRE(t.n > 0 && t.n < (1 << 30), DD_ERR_BAD_ARG, "adamw_step_multi: tensor %d: n = %lld is outside [1, 2^30)", i, (long long)t.n);
    if (int rc = check_keep("adamw_step_multi", "keep", i, keep[i])) return rc;
  }
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  for (int32_t base = 0; base < count; base += kMultiMax) {
    AdamWTable tab;
    tab.count = std::min<int32_t>(kMultiMax, count - base);
    int blocks = 0;      // < 48 * 2^22
    for (int i = 0; i < tab.count; ++i) {
      const dd_adam_tensor& t = tensors[base + i];
      tab.p[i] = t.p;
      tab.g[i] = t.g;
      tab.m[i] = t.m;
      tab.v[i] = t.v;
      tab.n[i] = (int)t.n;
      tab.keep[i] = keep[base + i];
      tab.first[i] = blocks;
      blocks += (int)((t.n + 255) / 256);
    }
    for (int i = tab.count; i < kMultiMax; ++i) {      // never read; kept defined
      tab.p[i] = tab.m[i] = tab.v[i] = nullptr;
      tab.g[i] = nullptr;
      tab.n[i] = 0;
      tab.keep[i] = 1.f;
      tab.first[i + 1] = 0;
    }
    tab.first[tab.count] = blocks;
    if (grad_scale_dev)
      hipLaunchKernelGGL(adamw_multi_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, tab, lr, beta1, beta2, eps,
                         (float)bc1, (float)sqrt(bc2), 0.f, grad_scale_dev);
    else
      hipLaunchKernelGGL(adamw_multi_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, tab, lr, beta1, beta2, eps,
                         (float)bc1, (float)sqrt(bc2), grad_scale, (const float*)nullptr);
    DD_LAUNCH_CHECK("adamw_step_multi");
  }
  return 0;
}

int dd_decay(float* p, int64_t n, float keep, void* stream) {
  DD_REQUIRE(p, DD_ERR_BAD_ARG, "decay: p is NULL");
  DD_REQUIRE(n > 0, DD_ERR_BAD_ARG, "decay: n = %lld, at least one element is needed", (long long)n);
  DD_REQUIRE((uintptr_t)p % 16 == 0, DD_ERR_BAD_ARG, "decay: p must be 16-byte aligned");
  if (int rc = check_keep("decay", "keep", -1, keep)) return rc;
  // four vectors per lane: a quarter of the Adam pass's workgroups, under the same cap less the spare compute units
  const int grid = stream_grid((n + 3) / 4, std::max(DD_NUM_CU - dd_adam_spare_internal(), 1));
  hipLaunchKernelGGL(decay_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, (long)n, keep);
  DD_LAUNCH_CHECK("decay");
  return 0;
}

}  // extern "C"

// The optimizer's shared code.  The Adam element update (one definition for every optimizer kernel: the same inputs give the same bits
// whichever kernel a tensor meets), the streaming kernel and the table kernel of dd_adam_step* (adam.hip) and dd_adamw_step* (adamw.hip)
// as ONE template each, and the host code around them.  adam_rankb.hip takes the element and the bias corrections.
#pragma once
#include <math.h>

#include <algorithm>

#include "dd_common.h"

// One element of torch.optim.Adam, written with explicit fused multiply-adds and contraction off: the vector kernel, its scalar
// tail and the multi-tensor kernel must produce the SAME bits for the same inputs (left to the compiler, `a * b + c` was
// contracted differently in the float4 loop and in the scalar kernels, so a tensor updated by one kernel or the other -- the
// overlapped optimizer picks by size and timing -- ended a last bit apart).
// Hardware square root and reciprocal (v_sqrt_f32 / v_rcp_f32, 1 ulp each) instead of the IEEE sequences, and packed fp32 for
// the rest: 34 vector instructions per four elements instead of 175.  The pass usually runs beside the conv backward, where its
// vector instructions compete with the conv kernels' own (tools/ubench/mfma_issue.hip: they do overlap the MFMAs of another
// wave but not its vector work): with the IEEE form the register-row data gradient took 1.95-1.97 ms in the step, with this one
// 1.70-1.78.
// Accuracy against torch.optim.Adam's arithmetic in fp64 (bounds: tests/_element_ref.py, from an fp32 model of these operations
// with a correctly rounded square root and reciprocal; held by tests/test_gpu_element_range.py over 30 decades of g and m, 60 of
// v, steps 1 .. 2^31 - 1): m and v are multiplies and fused multiply-adds only, so they are the IEEE result of this sequence bit
// for bit -- not exact: five roundings in v (within 6 x 2^-24 relative) and three in m (within 5 x 2^-24 of |b1 m| + |(1 - b1)
// g|, its terms' magnitude: where the two terms cancel, m's RELATIVE error is that times magnitude / |m|, and the update
// inherits it). The update p_new - p is within (5 magnitude / |m| + 5) 2^-24 of itself plus half an ulp of the larger of p and
// p_new. Zero, subnormal, infinite and NaN inputs give fp32 torch.optim.Adam's pattern of zeros, infinities and NaNs (a result
// below 2^-126 may be a subnormal where torch's order of operations underflows to zero).
// omb1 = 1.f - b1, omb2 = 1.f - b2 (fp32 subtractions: the same bits on the host and on the device).  A kernel that passes them as
// arguments keeps them in scalar registers; computed in the kernel they occupy vector registers (no scalar float ALU on gfx950).
__device__ __forceinline__ void adam_elem2(f32x2& p, f32x2& m, f32x2& v, f32x2 g, float gscale, float b1, float b2, float omb1,
                                           float omb2, float eps, float step_size, float inv_bc2) {
#pragma clang fp contract(off)
  const f32x2 gg = g * gscale;
  const f32x2 mm = __builtin_elementwise_fma(f32x2{b1, b1}, m, gg * omb1);
  const f32x2 vv = __builtin_elementwise_fma(f32x2{b2, b2}, v, (gg * omb2) * gg);
  m = mm;
  v = vv;
  const f32x2 s = {__builtin_amdgcn_sqrtf(vv.x), __builtin_amdgcn_sqrtf(vv.y)};
  const f32x2 denom = __builtin_elementwise_fma(s, f32x2{inv_bc2, inv_bc2}, f32x2{eps, eps});
  const f32x2 r = {__builtin_amdgcn_rcpf(denom.x), __builtin_amdgcn_rcpf(denom.y)};
  p = __builtin_elementwise_fma(f32x2{-step_size, -step_size}, mm * r, p);
}
__device__ __forceinline__ void adam_elem2(f32x2& p, f32x2& m, f32x2& v, f32x2 g, float gscale, float b1, float b2, float eps,
                                           float step_size, float inv_bc2) {
  adam_elem2(p, m, v, g, gscale, b1, b2, 1.f - b1, 1.f - b2, eps, step_size, inv_bc2);
}
__device__ __forceinline__ void adam_elem(float& p, float& m, float& v, float g, float gscale, float b1, float b2, float eps,
                                          float step_size, float bc2_sqrt) {      // the same operations on one element (tails, small tensors)
  f32x2 pp = {p, 0.f}, mm = {m, 0.f}, vv = {v, 0.f};
  adam_elem2(pp, mm, vv, f32x2{g, 0.f}, gscale, b1, b2, eps, step_size, 1.f / bc2_sqrt);
  p = pp.x; m = mm.x; v = vv.x;
}

// ---- the streaming kernel: dd_adam_step, dd_adam_step_dev, dd_adamw_step -------------------------------------------------------------
// DEV: the gradient scale is read from device memory (one uniform load: what dd_clip_scale wrote earlier on the stream).  DECAY:
// decoupled weight decay, p * keep in front of the element -- ONE rounded multiply (contraction is off in this function: never fused
// into the element's last multiply-add).  `keep` is a kernel argument and stays in a scalar register.
// Non-temporal 16-byte accesses: the pass runs beside the conv backward and should not push its 4.5 GB through the caches.  Workgroup 0
// takes the last n % 4 elements one by one.
// One text for the four kernels, shared as a TEMPLATE: shared as a function that several kernels call, the loop came out of the compiler
// with another schedule in the by-value kernel, the one tuned to run beside the conv backward.  Measured for the template (AMD clang
// 22.0.0git, roc-7.2.0, -O3, gfx950): every instantiation has 48 vector registers and no scratch, and from its first load to its branch
// the loop is one opcode sequence, that of a kernel written out by hand: 43 instructions, 44 with DECAY (tests/test_adam_surface.py
// holds the registers; tools/kernel_resources.py --diff compares two builds; profiles/adam_template_refactor_ab.json).  48 is the
// budget: what the conv backward's one-wave-per-SIMD kernels (440-464 registers) leave of a SIMD's 512.
template <bool DEV, bool DECAY>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long n, float lr, float b1, float b2, float eps, float bc1,
                                                   float bc2_sqrt, float gscale, const float* __restrict__ gscale_dev, float keep) {
#pragma clang fp contract(off)
  if constexpr (DEV) gscale = gscale_dev[0];
  const long n4 = n / 4;
  const float step_size = lr / bc1;
  const float inv_bc2 = 1.f / bc2_sqrt;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f32x4 pv = __builtin_nontemporal_load((f32x4*)p + i), mv = __builtin_nontemporal_load((f32x4*)m + i),
          vv = __builtin_nontemporal_load((f32x4*)v + i);
    const f32x4 gv = __builtin_nontemporal_load((const f32x4*)g + i);
    if constexpr (DECAY) pv = pv * keep;
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
    float pe = p[i], me = m[i], ve = v[i];
    if constexpr (DECAY) pe = pe * keep;
    adam_elem(pe, me, ve, g[i], gscale, b1, b2, eps, step_size, bc2_sqrt);
    p[i] = pe; m[i] = me; v[i] = ve;
  }
}

// ---- the table kernel: dd_adam_step_multi, dd_adam_step_multi_dev, dd_adamw_step_multi -----------------------------------------------
// The small tensors of a model (biases, BatchNorm vectors, 3x3 filters) in ONE launch: sixteen 6-us launches at the very end of the
// step are 0.1 ms nothing overlaps.  The table travels by value in the kernel arguments; block b works on entry t with
// first[t] <= b < first[t + 1] (dd_table_entry), and a block past its tensor's last element of its last 256 leaves.  With DECAY the
// table has one keep per tensor; without, it is the five arrays and `count` alone.
constexpr int ADAM_TABLE_MAX = 48;      // entries of one launch
template <bool DECAY>
struct AdamKeep {};
template <>
struct AdamKeep<true> {
  float keep[ADAM_TABLE_MAX];
};
template <bool DECAY>
struct AdamTable : AdamKeep<DECAY> {
  float* p[ADAM_TABLE_MAX];
  const float* g[ADAM_TABLE_MAX];
  float* m[ADAM_TABLE_MAX];
  float* v[ADAM_TABLE_MAX];
  int n[ADAM_TABLE_MAX];
  int first[ADAM_TABLE_MAX + 1];
  int count;
};

template <bool DEV, bool DECAY>
__global__ __launch_bounds__(256) void adam_multi_kernel(AdamTable<DECAY> tab, float lr, float b1, float b2, float eps, float bc1,
                                                         float bc2_sqrt, float gscale, const float* __restrict__ gscale_dev) {
#pragma clang fp contract(off)
  const int t = dd_table_entry(tab.first, tab.count);
  float* __restrict__ p = tab.p[t];
  const float* __restrict__ g = tab.g[t];
  float* __restrict__ m = tab.m[t];
  float* __restrict__ v = tab.v[t];
  const int i = ((int)blockIdx.x - tab.first[t]) * 256 + threadIdx.x;
  if (i >= tab.n[t]) return;
  if constexpr (DEV) gscale = gscale_dev[0];
  const float step_size = lr / bc1;
  float pe = p[i], me = m[i], ve = v[i];
  if constexpr (DECAY) pe = pe * tab.keep[t];
  adam_elem(pe, me, ve, g[i], gscale, b1, b2, eps, step_size, bc2_sqrt);
  p[i] = pe; m[i] = me; v[i] = ve;
}

// ---- the host code around them ---------------------------------------------------------------------------------------------------------
// The bias corrections of step `step`, in double: the same step gives every pass the same bits.
struct AdamBias {
  float bc1, bc2_sqrt;      // 1 - beta1^step, sqrt(1 - beta2^step)
};
static inline AdamBias adam_bias(float beta1, float beta2, int32_t step) {
  return {(float)(1.0 - pow((double)beta1, (double)step)), (float)sqrt(1.0 - pow((double)beta2, (double)step))};
}

// Workgroups of a streaming pass over n elements, 16 bytes per lane, on `cus` compute units: dd_adam_blocks_internal() PERSISTENT
// workgroups per CU, one by default.  The pass usually runs BESIDE the conv backward (optim.HipAdam.overlap_with_backward), whose
// one-wave-per-SIMD kernels take 440-464 of a SIMD's 512 registers: one Adam wave (48) fits beside them, and -- the point -- nothing of
// the launch is ever left QUEUED: blocks that wait for a CU are dispatched ahead of the next conv kernel when the current one ends, and
// a kernel of >= 456 registers then waits until they have all drained (tools/ubench/residency.hip; in the step: the c2 data gradient
// 2.2 ms from dispatch to end instead of 1.6).  Alone the pass is also fastest this way (0.536 ms for fc1's 481 MB = 6.3 TB/s; 4 blocks
// per CU: 0.586, 8: 0.595).
static inline int adam_stream_grid(int64_t n, int cus) {
  return (int)std::min<long>((n / 4 + 255) / 256 + 1, (long)cus * dd_adam_blocks_internal());
}

// The streaming pass, launched: the scale by value or -- gscale_dev -- read by the kernel.  The caller has checked its arguments.
template <bool DECAY>
int adam_stream_launch(const char* who, float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                       float eps, int32_t step, float grad_scale, const float* gscale_dev, float keep, void* stream) {
  const AdamBias bc = adam_bias(beta1, beta2, step);
  const int grid = adam_stream_grid(n, DD_NUM_CU);
  if (gscale_dev)
    hipLaunchKernelGGL((adam_kernel<true, DECAY>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long)n, lr, beta1, beta2,
                       eps, bc.bc1, bc.bc2_sqrt, 0.f, gscale_dev, keep);
  else
    hipLaunchKernelGGL((adam_kernel<false, DECAY>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long)n, lr, beta1, beta2,
                       eps, bc.bc1, bc.bc2_sqrt, grad_scale, (const float*)nullptr, keep);
  DD_LAUNCH_CHECK(who);
  return 0;
}

// The table pass, launched: `check(i, tensors[i])` (0 or a refusal) on the WHOLE table before the first launch, then one launch per
// ADAM_TABLE_MAX tensors.  `keep`: one per tensor with DECAY, not read without.
template <bool DECAY, typename Check>
int adam_table_launch(const char* who, const dd_adam_tensor* tensors, const float* keep, int32_t count, float lr, float beta1,
                      float beta2, float eps, int32_t step, float grad_scale, const float* gscale_dev, void* stream, Check check) {
  for (int32_t i = 0; i < count; ++i)
    if (int rc = check(i, tensors[i])) return rc;
  const AdamBias bc = adam_bias(beta1, beta2, step);
  for (int32_t base = 0; base < count; base += ADAM_TABLE_MAX) {
    AdamTable<DECAY> tab;
    tab.count = std::min<int32_t>(ADAM_TABLE_MAX, count - base);
    int blocks = 0;      // < 48 * 2^22
    for (int i = 0; i < ADAM_TABLE_MAX; ++i) {
      const bool used = i < tab.count;      // the entries past count are never read; kept defined
      const dd_adam_tensor t = used ? tensors[base + i] : dd_adam_tensor{};
      tab.p[i] = t.p;
      tab.g[i] = t.g;
      tab.m[i] = t.m;
      tab.v[i] = t.v;
      tab.n[i] = (int)t.n;
      if constexpr (DECAY) tab.keep[i] = used ? keep[base + i] : 1.f;
      tab.first[i] = blocks;
      blocks += (int)((t.n + 255) / 256);
    }
    tab.first[ADAM_TABLE_MAX] = blocks;
    if (gscale_dev)
      hipLaunchKernelGGL((adam_multi_kernel<true, DECAY>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, tab, lr, beta1, beta2, eps,
                         bc.bc1, bc.bc2_sqrt, 0.f, gscale_dev);
    else
      hipLaunchKernelGGL((adam_multi_kernel<false, DECAY>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, tab, lr, beta1, beta2, eps,
                         bc.bc1, bc.bc2_sqrt, grad_scale, (const float*)nullptr);
    DD_LAUNCH_CHECK(who);
  }
  return 0;
}

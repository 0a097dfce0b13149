// dd_box_loss_fwd / dd_box_loss_bwd: weighted BCE + soft threat score on the box head's probabilities (formulas: dd_hotpath.h).
//
// Two streaming passes over [batch][per_sample] (timing: DESIGN.md 3.4f).  The statistics pass reduces five sums per sample; with them the loss for
// ANY weight -- the per-sample "auto" weight included, which needs T before it can weigh A -- comes out of that one pass, and the
// finalise launch turns them into four gradient coefficients per sample, so the gradient pass divides by no statistic.
// A workgroup belongs to one sample; no atomics, every sum has a fixed order: two launches give the same bits.
#include <limits.h>

#include "dd_loss_stats.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRun = 4;                  // quads (of 4 elements) a thread adds in fp32 before it folds into fp64: 16 terms per run
constexpr int kMaxBlocksPerSample = 256;      // bounds the workspace by the batch alone; longer samples take more runs per thread
constexpr int kStats = 5;                // T, S, I, A, C
constexpr int kGradQuads = 4;            // quads per thread of the gradient pass

int stats_blocks(long n4) { return (int)max(1L, min((long)kMaxBlocksPerSample, (n4 + kThreads * kRun - 1) / (kThreads * kRun))); }

template <typename TT>
__device__ __forceinline__ f32x4 load_target4(const TT* t, long quad);
template <>
__device__ __forceinline__ f32x4 load_target4<float>(const float* t, long quad) { return ((const f32x4*)t)[quad]; }
template <>
__device__ __forceinline__ f32x4 load_target4<unsigned char>(const unsigned char* t, long quad) {
  return dd_bytes_f32x4(((const unsigned*)t)[quad]);
}

// -max(log p, -100) and -max(log(1 - p), -100).  u = fl(1 - p) loses up to half an ulp of 1, which is 1.5e-6 of log(1 - p) at
// p = 0.02; d = 1 - u is exact and is the p that u stands for, so log(u) * p / d = log1p(-p) to the accuracy of logf
// (dd_sigmoid_softplus uses the same identity).  p = 1: u = 0, -inf, clamped.  p below half an ulp of 1: d = 0 and log1p(-p) = -p.
__device__ __forceinline__ void neg_logs(float p, float& nlp, float& nlq) {
  nlp = -fmaxf(logf(p), -100.f);
  const float u = 1.f - p, d = 1.f - u;
  const float lq = d == 0.f ? -p : logf(u) * (p / d);
  nlq = -fmaxf(lq, -100.f);
}

__device__ __forceinline__ void add_quad(const f32x4 p, const f32x4 t, float (&s)[kStats]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float nlp, nlq;
    neg_logs(p[k], nlp, nlq);
    s[0] += t[k];
    s[1] += p[k];
    s[2] += p[k] * t[k];
    s[3] += t[k] * nlp;
    s[4] += (1.f - t[k]) * nlq;
  }
}

// grid = batch * bps workgroups; workgroup g reduces the quads blk * 256 + tid + r * bps * 256 of sample g / bps.
template <typename TT>
__global__ __launch_bounds__(kThreads) void box_loss_stats_kernel(const float* __restrict__ probs, const TT* __restrict__ target, long n4, int bps,
                                                                  double* __restrict__ partial) {
  const int b = blockIdx.x / bps, blk = blockIdx.x - b * bps;
  const long base = (long)b * n4, stride = (long)bps * kThreads;
  double acc[kStats] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (long i = (long)blk * kThreads + threadIdx.x; i < n4; i += kRun * stride) {
    float s[kStats] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (i + (kRun - 1) * stride < n4) {      // a whole run: the loads first, all in flight
      f32x4 p[kRun], t[kRun];
#pragma unroll
      for (int r = 0; r < kRun; ++r) {
        p[r] = ((const f32x4*)probs)[base + i + r * stride];
        t[r] = load_target4<TT>(target, base + i + r * stride);
      }
#pragma unroll
      for (int r = 0; r < kRun; ++r) add_quad(p[r], t[r], s);
    } else {
      for (long j = i; j < n4; j += stride) add_quad(((const f32x4*)probs)[base + j], load_target4<TT>(target, base + j), s);
    }
#pragma unroll
    for (int k = 0; k < kStats; ++k) acc[k] += (double)s[k];
  }
  dd_block_sum<kStats, kThreads>(acc, partial + (long)blockIdx.x * kStats);
}

// One workgroup; wave w takes the samples w, w + 4, ...: lane l adds the partials of workgroups l, l + 64, ... of the sample, the lanes
// are added by shuffle, lane 0 writes the sample's statistics and coefficients and keeps the wave's share of the two loss terms.
__global__ __launch_bounds__(kThreads) void box_loss_final_kernel(const double* __restrict__ partial, int batch, int bps, double per_sample,
                                                                  float pos_weight, double alpha, double beta, double eps,
                                                                  double* __restrict__ stats, float* __restrict__ coef, float* __restrict__ loss_out) {
  __shared__ double red[2][kThreads / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double inv_b = 1.0 / (double)batch, inv_bp = 1.0 / ((double)batch * per_sample);
  double bce = 0.0, ts = 0.0;
  for (int b = wave; b < batch; b += kThreads / 64) {
    double v[kStats] = {0.0, 0.0, 0.0, 0.0, 0.0};
    dd_sample_sum(partial, b, bps, lane, v);
    if (lane == 0) dd_sample_finish(v, b, per_sample, pos_weight, DD_POS_WEIGHT_AUTO, alpha, beta, eps, inv_b, inv_bp, bce, ts, stats, coef);
  }
  if (lane == 0) {
    red[0][wave] = bce;
    red[1][wave] = ts;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double l_bce = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) * inv_bp;
    const double l_ts = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) * inv_b;
    loss_out[0] = (float)(alpha * l_bce + beta * l_ts);
    loss_out[1] = (float)l_bce;
    loss_out[2] = (float)l_ts;
  }
}

// grid = batch * gps workgroups, workgroup g writes the quads blk * 1024 + tid + r * 256 (r < 4) of sample g / gps.
template <typename TT>
__global__ __launch_bounds__(kThreads) void box_loss_grad_kernel(const float* __restrict__ probs, const TT* __restrict__ target,
                                                                 const float* __restrict__ coef, long n4, int gps, float gscale,
                                                                 float* __restrict__ dprobs) {
  const int b = blockIdx.x / gps, blk = blockIdx.x - b * gps;
  const long base = (long)b * n4;
  const f32x4 c = *(const f32x4*)(coef + 4L * b) * gscale;
  const long first = (long)blk * (kThreads * kGradQuads) + threadIdx.x;
  f32x4 p[kGradQuads], t[kGradQuads];
#pragma unroll
  for (int r = 0; r < kGradQuads; ++r) {
    const long i = min(first + r * kThreads, n4 - 1);      // unconditional loads (all in flight); past the end the last quad again, not stored
    p[r] = ((const f32x4*)probs)[base + i];
    t[r] = load_target4<TT>(target, base + i);
  }
#pragma unroll
  for (int r = 0; r < kGradQuads; ++r) {
    f32x4 g;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float pv = p[r][k], tv = t[r][k], q = 1.f - pv;
      // the clamped logs have no slope at p = 0 / p = 1; v_rcp_f32 is within 1 ulp, the coefficients are rounded to fp32 anyway
      const float gp = pv > 0.f ? __builtin_amdgcn_rcpf(pv) : 0.f, gq = pv < 1.f ? __builtin_amdgcn_rcpf(q) : 0.f;
      g[k] = tv * -fmaf(c[0], gp, c[2]) + (1.f - tv) * fmaf(c[1], gq, c[3]);
    }
    if (first + r * kThreads < n4) ((f32x4*)dprobs)[base + first + r * kThreads] = g;
  }
}

int check_shape(const char* who, const void* probs, const void* target, int32_t target_dtype, int32_t batch, int64_t per_sample) {
  DD_REQUIRE(probs && target, DD_ERR_BAD_ARG, "%s: NULL pointer", who);
  DD_REQUIRE(batch >= 1 && per_sample > 0, DD_ERR_BAD_ARG, "%s: batch = %d and per_sample = %ld must be positive", who, batch, (long)per_sample);
  DD_REQUIRE(per_sample % 4 == 0 && per_sample <= ((int64_t)1 << 40) / batch, DD_ERR_UNSUPPORTED,
             "%s: per_sample = %ld must be a multiple of 4, batch * per_sample at most 2^40", who, (long)per_sample);
  DD_REQUIRE(target_dtype == DD_TARGET_F32 || target_dtype == DD_TARGET_U8, DD_ERR_UNSUPPORTED, "%s: unknown target dtype %d", who, target_dtype);
  DD_REQUIRE((uintptr_t)probs % 16 == 0 && (uintptr_t)target % (target_dtype == DD_TARGET_F32 ? 16 : 4) == 0, DD_ERR_BAD_ARG,
             "%s: misaligned buffer (probs and an fp32 target 16 bytes, a byte target 4)", who);
  return 0;
}

}  // namespace

extern "C" int64_t dd_box_loss_workspace_bytes(int32_t batch) {
  if (batch < 1) {
    dd_fail(DD_ERR_BAD_ARG, "box_loss_workspace_bytes: batch = %d must be positive", batch);
    return -1;
  }
  return (int64_t)batch * kMaxBlocksPerSample * kStats * (int64_t)sizeof(double);
}

extern "C" int dd_box_loss_fwd(const float* probs, const void* target, int32_t target_dtype, int32_t batch, int64_t per_sample,
                               float pos_weight, float bce_weight, float ts_weight, float ts_eps, float* loss_out, double* stats, float* coef,
                               void* workspace, void* stream) {
  if (int rc = check_shape("box_loss_fwd", probs, target, target_dtype, batch, per_sample)) return rc;
  DD_REQUIRE(loss_out && stats && coef && workspace, DD_ERR_BAD_ARG, "box_loss_fwd: NULL pointer");
  DD_REQUIRE((uintptr_t)loss_out % 4 == 0 && (uintptr_t)stats % 8 == 0 && (uintptr_t)coef % 16 == 0 && (uintptr_t)workspace % 8 == 0, DD_ERR_BAD_ARG,
             "box_loss_fwd: misaligned buffer (loss_out 4 bytes, stats and workspace 8, coef 16)");
  DD_REQUIRE(pos_weight > 0.f || pos_weight == DD_POS_WEIGHT_AUTO, DD_ERR_BAD_ARG, "box_loss_fwd: pos_weight = %g must be positive or DD_POS_WEIGHT_AUTO",
             (double)pos_weight);
  DD_REQUIRE(ts_eps >= 0.f && bce_weight >= 0.f && ts_weight >= 0.f, DD_ERR_BAD_ARG,
             "box_loss_fwd: ts_eps = %g, bce_weight = %g and ts_weight = %g must not be negative", (double)ts_eps, (double)bce_weight, (double)ts_weight);
  const long n4 = per_sample / 4;
  const int bps = stats_blocks(n4);
  DD_REQUIRE((long)batch * bps <= INT_MAX, DD_ERR_UNSUPPORTED, "box_loss_fwd: batch = %d needs too many workgroups", batch);
  const dim3 grid((unsigned)((long)batch * bps));
  double* partial = (double*)workspace;
  if (target_dtype == DD_TARGET_F32)
    hipLaunchKernelGGL(box_loss_stats_kernel<float>, grid, dim3(kThreads), 0, (hipStream_t)stream, probs, (const float*)target, n4, bps, partial);
  else
    hipLaunchKernelGGL(box_loss_stats_kernel<unsigned char>, grid, dim3(kThreads), 0, (hipStream_t)stream, probs, (const unsigned char*)target, n4, bps,
                       partial);
  DD_LAUNCH_CHECK("box_loss_fwd (statistics)");
  hipLaunchKernelGGL(box_loss_final_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (const double*)partial, batch, bps, (double)per_sample,
                     pos_weight, (double)bce_weight, (double)ts_weight, (double)ts_eps, stats, coef, loss_out);
  DD_LAUNCH_CHECK("box_loss_fwd (finalise)");
  return 0;
}

extern "C" int dd_box_loss_bwd(const float* probs, const void* target, int32_t target_dtype, int32_t batch, int64_t per_sample, const float* coef,
                               float grad_scale, float* dprobs, void* stream) {
  if (int rc = check_shape("box_loss_bwd", probs, target, target_dtype, batch, per_sample)) return rc;
  DD_REQUIRE(coef && dprobs, DD_ERR_BAD_ARG, "box_loss_bwd: NULL pointer");
  DD_REQUIRE((uintptr_t)coef % 16 == 0 && (uintptr_t)dprobs % 16 == 0, DD_ERR_BAD_ARG, "box_loss_bwd: coef and dprobs must be 16-byte aligned");
  const long n4 = per_sample / 4;
  const long gps = (n4 + kThreads * kGradQuads - 1) / (kThreads * kGradQuads);
  DD_REQUIRE(batch * gps <= INT_MAX, DD_ERR_UNSUPPORTED, "box_loss_bwd: %d x %ld elements need too many workgroups", batch, (long)per_sample);
  const dim3 grid((unsigned)(batch * gps));
  if (target_dtype == DD_TARGET_F32)
    hipLaunchKernelGGL(box_loss_grad_kernel<float>, grid, dim3(kThreads), 0, (hipStream_t)stream, probs, (const float*)target, coef, n4, (int)gps,
                       grad_scale, dprobs);
  else
    hipLaunchKernelGGL(box_loss_grad_kernel<unsigned char>, grid, dim3(kThreads), 0, (hipStream_t)stream, probs, (const unsigned char*)target, coef, n4,
                       (int)gps, grad_scale, dprobs);
  DD_LAUNCH_CHECK("box_loss_bwd");
  return 0;
}

// The device code box_loss.hip and rm_loss.hip share: both reduce five sums per sample (T, S, I, A, C) in a streaming pass and turn
// them into the loss terms and four gradient coefficients per sample in a one-workgroup finalise kernel.  No atomics, every sum has a
// fixed order.  All of it is forced inline: a kernel that calls these keeps the machine code it had with the text in its own file.
#pragma once
#include "dd_common.h"

// Four target bytes, loaded as one word, as fp32.
__device__ __forceinline__ f32x4 dd_bytes_f32x4(unsigned w) {
  return f32x4{(float)(w & 0xff), (float)((w >> 8) & 0xff), (float)((w >> 16) & 0xff), (float)(w >> 24)};
}

// The workgroup's totals of the threads' kStats sums, in a fixed order: the lanes of a wave by shuffle, then the four waves; thread
// k < kStats writes total k to out[k].
template <int kStats, int kThreads>
__device__ __forceinline__ void dd_block_sum(const double (&acc)[kStats], double* __restrict__ out) {
  __shared__ double red[kStats][kThreads / 64];
  static_assert(kThreads == 256, "dd_block_sum adds four waves");
#pragma unroll
  for (int k = 0; k < kStats; ++k) {
    double d = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_down(d, o);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = d;
  }
  __syncthreads();
  if (threadIdx.x < kStats) {
    const double* r = red[threadIdx.x];
    out[threadIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
  }
}

// One wave reduces sample b's partials in a finalise kernel: lane l adds those of workgroups l, l + 64, ... of the sample's n to its
// v[] (zeroed by the caller), then a shuffle tree leaves the kStats sums in lane 0.
template <int kStats>
__device__ __forceinline__ void dd_sample_sum(const double* partial, int b, int n, int lane, double (&v)[kStats]) {
  for (int j = lane; j < n; j += 64) {
#pragma unroll
    for (int k = 0; k < kStats; ++k) v[k] += partial[((long)b * n + j) * kStats + k];
  }
#pragma unroll
  for (int k = 0; k < kStats; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o);
  }
}

// Lane 0's step of a finalise kernel, from sample b's sums v = {T, S, I, A, C}: the weight (`auto_weight` is the file's sentinel for
// the sample's own negatives / positives), the two loss terms added to the wave's running bce and ts, the statistics and the four
// gradient coefficients stored.
__device__ __forceinline__ void dd_sample_finish(const double (&v)[5], int b, double per_sample, float pos_weight, float auto_weight, double alpha,
                                                 double beta, double eps, double inv_b, double inv_bp, double& bce, double& ts,
                                                 double* stats, float* coef) {
  const double T = v[0], S = v[1], I = v[2], A = v[3], Cq = v[4];
  const double w = pos_weight == auto_weight ? (per_sample - T) / fmax(T, 1.0) : (double)pos_weight;
  const double den = S + T - I + eps, num = I + eps;
  bce += w * A + Cq;
  ts += 1.0 - num / den;
#pragma unroll
  for (int k = 0; k < 5; ++k) stats[(long)b * 5 + k] = v[k];
  *(f32x4*)(coef + 4L * b) = f32x4{(float)(alpha * w * inv_bp), (float)(alpha * inv_bp), (float)(beta * inv_b / den),
                                   (float)(beta * inv_b * num / (den * den))};
}

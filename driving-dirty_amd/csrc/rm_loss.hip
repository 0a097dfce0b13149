// The road-map loss on the head's logits (include/dd_rm_loss.h; csrc/libdd_rm_loss.so, a library of its own):
//   dd_rm_loss_fwd / dd_rm_loss_fwd_u8_ptrs   weighted BCE-with-logits + soft threat score, the probabilities beside them
//   dd_rm_loss_bwd / dd_rm_loss_bwd_u8_ptrs   dL/dlogits from the saved probabilities
// The logit-domain counterpart of box_loss.hip, and the same plan (what the two share is dd_loss_stats.h): a statistics pass that reduces five sums per sample, from which the
// loss for ANY weight comes out (the per-sample "auto" weight needs T before it can weigh A), a finalise launch that turns them into
// four gradient coefficients per sample, and a gradient pass that divides by no statistic and calls no transcendental.
// Both big passes are streams.  A workgroup takes one piece of kChunk elements of ONE sample (the target's pointer -- a table entry in
// the _u8_ptrs forms -- depends on the workgroup alone and is read with scalar loads from the kernel arguments); a whole piece issues
// its 16-byte loads per lane of each operand before the first use (the statistics pass in two runs of kRun), a sample's last piece
// guards each vector.  Both paths
// compute a vector by the one function (`stat_quad` / `grad_quad`).
// No atomics, every sum has a fixed order: two launches give the same bits.  The probabilities are stored with plain stores: the
// backward reads them again while they may still be in the caches.
#include <limits.h>
#include <math.h>

#include "dd_loss_stats.h"

#include "../../include/dd_rm_loss.h"

namespace {

constexpr int kChunk = DD_RM_LOSS_CHUNK, kTableMax = DD_RM_LOSS_TABLE_MAX, kThreads = 256, kUnroll = kChunk / (4 * kThreads);
constexpr int kRun = 4;                    // vectors of the statistics pass whose loads are in flight together
constexpr int kStats = 5;                  // T, S, I, A, C
static_assert(kUnroll % kRun == 0, "a piece is a whole number of runs");
constexpr int kFinalThreads = 1024;        // the finalise launch: one workgroup of sixteen waves, a wave per sample in turn
static_assert(kUnroll * 4 * kThreads == kChunk && kUnroll >= 1 && kChunk % 1024 == 0, "a piece is a whole number of 16-byte vectors per lane");

// ---- the three forms of the target: where sample b's elements lie, and four of them as fp32
struct TargetF32 {
  const float* t;
  typedef const float* Sample;
  __device__ __forceinline__ Sample sample(int b, long per) const { return t + (long)b * per; }
  static __device__ __forceinline__ f32x4 quad(Sample s, long i) { return *(const f32x4*)(s + i); }
};
__device__ __forceinline__ f32x4 bytes4(const unsigned char* s, long i) { return dd_bytes_f32x4(*(const unsigned*)(s + i)); }
struct TargetU8 {
  const unsigned char* t;
  typedef const unsigned char* Sample;
  __device__ __forceinline__ Sample sample(int b, long per) const { return t + (long)b * per; }
  static __device__ __forceinline__ f32x4 quad(Sample s, long i) { return bytes4(s, i); }
};
struct TargetPtrs {      // by value in the kernel arguments
  const unsigned char* p[kTableMax];
  typedef const unsigned char* Sample;
  __device__ __forceinline__ Sample sample(int b, long) const { return p[b]; }
  static __device__ __forceinline__ f32x4 quad(Sample s, long i) { return bytes4(s, i); }
};

// THE per-vector function of the forward: the probabilities of four logits, and their terms added to the thread's fp32 sums
__device__ __forceinline__ f32x4 stat_quad(const f32x4 z, const f32x4 t, float (&s)[kStats]) {
  f32x4 p;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float sig, l1p;
    dd_sigmoid_softplus(z[k], sig, l1p);
    const float sp_pos = fmaxf(z[k], 0.f) + l1p, sp_neg = fmaxf(-z[k], 0.f) + l1p;
    s[0] += t[k];
    s[1] += sig;
    s[2] += sig * t[k];
    s[3] += t[k] * sp_neg;
    s[4] += (1.f - t[k]) * sp_pos;
    p[k] = sig;
  }
  return p;
}

// grid = batch * pps workgroups; workgroup g takes piece g % pps of sample g / pps and writes its five partials to partial[g][.].
template <typename Target>
__global__ __launch_bounds__(kThreads) void rm_loss_stats_kernel(const float* __restrict__ logits, const Target target, long per, int pps,
                                                                 float* __restrict__ probs, double* __restrict__ partial) {
  const int b = blockIdx.x / pps, piece = blockIdx.x - b * pps;
  const long off = (long)piece * kChunk;                       // < per
  const float* __restrict__ zs = logits + (long)b * per;
  float* __restrict__ ps = probs ? probs + (long)b * per : nullptr;
  const typename Target::Sample ts = target.sample(b, per);
  const long i0 = off + 4 * threadIdx.x;
  float s[kStats] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (off + kChunk <= per) {      // the same in every lane: a whole piece, in runs of kRun vectors: a run's loads first, all in flight
#pragma unroll 1                  // one run's registers, not the piece's: 32 elements' worth of temporaries cost half the occupancy
    for (int r = 0; r < kUnroll; r += kRun) {
      f32x4 zv[kRun], tv[kRun];
#pragma unroll
      for (int u = 0; u < kRun; ++u) {
        zv[u] = *(const f32x4*)(zs + i0 + (r + u) * 4 * kThreads);
        tv[u] = Target::quad(ts, i0 + (r + u) * 4 * kThreads);
      }
#pragma unroll
      for (int u = 0; u < kRun; ++u) {
        const f32x4 p = stat_quad(zv[u], tv[u], s);
        if (ps) *(f32x4*)(ps + i0 + (r + u) * 4 * kThreads) = p;
      }
    }
  } else {                     // the sample's last piece: every vector guarded
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const long i = i0 + u * 4 * kThreads;
      if (i < per) {              // i and per are multiples of 4: i + 4 <= per
        const f32x4 p = stat_quad(*(const f32x4*)(zs + i), Target::quad(ts, i), s);
        if (ps) *(f32x4*)(ps + i) = p;
      }
    }
  }
  double acc[kStats];
#pragma unroll
  for (int k = 0; k < kStats; ++k) acc[k] = (double)s[k];
  dd_block_sum<kStats, kThreads>(acc, partial + (long)blockIdx.x * kStats);
}

// One workgroup of sixteen waves; wave w takes the samples w, w + 16, ...: lane l adds the partials of pieces l, l + 64, ... of the
// sample, the lanes are added by shuffle, lane 0 writes the sample's statistics and coefficients and keeps the wave's share of the two
// loss terms; thread 0 adds the sixteen shares in order.
__global__ __launch_bounds__(kFinalThreads) void rm_loss_final_kernel(const double* __restrict__ partial, int batch, int pps, double per,
                                                                     float pos_weight, double alpha, double beta, double eps,
                                                                     double* __restrict__ stats, float* __restrict__ coef,
                                                                     float* __restrict__ loss_out) {
  constexpr int kWaves = kFinalThreads / 64;
  __shared__ double red[2][kWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double inv_b = 1.0 / (double)batch, inv_bp = 1.0 / ((double)batch * per);
  double bce = 0.0, ts = 0.0;
  for (int b = wave; b < batch; b += kWaves) {
    double v[kStats] = {0.0, 0.0, 0.0, 0.0, 0.0};
    dd_sample_sum(partial, b, pps, lane, v);
    if (lane == 0) dd_sample_finish(v, b, per, pos_weight, DD_RM_POS_WEIGHT_AUTO, alpha, beta, eps, inv_b, inv_bp, bce, ts, stats, coef);
  }
  if (lane == 0) {
    red[0][wave] = bce;
    red[1][wave] = ts;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sb = 0.0, st = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      sb += red[0][w];
      st += red[1][w];
    }
    const double l_bce = sb * inv_bp, l_ts = st * inv_b;
    loss_out[0] = (float)(alpha * l_bce + beta * l_ts);
    loss_out[1] = (float)l_bce;
    loss_out[2] = (float)l_ts;
  }
}

// THE per-vector function of the backward.  c = coef * grad_scale.  (1 - t) p (c1 + c3 q) - t q (c0 + c2 p) with q = 1 - p: the
// header's formula with p and q taken out of the brackets; for a 0 / 1 target one of the two products is an exact zero.
__device__ __forceinline__ f32x4 grad_quad(const f32x4 p, const f32x4 t, const f32x4 c) {
  f32x4 g;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float pv = p[k], tv = t[k], q = 1.f - pv;
    g[k] = (1.f - tv) * (pv * fmaf(c[3], q, c[1])) - tv * (q * fmaf(c[2], pv, c[0]));
  }
  return g;
}

// grid = batch * pps workgroups, the pieces of the statistics pass.
template <typename Target>
__global__ __launch_bounds__(kThreads) void rm_loss_grad_kernel(const float* __restrict__ probs, const Target target, const float* __restrict__ coef,
                                                                long per, int pps, float gscale, float* __restrict__ dlogits) {
  const int b = blockIdx.x / pps, piece = blockIdx.x - b * pps;
  const long off = (long)piece * kChunk;
  const float* __restrict__ ps = probs + (long)b * per;
  float* __restrict__ ds = dlogits + (long)b * per;
  const typename Target::Sample ts = target.sample(b, per);
  const f32x4 c = *(const f32x4*)(coef + 4L * b) * gscale;
  const long i0 = off + 4 * threadIdx.x;
  if (off + kChunk <= per) {
    f32x4 pv[kUnroll], tv[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      pv[u] = *(const f32x4*)(ps + i0 + u * 4 * kThreads);
      tv[u] = Target::quad(ts, i0 + u * 4 * kThreads);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) *(f32x4*)(ds + i0 + u * 4 * kThreads) = grad_quad(pv[u], tv[u], c);
  } else {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const long i = i0 + u * 4 * kThreads;
      if (i < per) *(f32x4*)(ds + i) = grad_quad(*(const f32x4*)(ps + i), Target::quad(ts, i), c);
    }
  }
}

// ---- the host side: every refusal before any device call
bool overlap(const void* a, const void* b, int64_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + (uintptr_t)bytes && y < x + (uintptr_t)bytes;
}

// 0, or the refusal.  `data`: the fp32 operand the pass reads (logits / probs), `out`: the one it writes (probs, may be NULL / dlogits).
int check_shape(const char* who, const char* data_name, const void* data, const char* out_name, const void* out, bool out_optional,
                int32_t batch, int64_t per) {
  DD_REQUIRE(data, DD_ERR_BAD_ARG, "%s: %s is NULL", who, data_name);
  DD_REQUIRE(out || out_optional, DD_ERR_BAD_ARG, "%s: %s is NULL", who, out_name);
  DD_REQUIRE(batch >= 1 && per > 0, DD_ERR_BAD_ARG, "%s: batch = %d and per_sample = %lld must be positive", who, batch, (long long)per);
  DD_REQUIRE(per % 4 == 0 && per <= ((int64_t)1 << 40) / batch, DD_ERR_UNSUPPORTED,
             "%s: per_sample = %lld must be a multiple of 4, batch * per_sample at most 2^40", who, (long long)per);
  DD_REQUIRE((uintptr_t)data % 16 == 0, DD_ERR_BAD_ARG, "%s: %s is not 16-byte aligned", who, data_name);
  DD_REQUIRE((uintptr_t)out % 16 == 0, DD_ERR_BAD_ARG, "%s: %s is not 16-byte aligned", who, out_name);
  DD_REQUIRE(!out || !overlap(data, out, (int64_t)batch * per * 4), DD_ERR_BAD_ARG, "%s: %s overlaps %s", who, out_name, data_name);
  return 0;
}

int check_stacked(const char* who, const void* target, int32_t kind) {
  DD_REQUIRE(target, DD_ERR_BAD_ARG, "%s: target is NULL", who);
  DD_REQUIRE(kind == DD_TARGET_F32 || kind == DD_TARGET_U8, DD_ERR_UNSUPPORTED, "%s: unknown target kind %d", who, kind);
  DD_REQUIRE((uintptr_t)target % (kind == DD_TARGET_F32 ? 16 : 4) == 0, DD_ERR_BAD_ARG, "%s: target is not %d-byte aligned", who,
             kind == DD_TARGET_F32 ? 16 : 4);
  return 0;
}

int check_table(const char* who, const unsigned char* const* ptrs, int32_t batch, TargetPtrs& tab) {
  DD_REQUIRE(ptrs, DD_ERR_BAD_ARG, "%s: target_ptrs is NULL", who);
  DD_REQUIRE(batch <= kTableMax, DD_ERR_UNSUPPORTED, "%s: batch = %d, a pointer table holds at most %d samples", who, batch, kTableMax);
  for (int i = 0; i < kTableMax; ++i) tab.p[i] = i < batch ? ptrs[i] : nullptr;
  for (int i = 0; i < batch; ++i) {
    DD_REQUIRE(tab.p[i], DD_ERR_BAD_ARG, "%s: target_ptrs[%d] is NULL", who, i);
    DD_REQUIRE((uintptr_t)tab.p[i] % 4 == 0, DD_ERR_BAD_ARG, "%s: target_ptrs[%d] is not 4-byte aligned", who, i);
  }
  return 0;
}

int pieces_per_sample(int64_t per) { return (int)((per + kChunk - 1) / kChunk); }      // <= 2^27: per <= 2^40

int check_fwd(const char* who, int32_t batch, int64_t per, float pos_weight, float bce_weight, float ts_weight, float ts_eps,
              const float* loss_out, const double* stats, const float* coef, const void* workspace, int64_t workspace_bytes) {
  DD_REQUIRE(loss_out, DD_ERR_BAD_ARG, "%s: loss_out is NULL", who);
  DD_REQUIRE(stats, DD_ERR_BAD_ARG, "%s: stats is NULL", who);
  DD_REQUIRE(coef, DD_ERR_BAD_ARG, "%s: coef is NULL", who);
  DD_REQUIRE(workspace, DD_ERR_BAD_ARG, "%s: workspace is NULL", who);
  DD_REQUIRE((uintptr_t)loss_out % 4 == 0, DD_ERR_BAD_ARG, "%s: loss_out is not 4-byte aligned", who);
  DD_REQUIRE((uintptr_t)stats % 8 == 0, DD_ERR_BAD_ARG, "%s: stats is not 8-byte aligned", who);
  DD_REQUIRE((uintptr_t)coef % 16 == 0, DD_ERR_BAD_ARG, "%s: coef is not 16-byte aligned", who);
  DD_REQUIRE((uintptr_t)workspace % 8 == 0, DD_ERR_BAD_ARG, "%s: workspace is not 8-byte aligned", who);
  // every comparison is false for a NaN
  DD_REQUIRE((pos_weight > 0.f && pos_weight < INFINITY) || pos_weight == DD_RM_POS_WEIGHT_AUTO, DD_ERR_BAD_ARG,
             "%s: pos_weight = %g must be positive and finite, or DD_RM_POS_WEIGHT_AUTO", who, (double)pos_weight);
  DD_REQUIRE(ts_eps >= 0.f && ts_eps < INFINITY, DD_ERR_BAD_ARG, "%s: ts_eps = %g must be finite and not negative", who, (double)ts_eps);
  DD_REQUIRE(bce_weight >= 0.f && bce_weight < INFINITY, DD_ERR_BAD_ARG, "%s: bce_weight = %g must be finite and not negative", who,
             (double)bce_weight);
  DD_REQUIRE(ts_weight >= 0.f && ts_weight < INFINITY, DD_ERR_BAD_ARG, "%s: ts_weight = %g must be finite and not negative", who,
             (double)ts_weight);
  const int64_t need = (int64_t)kStats * 8 * batch * pieces_per_sample(per);
  DD_REQUIRE(workspace_bytes >= need, DD_ERR_BAD_ARG, "%s: workspace_bytes = %lld, %d x %lld elements need %lld", who,
             (long long)workspace_bytes, batch, (long long)per, (long long)need);
  DD_REQUIRE((int64_t)batch * pieces_per_sample(per) <= INT_MAX, DD_ERR_UNSUPPORTED, "%s: %d x %lld elements need too many workgroups", who,
             batch, (long long)per);
  return 0;
}

template <typename Target>
int launch_fwd(const char* who, const float* logits, const Target& target, int32_t batch, int64_t per, float pos_weight, float bce_weight,
               float ts_weight, float ts_eps, float* probs, float* loss_out, double* stats, float* coef, void* workspace, void* stream) {
  const int pps = pieces_per_sample(per);
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(rm_loss_stats_kernel<Target>, dim3((unsigned)((long)batch * pps)), dim3(kThreads), 0, (hipStream_t)stream, logits, target,
                     (long)per, pps, probs, partial);
  DD_LAUNCH_CHECK(who);
  hipLaunchKernelGGL(rm_loss_final_kernel, dim3(1), dim3(kFinalThreads), 0, (hipStream_t)stream, (const double*)partial, batch, pps, (double)per,
                     pos_weight, (double)bce_weight, (double)ts_weight, (double)ts_eps, stats, coef, loss_out);
  DD_LAUNCH_CHECK(who);
  return 0;
}

int check_bwd(const char* who, int32_t batch, int64_t per, const float* coef, float grad_scale) {
  DD_REQUIRE(coef, DD_ERR_BAD_ARG, "%s: coef is NULL", who);
  DD_REQUIRE((uintptr_t)coef % 16 == 0, DD_ERR_BAD_ARG, "%s: coef is not 16-byte aligned", who);
  DD_REQUIRE(grad_scale == grad_scale, DD_ERR_BAD_ARG, "%s: grad_scale is NaN", who);
  DD_REQUIRE((int64_t)batch * pieces_per_sample(per) <= INT_MAX, DD_ERR_UNSUPPORTED, "%s: %d x %lld elements need too many workgroups", who,
             batch, (long long)per);
  return 0;
}

template <typename Target>
int launch_bwd(const char* who, const float* probs, const Target& target, int32_t batch, int64_t per, const float* coef, float grad_scale,
               float* dlogits, void* stream) {
  const int pps = pieces_per_sample(per);
  hipLaunchKernelGGL(rm_loss_grad_kernel<Target>, dim3((unsigned)((long)batch * pps)), dim3(kThreads), 0, (hipStream_t)stream, probs, target, coef,
                     (long)per, pps, grad_scale, dlogits);
  DD_LAUNCH_CHECK(who);
  return 0;
}

}  // namespace

extern "C" {

int dd_rm_loss_fwd(const float* logits, const void* target, int32_t target_kind, int32_t batch, int64_t per_sample, float pos_weight,
                   float bce_weight, float ts_weight, float ts_eps, float* probs, float* loss_out, double* stats, float* coef,
                   void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "rm_loss_fwd";
  if (int rc = check_shape(who, "logits", logits, "probs", probs, true, batch, per_sample)) return rc;
  if (int rc = check_stacked(who, target, target_kind)) return rc;
  if (int rc = check_fwd(who, batch, per_sample, pos_weight, bce_weight, ts_weight, ts_eps, loss_out, stats, coef, workspace, workspace_bytes))
    return rc;
  if (target_kind == DD_TARGET_F32)
    return launch_fwd(who, logits, TargetF32{(const float*)target}, batch, per_sample, pos_weight, bce_weight, ts_weight, ts_eps, probs, loss_out,
                      stats, coef, workspace, stream);
  return launch_fwd(who, logits, TargetU8{(const unsigned char*)target}, batch, per_sample, pos_weight, bce_weight, ts_weight, ts_eps, probs,
                    loss_out, stats, coef, workspace, stream);
}

int dd_rm_loss_fwd_u8_ptrs(const float* logits, const unsigned char* const* target_ptrs, int32_t batch, int64_t per_sample,
                           float pos_weight, float bce_weight, float ts_weight, float ts_eps, float* probs, float* loss_out, double* stats,
                           float* coef, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "rm_loss_fwd_u8_ptrs";
  TargetPtrs tab;
  if (int rc = check_shape(who, "logits", logits, "probs", probs, true, batch, per_sample)) return rc;
  if (int rc = check_table(who, target_ptrs, batch, tab)) return rc;
  if (int rc = check_fwd(who, batch, per_sample, pos_weight, bce_weight, ts_weight, ts_eps, loss_out, stats, coef, workspace, workspace_bytes))
    return rc;
  return launch_fwd(who, logits, tab, batch, per_sample, pos_weight, bce_weight, ts_weight, ts_eps, probs, loss_out, stats, coef, workspace, stream);
}

int dd_rm_loss_bwd(const float* probs, const void* target, int32_t target_kind, int32_t batch, int64_t per_sample, const float* coef,
                   float grad_scale, float* dlogits, void* stream) {
  const char* who = "rm_loss_bwd";
  if (int rc = check_shape(who, "probs", probs, "dlogits", dlogits, false, batch, per_sample)) return rc;
  if (int rc = check_stacked(who, target, target_kind)) return rc;
  if (int rc = check_bwd(who, batch, per_sample, coef, grad_scale)) return rc;
  if (target_kind == DD_TARGET_F32)
    return launch_bwd(who, probs, TargetF32{(const float*)target}, batch, per_sample, coef, grad_scale, dlogits, stream);
  return launch_bwd(who, probs, TargetU8{(const unsigned char*)target}, batch, per_sample, coef, grad_scale, dlogits, stream);
}

int dd_rm_loss_bwd_u8_ptrs(const float* probs, const unsigned char* const* target_ptrs, int32_t batch, int64_t per_sample,
                           const float* coef, float grad_scale, float* dlogits, void* stream) {
  const char* who = "rm_loss_bwd_u8_ptrs";
  TargetPtrs tab;
  if (int rc = check_shape(who, "probs", probs, "dlogits", dlogits, false, batch, per_sample)) return rc;
  if (int rc = check_table(who, target_ptrs, batch, tab)) return rc;
  if (int rc = check_bwd(who, batch, per_sample, coef, grad_scale)) return rc;
  return launch_bwd(who, probs, tab, batch, per_sample, coef, grad_scale, dlogits, stream);
}

}  // extern "C"

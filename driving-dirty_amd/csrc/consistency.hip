// The mirror consistency loss on pairs of logit maps (include/dd_consistency.h; csrc/libdd_consistency.so, a library of its own):
//   dd_cons_fwd        L = mean (P(a) - P(m'))^2 with m' = m's rows reversed, the per-pair sums Q_b and disagreement counts D_b
//   dd_cons_fwd_grad   the same pass, also writing dL/da and dL/dm
// ONE kernel template, `cons_kernel<GRAD, VEC>`: the gradient is a compile-time branch of the pass, so both entry points add the same
// terms in the same order and give the same bits of loss and stats.  The plan is rm_loss.hip's (what they share is dd_loss_stats.h): a
// workgroup takes one piece of kChunk elements of ONE pair and writes one fp64 partial pair; a one-workgroup finishing launch adds the
// pieces in a fixed order.  No atomics.
// A stream bound by memory: with the gradient it reads two maps and writes two.  A lane owns kUnroll groups of four consecutive
// elements, a sweep of the workgroup (4 * kThreads elements) apart, and issues every load of its piece before the first use: eight
// 16-byte loads in flight per lane (VEC), or thirty-two 4-byte ones.  Groups past the end of the pair are clamped to its last group for
// the load and skipped afterwards, so no load is behind a branch.  With w % 4 == 0 a group never straddles a row: its mirrored partner
// is four consecutive elements of the reversed row, one 16-byte access as well.  Both paths give an element to the same lane in the
// same order and compute it by the one function `cons_elem`: the same bits.
// The gradients are stored with plain stores: the backward reads them again while they may still be in the caches.
#include <limits.h>
#include <math.h>

#include "dd_loss_stats.h"

#include "../../include/dd_consistency.h"

#pragma clang fp contract(off)      // P(a) - P(m') is ONE rounded subtraction: the product that ends the sigmoid (e * r) is not fused into it

namespace {

constexpr int kChunk = DD_CONS_CHUNK, kThreads = 256, kSweep = 4 * kThreads, kUnroll = kChunk / kSweep;
constexpr int kStats = 2;                  // Q, D
constexpr int kFinalThreads = 1024;        // the finishing launch: one workgroup of sixteen waves, a wave per pair in turn
static_assert(kUnroll * kSweep == kChunk && kUnroll >= 1, "a piece is a whole number of sweeps");

// THE per-element function of every kernel below.  g = grad_scale * 2 / N.
template <bool GRAD>
__device__ __forceinline__ void cons_elem(float a, float m, float g, float& q, unsigned& dis, float& da, float& dm) {
  float pa, pm, l1p;
  dd_sigmoid_softplus(a, pa, l1p);      // the dense head's one sigmoid; the softplus half is dead code here
  dd_sigmoid_softplus(m, pm, l1p);
  const float d = pa - pm;
  q = fmaf(d, d, q);
  dis += (a > 0.f) != (m > 0.f) ? 1u : 0u;
  if constexpr (GRAD) {
    const float t = g * d;
    da = t * (pa * (1.f - pa));
    dm = -(t * (pm * (1.f - pm)));
  }
}

// offset in a pair of the mirrored partner of offset `i` = r * w + c: (h - 1 - r) * w + c.  All below 2^31; the difference wraps as it should.
__device__ __forceinline__ unsigned mirrored(unsigned i, unsigned h, unsigned w) { return i + (h - 1 - 2 * (i / w)) * w; }

// grid = batch * pps workgroups; workgroup x takes piece x % pps of pair x / pps and writes its two partials to partial[x][.].
template <bool GRAD, bool VEC>
__global__ __launch_bounds__(kThreads) void cons_kernel(const float* __restrict__ a, const float* __restrict__ m, unsigned h, unsigned w,
                                                        unsigned per, int pps, float g, float* __restrict__ da, float* __restrict__ dm,
                                                        double* __restrict__ partial) {
  const int b = blockIdx.x / pps, piece = blockIdx.x - b * pps;
  const long base = (long)b * per;
  const float* __restrict__ as = a + base;
  const float* __restrict__ ms = m + base;
  const unsigned i0 = (unsigned)piece * kChunk + 4 * threadIdx.x;      // piece * kChunk < per < 2^31: no group's offset wraps
  float q = 0.f;
  unsigned dis = 0;
  if constexpr (VEC) {      // per % 4 == 0: a group that begins below per ends there too
    f32x4 va[kUnroll], vm[kUnroll];
    unsigned im[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const unsigned i = min(i0 + u * kSweep, per - 4);      // past the end: the last group again, loaded and not used
      im[u] = mirrored(i, h, w);
      va[u] = *(const f32x4*)(as + i);
      vm[u] = *(const f32x4*)(ms + im[u]);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const unsigned i = i0 + u * kSweep;
      if (i >= per) continue;
      float ga[4], gm[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) cons_elem<GRAD>(va[u][k], vm[u][k], g, q, dis, ga[k], gm[k]);
      if constexpr (GRAD) {
        *(f32x4*)(da + base + i) = f32x4{ga[0], ga[1], ga[2], ga[3]};
        *(f32x4*)(dm + base + im[u]) = f32x4{gm[0], gm[1], gm[2], gm[3]};
      }
    }
  } else {
    float va[kUnroll][4], vm[kUnroll][4];
    unsigned im[kUnroll][4];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned i = min(i0 + u * kSweep + k, per - 1);      // past the end: the last element again, loaded and not used
        im[u][k] = mirrored(i, h, w);
        va[u][k] = as[i];
        vm[u][k] = ms[im[u][k]];
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned i = i0 + u * kSweep + k;
        if (i >= per) continue;
        float ga, gm;
        cons_elem<GRAD>(va[u][k], vm[u][k], g, q, dis, ga, gm);
        if constexpr (GRAD) {
          da[base + i] = ga;
          dm[base + im[u][k]] = gm;
        }
      }
    }
  }
  const double acc[kStats] = {(double)q, (double)dis};
  dd_block_sum<kStats, kThreads>(acc, partial + (long)blockIdx.x * kStats);
}

// One workgroup of sixteen waves; wave v takes the pairs v, v + 16, ...: lane l adds the partials of pieces l, l + 64, ... of the pair,
// the lanes are added by shuffle, lane 0 writes the pair's statistics and keeps the wave's share of the loss; thread 0 adds the
// sixteen shares in order.
__global__ __launch_bounds__(kFinalThreads) void cons_final_kernel(const double* __restrict__ partial, int batch, int pps, double inv_n,
                                                                   double* __restrict__ stats, float* __restrict__ loss) {
  constexpr int kWaves = kFinalThreads / 64;
  __shared__ double red[kWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double total = 0.0;
  for (int b = wave; b < batch; b += kWaves) {
    double v[kStats] = {0.0, 0.0};
    dd_sample_sum(partial, b, pps, lane, v);
    if (lane == 0) {
      stats[2L * b] = v[0];
      stats[2L * b + 1] = v[1];
      total += v[0];
    }
  }
  if (lane == 0) red[wave] = total;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) s += red[v];
    loss[0] = (float)(s * inv_n);
  }
}

// ---- the host side: every refusal before any device call
bool overlap(const void* p, const void* q, int64_t bytes) {
  const uintptr_t x = (uintptr_t)p, y = (uintptr_t)q;
  return x < y + (uintptr_t)bytes && y < x + (uintptr_t)bytes;
}

int pieces_per_pair(int64_t per) { return (int)((per + kChunk - 1) / kChunk); }      // < 2^19: per < 2^31

template <bool GRAD>
int launch(const char* who, const float* a, const float* m, int32_t batch, int32_t h, int32_t w, float grad_scale, float* da, float* dm,
           float* loss, double* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  DD_REQUIRE(a, DD_ERR_BAD_ARG, "%s: a is NULL", who);
  DD_REQUIRE(m, DD_ERR_BAD_ARG, "%s: m is NULL", who);
  DD_REQUIRE(!GRAD || da, DD_ERR_BAD_ARG, "%s: da is NULL", who);
  DD_REQUIRE(!GRAD || dm, DD_ERR_BAD_ARG, "%s: dm is NULL", who);
  DD_REQUIRE(loss, DD_ERR_BAD_ARG, "%s: loss is NULL", who);
  DD_REQUIRE(stats, DD_ERR_BAD_ARG, "%s: stats is NULL", who);
  DD_REQUIRE(workspace, DD_ERR_BAD_ARG, "%s: workspace is NULL", who);
  DD_REQUIRE(batch >= 1 && h >= 1 && w >= 1, DD_ERR_BAD_ARG, "%s: batch = %d, h = %d and w = %d must be positive", who, batch, h, w);
  const int64_t per = (int64_t)h * w;
  DD_REQUIRE(per < ((int64_t)1 << 31) && per <= ((int64_t)1 << 40) / batch, DD_ERR_UNSUPPORTED,
             "%s: [%d,%d,%d] is too large: h * w must stay below 2^31, batch * h * w at most 2^40", who, batch, h, w);
  DD_REQUIRE((uintptr_t)a % 4 == 0, DD_ERR_BAD_ARG, "%s: a is not 4-byte aligned", who);
  DD_REQUIRE((uintptr_t)m % 4 == 0, DD_ERR_BAD_ARG, "%s: m is not 4-byte aligned", who);
  DD_REQUIRE((uintptr_t)da % 4 == 0, DD_ERR_BAD_ARG, "%s: da is not 4-byte aligned", who);
  DD_REQUIRE((uintptr_t)dm % 4 == 0, DD_ERR_BAD_ARG, "%s: dm is not 4-byte aligned", who);
  DD_REQUIRE((uintptr_t)loss % 4 == 0, DD_ERR_BAD_ARG, "%s: loss is not 4-byte aligned", who);
  DD_REQUIRE((uintptr_t)stats % 8 == 0, DD_ERR_BAD_ARG, "%s: stats is not 8-byte aligned", who);
  DD_REQUIRE((uintptr_t)workspace % 8 == 0, DD_ERR_BAD_ARG, "%s: workspace is not 8-byte aligned", who);
  DD_REQUIRE(grad_scale - grad_scale == 0.f, DD_ERR_BAD_ARG, "%s: grad_scale = %g must be finite", who, (double)grad_scale);      // false for a NaN too
  const int pps = pieces_per_pair(per);
  const int64_t need = (int64_t)kStats * 8 * batch * pps;
  DD_REQUIRE(workspace_bytes >= need, DD_ERR_BAD_ARG, "%s: workspace_bytes = %lld, %d x %lld elements need %lld", who,
             (long long)workspace_bytes, batch, (long long)per, (long long)need);
  DD_REQUIRE((int64_t)batch * pps <= INT_MAX, DD_ERR_UNSUPPORTED, "%s: %d x %lld elements need too many workgroups", who, batch, (long long)per);
  if constexpr (GRAD) {
    const int64_t bytes = (int64_t)batch * per * 4;
    DD_REQUIRE(!overlap(da, a, bytes) && !overlap(da, m, bytes), DD_ERR_BAD_ARG,
               "%s: da overlaps an input: the row reversal cannot be done in place", who);
    DD_REQUIRE(!overlap(dm, a, bytes) && !overlap(dm, m, bytes), DD_ERR_BAD_ARG,
               "%s: dm overlaps an input: the row reversal cannot be done in place", who);
    DD_REQUIRE(!overlap(da, dm, bytes), DD_ERR_BAD_ARG, "%s: da overlaps dm", who);
  }
  const bool vec = w % 4 == 0 && (((uintptr_t)a | (uintptr_t)m | (uintptr_t)da | (uintptr_t)dm) & 15) == 0;
  const float g = (float)(2.0 * (double)grad_scale / ((double)batch * (double)per));
  double* partial = (double*)workspace;
  const dim3 grid((unsigned)((long)batch * pps)), block(kThreads);
  if (vec)
    hipLaunchKernelGGL((cons_kernel<GRAD, true>), grid, block, 0, (hipStream_t)stream, a, m, (unsigned)h, (unsigned)w, (unsigned)per, pps, g, da,
                       dm, partial);
  else
    hipLaunchKernelGGL((cons_kernel<GRAD, false>), grid, block, 0, (hipStream_t)stream, a, m, (unsigned)h, (unsigned)w, (unsigned)per, pps, g, da,
                       dm, partial);
  DD_LAUNCH_CHECK(who);
  hipLaunchKernelGGL(cons_final_kernel, dim3(1), dim3(kFinalThreads), 0, (hipStream_t)stream, (const double*)partial, batch, pps,
                     1.0 / ((double)batch * (double)per), stats, loss);
  DD_LAUNCH_CHECK(who);
  return 0;
}

}  // namespace

extern "C" {

int dd_cons_fwd(const float* a, const float* m, int32_t batch, int32_t h, int32_t w, float* loss, double* stats, void* workspace,
                int64_t workspace_bytes, void* stream) {
  return launch<false>("cons_fwd", a, m, batch, h, w, 0.f, nullptr, nullptr, loss, stats, workspace, workspace_bytes, stream);
}

int dd_cons_fwd_grad(const float* a, const float* m, int32_t batch, int32_t h, int32_t w, float grad_scale, float* da, float* dm, float* loss,
                     double* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  return launch<true>("cons_fwd_grad", a, m, batch, h, w, grad_scale, da, dm, loss, stats, workspace, workspace_bytes, stream);
}

}  // extern "C"

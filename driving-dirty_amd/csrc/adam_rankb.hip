// dd_adam_step_rankb: the Adam pass of a big Linear weight with its weight gradient formed INSIDE the pass.
//
// The weight gradient of a Linear layer over an M-row batch is a rank-M product, dW[n][k] = sum_b dY[b][n] X[b][k] with M <= 32
// per GPU (M = world x batch when the factors were all-gathered: ddp.GradSync factor mode).  For the three tensors that ARE the
// optimizer's traffic -- the encoder's fc1 940032 -> 128 (reference components.py:27,105; 481 MB), the road-map head 64 -> 640000
// (roadmap_bce_v2.py:50,75; 164 MB), the decoder's fc2 128 -> 1253376 (components.py:70; 642 MB) -- writing dW (dd_linear_wgrad) and
// reading it back (dd_adam_step) are two full passes over the largest tensors of the step that nothing needs: here every gradient
// element is produced in MFMA accumulators from M products and consumed by the Adam update of the same lane.  HBM traffic per element:
// p, m, v read + written = 6 passes (24 B) instead of 8 (wgrad's write + Adam's 7), plus the factors (X: 120 MB for fc1, dY: 82 MB for
// the head), which the weight-gradient kernel read too.
//
// Shape.  The pass runs BESIDE the conv backward (optim.HipAdam, side stream), whose one-wave-per-SIMD kernels leave 48 of a SIMD's
// 512 registers: so one persistent workgroup per CU and a wave tile small enough for that budget -- 16 output rows x
// 64 columns in four v_mfma_f32_16x16x4_f32 accumulators (16 registers).  Lane (r = lane & 15, q = lane >> 4) loads 16 bytes
// X[4s + q][k0 + 4r .. 4r + 3] per contraction step: four B operands whose "column j" is the strided set {4j + c}, so accumulator c
// register i holds dW[n0 + 4q + i][k0 + 4r + c] and the four accumulators give each lane FOUR CONSECUTIVE columns of a row:
// p / m / v move as 16-byte accesses, 256 contiguous bytes per quarter-wave.  Tiles are numbered n-tile fastest, so the waves of a
// workgroup (and of its neighbour) share one X tile through the caches while each streams its own rows of p, m, v.
//
// The bias of the layer (optional): its gradient is the column sum of dY, which the k0 = 0 tile of every n-tile has in registers
// anyway; that wave applies the same Adam update to bias / its moments -- no second pass over dY (82 MB for the head), no ATen sum.
#include <math.h>
#include <stdlib.h>

#include "dd_common.h"
#include "dd_adam.h"

namespace {

// DD_MFMA16 here: this file is compiled with -mllvm -amdgpu-mfma-vgpr-form (build.py): the accumulators stay in
// ordinary vector registers -- left to the default the four accumulators go to the accumulation registers and are COPIED to vector
// registers for the epilogue: 32 registers for 16, and the whole kernel has 72.

struct RankbArgs {
  float* p;
  float* m;
  float* v;
  const float* dy;
  const float* x;
  float* bp;
  float* bm;
  float* bv;
  int M, N, K;
  int ntile_n, ntile_k;
  int per;                 // group-tiles per workgroup: workgroup b takes [b * per, (b + 1) * per) of the (n-group, k-tile) list, k fastest
  int total;               // ceil(ntile_n / 4) * ntile_k group-tiles
  float b1, b2, omb1, omb2, eps, step_size, inv_bc2, bc2_sqrt, gscale;
};

// ---- the LDS form: the shipped one ------------------------------------------------------------------------------------------------
// Same tile, same order, same arithmetic; what changes is how often a wave waits for memory.  Beside the conv backward a round trip to
// HBM takes 2-3 us, and the form above makes four per tile (two batches of factor loads, two of p / m / v): 1.5 TB/s in the step where
// the plain Adam kernel moves 2.3.  Here the workgroup's X tile (32 batch rows x 64 columns, 8 KB, shared by its four waves) is loaded
// ONE TILE AHEAD into 8 registers per lane while the current tile's p / m / v are on their way, and passes through LDS; the workgroup's
// dY tile (batch rows x 64 outputs) is loaded once per n-group -- the waves stay on their rows while they walk along k -- and stays in
// LDS.  A tile then costs the two round trips of its p / m / v and nothing else.  MC = 32-row chunks of the batch (1: rows <= 32; 2:
// rows <= 64, the gathered factors of two ranks); LDS 8 KB (X) + MC x 8 KB (dY): fits beside the c2 weight gradient's 133 KB.
// The tile epilogue shared by the two LDS forms: accumulator c, register i of lane (r, q) is dW[16 nt + 4q + i][64 kt + 4r + c]; p / m / v of
// RG rows per lane are in flight together (one round trip per RG rows, 12 registers per row).
template <int RG>
__device__ __forceinline__ void rankb_epilogue(const RankbArgs& a, int nt, int kt, const f32x4& acc0, const f32x4& acc1, const f32x4& acc2,
                                               const f32x4& acc3) {
  const int lane = dd_fresh_lane();
  const int r = lane & 15, q = lane >> 4;
  const long tile = (long)nt * 16 * a.K + kt * 64;
  const long left = ((long)a.N * a.K - tile) * 4;          // bytes from the tile's first element to the end of the tensor
  const int span = (int)min(left, (long)16 * a.K * 4);    // 16 rows: < 2^31 (host check); rows past N: out of range, dropped
  const __amdgpu_buffer_rsrc_t ps = dd_rsrc(a.p + tile, span), ms = dd_rsrc(a.m + tile, span), vs = dd_rsrc(a.v + tile, span);
  if (kt * 64 + 4 * r >= a.K) return;                     // K % 4 == 0: a 16-byte group is all in or all out
  const int off = (4 * q * a.K + 4 * r) * 4;
#pragma unroll
  for (int i0 = 0; i0 < 4; i0 += RG) {
    f32x4 pa[RG], ma[RG], va[RG];
#pragma unroll
    for (int j = 0; j < RG; ++j) {
      const int so = (i0 + j) * a.K * 4;
      pa[j] = dd_bload4<DD_AUX_NT>(ps, off, so);
      ma[j] = dd_bload4<DD_AUX_NT>(ms, off, so);
      va[j] = dd_bload4<DD_AUX_NT>(vs, off, so);
    }
#pragma unroll
    for (int j = 0; j < RG; ++j) {
      const int i = i0 + j, so = i * a.K * 4;
      const f32x4 g = {acc0[i], acc1[i], acc2[i], acc3[i]};
#pragma unroll
      for (int cc = 0; cc < 4; cc += 2) {
        f32x2 pe = {pa[j][cc], pa[j][cc + 1]}, me = {ma[j][cc], ma[j][cc + 1]}, ve = {va[j][cc], va[j][cc + 1]};
        adam_elem2(pe, me, ve, f32x2{g[cc], g[cc + 1]}, a.gscale, a.b1, a.b2, a.omb1, a.omb2, a.eps, a.step_size, a.inv_bc2);
        pa[j][cc] = pe.x; pa[j][cc + 1] = pe.y; ma[j][cc] = me.x; ma[j][cc + 1] = me.y; va[j][cc] = ve.x; va[j][cc + 1] = ve.y;
      }
      dd_bstore<DD_AUX_NT>(ps, off, pa[j], so);
      dd_bstore<DD_AUX_NT>(ms, off, ma[j], so);
      dd_bstore<DD_AUX_NT>(vs, off, va[j], so);
    }
  }
}

// bias[16 nt .. 16 nt + 15] from the column sums of the dY tile in LDS (the k-tile-0 wave of an n-tile owns them)
__device__ __forceinline__ void rankb_bias(const RankbArgs& a, const float* yl, int nt, int wave) {
  const int lane = dd_fresh_lane();
  const int r = lane & 15, nn = nt * 16 + r;
  if ((lane >> 4) != 0 || nn >= a.N) return;
  float tot = 0.f;
  for (int m = 0; m < a.M; ++m) tot += yl[m * 64 + ((16 * wave + r) ^ (16 * (m & 3)))];
  float pe = a.bp[nn], me = a.bm[nn], ve = a.bv[nn];
  adam_elem(pe, me, ve, tot, a.gscale, a.b1, a.b2, a.eps, a.step_size, a.bc2_sqrt);
  a.bp[nn] = pe; a.bm[nn] = me; a.bv[nn] = ve;
}

// contraction over one 32-row chunk: A = dY (yp: this lane's column, swizzled), B = X (xp: this lane's 4 columns), both from LDS
template <int XS = 64>      // XS: floats of a batch row of the X tile in LDS
__device__ __forceinline__ void rankb_mfma_chunk(const float* yp, const float* xp, int rows_left, f32x4& acc0, f32x4& acc1, f32x4& acc2,
                                                 f32x4& acc3) {
  const int pairs = min(4, (rows_left + 7) / 8);          // two contraction steps per trip (rows past M are zeros in LDS): the second
  for (int s = 0; s < 2 * pairs; s += 2) {                // pair of LDS reads is issued under the first four MFMAs
    const float av0 = yp[s * 256], av1 = yp[s * 256 + 256];
    const f32x4 bv0 = *(const f32x4*)(xp + s * 4 * XS), bv1 = *(const f32x4*)(xp + (s + 1) * 4 * XS);
    acc0 = DD_MFMA16(av0, bv0.x, acc0);
    acc1 = DD_MFMA16(av0, bv0.y, acc1);
    acc2 = DD_MFMA16(av0, bv0.z, acc2);
    acc3 = DD_MFMA16(av0, bv0.w, acc3);
    acc0 = DD_MFMA16(av1, bv1.x, acc0);
    acc1 = DD_MFMA16(av1, bv1.y, acc1);
    acc2 = DD_MFMA16(av1, bv1.z, acc2);
    acc3 = DD_MFMA16(av1, bv1.w, acc3);
  }
}

// ---- the kernels (adam_rankb_kernels.inc), twice ----------------------------------------------------------------------------------
// adam_rankb_*: the scale arrives by value in RankbArgs (dd_adam_step_rankb; these run beside the conv backward and keep its budget).
#define RANKB_KERNEL(name) __global__ __launch_bounds__(256) void adam_rankb_##name(const RankbArgs a)
#define RANKB_ENTER
#include "adam_rankb_kernels.inc"
#undef RANKB_KERNEL
#undef RANKB_ENTER
// devscale_*: the scale is read from device memory when the kernel starts (dd_adam_step_rankb_dev: what dd_clip_scale wrote earlier on
// the stream) -- one uniform load into the argument block's copy, then the same text: the same scale gives the same bits.  A clipped step
// runs its passes after the backward, by themselves (HipAdam.set_clip refuses the side stream): these have no budget to keep.
#define RANKB_KERNEL(name) __global__ __launch_bounds__(256) void devscale_##name(RankbArgs a, const float* __restrict__ gscale_dev)
#define RANKB_ENTER a.gscale = gscale_dev[0];
#include "adam_rankb_kernels.inc"
#undef RANKB_KERNEL
#undef RANKB_ENTER

// dd_adam_step_rankb / dd_adam_step_rankb_dev: one host path, the scale by value or -- gscale_dev -- read by the kernel
int rankb_launch(float* p, float* m, float* v, const float* dy, const float* x, int32_t rows, int32_t n, int32_t k,
                 float* bias_p, float* bias_m, float* bias_v, float lr, float beta1, float beta2, float eps, int32_t step,
                 float grad_scale, const float* gscale_dev, void* stream) {
  DD_REQUIRE(p && m && v && dy && x && step >= 1, DD_ERR_BAD_ARG, "adam_rankb: bad argument");
  DD_REQUIRE(rows > 0 && n > 0 && k > 0, DD_ERR_BAD_ARG, "adam_rankb: non-positive size");
  DD_REQUIRE(rows <= 64, DD_ERR_UNSUPPORTED, "adam_rankb: %d batch rows > 64", rows);
  DD_REQUIRE(k % 4 == 0 && n % 4 == 0, DD_ERR_UNSUPPORTED, "adam_rankb: N = %d and K = %d must be multiples of 4", n, k);
  DD_REQUIRE(((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)x | (uintptr_t)dy) % 16 == 0, DD_ERR_BAD_ARG, "adam_rankb: buffers must be 16-byte aligned");
  DD_REQUIRE((bias_p != nullptr) == (bias_m != nullptr) && (bias_p != nullptr) == (bias_v != nullptr), DD_ERR_BAD_ARG,
             "adam_rankb: bias, its exp_avg and exp_avg_sq come together or not at all");
  DD_REQUIRE((int64_t)(rows + 4) * n < ((int64_t)1 << 29) && (int64_t)(rows + 4) * k < ((int64_t)1 << 29) && (int64_t)16 * k < ((int64_t)1 << 29),
             DD_ERR_UNSUPPORTED, "adam_rankb: factors of 2 GB or more");
  const AdamBias bc = adam_bias(beta1, beta2, step);
  RankbArgs a;
  a.p = p; a.m = m; a.v = v; a.dy = dy; a.x = x; a.bp = bias_p; a.bm = bias_m; a.bv = bias_v;
  a.M = rows; a.N = n; a.K = k;
  a.ntile_n = (n + 15) / 16;
  a.ntile_k = (k + 63) / 64;
  a.b1 = beta1; a.b2 = beta2; a.eps = eps;
  a.omb1 = 1.f - beta1; a.omb2 = 1.f - beta2;
  a.step_size = lr / bc.bc1;
  a.bc2_sqrt = bc.bc2_sqrt;
  a.inv_bc2 = 1.f / a.bc2_sqrt;
  a.gscale = grad_scale;
  const bool short_rows = rows <= 32 && a.ntile_k == 1;      // adam_rankb_short_kernel: its work list is of n-groups
  // the pass by itself (more than one workgroup per CU: nothing to fit beside) on long rows: 16-row x 256-column tiles
  const bool wide = rows <= 32 && !short_rows && a.ntile_k >= 64 && dd_adam_blocks_internal() > 1;
  const long total = wide ? (long)a.ntile_n * ((k + 255) / 256) : (long)((a.ntile_n + 3) / 4) * (short_rows ? 1 : a.ntile_k);
  DD_REQUIRE(total < ((long)1 << 31), DD_ERR_UNSUPPORTED, "adam_rankb: too many tiles");
  a.total = (int)total;
  // one persistent workgroup per CU, as dd_adam_step (adam_stream_grid, dd_adam.h): nothing of this launch is ever queued ahead of a conv kernel
  const int per_cu = dd_adam_blocks_internal();
  const int grid = (int)min(total, (long)max(DD_NUM_CU - dd_adam_spare_internal(), 1) * per_cu);
  a.per = (int)((total + grid - 1) / grid);
  hipStream_t st = (hipStream_t)stream;
  // (two k-tiles per group -- the decoder's fc2, K = 128 -- ran on a <2, RG = 1> build of the short form (its RG = 2 build needs 76 registers):
  // 2.98 ms beside the conv backward for 0.80 alone; the long-row form below keeps two rows of p / m / v in flight for it)
  if (gscale_dev) {
    if (wide) hipLaunchKernelGGL(devscale_wide_kernel, dim3(grid), dim3(256), 0, st, a, gscale_dev);
    else if (short_rows) hipLaunchKernelGGL((devscale_short_kernel<1, 2>), dim3(grid), dim3(256), 0, st, a, gscale_dev);
    else if (rows <= 32) hipLaunchKernelGGL((devscale_lds_kernel<1, 2>), dim3(grid), dim3(256), 0, st, a, gscale_dev);
    else hipLaunchKernelGGL((devscale_lds_kernel<2, 1>), dim3(grid), dim3(256), 0, st, a, gscale_dev);
  }
  else if (wide) hipLaunchKernelGGL(adam_rankb_wide_kernel, dim3(grid), dim3(256), 0, st, a);
  else if (short_rows) hipLaunchKernelGGL((adam_rankb_short_kernel<1, 2>), dim3(grid), dim3(256), 0, st, a);
  else if (rows <= 32) hipLaunchKernelGGL((adam_rankb_lds_kernel<1, 2>), dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((adam_rankb_lds_kernel<2, 1>), dim3(grid), dim3(256), 0, st, a);
  DD_LAUNCH_CHECK("adam_rankb");
  return 0;
}

}  // namespace

extern "C" {

int dd_adam_step_rankb(float* p, float* m, float* v, const float* dy, const float* x, int32_t rows, int32_t n, int32_t k,
                       float* bias_p, float* bias_m, float* bias_v, float lr, float beta1, float beta2, float eps, int32_t step,
                       float grad_scale, void* stream) {
  return rankb_launch(p, m, v, dy, x, rows, n, k, bias_p, bias_m, bias_v, lr, beta1, beta2, eps, step, grad_scale, nullptr, stream);
}

int dd_adam_step_rankb_dev(float* p, float* m, float* v, const float* dy, const float* x, int32_t rows, int32_t n, int32_t k,
                           float* bias_p, float* bias_m, float* bias_v, float lr, float beta1, float beta2, float eps, int32_t step,
                           const float* grad_scale_dev, void* stream) {
  DD_REQUIRE(grad_scale_dev && (uintptr_t)grad_scale_dev % 4 == 0, DD_ERR_BAD_ARG, "adam_rankb_dev: bad argument");
  return rankb_launch(p, m, v, dy, x, rows, n, k, bias_p, bias_m, bias_v, lr, beta1, beta2, eps, step, 0.f, grad_scale_dev, stream);
}

}  // extern "C"

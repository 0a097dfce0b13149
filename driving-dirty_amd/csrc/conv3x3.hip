// 3x3 convolution family for the encoder conv stack (reference src/autoencoder/components.py:19-21,41-43)
// as implicit GEMM on the fp32 matrix cores of gfx950 (v_mfma_f32_32x32x2_f32), NHWC activations.
//
// Decomposition ("strip marching"): one WAVE owns a strip of 32 output pixels and marches down the rows of
// an image column.  It keeps the three input rows a 3x3 window needs in its own LDS ring (3 slots),
// prefetches the next row(s) into registers while the matrix cores work on the current row, and never
// synchronises with another wave: no barrier in the main loop.  The GEMM view is M = 32 pixels, N = 32
// output channels, K = 9 taps x Cin; the fp32 MFMA issues once per 64 cycles per SIMD, so LDS (2 x
// ds_read_b128 per 4 MFMAs) and HBM (one 4.3 KB row per 9216 MFMA cycles) are far from binding: the kernels
// are MFMA-issue bound by construction.
//
// Scheduling: the grid is exactly the number of resident workgroups; the B*strips*rows "row tiles" are cut
// into one contiguous, equal range per wave (an image column after the other), so every wave does the same
// number of MFMAs and pays a ring prologue only where its range starts or crosses into the next column.
//
// Memory addressing: every global access is a raw buffer load/store whose descriptor covers ONE image row
// (or zero bytes for a row outside the image).  Out-of-image pixels are then hardware range-check zeros /
// dropped stores: no clamps, no selects, no branches around memory instructions, and an indexing bug cannot
// fault the GPU.
//
//   conv_strip_fwd <CIN,S,EPI>  forward (bias+ReLU epilogue) and stride-1 data gradient (ReLU-mask epilogue)
//   conv_s2_dgrad               data gradient of the stride-2 conv, by output parity class (no zero insertion)
//   conv_wgrad <CIN,S>          weight + bias gradient, register accumulators, deterministic two-stage reduction
// These serve c1, c3, the BatchNorm variants and every stride-1 data gradient (ring and row loaders: dd_conv_strip.h).  c2's Winograd families,
// conv_wino2.inc (default) and conv_wino.inc, are files of their own compiled INTO this translation unit (included at the end): hipcc derives the
// argument ranges of the shared helpers from ALL their call sites in a translation unit, and apart 16 kernels get other address code.
#include <stdlib.h>

#include "dd_conv_strip.h"

namespace {

// ------------------------------------------------------------------------------------------------
// forward / stride-1 dgrad
// ------------------------------------------------------------------------------------------------
template <int CIN, int S, int EPI, int WPB, bool AFF = false>
__global__ __launch_bounds__(WPB * 64) void conv_strip_fwd(const float* __restrict__ x, const float* __restrict__ wp,
                                                           const float* __restrict__ bias,
                                                           const float* __restrict__ msk, float* __restrict__ y,
                                                           unsigned* __restrict__ bits_out, int B, int H, int W, int Ho,
                                                           int Wo, int nstrips, const float* __restrict__ aff = nullptr,
                                                           float* __restrict__ stats = nullptr) {
  using C = StripCfg<CIN, S>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  {
    f32x4* wl4 = (f32x4*)smem;
    const f32x4* wg4 = (const f32x4*)wp;
    for (int i = tid; i < C::WFLOATS / 4; i += WPB * 64) wl4[i] = wg4[i];
  }
  __syncthreads();
  char* ring = smem + C::WFLOATS * 4 + wave * C::WAVEB;
  char* spill = ring + 3 * C::SLOTB;
  const char* wl = smem;
  const int h = lane >> 5, n = lane & 31;
  const float bv = (EPI == DD_EPI_BIAS || EPI == DD_EPI_BIAS_RELU || EPI == EPI_BIAS_RELU_BITS || EPI == EPI_BIAS_STATS) ? bias[n] : 0.f;
  f32x4 asc = {1.f, 1.f, 1.f, 1.f}, ash = {0.f, 0.f, 0.f, 0.f};
  if (AFF) {
    asc = *(const f32x4*)(aff + 4 * (lane & 7));
    ash = *(const f32x4*)(aff + 32 + 4 * (lane & 7));
  }
  const float msc = (EPI == EPI_RELU_MASK_AFF) ? aff[64 + n] : 1.f, msh = (EPI == EPI_RELU_MASK_AFF) ? aff[96 + n] : 0.f;
  float st_n = 0.f, st_piv = 0.f, st_sum = 0.f, st_sq = 0.f;   // batch statistics of this lane's channel about its first value (DdMoments)

  long idx, end;
  dd_range((long)B * nstrips * Ho, blockIdx.x * WPB + wave, gridDim.x * WPB, idx, end);
  while (idx < end) {
    const long col = idx / Ho;
    const int y0 = (int)(idx - col * Ho);
    const int y1 = (int)min((long)Ho, y0 + (end - idx));
    idx += y1 - y0;
    const int b = (int)(col / nstrips), x0 = (int)(col % nstrips) * 32;
    const float* xb = x + (long)b * H * W * CIN;
    const int gx0 = S * x0 - 1;

#pragma unroll
    for (int d = 0; d < 3; ++d) {   // prologue: the three rows output row y0 needs
      f32x4 t[C::NLOAD];
      const int iy = S * y0 - 1 + d;
      load_row<CIN, S>(xb, H, W, iy, gx0, lane, t);
      if constexpr (AFF) store_row_aff<S, true>(ring + ((iy + 1) % 3) * C::SLOTB, spill, lane, t, iy >= 0 && iy < H, gx0, W, asc, ash);
      else store_row<CIN, S, true>(ring + ((iy + 1) % 3) * C::SLOTB, spill, lane, t);
    }

    for (int yy = y0; yy < y1; ++yy) {
      // prefetch the S new input rows output row yy+1 needs (in flight under the MFMAs below)
      f32x4 pre[S][C::NLOAD];
#pragma unroll
      for (int s = 0; s < S; ++s) load_row<CIN, S>(xb, H, W, S * yy + 2 + s, gx0, lane, pre[s]);

      const long orow = ((long)(b * Ho + yy) * Wo) * 32;
      float mreg[16];
      if (EPI == DD_EPI_RELU_MASK || EPI == EPI_RELU_MASK_AFF) {
        const __amdgpu_buffer_rsrc_t ms = dd_rsrc(msk + orow, Wo * 128);
#pragma unroll
        for (int r = 0; r < 16; ++r) mreg[r] = dd_bload1<DD_AUX_NT>(ms, ((x0 + dd_acc_row(r, lane)) * 32 + n) * 4);
      }
      if (EPI == EPI_RELU_BITS) {   // one uint32 per pixel: 32x fewer mask bytes than the fp32 activation
        const __amdgpu_buffer_rsrc_t ms = dd_rsrc((const unsigned*)msk + (long)(b * Ho + yy) * Wo, Wo * 4);
#pragma unroll
        for (int r = 0; r < 16; ++r) mreg[r] = dd_bload1<DD_AUX_NT>(ms, (x0 + dd_acc_row(r, lane)) * 4);
      }
      // keep the loads ABOVE the MFMA chain: left alone, hipcc sinks them to their first use (the ring store
      // behind the chain) and the wave then eats a full HBM round trip per row
      __builtin_amdgcn_sched_barrier(0);

      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;

      if (CIN == 32) {
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
          const char* rowb = ring + ((S * yy + dy) % 3) * C::SLOTB;   // slot of input row S*yy-1+dy
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const int q = S * n + dx;
            const char* pa = rowb + q * 128;
            const int sw = swz<32>(q);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const f32x4 a = *(const f32x4*)(pa + (((2 * j + h) ^ sw) << 4));
              const f32x4 w = *(const f32x4*)(wl + (((dy * 3 + dx) * 4 + j) * 64 + lane) * 16);
              acc = DD_MFMA(a.x, w.x, acc);
              acc = DD_MFMA(a.y, w.y, acc);
              acc = DD_MFMA(a.z, w.z, acc);
              acc = DD_MFMA(a.w, w.w, acc);
            }
          }
        }
      } else {  // CIN == 4 (3 real channels): k-step = one channel of a PAIR of taps (lower / upper half-wave)
#pragma unroll
        for (int jp = 0; jp < 5; ++jp) {
          const int tap = min(2 * jp + h, 8);   // tap 9 does not exist: its packed weights are zero
          const int dy = tap / 3, dx = tap - 3 * dy;
          const char* rowb = ring + ((S * yy + dy) % 3) * C::SLOTB;
          const f32x4 a = *(const f32x4*)(rowb + (S * n + dx) * 16);
          const f32x4 w = *(const f32x4*)(wl + (jp * 64 + lane) * 16);
          acc = DD_MFMA(a.x, w.x, acc);
          acc = DD_MFMA(a.y, w.y, acc);
          acc = DD_MFMA(a.z, w.z, acc);
        }
      }

      // retire the prefetched rows into the ring BEFORE the epilogue stores are issued: the wait on the
      // (long landed) loads then never has to drain this row's stores (vmcnt counts loads and stores together)
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int iy = S * yy + 2 + s;
        if constexpr (AFF) store_row_aff<S, true>(ring + ((iy + 1) % 3) * C::SLOTB, spill, lane, pre[s], iy >= 0 && iy < H, gx0, W, asc, ash);
        else store_row<CIN, S, true>(ring + ((iy + 1) % 3) * C::SLOTB, spill, lane, pre[s]);
      }

      // epilogue: lane = output channel, register = pixel -> 128 contiguous bytes per pixel per store;
      // pixels right of the image fall outside the row descriptor and are dropped by the hardware
      const __amdgpu_buffer_rsrc_t ys = dd_rsrc(y + orow, Wo * 128);
      unsigned sign_word = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = acc[r];
        if (EPI == DD_EPI_BIAS || EPI == EPI_BIAS_STATS) v += bv;
        if (EPI == EPI_BIAS_STATS && x0 + dd_acc_row(r, lane) < Wo) {   // batch statistics: lane = channel, no shuffles in the loop
          if (st_n == 0.f) st_piv = v;
          const float dv = v - st_piv;
          st_sum += dv;
          st_sq += dv * dv;
          st_n += 1.f;
        }
        if (EPI == DD_EPI_BIAS_RELU || EPI == EPI_BIAS_RELU_BITS) v = fmaxf(v + bv, 0.f);
        if (EPI == DD_EPI_RELU_MASK) v = (mreg[r] > 0.f) ? v : 0.f;
        if (EPI == EPI_RELU_MASK_AFF) v = (mreg[r] * msc + msh > 0.f) ? v : 0.f;
        if (EPI == EPI_RELU_BITS) v = ((__builtin_bit_cast(unsigned, mreg[r]) >> n) & 1u) ? v : 0.f;
        dd_bstore1<DD_AUX_NT>(ys, ((x0 + dd_acc_row(r, lane)) * 32 + n) * 4, v);
        if (EPI == EPI_BIAS_RELU_BITS) {
          // lanes 0-31 hold the 32 channels of pixel i = (r&3)+8(r>>2), lanes 32-63 those of pixel i+4: one ballot =
          // two mask words.  Lane p (< 32) keeps the word of strip pixel p, so the row's 32 words leave as ONE store.
          const unsigned long long m = __ballot(v > 0.f);
          const int i0 = (r & 3) + 8 * (r >> 2);
          if (n == i0) sign_word = (unsigned)m;
          if (n == i0 + 4) sign_word = (unsigned)(m >> 32);
        }
      }
      if (EPI == EPI_BIAS_RELU_BITS) {
        const __amdgpu_buffer_rsrc_t bs = dd_rsrc(bits_out + (long)(b * Ho + yy) * Wo, Wo * 4);
        __builtin_amdgcn_raw_buffer_store_b32(sign_word, bs, (h == 0) ? (x0 + n) * 4 : -16, 0, 0);
      }
    }
  }
  if (EPI == EPI_BIAS_STATS) {   // one row per wave (layout: bn2d.hip): lanes c and c + 32 hold channel c; the row of a wave without
    DdMoments a = {st_n, st_piv, st_sum, st_sq};   // work stays zero (the launcher's memset)
    const DdMoments o = {__shfl_xor(st_n, 32), __shfl_xor(st_piv, 32), __shfl_xor(st_sum, 32), __shfl_xor(st_sq, 32)};
    dd_moments_merge(a, o);
    double mean, m2;
    dd_moments_finish(a, mean, m2);
    if (lane < 32 && a.n > 0.0) {
      float* row = stats + (long)(blockIdx.x * WPB + wave) * 128;
      row[lane] = (float)a.n;
      row[32 + lane] = (float)mean;
      row[64 + lane] = (float)m2;
      row[96 + lane] = (float)(mean - (double)(float)mean);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// stride-2 data gradient.  dx[yi][xi] collects, per parity class (yi&1, xi&1), 1/2/2/4 taps:
//   yi = 2r   : ky = 1 from dy row r            yi = 2r+1 : ky = 0 from row r+1, ky = 2 from row r
// (same along x), so a pair of output rows x 64 output pixels costs the same 144 MFMAs the forward
// spends on 32 output pixels -- no multiplies by inserted zeros.
// ------------------------------------------------------------------------------------------------
template <int WPB, int MASK>   // 0: none, 1: fp32 activation (> 0), 2: packed sign bits, 3: pre-BN tensor with (scale, shift)
__global__ __launch_bounds__(WPB * 64) void conv_s2_dgrad(const float* __restrict__ dy, const float* __restrict__ wp,
                                                          const float* __restrict__ msk, float* __restrict__ dx,
                                                          int B, int H, int W, int Ho, int Wo, int nstrips,
                                                          const float* __restrict__ aff = nullptr) {
  using C = StripCfg<32, 1>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  {
    f32x4* wl4 = (f32x4*)smem;
    const f32x4* wg4 = (const f32x4*)wp;
    for (int i = tid; i < C::WFLOATS / 4; i += WPB * 64) wl4[i] = wg4[i];
  }
  __syncthreads();
  const int nr = (H + 1) / 2;   // output row pairs per column
  const float msc = (MASK == 3) ? aff[64 + (lane & 31)] : 1.f, msh = (MASK == 3) ? aff[96 + (lane & 31)] : 0.f;
  char* ring = smem + C::WFLOATS * 4 + wave * C::WAVEB;
  char* spill = ring + 3 * C::SLOTB;
  const char* wl = smem;
  const int h = lane >> 5, n = lane & 31;

  long idx, end;
  dd_range((long)B * nstrips * nr, blockIdx.x * WPB + wave, gridDim.x * WPB, idx, end);
  while (idx < end) {
    const long col = idx / nr;
    const int r0 = (int)(idx - col * nr);
    const int r1 = (int)min((long)nr, r0 + (end - idx));
    idx += r1 - r0;
    const int b = (int)(col / nstrips), s0 = (int)(col % nstrips) * 32;
    const float* dyb = dy + (long)b * Ho * Wo * 32;

#pragma unroll
    for (int d = 0; d < 2; ++d) {
      f32x4 t[C::NLOAD];
      load_row<32, 1>(dyb, Ho, Wo, r0 + d, s0, lane, t);
      store_row<32, 1, true>(ring + ((r0 + d) % 3) * C::SLOTB, spill, lane, t);
    }

    for (int r = r0; r < r1; ++r) {
      f32x4 pre[C::NLOAD];
      load_row<32, 1>(dyb, Ho, Wo, r + 2, s0, lane, pre);
      __builtin_amdgcn_sched_barrier(0);   // loads stay above the MFMA chains (see conv_strip_fwd)

      const char* row_r = ring + (r % 3) * C::SLOTB;
      const char* row_r1 = ring + ((r + 1) % 3) * C::SLOTB;
      // One parity tile at a time: its ReLU-mask values are requested BEFORE its MFMA chain and consumed after,
      // so the epilogue never waits on HBM; only one 32x32 accumulator is live.
      // tap list per tile: (row offset 0/1, pixel offset 0/1, weight tap ky*3+kx)
#define DD_TILE(PY, PX, NTAP, ...)                                                              \
  {                                                                                             \
    constexpr int taps[NTAP][3] = {__VA_ARGS__};                                                \
    const int yi = 2 * r + (PY);                                                                \
    const long orow = ((long)(b * H + min(yi, H - 1)) * W) * 32;                                \
    const int obytes = (yi < H) ? W * 128 : 0;                                                  \
    float mreg[16];                                                                             \
    if (MASK == 1 || MASK == 3) {                                                               \
      const __amdgpu_buffer_rsrc_t ms = dd_rsrc(msk + orow, obytes);                            \
      _Pragma("unroll") for (int rr = 0; rr < 16; ++rr)                                         \
        mreg[rr] = dd_bload1<DD_AUX_NT>(ms, ((2 * (s0 + dd_acc_row(rr, lane)) + (PX)) * 32 + n) * 4); \
      __builtin_amdgcn_sched_barrier(0);                                                        \
    }                                                                                           \
    if (MASK == 2) {                                                                            \
      const __amdgpu_buffer_rsrc_t ms = dd_rsrc((const unsigned*)msk + (long)(b * H + min(yi, H - 1)) * W, obytes / 32); \
      _Pragma("unroll") for (int rr = 0; rr < 16; ++rr)                                         \
        mreg[rr] = dd_bload1<DD_AUX_NT>(ms, (2 * (s0 + dd_acc_row(rr, lane)) + (PX)) * 4);      \
      __builtin_amdgcn_sched_barrier(0);                                                        \
    }                                                                                           \
    f32x16 acc;                                                                                 \
    _Pragma("unroll") for (int i = 0; i < 16; ++i) acc[i] = 0.f;                                \
    _Pragma("unroll") for (int t = 0; t < NTAP; ++t) {                                          \
      const char* rowp = taps[t][0] ? row_r1 : row_r;                                           \
      const int q = n + taps[t][1];                                                             \
      const char* pa = rowp + q * 128;                                                          \
      const int sw = swz<32>(q);                                                                \
      _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                           \
        const f32x4 a = *(const f32x4*)(pa + (((2 * j + h) ^ sw) << 4));                        \
        const f32x4 w = *(const f32x4*)(wl + ((taps[t][2] * 4 + j) * 64 + lane) * 16);          \
        acc = DD_MFMA(a.x, w.x, acc);                                                           \
        acc = DD_MFMA(a.y, w.y, acc);                                                           \
        acc = DD_MFMA(a.z, w.z, acc);                                                           \
        acc = DD_MFMA(a.w, w.w, acc);                                                           \
      }                                                                                         \
    }                                                                                           \
    const __amdgpu_buffer_rsrc_t os = dd_rsrc(dx + orow, obytes);                               \
    _Pragma("unroll") for (int rr = 0; rr < 16; ++rr) {                                         \
      float v = acc[rr];                                                                        \
      if (MASK == 1) v = (mreg[rr] > 0.f) ? v : 0.f;                                            \
      if (MASK == 3) v = (mreg[rr] * msc + msh > 0.f) ? v : 0.f;                                \
      if (MASK == 2) v = ((__builtin_bit_cast(unsigned, mreg[rr]) >> n) & 1u) ? v : 0.f;        \
      dd_bstore1<DD_AUX_NT>(os, ((2 * (s0 + dd_acc_row(rr, lane)) + (PX)) * 32 + n) * 4, v);    \
    }                                                                                           \
  }
      DD_TILE(1, 1, 4, {1, 1, 0}, {1, 0, 2}, {0, 1, 6}, {0, 0, 8})   // (ky,kx) = (0,0) (0,2) (2,0) (2,2)
      store_row<32, 1, true>(ring + ((r + 2) % 3) * C::SLOTB, spill, lane, pre);   // slot (r+2)%3 is not read by this pair
      DD_TILE(0, 1, 2, {0, 1, 3}, {0, 0, 5})                         // (1,0) (1,2)
      DD_TILE(1, 0, 2, {1, 0, 1}, {0, 0, 7})                         // (0,1) (2,1)
      DD_TILE(0, 0, 1, {0, 0, 4})                                    // (1,1)
#undef DD_TILE
    }
  }
}

// ------------------------------------------------------------------------------------------------
// weight / bias gradient.  GEMM view: M = 32 output channels, N = 32 input channels (one 32x32 tile per
// tap, 9 register accumulators), K = pixels.  A = dy (straight from HBM, 256 contiguous bytes per
// wave-load), B = x rows from the LDS ring (ds_read_b32, 32 consecutive dwords per half-wave).
// Each wave accumulates over its whole range and writes ONE partial.
// ------------------------------------------------------------------------------------------------
template <int CIN, int S, int WPB, bool AFF = false>
__global__ __launch_bounds__(WPB * 64) void conv_wgrad(const float* __restrict__ x, const float* __restrict__ dy,
                                                       float* __restrict__ part, float* __restrict__ bpart, int B,
                                                       int H, int W, int Ho, int Wo, int nstrips,
                                                       const float* __restrict__ aff = nullptr) {
  using C = StripCfg<CIN, S>;
  constexpr int NT = (CIN == 32) ? 9 : 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  char* ring = smem + wave * C::WAVEB;
  char* spill = ring + 3 * C::SLOTB;
  const int h = lane >> 5, n = lane & 31;
  const int gw = blockIdx.x * WPB + wave;
  f32x4 asc = {1.f, 1.f, 1.f, 1.f}, ash = {0.f, 0.f, 0.f, 0.f};
  if (AFF) {
    asc = *(const f32x4*)(aff + 4 * (lane & 7));
    ash = *(const f32x4*)(aff + 32 + 4 * (lane & 7));
  }

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum = 0.f;

  // CIN == 4: output column j = lane&31 stands for (tap, channel) = (j/3, j%3); columns >= 27 are ignored.
  const int tap4 = min(n / 3, 8), c4 = n % 3;
  const int dy4 = tap4 / 3, dx4 = tap4 - 3 * dy4;

  long idx, end;
  dd_range((long)B * nstrips * Ho, gw, gridDim.x * WPB, idx, end);
  while (idx < end) {
    const long col = idx / Ho;
    const int y0 = (int)(idx - col * Ho);
    const int y1 = (int)min((long)Ho, y0 + (end - idx));
    idx += y1 - y0;
    const int b = (int)(col / nstrips), x0 = (int)(col % nstrips) * 32;
    const float* xb = x + (long)b * H * W * CIN;
    const float* dyb = dy + (long)b * Ho * Wo * 32;
    const int gx0 = S * x0 - 1;
    const int aoff = ((x0 + h) * 32 + n) * 4;   // + 256 bytes per pixel pair

#pragma unroll
    for (int d = 0; d < 3; ++d) {
      f32x4 t[C::NLOAD];
      const int iy = S * y0 - 1 + d;
      load_row<CIN, S>(xb, H, W, iy, gx0, lane, t);
      if constexpr (AFF) store_row_aff<S, false>(ring + ((iy + 1) % 3) * C::SLOTB, spill, lane, t, iy >= 0 && iy < H, gx0, W, asc, ash);
      else store_row<CIN, S, false>(ring + ((iy + 1) % 3) * C::SLOTB, spill, lane, t);
    }
    float areg[16];
    {
      const __amdgpu_buffer_rsrc_t as = dd_rsrc(dyb + (long)y0 * Wo * 32, Wo * 128);
#pragma unroll
      for (int pp = 0; pp < 16; ++pp) areg[pp] = dd_bload1<DD_AUX_NT>(as, aoff + pp * 256);
    }

    for (int yy = y0; yy < y1; ++yy) {
      f32x4 pre[S][C::NLOAD];
#pragma unroll
      for (int s = 0; s < S; ++s) load_row<CIN, S>(xb, H, W, S * yy + 2 + s, gx0, lane, pre[s]);
      float anext[16];
      {
        const bool ok = yy + 1 < Ho;
        const __amdgpu_buffer_rsrc_t as = dd_rsrc(dyb + (long)(ok ? yy + 1 : 0) * Wo * 32, ok ? Wo * 128 : 0);
#pragma unroll
        for (int pp = 0; pp < 16; ++pp) anext[pp] = dd_bload1<DD_AUX_NT>(as, aoff + pp * 256);
      }
      __builtin_amdgcn_sched_barrier(0);   // loads stay above the MFMA chains (see conv_strip_fwd)

      if (CIN == 32) {
        const char* rb0 = ring + ((S * yy + 0) % 3) * C::SLOTB;
        const char* rb1 = ring + ((S * yy + 1) % 3) * C::SLOTB;
        const char* rb2 = ring + ((S * yy + 2) % 3) * C::SLOTB;
#pragma unroll
        for (int pp = 0; pp < 16; ++pp) {
          const float a = areg[pp];
          bsum += a;
          const int off = (S * (2 * pp + h)) * 128 + n * 4;
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            acc[0 + dx] = DD_MFMA(a, *(const float*)(rb0 + off + dx * 128), acc[0 + dx]);
            acc[3 + dx] = DD_MFMA(a, *(const float*)(rb1 + off + dx * 128), acc[3 + dx]);
            acc[6 + dx] = DD_MFMA(a, *(const float*)(rb2 + off + dx * 128), acc[6 + dx]);
          }
        }
      } else {
        const char* rb = ring + ((S * yy + dy4) % 3) * C::SLOTB + dx4 * 16 + c4 * 4;
#pragma unroll
        for (int pp = 0; pp < 16; ++pp) {
          const float a = areg[pp];
          bsum += a;
          acc[0] = DD_MFMA(a, *(const float*)(rb + (S * (2 * pp + h)) * 16), acc[0]);
        }
      }

#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int iy = S * yy + 2 + s;
        if constexpr (AFF) store_row_aff<S, false>(ring + ((iy + 1) % 3) * C::SLOTB, spill, lane, pre[s], iy >= 0 && iy < H, gx0, W, asc, ash);
        else store_row<CIN, S, false>(ring + ((iy + 1) % 3) * C::SLOTB, spill, lane, pre[s]);
      }
#pragma unroll
      for (int pp = 0; pp < 16; ++pp) areg[pp] = anext[pp];
    }
  }

#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) part[(((long)gw * NT + t) * 16 + r) * 64 + lane] = acc[t][r];
  bpart[(long)gw * 64 + lane] = bsum;
}

// Second stage: sum the per-wave partials in a fixed order and scatter to OIHW.  One block per (tap, register)
// row of 64 lanes; 16 wave-groups each sum a strided sixteenth of the partials (4 loads in flight), then a
// fixed-order LDS tree: deterministic, and 75 MB of partials are read by 145 x 1024 threads instead of 145 x 256.
template <int CIN>
__global__ __launch_bounds__(1024) void conv_wgrad_reduce(const float* __restrict__ part,
                                                          const float* __restrict__ bpart, float* __restrict__ dw,
                                                          float* __restrict__ db, int nw) {
  constexpr int NT = (CIN == 32) ? 9 : 1;
  constexpr int G = 16;
  __shared__ double red[G][64];
  const int l = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int row = blockIdx.x;   // (t*16 + r), or NT*16 for the bias
  const float* src = (row < NT * 16) ? part + (long)row * 64 + l : bpart + l;
  const long stride = (row < NT * 16) ? (long)NT * 16 * 64 : 64;
  // The partials of different images largely CANCEL in these sums (the upstream gradient has zero batch mean behind a
  // train-mode BatchNorm, the activations a large common mean), so the second stage runs in fp64: a few thousand adds.
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int w = g;
  for (; w + 3 * G < nw; w += 4 * G) {
    s0 += (double)src[(long)w * stride];
    s1 += (double)src[(long)(w + G) * stride];
    s2 += (double)src[(long)(w + 2 * G) * stride];
    s3 += (double)src[(long)(w + 3 * G) * stride];
  }
  for (; w < nw; w += G) s0 += (double)src[(long)w * stride];
  red[g][l] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (g != 0) return;
  double sd = 0.0;
#pragma unroll
  for (int i = 0; i < G; ++i) sd += red[i][l];
  const float s = (float)sd;
  if (row < NT * 16) {
    const int t = row >> 4, r = row & 15;
    const int o = dd_acc_row(r, l), j = l & 31;
    if (CIN == 32) {
      dw[((long)o * 32 + j) * 9 + t] = s;
    } else if (j < 27) {
      dw[((long)o * 3 + (j % 3)) * 9 + (j / 3)] = s;
    }
  } else {
    const double other = __shfl_xor(sd, 32);   // lanes l and l+32 hold the two pixel parities of channel l&31
    if (l < 32) db[l] = (float)(sd + other);
  }
}

// ------------------------------------------------------------------------------------------------
// weight packing: PyTorch OIHW -> the per-lane B-operand image the kernels read with ds_read_b128.
//   CIN=32: packed[((t*4 + j)*64 + lane)*4 + i] = Weff[n = lane&31][c = 8j + 4(lane>>5) + i][t]
//   CIN=4 : packed[(jp*64 + lane)*4 + i]        = W[n][i][tap = 2jp + (lane>>5)]  (0 for tap 9 / i == 3)
// kind 0: Weff = W;  kind 1: Weff[n][c][t] = W[c][n][8-t] (stride-1 dgrad);  kind 2: Weff[n][c][t] = W[c][n][t].
// ------------------------------------------------------------------------------------------------
__global__ void conv_pack_kernel(const float* __restrict__ w, float* __restrict__ p, int cin_real, int kind) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (cin_real == 32) {
    if (idx >= 36 * 64 * 4) return;
    const int i = idx & 3, lane = (idx >> 2) & 63, g = idx >> 8;
    const int j = g & 3, t = g >> 2;
    const int n = lane & 31, c = 8 * j + 4 * (lane >> 5) + i;
    float v;
    if (kind == 0) v = w[((long)n * 32 + c) * 9 + t];
    else if (kind == 1) v = w[((long)c * 32 + n) * 9 + (8 - t)];
    else v = w[((long)c * 32 + n) * 9 + t];
    p[idx] = v;
  } else {
    if (idx >= 5 * 64 * 4) return;
    const int i = idx & 3, lane = (idx >> 2) & 63, jp = idx >> 8;
    const int n = lane & 31, tap = 2 * jp + (lane >> 5);
    p[idx] = (tap < 9 && i < 3) ? w[((long)n * 3 + i) * 9 + tap] : 0.f;
  }
}

// Sign words of a 32-channel NHWC activation: bits[p] bit c = x[p][c] > 0 -- what dd_conv_fwd_relu_bits writes beside its output, for an
// activation another kernel produced (the strip mosaic in front of SpatialMappingCNN's out_conv, when that layer's data gradient runs on
// the Winograd kernels).  A wave takes 64 pixels: each ballot covers two (lanes = channels, fully coalesced 256-byte loads), lane p keeps
// the word of pixel p, the 64 words leave as one store.
__global__ __launch_bounds__(256) void relu_sign_bits_kernel(const float* __restrict__ x, unsigned* __restrict__ bits, long npix) {
  const int lane = threadIdx.x & 63;
  const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long)gridDim.x * blockDim.x) >> 6;
  for (long p0 = wave * 64; p0 < npix; p0 += nwaves * 64) {
    unsigned word = 0;
#pragma unroll 8
    for (int i = 0; i < 32; ++i) {
      const long p = p0 + 2 * i + (lane >> 5);
      const float v = p < npix ? x[p * 32 + (lane & 31)] : 0.f;
      const unsigned long long m = __ballot(v > 0.f);
      if (lane == 2 * i) word = (unsigned)m;
      if (lane == 2 * i + 1) word = (unsigned)(m >> 32);
    }
    if (p0 + lane < npix) bits[p0 + lane] = word;
  }
}

// out_pad [B, H + 2, W + 2, 32] = dy [B, H, W, 32] * (the ReLU was open: bit c of bits_pad[pixel]) in the interior, ZERO on the border ring:
// the output gradient of a padding-0 3x3 layer laid out for the padding-1 kernels (its border outputs do not exist, so they carry no
// gradient), with the layer's own ReLU backward applied from the sign words its forward wrote.
__global__ __launch_bounds__(256) void relu_bwd_pad_bits_kernel(const float* __restrict__ dy, const unsigned* __restrict__ bits_pad,
                                                                f32x4* __restrict__ out_pad, int B, int H, int W, int dy_cstore, int dy_coff) {
  const long total = (long)B * (H + 2) * (W + 2) * 8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int q = (int)(i & 7);
    const long pp = i >> 3;
    const int xx = (int)(pp % (W + 2)), yy = (int)((pp / (W + 2)) % (H + 2));
    const long b = pp / ((long)(W + 2) * (H + 2));
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (xx >= 1 && xx <= W && yy >= 1 && yy <= H) {
      const f32x4 g = *(const f32x4*)(dy + ((b * H + (yy - 1)) * W + (xx - 1)) * dy_cstore + dy_coff + 4 * q);
      const unsigned m = bits_pad[pp] >> (4 * q);
      o.x = (m & 1u) ? g.x : 0.f;
      o.y = (m & 2u) ? g.y : 0.f;
      o.z = (m & 4u) ? g.z : 0.f;
      o.w = (m & 8u) ? g.w : 0.f;
    }
    __builtin_nontemporal_store(o, out_pad + i);
  }
}

__global__ void relu_bwd_kernel(const f32x4* __restrict__ dy, const f32x4* __restrict__ y, f32x4* __restrict__ out,
                                long n4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const f32x4 g = dy[i], v = y[i];
    f32x4 o;
    o.x = v.x > 0.f ? g.x : 0.f;
    o.y = v.y > 0.f ? g.y : 0.f;
    o.z = v.z > 0.f ? g.z : 0.f;
    o.w = v.w > 0.f ? g.w : 0.f;
    out[i] = o;
  }
}

template <int CIN, int S, int EPI, int WPB, bool AFF = false>
int launch_fwd(const float* x, const float* wp, const float* bias, const float* msk, float* y, const dd_conv_desc* d,
               hipStream_t st, unsigned* bits_out = nullptr, const float* aff = nullptr, float* stats = nullptr) {
  using C = StripCfg<CIN, S>;
  const int Ho = dd_conv_out(d->height, S), Wo = dd_conv_out(d->width, S);
  const int nstrips = (Wo + 31) / 32;
  const size_t lds = C::WFLOATS * 4 + (size_t)WPB * C::WAVEB;
  const int per_cu = (int)max((size_t)1, min((size_t)2, (size_t)(160 * 1024) / lds));
  const int grid = resident_grid(d, (long)d->batch * nstrips * Ho, WPB, per_cu);
  auto k = conv_strip_fwd<CIN, S, EPI, WPB, AFF>;
  if (int rc = dd_allow_lds((const void*)k, lds)) return rc;
  hipLaunchKernelGGL(k, dim3(grid), dim3(WPB * 64), lds, st, x, wp, bias, msk, y, bits_out, d->batch, d->height, d->width,
                     Ho, Wo, nstrips, aff, stats);
  DD_LAUNCH_CHECK("conv_strip_fwd");
  return 0;
}

// Data gradient of the stride-2 layer; MASK: 0 none, 1 fp32 ReLU source, 2 ReLU bits, 3 pre-BatchNorm tensor + affine.
template <int MASK>
int launch_s2_dgrad(const float* dy, const float* packed_dgrad, const float* relu_src, float* dx, const dd_conv_desc* d, hipStream_t st,
                    const float* aff) {
  using C = StripCfg<32, 1>;
  constexpr int WPB = 8;
  const int H = d->height, W = d->width, Ho = dd_conv_out(H, 2), Wo = dd_conv_out(W, 2);
  const int ns = (W + 1) / 2, nr = (H + 1) / 2;
  const int nstrips = (ns + 31) / 32;
  const size_t lds = C::WFLOATS * 4 + (size_t)WPB * C::WAVEB;
  const int grid = resident_grid(d, (long)d->batch * nstrips * nr, WPB, 1);
  auto k = conv_s2_dgrad<WPB, MASK>;
  if (int rc = dd_allow_lds((const void*)k, lds)) return rc;
  hipLaunchKernelGGL(k, dim3(grid), dim3(WPB * 64), lds, st, dy, packed_dgrad, relu_src, dx, d->batch, H, W, Ho, Wo, nstrips, aff);
  DD_LAUNCH_CHECK("conv_s2_dgrad");
  return 0;
}

int conv_dgrad_impl(const float* dy, const float* packed_dgrad, const float* relu_src, int mask_mode, float* dx,
                    const dd_conv_desc* d, void* stream, const float* aff = nullptr) {
  if (int rc = check_desc(d)) return rc;
  DD_REQUIRE(dy && packed_dgrad && dx, DD_ERR_BAD_ARG, "conv_dgrad: NULL pointer");
  DD_REQUIRE(d->cin_real == 32, DD_ERR_UNSUPPORTED, "conv_dgrad: Cin %d (the first layer has no data gradient)", d->cin_real);
  hipStream_t st = (hipStream_t)stream;
  if (d->stride == 1) {
    // a stride-1 k3 p1 data gradient IS a k3 p1 convolution of dy with the flipped / transposed weights
    if (mask_mode == 3) return launch_fwd<32, 1, EPI_RELU_MASK_AFF, 8>(dy, packed_dgrad, nullptr, relu_src, dx, d, st, nullptr, aff);
    if (mask_mode == 2) return launch_fwd<32, 1, EPI_RELU_BITS, 8>(dy, packed_dgrad, nullptr, relu_src, dx, d, st);
    return mask_mode ? launch_fwd<32, 1, DD_EPI_RELU_MASK, 8>(dy, packed_dgrad, nullptr, relu_src, dx, d, st)
                     : launch_fwd<32, 1, DD_EPI_NONE, 8>(dy, packed_dgrad, nullptr, nullptr, dx, d, st);
  }
  switch (mask_mode) {
    case 3: return launch_s2_dgrad<3>(dy, packed_dgrad, relu_src, dx, d, st, aff);
    case 2: return launch_s2_dgrad<2>(dy, packed_dgrad, relu_src, dx, d, st, aff);
    case 1: return launch_s2_dgrad<1>(dy, packed_dgrad, relu_src, dx, d, st, aff);
    default: return launch_s2_dgrad<0>(dy, packed_dgrad, relu_src, dx, d, st, aff);
  }
}

int conv_wgrad_impl(const float* x, const float* aff, const float* dy, float* dw_oihw, float* dbias, void* workspace,
                    int64_t workspace_bytes, const dd_conv_desc* d, void* stream) {
  if (int rc = check_desc(d)) return rc;
  DD_REQUIRE(x && dy && dw_oihw && dbias && workspace, DD_ERR_BAD_ARG, "conv_wgrad: NULL pointer");
  DD_REQUIRE(workspace_bytes >= dd_conv_wgrad_workspace_bytes(d), DD_ERR_WORKSPACE, "conv_wgrad: workspace %ld < %ld bytes",
             (long)workspace_bytes, (long)dd_conv_wgrad_workspace_bytes(d));
  hipStream_t st = (hipStream_t)stream;
  constexpr int WPB = 4;
  const int S = d->stride, H = d->height, W = d->width, Ho = dd_conv_out(H, S), Wo = dd_conv_out(W, S);
  const int nstrips = (Wo + 31) / 32;
  const int nt = d->cin_real == 32 ? 9 : 1;
  // Cin 32: 144 accumulator registers -> one wave per SIMD -> one 4-wave block per CU; Cin 3: two
  const int grid = resident_grid(d, (long)d->batch * nstrips * Ho, WPB, d->cin_store == 4 ? 2 : 1);
  const int nw = grid * WPB;
  float* part = (float*)workspace;
  float* bpart = part + (size_t)nw * nt * 1024;
#define DD_WG(CIN, SS, AFF)                                                                                         \
  {                                                                                                                 \
    auto k = conv_wgrad<CIN, SS, WPB, AFF>;                                                                         \
    const size_t lds = (size_t)WPB * StripCfg<CIN, SS>::WAVEB;                                                      \
    if (int rc = dd_allow_lds((const void*)k, lds)) return rc;                                                      \
    hipLaunchKernelGGL(k, dim3(grid), dim3(WPB * 64), lds, st, x, dy, part, bpart, d->batch, H, W, Ho, Wo, nstrips, \
                       aff);                                                                                        \
  }
  if (d->cin_store == 4) DD_WG(4, 1, false)
  else if (S == 1 && aff) DD_WG(32, 1, true)
  else if (S == 1) DD_WG(32, 1, false)
  else if (aff) DD_WG(32, 2, true)
  else DD_WG(32, 2, false)
#undef DD_WG
  DD_LAUNCH_CHECK("conv_wgrad");
  if (d->cin_store == 4)
    hipLaunchKernelGGL(conv_wgrad_reduce<4>, dim3(nt * 16 + 1), dim3(1024), 0, st, part, bpart, dw_oihw, dbias, nw);
  else
    hipLaunchKernelGGL(conv_wgrad_reduce<32>, dim3(nt * 16 + 1), dim3(1024), 0, st, part, bpart, dw_oihw, dbias, nw);
  DD_LAUNCH_CHECK("conv_wgrad_reduce");
  return 0;
}

}  // namespace

extern "C" {

int64_t dd_conv_packed_floats(const dd_conv_desc* d, int32_t kind) {
  if (check_desc(d)) return -1;
  if (kind != 0 && d->cin_real != 32) return -1;
  return d->cin_real == 32 ? 36 * 64 * 4 : 5 * 64 * 4;
}

int dd_conv_pack(const float* w_oihw, float* packed, const dd_conv_desc* d, int32_t kind, void* stream) {
  if (int rc = check_desc(d)) return rc;
  DD_REQUIRE(w_oihw && packed, DD_ERR_BAD_ARG, "conv_pack: NULL pointer");
  DD_REQUIRE(kind >= 0 && kind <= 2, DD_ERR_BAD_ARG, "conv_pack: kind %d", kind);
  DD_REQUIRE(kind == 0 || d->cin_real == 32, DD_ERR_UNSUPPORTED, "conv_pack: dgrad packing needs Cin 32");
  const int n = d->cin_real == 32 ? 36 * 64 * 4 : 5 * 64 * 4;
  hipLaunchKernelGGL(conv_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, w_oihw, packed,
                     d->cin_real, kind);
  DD_LAUNCH_CHECK("conv_pack");
  return 0;
}

int dd_conv_fwd(const float* x, const float* packed_fwd, const float* bias, const float* mask, float* y,
                const dd_conv_desc* d, int32_t epilogue, void* stream) {
  if (int rc = check_desc(d)) return rc;
  DD_REQUIRE(x && packed_fwd && y, DD_ERR_BAD_ARG, "conv_fwd: NULL pointer");
  DD_REQUIRE(epilogue != DD_EPI_RELU_MASK || mask, DD_ERR_BAD_ARG, "conv_fwd: RELU_MASK epilogue needs a mask");
  DD_REQUIRE((epilogue != DD_EPI_BIAS && epilogue != DD_EPI_BIAS_RELU) || bias, DD_ERR_BAD_ARG, "conv_fwd: bias epilogue needs a bias");
  hipStream_t st = (hipStream_t)stream;
#define DD_DISPATCH(CIN, S, WPB)                                                                                    \
  switch (epilogue) {                                                                                               \
    case DD_EPI_NONE: return launch_fwd<CIN, S, DD_EPI_NONE, WPB>(x, packed_fwd, bias, mask, y, d, st);             \
    case DD_EPI_BIAS: return launch_fwd<CIN, S, DD_EPI_BIAS, WPB>(x, packed_fwd, bias, mask, y, d, st);             \
    case DD_EPI_BIAS_RELU: return launch_fwd<CIN, S, DD_EPI_BIAS_RELU, WPB>(x, packed_fwd, bias, mask, y, d, st);   \
    case DD_EPI_RELU_MASK: return launch_fwd<CIN, S, DD_EPI_RELU_MASK, WPB>(x, packed_fwd, bias, mask, y, d, st);   \
    default: return dd_fail(DD_ERR_BAD_ARG, "conv_fwd: epilogue %d", epilogue);                                     \
  }
  if (d->cin_store == 4) { DD_DISPATCH(4, 1, 8) }
  if (d->stride == 1) { DD_DISPATCH(32, 1, 8) }
  DD_DISPATCH(32, 2, 4)
#undef DD_DISPATCH
}

int dd_conv_fwd_relu_bits(const float* x, const float* packed_fwd, const float* bias, float* y, uint32_t* relu_bits,
                          const dd_conv_desc* d, void* stream) {
  if (int rc = check_desc(d)) return rc;
  DD_REQUIRE(x && packed_fwd && bias && y && relu_bits, DD_ERR_BAD_ARG, "conv_fwd_relu_bits: NULL pointer");
  hipStream_t st = (hipStream_t)stream;
  if (d->cin_store == 4) return launch_fwd<4, 1, EPI_BIAS_RELU_BITS, 8>(x, packed_fwd, bias, nullptr, y, d, st, relu_bits);
  if (d->stride == 1) return launch_fwd<32, 1, EPI_BIAS_RELU_BITS, 8>(x, packed_fwd, bias, nullptr, y, d, st, relu_bits);
  return launch_fwd<32, 2, EPI_BIAS_RELU_BITS, 4>(x, packed_fwd, bias, nullptr, y, d, st, relu_bits);
}

int dd_conv_dgrad(const float* dy, const float* packed_dgrad, const float* relu_src, float* dx, const dd_conv_desc* d,
                  void* stream) {
  return conv_dgrad_impl(dy, packed_dgrad, relu_src, relu_src ? 1 : 0, dx, d, stream);
}

int dd_conv_dgrad_relu_bits(const float* dy, const float* packed_dgrad, const uint32_t* relu_bits, float* dx,
                            const dd_conv_desc* d, void* stream) {
  DD_REQUIRE(relu_bits, DD_ERR_BAD_ARG, "conv_dgrad_relu_bits: NULL mask");
  return conv_dgrad_impl(dy, packed_dgrad, (const float*)relu_bits, 2, dx, d, stream);
}

int dd_conv_dgrad_bn(const float* dy, const float* packed_dgrad, const float* pre_bn, const float* affine, float* dx,
                     const dd_conv_desc* d, void* stream) {
  DD_REQUIRE(pre_bn && affine, DD_ERR_BAD_ARG, "conv_dgrad_bn: NULL mask / affine");
  return conv_dgrad_impl(dy, packed_dgrad, pre_bn, 3, dx, d, stream, affine);
}

int64_t dd_conv_wgrad_workspace_bytes(const dd_conv_desc* d) {
  if (check_desc(d)) return -1;
  const int nt = d->cin_real == 32 ? 9 : 1;
  const int64_t waves = 4 * (int64_t)DD_NUM_CU * 2;   // upper bound of resident waves of any instantiation
  return waves * ((int64_t)nt * 1024 + 64) * 4;
}

int dd_conv_wgrad(const float* x, const float* dy, float* dw_oihw, float* dbias, void* workspace,
                  int64_t workspace_bytes, const dd_conv_desc* d, void* stream) {
  return conv_wgrad_impl(x, nullptr, dy, dw_oihw, dbias, workspace, workspace_bytes, d, stream);
}

int dd_conv_wgrad_bn(const float* pre_bn, const float* affine, const float* dy, float* dw_oihw, float* dbias, void* workspace,
                     int64_t workspace_bytes, const dd_conv_desc* d, void* stream) {
  DD_REQUIRE(affine, DD_ERR_BAD_ARG, "conv_wgrad_bn: NULL affine");
  DD_REQUIRE(d && d->cin_real == 32, DD_ERR_UNSUPPORTED, "conv_wgrad_bn: the input of a BN'd layer has 32 channels");
  return conv_wgrad_impl(pre_bn, affine, dy, dw_oihw, dbias, workspace, workspace_bytes, d, stream);
}

int64_t dd_conv_stats_floats(void) { return (int64_t)DD_NUM_CU * 2 * 8 * 64 * 2; }

int dd_conv_fwd_stats(const float* x, const float* packed_fwd, const float* bias, const float* in_affine, float* u,
                      float* stats, const dd_conv_desc* d, void* stream) {
  if (int rc = check_desc(d)) return rc;
  DD_REQUIRE(x && packed_fwd && bias && u && stats, DD_ERR_BAD_ARG, "conv_fwd_stats: NULL pointer");
  DD_REQUIRE(!(in_affine && d->cin_store == 4), DD_ERR_UNSUPPORTED, "conv_fwd_stats: the image layer has no BN'd input");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(stats, 0, dd_conv_stats_floats() * sizeof(float), st) != hipSuccess)
    return dd_fail(DD_ERR_LAUNCH, "conv_fwd_stats: hipMemsetAsync failed");
  if (d->cin_store == 4) return launch_fwd<4, 1, EPI_BIAS_STATS, 8>(x, packed_fwd, bias, nullptr, u, d, st, nullptr, nullptr, stats);
  if (d->stride == 1)
    return in_affine ? launch_fwd<32, 1, EPI_BIAS_STATS, 8, true>(x, packed_fwd, bias, nullptr, u, d, st, nullptr, in_affine, stats)
                     : launch_fwd<32, 1, EPI_BIAS_STATS, 8, false>(x, packed_fwd, bias, nullptr, u, d, st, nullptr, nullptr, stats);
  return in_affine ? launch_fwd<32, 2, EPI_BIAS_STATS, 4, true>(x, packed_fwd, bias, nullptr, u, d, st, nullptr, in_affine, stats)
                   : launch_fwd<32, 2, EPI_BIAS_STATS, 4, false>(x, packed_fwd, bias, nullptr, u, d, st, nullptr, nullptr, stats);
}

int dd_relu_bwd(const float* dy, const float* y, float* out, int64_t n, void* stream) {
  DD_REQUIRE(dy && y && out && n > 0, DD_ERR_BAD_ARG, "relu_bwd: bad argument");
  DD_REQUIRE(n % 4 == 0, DD_ERR_UNSUPPORTED, "relu_bwd: n %% 4 != 0");
  const long n4 = n / 4;
  const int grid = dd_grid_for(n4);
  hipLaunchKernelGGL(relu_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const f32x4*)dy, (const f32x4*)y,
                     (f32x4*)out, n4);
  DD_LAUNCH_CHECK("relu_bwd");
  return 0;
}

int dd_relu_sign_bits(const float* x, uint32_t* bits, int64_t npix, void* stream) {
  DD_REQUIRE(x && bits && npix > 0, DD_ERR_BAD_ARG, "relu_sign_bits: bad argument");
  const long waves = (npix + 63) / 64;
  const int grid = (int)min((waves + 3) / 4, (long)DD_NUM_CU * 8);
  hipLaunchKernelGGL(relu_sign_bits_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, bits, (long)npix);
  DD_LAUNCH_CHECK("relu_sign_bits");
  return 0;
}

int dd_relu_bwd_pad_bits(const float* dy, const uint32_t* bits_pad, float* out_pad, int32_t batch, int32_t h, int32_t w, int32_t dy_cstore,
                         int32_t dy_coff, void* stream) {
  DD_REQUIRE(dy && bits_pad && out_pad && batch > 0 && h > 0 && w > 0, DD_ERR_BAD_ARG, "relu_bwd_pad_bits: bad argument");
  DD_REQUIRE(dy_cstore >= 32 && dy_cstore % 4 == 0 && dy_coff >= 0 && dy_coff % 4 == 0 && dy_coff + 32 <= dy_cstore, DD_ERR_BAD_ARG,
             "relu_bwd_pad_bits: dy's 32 channels must be a 4-aligned slice of its %d stored ones (offset %d)", dy_cstore, dy_coff);
  DD_REQUIRE((((uintptr_t)dy | (uintptr_t)out_pad) & 15) == 0, DD_ERR_BAD_ARG, "relu_bwd_pad_bits: dy and out_pad must be 16-byte aligned");
  const long total = (long)batch * (h + 2) * (w + 2) * 8;
  const int grid = dd_grid_for(total);
  hipLaunchKernelGGL(relu_bwd_pad_bits_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, dy, bits_pad, (f32x4*)out_pad,
                     batch, h, w, dy_cstore, dy_coff);
  DD_LAUNCH_CHECK("relu_bwd_pad_bits");
  return 0;
}

}  // extern "C"

#include "conv_wino2.inc"
#include "conv_wino.inc"

// bf16 mixed precision for the autoencoder's decoder conv stack (reference src/autoencoder/components.py:88-92), the layers the
// encoder's bf16 kernels (conv3x3_bf16.hip) do not cover:
//   dc1  ConvTranspose2d 64 -> 32, k3 p1, + ReLU   (reads fc2's fp32 NCHW-flat output, rounding it to bf16 as it loads)
//   dc3  ConvTranspose2d 32 -> 32, k2 s2, + ReLU   (fused with dc4 in the forward: a3 is written once, never read back there)
//   dc4  ConvTranspose2d 32 -> 3,  k1, no ReLU     (y_hat straight to NCHW)
// dc2 (k3 p1, 32 -> 32) is the encoder's c2 layer on transposed, flipped weights and runs on dd_conv_bf16_*.
//
// Contract (oracle: tests/test_gpu_ae_bf16.py, the decoder half of oracle/bf16_parts.py's "torch autocast equivalent"):
// every conv reads bf16-rounded inputs and weights, accumulates in fp32 and rounds its output to bf16 once, after bias and
// ReLU; y_hat is rounded once and stored as fp32; dL/dy_hat and every pre-activation gradient are rounded to bf16 once;
// the gradient handed back to fc2 is the bf16-rounded dL/d(decoder input) as fp32 NCHW-flat; weight and bias gradients are
// fp32 sums of bf16 products, reduced in a fixed order (per-workgroup partials over a fixed grid, then one column sum), so
// they are deterministic.
//
// dc1's forward runs on the bf16 matrix cores; dc3 / dc4 run on the vector FMA pipe (one output pixel per lane, weights broadcast
// from LDS).  At bs 32 the kernels of this file take ~1.0 ms of the 6.6 ms bf16 step.
// Every global access is either range-checked on the host (sizes are validated before launch) or guarded per lane.
#include "dd_common.h"

namespace {

__device__ __forceinline__ float bfr(float v) { return dd_bf16_lo(dd_pack_bf16(v, 0.f)); }
__device__ __forceinline__ float bf_at(const unsigned short* p, long i) { return __builtin_bit_cast(float, (unsigned)p[i] << 16); }

// 32 bf16 channels of one NHWC pixel (64 bytes, 16-byte aligned) <-> 16 packed words
__device__ __forceinline__ void load_px32(const unsigned short* base, long pix, unsigned (&u)[16]) {
  const u32x4* p = (const u32x4*)(base + pix * 32);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const u32x4 v = p[q];
    u[4 * q] = v.x; u[4 * q + 1] = v.y; u[4 * q + 2] = v.z; u[4 * q + 3] = v.w;
  }
}
__device__ __forceinline__ float px_ch(const unsigned (&u)[16], int c) { return (c & 1) ? dd_bf16_hi(u[c >> 1]) : dd_bf16_lo(u[c >> 1]); }
__device__ __forceinline__ void store_px32(unsigned short* base, long pix, const float (&v)[32]) {
  u32x4* p = (u32x4*)(base + pix * 32);
#pragma unroll
  for (int q = 0; q < 4; ++q)
    p[q] = u32x4{dd_pack_bf16(v[8 * q], v[8 * q + 1]), dd_pack_bf16(v[8 * q + 2], v[8 * q + 3]), dd_pack_bf16(v[8 * q + 4], v[8 * q + 5]),
                 dd_pack_bf16(v[8 * q + 6], v[8 * q + 7])};
}

constexpr int kThreads = 256;
constexpr int kMaxGrid = 256;          // partial-sum grids: fixed, so the reduction order (and the workspace) depends on the shape only

__device__ __forceinline__ void acc4(float* acc, float v, f32x4 w) {
  acc[0] = fmaf(v, w.x, acc[0]); acc[1] = fmaf(v, w.y, acc[1]); acc[2] = fmaf(v, w.z, acc[2]); acc[3] = fmaf(v, w.w, acc[3]);
}

// ------------------------------------------------------------------------------------------------ dc1 (64 -> 32, k3 p1)
// dc1's input lives as two NHWC bf16 images of 32 channels (channels 0-31, 32-63): the weight and data gradients are then exactly
// two launches each of the encoder's c2 kernels (dd_conv_bf16_wgrad / _dgrad: a weight gradient splits over input channels, a data
// gradient over its output channels, neither with a rounding in between), and the forward below reads 16-byte operand pieces.

// fc2's fp32 NCHW-flat [B,64,H,W] -> two bf16 NHWC [B,H,W,32]; thread = (pixel, 8 channels): 8 plane reads coalesced along x
__global__ __launch_bounds__(kThreads) void split64_kernel(const float* __restrict__ h, unsigned short* __restrict__ lo,
                                                           unsigned short* __restrict__ hi, int B, int H, int W) {
  const long hw = (long)H * W, n = (long)B * hw * 8;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
    const int g = (int)(i / ((long)B * hw));               // channel group of 8: consecutive threads walk pixels
    const long p = i - (long)g * B * hw;
    const int b = (int)(p / hw);
    const long yx = p - (long)b * hw;
    const float* src = h + ((long)b * 64 + 8 * g) * hw + yx;
    u32x4 o;
    o.x = dd_pack_bf16(src[0], src[hw]); o.y = dd_pack_bf16(src[2 * hw], src[3 * hw]);
    o.z = dd_pack_bf16(src[4 * hw], src[5 * hw]); o.w = dd_pack_bf16(src[6 * hw], src[7 * hw]);
    unsigned short* dst = (g < 4 ? lo : hi) + p * 32 + (g & 3) * 8;
    *(u32x4*)dst = o;
  }
}

// the inverse, for the data gradient: two bf16 NHWC [B,H,W,32] -> fp32 NCHW-flat [B,64,H,W] (values stay bf16-exact)
__global__ __launch_bounds__(kThreads) void merge64_kernel(const unsigned short* __restrict__ lo, const unsigned short* __restrict__ hi,
                                                           float* __restrict__ gh, int B, int H, int W) {
  const long hw = (long)H * W, n = (long)B * hw * 8;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
    const int g = (int)(i / ((long)B * hw));
    const long p = i - (long)g * B * hw;
    const int b = (int)(p / hw);
    const long yx = p - (long)b * hw;
    const u32x4 v = *(const u32x4*)((g < 4 ? lo : hi) + p * 32 + (g & 3) * 8);
    float* dst = gh + ((long)b * 64 + 8 * g) * hw + yx;
    dst[0] = dd_bf16_lo(v.x); dst[hw] = dd_bf16_hi(v.x); dst[2 * hw] = dd_bf16_lo(v.y); dst[3 * hw] = dd_bf16_hi(v.y);
    dst[4 * hw] = dd_bf16_lo(v.z); dst[5 * hw] = dd_bf16_hi(v.z); dst[6 * hw] = dd_bf16_lo(v.w); dst[7 * hw] = dd_bf16_hi(v.w);
  }
}

// forward on v_mfma_f32_32x32x16_bf16: one wave = 32 consecutive output pixels of a row x 32 output channels, K = 9 taps x 64 input
// channels = 36 k16 steps.  A = weights (row = output channel), from an LDS image packed per (step, lane); B = pixels (column =
// pixel n, 8 channels of one tap per lane = one 16-byte load, zero outside the image).  Accumulator register r of lane l holds
// channel (r&3) + 8(r>>2) + 4(l>>5) of pixel l&31.
constexpr int kDc1Steps = 36;
constexpr int kWaves = kThreads / 64;

__global__ __launch_bounds__(kThreads) void dc1_fwd_mfma_kernel(const unsigned short* __restrict__ xlo, const unsigned short* __restrict__ xhi,
                                                                const float* __restrict__ w1, const float* __restrict__ b1,
                                                                unsigned short* __restrict__ a1, unsigned* __restrict__ bits, int B, int H,
                                                                int W) {
  __shared__ __attribute__((aligned(16))) unsigned wpk[kDc1Steps * 64 * 4];     // [step][lane] 8 bf16 = 36 KB
  __shared__ float bl[32];
  for (int i = threadIdx.x; i < kDc1Steps * 64 * 4; i += kThreads) {
    const int s = i >> 8, lane = (i >> 2) & 63, jj = i & 3;                      // word jj = elements 2jj, 2jj+1
    const int tap = s >> 2, cb = s & 3, co = lane & 31;
    const int ci = cb * 16 + 8 * (lane >> 5) + 2 * jj;
    // the equivalent convolution's weight Wc[co][ci][tap] = w1[ci][co][8 - tap] (transposed, flipped)
    wpk[i] = dd_pack_bf16(w1[(ci * 32 + co) * 9 + 8 - tap], w1[((ci + 1) * 32 + co) * 9 + 8 - tap]);
  }
  if (threadIdx.x < 32) bl[threadIdx.x] = b1[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 31, hh = lane >> 5;
  const int ntx = (W + 31) / 32;
  const long ntiles = (long)B * H * ntx;
  const bf16x8* wl = (const bf16x8*)wpk;
  for (long tile = (long)blockIdx.x * kWaves + wave; tile < ntiles; tile += (long)gridDim.x * kWaves) {
    const int b = (int)(tile / ((long)H * ntx));
    const int r = (int)(tile - (long)b * H * ntx), y = r / ntx, x = (r - y * ntx) * 32 + n;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int iy = y + tap / 3 - 1, ix = x + tap % 3 - 1;
      const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
      const long pix = ((long)b * H + (ok ? iy : 0)) * W + (ok ? ix : 0);
      u32x4 v[4];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        const unsigned short* img = cb < 2 ? xlo : xhi;
        v[cb] = ok ? *(const u32x4*)(img + pix * 32 + (cb & 1) * 16 + 8 * hh) : u32x4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
        acc = DD_MFMA_BF16(wl[(tap * 4 + cb) * 64 + lane], __builtin_bit_cast(bf16x8, v[cb]), acc);
    }
    unsigned mine = 0;
    float v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int co = dd_acc_row_half(q, hh);
      v[q] = fmaxf(acc[q] + bl[co], 0.f);
      mine |= (v[q] > 0.f ? 1u : 0u) << co;
    }
    const unsigned word = mine | (unsigned)__shfl_xor((int)mine, 32);
    if (x < W) {
      const long op = ((long)b * H + y) * W + x;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        u32x2 w2;
        w2.x = dd_pack_bf16(v[4 * g], v[4 * g + 1]);
        w2.y = dd_pack_bf16(v[4 * g + 2], v[4 * g + 3]);
        *(u32x2*)(a1 + op * 32 + 8 * g + 4 * hh) = w2;
      }
      if (bits && hh == 0) bits[op] = word;
    }
  }
}

// ------------------------------------------------------------------------------------------------ dc3 (32 -> 32, k2 s2) + dc4 (32 -> 3, k1)
constexpr int kPh = 32 * 32 + 4;       // one phase's [ci][co] block, padded: neighbouring lanes read neighbouring phases

__global__ __launch_bounds__(kThreads) void dc34_fwd_kernel(const unsigned short* __restrict__ a2, const float* __restrict__ w3,
                                                            const float* __restrict__ b3, const float* __restrict__ w4,
                                                            const float* __restrict__ b4, unsigned short* __restrict__ a3,
                                                            float* __restrict__ yout, int B, int H, int W) {
  __shared__ __attribute__((aligned(16))) float w3l[4 * kPh];         // [phase][ci][co]
  __shared__ float w4l[32 * 3], b3l[32], b4l[3];
  for (int i = threadIdx.x; i < 4 * 32 * 32; i += kThreads) {
    const int ph = i >> 10, ci = (i >> 5) & 31, co = i & 31;
    w3l[ph * kPh + ci * 32 + co] = bfr(w3[(ci * 32 + co) * 4 + ph]);
  }
  if (threadIdx.x < 96) w4l[threadIdx.x] = bfr(w4[threadIdx.x]);
  if (threadIdx.x < 32) b3l[threadIdx.x] = b3[threadIdx.x];
  if (threadIdx.x < 3) b4l[threadIdx.x] = b4[threadIdx.x];
  __syncthreads();
  const int Ho = 2 * H, Wo = 2 * W;
  const long ohw = (long)Ho * Wo, npix = (long)B * ohw;
  for (long p = (long)blockIdx.x * kThreads + threadIdx.x; p < npix; p += (long)gridDim.x * kThreads) {
    const int b = (int)(p / ohw);
    const int yx = (int)(p - (long)b * ohw), oy = yx / Wo, ox = yx - oy * Wo;
    const int ph = (oy & 1) * 2 + (ox & 1);
    unsigned u[16];
    load_px32(a2, ((long)b * H + (oy >> 1)) * W + (ox >> 1), u);
    float acc[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) acc[c] = b3l[c];
#pragma unroll 4
    for (int ci = 0; ci < 32; ++ci) {
      const float v = px_ch(u, ci);
      const f32x4* wr = (const f32x4*)(w3l + ph * kPh + ci * 32);
#pragma unroll
      for (int q = 0; q < 8; ++q) acc4(acc + 4 * q, v, wr[q]);
    }
    float y0 = b4l[0], y1 = b4l[1], y2 = b4l[2];
#pragma unroll
    for (int c = 0; c < 32; ++c) {
      acc[c] = bfr(fmaxf(acc[c], 0.f));          // a3 as stored: dc4 reads the bf16 value
      y0 = fmaf(acc[c], w4l[c * 3], y0);
      y1 = fmaf(acc[c], w4l[c * 3 + 1], y1);
      y2 = fmaf(acc[c], w4l[c * 3 + 2], y2);
    }
    store_px32(a3, p, acc);
    float* o = yout + (long)b * 3 * ohw + yx;
    o[0] = bfr(y0); o[ohw] = bfr(y1); o[2 * ohw] = bfr(y2);
  }
}

// dc4 backward: g3 = bf16(relu'(a3) * sum_k bf16(gy_k) * w4[c][k]) and the partials of dw4[c][k] = sum a3[c] * bf16(gy_k), db4[k] = sum bf16(gy_k)
constexpr int kDc4N = 99;
__global__ __launch_bounds__(kThreads) void dc4_bwd_kernel(const float* __restrict__ gy, const unsigned short* __restrict__ a3,
                                                           const float* __restrict__ w4, unsigned short* __restrict__ g3,
                                                           float* __restrict__ part, int B, int Ho, int Wo) {
  __shared__ float w4l[96];
  __shared__ float red[kThreads * 33];
  if (threadIdx.x < 96) w4l[threadIdx.x] = bfr(w4[threadIdx.x]);
  __syncthreads();
  float acc[kDc4N];
#pragma unroll
  for (int i = 0; i < kDc4N; ++i) acc[i] = 0.f;
  const long ohw = (long)Ho * Wo, npix = (long)B * ohw;
  for (long p = (long)blockIdx.x * kThreads + threadIdx.x; p < npix; p += (long)gridDim.x * kThreads) {
    const int b = (int)(p / ohw);
    const long yx = p - (long)b * ohw;
    const float* gp = gy + (long)b * 3 * ohw + yx;
    const float g0 = bfr(gp[0]), g1 = bfr(gp[ohw]), g2 = bfr(gp[2 * ohw]);
    unsigned u[16];
    load_px32(a3, p, u);
    float v[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) {
      const float a = px_ch(u, c);
      const float s = fmaf(g2, w4l[c * 3 + 2], fmaf(g1, w4l[c * 3 + 1], g0 * w4l[c * 3]));
      v[c] = a > 0.f ? s : 0.f;
      acc[c * 3] = fmaf(a, g0, acc[c * 3]);
      acc[c * 3 + 1] = fmaf(a, g1, acc[c * 3 + 1]);
      acc[c * 3 + 2] = fmaf(a, g2, acc[c * 3 + 2]);
    }
    acc[96] += g0; acc[97] += g1; acc[98] += g2;
    store_px32(g3, p, v);
  }
  // block sum in three rounds of 33 values, each summed by one thread over the 256 lanes in lane order
  float* out = part + (long)blockIdx.x * kDc4N;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 33; ++j) red[threadIdx.x * 33 + j] = acc[r * 33 + j];
    __syncthreads();
    if (threadIdx.x < 33) {
      float s = 0.f;
      for (int t = 0; t < kThreads; ++t) s += red[t * 33 + threadIdx.x];
      out[r * 33 + threadIdx.x] = s;
    }
  }
}

// dc3 data gradient with dc2's ReLU mask: g2[y,x,ci] = bit ? bf16(sum_{phase,co} g3[2y+i, 2x+j, co] * w3[ci][co][i][j]) : 0
__global__ __launch_bounds__(kThreads) void dc3_dgrad_kernel(const unsigned short* __restrict__ g3, const float* __restrict__ w3,
                                                             const unsigned* __restrict__ bits2, unsigned short* __restrict__ g2,
                                                             int B, int H, int W) {
  __shared__ __attribute__((aligned(16))) float wl[4 * 32 * 32];      // [phase][co][ci]
  for (int i = threadIdx.x; i < 4 * 32 * 32; i += kThreads) {
    const int ph = i >> 10, co = (i >> 5) & 31, ci = i & 31;
    wl[i] = bfr(w3[(ci * 32 + co) * 4 + ph]);
  }
  __syncthreads();
  const long hw = (long)H * W, npix = (long)B * hw;
  const int Wo = 2 * W;
  for (long p = (long)blockIdx.x * kThreads + threadIdx.x; p < npix; p += (long)gridDim.x * kThreads) {
    const int b = (int)(p / hw);
    const int yx = (int)(p - (long)b * hw), y = yx / W, x = yx - y * W;
    float acc[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) acc[c] = 0.f;
    for (int ph = 0; ph < 4; ++ph) {
      unsigned u[16];
      load_px32(g3, ((long)b * 2 * H + 2 * y + (ph >> 1)) * Wo + 2 * x + (ph & 1), u);
#pragma unroll 4
      for (int co = 0; co < 32; ++co) {
        const float g = px_ch(u, co);
        const f32x4* wr = (const f32x4*)(wl + (ph * 32 + co) * 32);
#pragma unroll
        for (int q = 0; q < 8; ++q) acc4(acc + 4 * q, g, wr[q]);
      }
    }
    const unsigned m = bits2[p];
#pragma unroll
    for (int c = 0; c < 32; ++c) acc[c] = ((m >> c) & 1u) ? acc[c] : 0.f;
    store_px32(g2, p, acc);
  }
}

// dc3 weight gradient partials: a tile is 64 consecutive input pixels; thread = (phase*32 + co, 16 input channels)
constexpr int kDc3N = 4096 + 32;
__global__ __launch_bounds__(kThreads) void dc3_wgrad_kernel(const unsigned short* __restrict__ a2, const unsigned short* __restrict__ g3,
                                                             float* __restrict__ part, int B, int H, int W) {
  __shared__ __attribute__((aligned(16))) float as[64 * 32];          // [px][ci]
  __shared__ float gs[64 * 128];                                       // [px][phase*32 + co]
  __shared__ float bs[128];
  const int n = threadIdx.x & 127, mg = threadIdx.x >> 7;
  float acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  float bacc = 0.f;
  const long hw = (long)H * W, npix = (long)B * hw, ntiles = (npix + 63) / 64;
  const int Wo = 2 * W;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long p0 = tile * 64;
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 32; i += kThreads) as[i] = (p0 + (i >> 5) < npix) ? bf_at(a2, p0 * 32 + i) : 0.f;
    for (int i = threadIdx.x; i < 64 * 128; i += kThreads) {
      const int px = i >> 7, k = i & 127, ph = k >> 5, co = k & 31;
      const long p = p0 + px;
      float v = 0.f;
      if (p < npix) {
        const int b = (int)(p / hw);
        const int yx = (int)(p - (long)b * hw), y = yx / W, x = yx - y * W;
        v = bf_at(g3, (((long)b * 2 * H + 2 * y + (ph >> 1)) * Wo + 2 * x + (ph & 1)) * 32 + co);
      }
      gs[i] = v;
    }
    __syncthreads();
    for (int px = 0; px < 64; ++px) {
      const float g = gs[px * 128 + n];
      if (mg == 0) bacc += g;
      const f32x4* ar = (const f32x4*)(as + px * 32 + mg * 16);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc4(acc + 4 * q, g, ar[q]);
    }
  }
  float* out = part + (long)blockIdx.x * kDc3N;
  const int ph = n >> 5, co = n & 31;
#pragma unroll
  for (int i = 0; i < 16; ++i) out[((mg * 16 + i) * 32 + co) * 4 + ph] = acc[i];      // dw3[ci][co][i][j]
  __syncthreads();
  if (mg == 0) bs[n] = bacc;
  __syncthreads();
  if (threadIdx.x < 32) out[4096 + threadIdx.x] = ((bs[threadIdx.x] + bs[32 + threadIdx.x]) + bs[64 + threadIdx.x]) + bs[96 + threadIdx.x];
}

// second stage of every weight gradient here: column i of the [nblk][n] partials, summed in block order -> dw[i] (i < nw) or db[i - nw]
__global__ __launch_bounds__(kThreads) void dec_reduce_kernel(const float* __restrict__ part, int nblk, int n, int nw,
                                                              float* __restrict__ dw, float* __restrict__ db) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  dd_sum_strided(s, part + i, n, nblk);
  if (i < nw) dw[i] = s;
  else db[i - nw] = s;
}

// ------------------------------------------------------------------------------------------------ host side
int check_dims(int B, int H, int W, const char* who) {
  DD_REQUIRE(B > 0 && H > 0 && W > 0, DD_ERR_BAD_ARG, "%s: non-positive size (B %d, %dx%d)", who, B, H, W);
  // the largest tensor of the stack (dc3's output, 32 channels at 2H x 2W) must stay addressable with the kernels' int row arithmetic
  DD_REQUIRE((long)B * 4 * H * W * 64 < (1L << 40) && 2L * H * 2L * W < (1L << 30), DD_ERR_UNSUPPORTED, "%s: %dx%d too large", who, H, W);
  return 0;
}

int aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int grid_for(long items) {
  const long g = (items + kThreads - 1) / kThreads;
  return (int)(g < 1 ? 1 : g > DD_NUM_CU * 2 ? DD_NUM_CU * 2 : g);
}
int partial_grid(int layer, long tiles) {      // dc3: three 41 KB workgroups per CU; dc4: its 99 accumulators are the cost, one per CU
  const long cap = layer == 3 ? 3L * DD_NUM_CU : (long)kMaxGrid;
  return (int)(tiles < 1 ? 1 : tiles > cap ? cap : tiles);
}

long wgrad_tiles(int layer, int B, int H, int W) {
  if (layer == 3) return ((long)B * H * W + 63) / 64;
  return ((long)B * 4 * H * W + kThreads - 1) / kThreads;      // layer 4: one pixel of the 2H x 2W grid per lane
}
int wgrad_cols(int layer) { return layer == 3 ? kDc3N : kDc4N; }

int reduce(const float* part, int nblk, int n, int nw, float* dw, float* db, hipStream_t st) {
  hipLaunchKernelGGL(dec_reduce_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, st, part, nblk, n, nw, dw, db);
  DD_LAUNCH_CHECK("dec_bf16 reduce");
  return 0;
}

int check_ws(int layer, int B, int H, int W, void* ws, int64_t ws_bytes, int* nblk) {
  *nblk = partial_grid(layer, wgrad_tiles(layer, B, H, W));
  const int64_t need = (int64_t)*nblk * wgrad_cols(layer) * 4;
  DD_REQUIRE(ws != nullptr && ws_bytes >= need, DD_ERR_BAD_ARG, "dec_bf16 wgrad: workspace %lld < %lld bytes", (long long)ws_bytes,
             (long long)need);
  return 0;
}

}  // namespace

extern "C" {

int dd_dec_bf16_split64(const float* h, uint16_t* x_lo, uint16_t* x_hi, int32_t batch, int32_t dh, int32_t dw, void* stream) {
  if (int rc = check_dims(batch, dh, dw, "dec_bf16_split64")) return rc;
  DD_REQUIRE(h && x_lo && x_hi, DD_ERR_BAD_ARG, "dec_bf16_split64: NULL pointer");
  DD_REQUIRE(aligned16(x_lo) && aligned16(x_hi), DD_ERR_BAD_ARG, "dec_bf16_split64: misaligned buffer");
  hipLaunchKernelGGL(split64_kernel, dim3(grid_for(8L * batch * dh * dw)), dim3(kThreads), 0, (hipStream_t)stream, h,
                     (unsigned short*)x_lo, (unsigned short*)x_hi, batch, dh, dw);
  DD_LAUNCH_CHECK("dec_bf16_split64");
  return 0;
}

int dd_dec_bf16_merge64(const uint16_t* g_lo, const uint16_t* g_hi, float* gh, int32_t batch, int32_t dh, int32_t dw, void* stream) {
  if (int rc = check_dims(batch, dh, dw, "dec_bf16_merge64")) return rc;
  DD_REQUIRE(g_lo && g_hi && gh, DD_ERR_BAD_ARG, "dec_bf16_merge64: NULL pointer");
  DD_REQUIRE(aligned16(g_lo) && aligned16(g_hi), DD_ERR_BAD_ARG, "dec_bf16_merge64: misaligned buffer");
  hipLaunchKernelGGL(merge64_kernel, dim3(grid_for(8L * batch * dh * dw)), dim3(kThreads), 0, (hipStream_t)stream,
                     (const unsigned short*)g_lo, (const unsigned short*)g_hi, gh, batch, dh, dw);
  DD_LAUNCH_CHECK("dec_bf16_merge64");
  return 0;
}

int dd_dec_bf16_dc1_fwd(const uint16_t* x_lo, const uint16_t* x_hi, const float* w1, const float* b1, uint16_t* a1, uint32_t* relu_bits,
                        int32_t batch, int32_t dh, int32_t dw, void* stream) {
  if (int rc = check_dims(batch, dh, dw, "dec_bf16_dc1_fwd")) return rc;
  DD_REQUIRE(x_lo && x_hi && w1 && b1 && a1, DD_ERR_BAD_ARG, "dec_bf16_dc1_fwd: NULL pointer");
  DD_REQUIRE(aligned16(x_lo) && aligned16(x_hi) && aligned16(a1), DD_ERR_BAD_ARG, "dec_bf16_dc1_fwd: misaligned buffer");
  const long tiles = (long)batch * dh * ((dw + 31) / 32);
  const long grid = (tiles + kWaves - 1) / kWaves;
  hipLaunchKernelGGL(dc1_fwd_mfma_kernel, dim3((unsigned)(grid < DD_NUM_CU * 4 ? grid : DD_NUM_CU * 4)), dim3(kThreads), 0,
                     (hipStream_t)stream, (const unsigned short*)x_lo, (const unsigned short*)x_hi, w1, b1, (unsigned short*)a1,
                     relu_bits, batch, dh, dw);
  DD_LAUNCH_CHECK("dec_bf16_dc1_fwd");
  return 0;
}

int64_t dd_dec_bf16_wgrad_workspace_bytes(int32_t layer, int32_t batch, int32_t dh, int32_t dw) {
  if (layer != 3 && layer != 4) {
    dd_fail(DD_ERR_BAD_ARG, "dec_bf16 wgrad: layer %d (3 or 4)", layer);
    return -1;
  }
  if (check_dims(batch, dh, dw, "dec_bf16 wgrad")) return -1;
  return (int64_t)partial_grid(layer, wgrad_tiles(layer, batch, dh, dw)) * wgrad_cols(layer) * 4;
}

int dd_dec_bf16_dc34_fwd(const uint16_t* a2, const float* w3, const float* b3, const float* w4, const float* b4, uint16_t* a3,
                         float* y, int32_t batch, int32_t dh, int32_t dw, void* stream) {
  if (int rc = check_dims(batch, dh, dw, "dec_bf16_dc34_fwd")) return rc;
  DD_REQUIRE(a2 && w3 && b3 && w4 && b4 && a3 && y, DD_ERR_BAD_ARG, "dec_bf16_dc34_fwd: NULL pointer");
  DD_REQUIRE(aligned16(a2) && aligned16(a3), DD_ERR_BAD_ARG, "dec_bf16_dc34_fwd: misaligned buffer");
  hipLaunchKernelGGL(dc34_fwd_kernel, dim3(grid_for(4L * batch * dh * dw)), dim3(kThreads), 0, (hipStream_t)stream,
                     (const unsigned short*)a2, w3, b3, w4, b4, (unsigned short*)a3, y, batch, dh, dw);
  DD_LAUNCH_CHECK("dec_bf16_dc34_fwd");
  return 0;
}

int dd_dec_bf16_dc4_bwd(const float* gy, const uint16_t* a3, const float* w4, uint16_t* g3, float* dweight, float* dbias,
                        int32_t batch, int32_t dh, int32_t dw, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_dims(batch, dh, dw, "dec_bf16_dc4_bwd")) return rc;
  DD_REQUIRE(gy && a3 && w4 && g3 && dweight && dbias, DD_ERR_BAD_ARG, "dec_bf16_dc4_bwd: NULL pointer");
  DD_REQUIRE(aligned16(a3) && aligned16(g3), DD_ERR_BAD_ARG, "dec_bf16_dc4_bwd: misaligned buffer");
  int nblk = 0;
  if (int rc = check_ws(4, batch, dh, dw, workspace, workspace_bytes, &nblk)) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dc4_bwd_kernel, dim3(nblk), dim3(kThreads), 0, st, gy, (const unsigned short*)a3, w4, (unsigned short*)g3,
                     (float*)workspace, batch, 2 * dh, 2 * dw);
  DD_LAUNCH_CHECK("dec_bf16_dc4_bwd");
  return reduce((const float*)workspace, nblk, kDc4N, 96, dweight, dbias, st);
}

int dd_dec_bf16_dc3_dgrad(const uint16_t* g3, const float* w3, const uint32_t* relu_bits, uint16_t* g2, int32_t batch, int32_t dh,
                          int32_t dw, void* stream) {
  if (int rc = check_dims(batch, dh, dw, "dec_bf16_dc3_dgrad")) return rc;
  DD_REQUIRE(g3 && w3 && relu_bits && g2, DD_ERR_BAD_ARG, "dec_bf16_dc3_dgrad: NULL pointer");
  DD_REQUIRE(aligned16(g3) && aligned16(g2), DD_ERR_BAD_ARG, "dec_bf16_dc3_dgrad: misaligned buffer");
  hipLaunchKernelGGL(dc3_dgrad_kernel, dim3(grid_for((long)batch * dh * dw)), dim3(kThreads), 0, (hipStream_t)stream,
                     (const unsigned short*)g3, w3, relu_bits, (unsigned short*)g2, batch, dh, dw);
  DD_LAUNCH_CHECK("dec_bf16_dc3_dgrad");
  return 0;
}

int dd_dec_bf16_dc3_wgrad(const uint16_t* a2, const uint16_t* g3, float* dweight, float* dbias, int32_t batch, int32_t dh, int32_t dw,
                          void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_dims(batch, dh, dw, "dec_bf16_dc3_wgrad")) return rc;
  DD_REQUIRE(a2 && g3 && dweight && dbias, DD_ERR_BAD_ARG, "dec_bf16_dc3_wgrad: NULL pointer");
  int nblk = 0;
  if (int rc = check_ws(3, batch, dh, dw, workspace, workspace_bytes, &nblk)) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dc3_wgrad_kernel, dim3(nblk), dim3(kThreads), 0, st, (const unsigned short*)a2, (const unsigned short*)g3,
                     (float*)workspace, batch, dh, dw);
  DD_LAUNCH_CHECK("dec_bf16_dc3_wgrad");
  return reduce((const float*)workspace, nblk, kDc3N, 4096, dweight, dbias, st);
}

}  // extern "C"

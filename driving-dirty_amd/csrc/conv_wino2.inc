// c2 (the 32 -> 32 stride-1 layer), the default path: forward and data gradient (conv_wino2r_fwd; conv_wino2_fwd behind DD_WINO2_RING*),
// the fused 3 -> 32 weight gradient, the weight gradient (conv_wino2_wgrad) and the packing.  Part of conv3x3.hip's translation unit (included at its end).
// Winograd F(2x2, 3x3): the transform of conv_wino.inc (inputs v, weights u, outputs y) along y as well -- a 2x2 output tile from a 4x4 input patch with 16
// multiplies instead of 36 (4/9 of the direct form's matrix-core work, 2/3 of the 1-D form's).  Needs four ring rows
// per wave and 64 KB of transformed weights, which leaves room for ONE wave per SIMD (4-wave workgroups, 134 KB): every
// non-MFMA instruction therefore has to sit in the shadow of an MFMA, and no MFMA may wait for a VALU result.
// Per iteration a wave produces 2 output rows x 32 pixels = 16 tiles: 16 positions x 2 channel halves x 8 k-steps =
// 256 v_mfma_f32_16x16x4_f32 (8192 cycles).  Lane (tile t = lane&15, q = lane>>4) transforms input channels 8q..8q+7
// of its own tile; per channel quad g the x-stage results w[4][4] live in registers, the y-stage row V[u][0..3] of the
// NEXT position row is computed while the current row's 32 MFMAs execute, and its 8 U vectors are read a stage earlier.
namespace {

constexpr int WINO2_UFLOATS = 16 * 2 * 2 * 64 * 4;      // [pos = 4u+v][half][chunk][lane][4]

template <int EPI, int WPB>   // EPI_BIAS_RELU_BITS (forward) or EPI_RELU_BITS (data gradient)
__global__ __launch_bounds__(WPB * 64) void conv_wino2_fwd(const float* __restrict__ x, const float* __restrict__ up,
                                                           const float* __restrict__ bias, const unsigned* __restrict__ bits_in,
                                                           float* __restrict__ y, unsigned* __restrict__ bits_out, int B, int H,
                                                           int W, int nstrips, const float* __restrict__ x4 = nullptr,
                                                           float* __restrict__ w1part = nullptr) {
  using C = StripCfg<32, 1>;
  using C4 = StripCfg<4, 1>;
  constexpr int RINGB = 4 * C::SLOTB + C::SPILLB;
  constexpr bool W1 = (EPI == EPI_RELU_BITS_W1);
  constexpr bool MASKED = (EPI == EPI_RELU_BITS) || W1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  {
    f32x4* ul4 = (f32x4*)smem;
    const f32x4* ug4 = (const f32x4*)up;
    for (int i = tid; i < WINO2_UFLOATS / 4; i += WPB * 64) ul4[i] = ug4[i];
  }
  // W1: the 3 -> 32 layer's weight gradient dW1[co][(ky,kx,ci)] += g1[pixel][co] * x[pixel + (ky-1, kx-1)][ci] taken from
  // the outputs while they are in registers (they are exactly the A operand of a 16x16x4 MFMA: lane = channel, k = the
  // four tiles 4q+r of the lane groups); B = the image patch, gathered from a 4-row ring of the NHWC4 input (16 bytes a
  // pixel) in LDS with one ds_read_b32 per MFMA pair.  Column 27 reads a constant 1 (bias gradient), 28..31 are ignored.
  constexpr int W2_XRINGB = 4 * C4::SLOTB + C4::SPILLB;
  constexpr int W2_XBASE = WINO2_UFLOATS * 4 + WPB * RINGB;
  if (W1 && tid < 32) ((float*)(smem + W2_XBASE + WPB * W2_XRINGB))[tid] = 1.f;
  __syncthreads();
  char* xring = smem + W2_XBASE + wave * W2_XRINGB;
  char* xspill = xring + 4 * C4::SLOTB;
  f32x4 wacc[2][2];      // [channel half][column half] of dW1, this wave's share
#pragma unroll
  for (int hf = 0; hf < 2; ++hf)
#pragma unroll
    for (int nh = 0; nh < 2; ++nh) wacc[hf][nh] = f32x4{0.f, 0.f, 0.f, 0.f};
  char* ring = smem + WINO2_UFLOATS * 4 + wave * RINGB;
  char* spill = ring + 4 * C::SLOTB;
  const f32x4* ul = (const f32x4*)smem;
  const int t16 = lane & 15, q4 = lane >> 4;
  int xky[2], xlane[2];      // W1: this lane's patch column c = t16 + 16 nh -> tap row, byte offset inside a ring slot
#pragma unroll
  for (int nh = 0; nh < 2; ++nh) {
    const int c = min(t16 + 16 * nh, 26), tap = c / 3, ci = c - 3 * tap, ky = tap / 3, kx = tap - 3 * ky;
    xky[nh] = ky;
    xlane[nh] = (8 * q4 + kx) * 16 + ci * 4;
  }
  const float bv0 = (EPI == EPI_BIAS_RELU_BITS) ? bias[t16] : 0.f, bv1 = (EPI == EPI_BIAS_RELU_BITS) ? bias[16 + t16] : 0.f;
  const f32x4 bias0 = {bv0, bv0, bv0, bv0}, bias1 = {bv1, bv1, bv1, bv1};
  const int HT = (H + 1) / 2;                         // tile rows

  long idx, end;
  dd_range((long)B * nstrips * HT, blockIdx.x * WPB + wave, gridDim.x * WPB, idx, end);
  while (idx < end) {
    const long col = idx / HT;
    const int r0 = (int)(idx - col * HT);
    const int r1 = (int)min((long)HT, r0 + (end - idx));
    idx += r1 - r0;
    const int b = (int)(col / nstrips), x0 = (int)(col % nstrips) * 32;
    const float* xb = x + (long)b * H * W * 32;
    const float* x4b = x4 + (long)b * H * W * 4;
    const int gx0 = x0 - 1;

#pragma unroll
    for (int d = 0; d < 4; ++d) {      // input rows 2*r0 - 1 .. 2*r0 + 2; slot of row iy = (iy + 1) & 3
      f32x4 t[C::NLOAD];
      const int iy = 2 * r0 - 1 + d;
      load_row<32, 1>(xb, H, W, iy, gx0, lane, t);
      store_row<32, 1, true>(ring + ((iy + 1) & 3) * C::SLOTB, spill, lane, t);
      if (W1) {      // the same four rows of the image, same slots
        f32x4 t4[C4::NLOAD];
        load_row<4, 1>(x4b, H, W, iy, gx0, lane, t4);
        store_row<4, 1, false>(xring + ((iy + 1) & 3) * C4::SLOTB, xspill, lane, t4);
      }
    }

    // Operand pipeline.  With one wave per SIMD an instruction hides only in the ~24 issue cycles an MFMA leaves free,
    // so (a) every stage is ONE scheduling region in which the 32 MFMAs and the work for LATER stages are interleaved
    // (sched_group_barrier), and (b) nothing in a stage waits for a load issued in the same stage:
    //   patch reads of the next channel quad (or of the next tile-row's first quad)   issued in stage 2 (6)
    //   their x-stage (64 VALU, in place: the old w is dead once V of stage 3 (7) exists)   in stage 3 (7)
    //   U vectors of stage s+1   read in stage s;   V of stage s+1   computed from w in stage s
    //   arriving rows -> ring   in stage 4 (the last patch read of this tile-row left in stage 2)
    auto rowslot = [&](int tr, int r) { return ring + ((2 * tr + r) & 3) * C::SLOTB; };      // slot of input row 2*tr - 1 + r
    auto patch_read = [&](int tr, int g, f32x4 (&d)[4][4]) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const char* rp = rowslot(tr, r);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int px = 2 * t16 + c;
          d[r][c] = *(const f32x4*)(rp + px * 128 + (((2 * q4 + g) ^ swz<32>(px)) << 4));
        }
      }
    };
    auto xstage = [&](const f32x4 (&d)[4][4], f32x4 (&w)[4][4]) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        w[r][0] = pk_sub4(d[r][0], d[r][2]);
        w[r][1] = pk_add4(d[r][1], d[r][2]);
        w[r][2] = pk_sub4(d[r][2], d[r][1]);
        w[r][3] = pk_sub4(d[r][1], d[r][3]);
      }
    };
    auto ystage = [&](int u, const f32x4 (&w)[4][4], f32x4 (&v)[4]) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (u == 0) v[c] = pk_sub4(w[0][c], w[2][c]);
        else if (u == 1) v[c] = pk_add4(w[1][c], w[2][c]);
        else if (u == 2) v[c] = pk_sub4(w[2][c], w[1][c]);
        else v[c] = pk_sub4(w[1][c], w[3][c]);
      }
    };
    auto uread = [&](int g, int u, f32x4 (&uu)[4][2]) {
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) uu[v][hf] = ul[((((u * 4 + v) * 2 + hf) * 2 + g) * 64) + lane];
    };

    f32x4 dp[4][4];                 // patch of the quad whose x-stage comes next
    f32x4 wq[4][4];                 // x-stage results of the current channel quad
    f32x4 vq[2][4], uq[2][4][2];    // V row and U vectors of the current / next stage
    patch_read(r0, 0, dp);
    xstage(dp, wq);
    ystage(0, wq, vq[0]);
    uread(0, 0, uq[0]);

    for (int tr = r0; tr < r1; ++tr) {
      f32x4 pre[2][C::NLOAD];
      load_row_img<32, 1>(xb, H, W, 2 * tr + 3, gx0, lane, pre[0]);
      load_row_img<32, 1>(xb, H, W, 2 * tr + 4, gx0, lane, pre[1]);
      f32x4 xpre[2][C4::NLOAD];
      unsigned mw[2][8];
      if (MASKED) {   // sign words of this lane's 2 x 8 output pixels (tiles 4q..4q+3)
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          const int oy = 2 * tr + a;
          const int mso = (oy < H) ? oy * W * 4 : 0;
          const __amdgpu_buffer_rsrc_t ms = dd_rsrc(bits_in + (long)b * H * W, (oy < H) ? mso + W * 4 : 0);
#pragma unroll
          for (int i = 0; i < 8; ++i) mw[a][i] = __builtin_amdgcn_raw_buffer_load_b32(ms, (x0 + 8 * q4 + i) * 4, mso, 0);
        }
      }

      f32x4 acc[16][2];
#pragma unroll
      for (int st = 0; st < 8; ++st) {
        const int g = st >> 2, u = st & 3;
        __builtin_amdgcn_sched_barrier(0);
        // ---- work for later stages (independent of this stage's MFMAs) ----
        if (st == 2) patch_read(tr, 1, dp);
        if (st == 6) patch_read(tr + 1, 0, dp);
        if (st == 3 || st == 7) xstage(dp, wq);
        if (st + 1 < 8) {
          uread((st + 1) >> 2, (st + 1) & 3, uq[(st + 1) & 1]);
          ystage((st + 1) & 3, wq, vq[(st + 1) & 1]);
        } else {
          uread(0, 0, uq[0]);
          ystage(0, wq, vq[0]);
        }
        if (W1 && st == 7) {      // image rows for the next tile-row: they land after this tile-row's epilogue has read the old ones
          load_row_img<4, 1>(x4b, H, W, 2 * tr + 3, gx0, lane, xpre[0]);
          load_row_img<4, 1>(x4b, H, W, 2 * tr + 4, gx0, lane, xpre[1]);
        }
        if (st == 4) {      // rows 2tr+3, 2tr+4 replace rows 2tr-1, 2tr in the ring
          store_row<32, 1, true>(ring + ((2 * tr + 4) & 3) * C::SLOTB, spill, lane, pre[0]);
          store_row<32, 1, true>(ring + ((2 * tr + 5) & 3) * C::SLOTB, spill, lane, pre[1]);
        }
        // ---- this stage's 32 MFMAs ----
        const f32x4(&vv)[4] = vq[st & 1];
        const f32x4(&uu)[4][2] = uq[st & 1];
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
              // the first MFMA of an accumulator takes a literal zero (no register clears) -- or, at position (1,1), the
              // bias: A^T e11 A = all ones, so a constant in M[1][1] reaches all four outputs of the tile once
              const f32x4 init = (EPI == EPI_BIAS_RELU_BITS && u == 1 && v == 1) ? (hf ? bias1 : bias0) : zero;
              acc[u * 4 + v][hf] = DD_MFMA16(vv[v][j], uu[v][hf][j], (g == 0 && j == 0) ? init : acc[u * 4 + v][hf]);
            }
        // interleave: one MFMA, then a few of the other instructions, 32 times
#pragma unroll
        for (int i = 0; i < 32; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // MFMA
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // DS read
          __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);      // VALU
          __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);      // DS write
        }
        __builtin_amdgcn_sched_barrier(0);
      }

      // output transform + epilogue: lane = channel t16 (+16 per half), register r = tile 4q + r
      unsigned keep[2][8];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int i = 0; i < 8; ++i) keep[a][i] = 0;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int oy = 2 * tr + a;
        const long opix = (long)(b * H + min(oy, H - 1)) * W;
        const __amdgpu_buffer_rsrc_t ys = dd_rsrc(y + (W1 ? 0 : opix * 32), (!W1 && oy < H) ? W * 128 : 0);
        const char* xa[2];      // W1: this lane's patch element of output pixel (row a, tile 4q, e = 0): ring slot of image row oy + ky - 1
#pragma unroll
        for (int nh = 0; nh < 2; ++nh) {
          const char* in_ring = xring + ((2 * tr + a + xky[nh]) & 3) * C4::SLOTB + xlane[nh];
          xa[nh] = (t16 + 16 * nh >= 27) ? smem + W2_XBASE + WPB * W2_XRINGB : in_ring;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int opx = x0 + 2 * (4 * q4 + r) + e;
            float o[2];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
              float z[4];      // z[u] = x-direction output transform of position row u
#pragma unroll
              for (int u = 0; u < 4; ++u) {
                const float m0 = acc[u * 4 + 0][hf][r], m1 = acc[u * 4 + 1][hf][r], m2 = acc[u * 4 + 2][hf][r], m3 = acc[u * 4 + 3][hf][r];
                z[u] = e == 0 ? (m0 + m1) + m2 : (m1 - m2) - m3;
              }
              float v = a == 0 ? (z[0] + z[1]) + z[2] : (z[1] - z[2]) - z[3];
              if (EPI == EPI_BIAS_RELU_BITS) v = fmaxf(v, 0.f);      // the bias came in through the accumulator
              // (sign-extended 1-bit field = all ones or zero, then one AND: two vector instructions per element instead of the
              // and / compare / select of `bit ? v : 0`)
              if (MASKED) v = __builtin_bit_cast(float, __builtin_bit_cast(int, v) & __builtin_amdgcn_sbfe((int)mw[a][2 * r + e], (unsigned)(t16 + 16 * hf), 1u));
              o[hf] = v;
              if (!W1) dd_bstore1<DD_AUX_NT>(ys, (opx * 32 + t16 + 16 * hf) * 4, v);
            }
            if (W1) {
              const float b0 = *(const float*)(xa[0] + (2 * r + e) * 16), b1 = *(const float*)(xa[1] + (2 * r + e) * 16);
              wacc[0][0] = DD_MFMA16(o[0], b0, wacc[0][0]);
              wacc[0][1] = DD_MFMA16(o[0], b1, wacc[0][1]);
              wacc[1][0] = DD_MFMA16(o[1], b0, wacc[1][0]);
              wacc[1][1] = DD_MFMA16(o[1], b1, wacc[1][1]);
            }
            if (EPI == EPI_BIAS_RELU_BITS) {
              const unsigned long long b0 = __ballot(o[0] > 0.f), b1 = __ballot(o[1] > 0.f);
              const int G = (lane & 31) >> 3;
              keep[a][2 * r + e] = (unsigned)((b0 >> (16 * G)) & 0xffffull) | ((unsigned)((b1 >> (16 * G)) & 0xffffull) << 16);
            }
          }
        }
        if (EPI == EPI_BIAS_RELU_BITS) {
          const int P = lane & 31, sel = P & 7;
          unsigned word = keep[a][0];
#pragma unroll
          for (int i = 1; i < 8; ++i) word = (sel == i) ? keep[a][i] : word;
          const __amdgpu_buffer_rsrc_t bs = dd_rsrc(bits_out + opix, (oy < H) ? W * 4 : 0);
          __builtin_amdgcn_raw_buffer_store_b32(word, bs, (lane < 32) ? (x0 + P) * 4 : -16, 0, 0);
        }
      }
      if (W1) {
        store_row<4, 1, false>(xring + ((2 * tr + 4) & 3) * C4::SLOTB, xspill, lane, xpre[0]);
        store_row<4, 1, false>(xring + ((2 * tr + 5) & 3) * C4::SLOTB, xspill, lane, xpre[1]);
      }
    }
  }
  if (W1) {
    const long gw = (long)blockIdx.x * WPB + wave;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
      for (int nh = 0; nh < 2; ++nh)
#pragma unroll
        for (int i = 0; i < 4; ++i) w1part[((gw * 2 + hf) * 2 + nh) * 256 + i * 64 + lane] = wacc[hf][nh][i];
  }
}

// ------------------------------------------------------------------------------------------------
// The same arithmetic with the input rows held in REGISTERS (default; conv_wino2_fwd above is the LDS-ring form kept for A/B).
// A lane's x-stage results of one input row (its tile, its 8 channels: 8 float4) serve two tile-rows -- rows 2tr+1, 2tr+2 are
// r = 2, 3 of tile-row tr and r = 0, 1 of tile-row tr+1 -- so four such rows (128 VGPRs) rotate and every input row is loaded
// (straight from global memory: 16 bytes a lane, the row's 4.3 KB twice out of L1) and x-transformed ONCE, not twice; no ring,
// no LDS writes, LDS holds only U.  The stages run u-major (s = 2u + g): position row u is complete after stage 2u+1, so the
// accumulators are two rows of 32 registers, and the output transform of row u -- A^T along x, then its term of the y sum --
// sits in the shadow of the next row's MFMAs; output row 2tr leaves in stage 7, output row 2tr+1 in stages 0-1 of the NEXT
// tile-row (the first pass of a column sees an empty store window and zero mask words).  Same operands in the same order as
// conv_wino2_fwd: the same bits.
// ------------------------------------------------------------------------------------------------
template <int EPI, int WPB>
__global__ __launch_bounds__(WPB * 64) void conv_wino2r_fwd(const float* __restrict__ x, const float* __restrict__ up,
                                                            const float* __restrict__ bias, const unsigned* __restrict__ bits_in,
                                                            float* __restrict__ y, unsigned* __restrict__ bits_out, int B, int H,
                                                            int W, int nstrips, const float* __restrict__ x4 = nullptr,
                                                            float* __restrict__ w1part = nullptr, int pf_rows = 0) {
  using C4 = StripCfg<4, 1>;
  constexpr bool W1 = (EPI == EPI_RELU_BITS_W1);
  constexpr bool MASKED = (EPI == EPI_RELU_BITS) || W1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  {
    // U image -> LDS with the input channels regrouped: here lane group q4 and quad g hold channels 16 g + 4 q4 .. + 3 (the
    // packed image has 8 q4 + 4 g .. + 3), so that the four lane groups of a patch load read 64 contiguous bytes of a pixel.
    // [pos][half][g][lane = 16 q4 + t16]  <-  [pos][half][q4 & 1][16 (2 g + (q4 >> 1)) + t16]
    f32x4* ul4 = (f32x4*)smem;
    const f32x4* ug4 = (const f32x4*)up;
#pragma unroll 4
    for (int i = tid; i < WINO2_UFLOATS / 4; i += WPB * 64) {
      const int ln = i & 63, gq = (i >> 6) & 1, hi = i >> 7, qq = ln >> 4;
      ul4[i] = ug4[(hi * 2 + (qq & 1)) * 64 + (2 * gq + (qq >> 1)) * 16 + (ln & 15)];
    }
  }
  constexpr int W2_XRINGB = 4 * C4::SLOTB + C4::SPILLB;
  constexpr int W2_XBASE = WINO2_UFLOATS * 4;
  if (W1 && tid < 32) ((float*)(smem + W2_XBASE + WPB * W2_XRINGB))[tid] = 1.f;
  if (W1)      // the first pass of a column multiplies masked-out zeros with whatever the image ring holds: keep that finite
    for (int i = tid; i < WPB * W2_XRINGB / 16; i += WPB * 64) ((f32x4*)(smem + W2_XBASE))[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  char* xring = smem + W2_XBASE + wave * W2_XRINGB;      // W1: 4-row ring of the NHWC4 image, slot of row iy = (iy + 1) & 3
  char* xspill = xring + 4 * C4::SLOTB;
  f32x4 wacc[2][2];
#pragma unroll
  for (int hf = 0; hf < 2; ++hf)
#pragma unroll
    for (int nh = 0; nh < 2; ++nh) wacc[hf][nh] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ulane = (int)(unsigned long)(__attribute__((address_space(3))) char*)smem + lane * 16;      // LDS byte address of U[..][lane]
  const int t16 = lane & 15, q4 = lane >> 4;
  int xky[2], xlane[2];
#pragma unroll
  for (int nh = 0; nh < 2; ++nh) {
    const int c = min(t16 + 16 * nh, 26), tap = c / 3, ci = c - 3 * tap, ky = tap / 3, kx = tap - 3 * ky;
    xky[nh] = ky;
    xlane[nh] = (8 * q4 + kx) * 16 + ci * 4;
  }
  const float bv0 = (EPI == EPI_BIAS_RELU_BITS) ? bias[t16] : 0.f, bv1 = (EPI == EPI_BIAS_RELU_BITS) ? bias[16 + t16] : 0.f;
  const f32x4 bias0 = {bv0, bv0, bv0, bv0}, bias1 = {bv1, bv1, bv1, bv1};
  const int HT = (H + 1) / 2;

  f32x4 accr[2][4][2];      // [position row u & 1][v][channel half]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) accr[i][v][hf] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x2 o1[2][2][2];        // [register pair][column e][channel half]: output row 2tr+1 on its way (z1 - z2 - z3)
#pragma unroll
  for (int i = 0; i < 8; ++i) o1[i >> 2][(i >> 1) & 1][i & 1] = f32x2{0.f, 0.f};

  float pfacc = 0.f;
  long idx, end;
  dd_range((long)B * nstrips * HT, blockIdx.x * WPB + wave, gridDim.x * WPB, idx, end);
  while (idx < end) {
    const long col = idx / HT;
    const int r0 = (int)(idx - col * HT);
    const int r1 = (int)min((long)HT, r0 + (end - idx));
    idx += r1 - r0;
    const int b = (int)(col / nstrips), x0 = (int)(col % nstrips) * 32;
    const float* xb = x + (long)b * H * W * 32;
    const float* x4b = x4 + (long)b * H * W * 4;
    // Descriptors: ONE per tensor and column -- base = the image, num_records = the whole image; the row goes into the scalar
    // offset (range-checked together with the lane offset on this part: tools/ubench/soffset_probe.hip), so rows -1 and H fall
    // out of range by themselves, and the pixels left and right of a row are put out of range by the LANE offsets, which do not
    // change down a column (poff, pst, boff below).  A descriptor per row (base + row * pitch in 64 bits, the 16-bit split of the
    // address, the size select) cost the wave ~500 of its ~11,700 cycles per tile-row.
    float* yb = y + (W1 ? 0 : (long)b * H * W * 32);
    unsigned* bob = bits_out + (EPI == EPI_BIAS_RELU_BITS ? (long)b * H * W : 0);
    const unsigned* bib = bits_in + (MASKED ? (long)b * H * W : 0);
    const int pitch = W * 128, pitchb = W * 4;
    constexpr int FAR = 1 << 30;      // beyond any image (the launcher checks H * W * 128 < 2^30), no wrap with a row offset on top
    const __amdgpu_buffer_rsrc_t xrs = dd_rsrc(xb, H * pitch), bors = dd_rsrc(bob, H * pitchb), birs = dd_rsrc(bib, H * pitchb);
    const i32x4 yrs = dd_rsrc_words(yb, W1 ? 0 : H * pitch);
    const int gx0 = x0 - 1;
    int poff[4];      // byte offset of this lane's patch column c inside an input row (left / right of the image: out of range -> 0)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int px = gx0 + 2 * t16 + c;
      poff[c] = (px >= 0 && px < W) ? px * 128 + q4 * 16 : FAR;
    }
    int pst[8];       // byte offset of this lane's output pixel 2r + e of a tile-row's 8, channel t16 (+ 16 hf: the instruction offset)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int px = x0 + 8 * q4 + q;
      pst[q] = (px < W) ? px * 128 + t16 * 4 : FAR;
    }
    int pmk[8];       // ... and of its sign word (zero right of the row: with W1 the masked gradient of such a pixel meets image pixels W-1)
#pragma unroll
    for (int q = 0; q < 8; ++q) pmk[q] = (MASKED && x0 + 8 * q4 + q < W) ? (x0 + 8 * q4 + q) * 4 : FAR;
    // L2 prefetch (pf_rows tile-rows ahead): one dword of each 64-byte half of the strip's 34 pixels of an input row
    const int pfoff = (lane < 34 && gx0 + lane >= 0 && gx0 + lane < W) ? (gx0 + lane) * 128 : FAR;
    const int boff = (lane < 32 && x0 + (lane & 31) < W) ? (x0 + (lane & 31)) * 4 : FAR;      // the sign word lane P < 32 stores

    auto row_load = [&](int iy, f32x4 (&R)[2][4]) {      // input row iy: patch columns 2 t16 .. + 3, channels 16 g + 4 q4 .. + 3
      const int so = iy * pitch;      // row -1: a huge unsigned offset, out of range like row H
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int c = 0; c < 4; ++c) R[g][c] = dd_bload4(xrs, poff[c] + g * 64, so);
    };
    auto xstage = [&](const f32x4 (&L)[2][4], f32x4 (&R)[2][4]) {      // landing registers -> row registers (or in place)
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const f32x4 d0 = L[g][0], d1 = L[g][1], d2 = L[g][2], d3 = L[g][3];
        R[g][0] = pk_sub4(d0, d2);
        R[g][1] = pk_add4a(d1, d2);
        R[g][2] = pk_sub4(d2, d1);
        R[g][3] = pk_sub4(d1, d3);
      }
    };
    auto ystage = [&](int u, int g, const f32x4 (&A0)[2][4], const f32x4 (&A1)[2][4], const f32x4 (&A2)[2][4], const f32x4 (&A3)[2][4],
                      f32x4 (&v)[4]) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (u == 0) v[c] = pk_sub4(A0[g][c], A2[g][c]);
        else if (u == 1) v[c] = pk_add4a(A1[g][c], A2[g][c]);
        else if (u == 2) v[c] = pk_sub4(A2[g][c], A1[g][c]);
        else v[c] = pk_sub4(A1[g][c], A3[g][c]);
      }
    };
    // U vectors go from LDS straight into ACCUMULATION registers and from there into the MFMAs' B operand: they never hold a
    // VGPR (64 of them in the ring form).  The compiler does not see these reads: u_wait() below stands between them and their use.
    auto uread = [&](int g, int u, f32x4 (&uu)[4][2]) {
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
          asm volatile("ds_read_b128 %0, %1 offset:%2" : "=a"(uu[v][hf]) : "v"(ulane), "n"(((((u * 4 + v) * 2 + hf) * 2 + g) * 1024)));
    };
    auto uread1 = [&](int g, int u, int v, int hf, f32x4& d) {
      asm volatile("ds_read_b128 %0, %1 offset:%2" : "=a"(d) : "v"(ulane), "n"(((((u * 4 + v) * 2 + hf) * 2 + g) * 1024)));
    };
    auto u_wait = [&](f32x4 (&uu)[4][2]) {
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+a"(uu[0][0]), "+a"(uu[0][1]), "+a"(uu[1][0]), "+a"(uu[1][1]), "+a"(uu[2][0]), "+a"(uu[2][1]), "+a"(uu[3][0]), "+a"(uu[3][1]));
    };
    auto mask_load = [&](int oy, unsigned (&m)[8]) {      // sign words of this lane's 8 output pixels (tiles 4q .. 4q+3) of row oy
      const int so = oy * pitchb;
#pragma unroll
      for (int i = 0; i < 8; ++i) m[i] = __builtin_amdgcn_raw_buffer_load_b32(birs, pmk[i], so, 0);
    };
    auto acc_read2 = [&](float a0, float a1, f32x2& d) {
      float lo, hi;
      asm volatile("v_accvgpr_read_b32 %0, %2\n\tv_accvgpr_read_b32 %1, %3" : "=v"(lo), "=v"(hi) : "a"(a0), "a"(a1));
      d = f32x2{lo, hi};
    };
    // x-direction output transform of position row u (accumulators accr[u & 1]) and its term of the two y sums.  The reads are
    // pinned to the stage that calls this (volatile): left to itself the compiler puts each one right behind the MFMA that
    // finishes the accumulator, a stage earlier, and waits there for the result.
    auto transform_row = [&](int u, f32x2 (&o0)[2][2][2]) {
      asm volatile("s_nop 7\n\ts_nop 7");      // the last MFMA of accr[u & 1] is >= 11 wait states away (the compiler cannot count for us)
#pragma unroll
      for (int rp = 0; rp < 2; ++rp)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const f32x4(&m)[4][2] = accr[u & 1];
          f32x2 mm[4];
#pragma unroll
          for (int v = 0; v < 4; ++v) acc_read2(m[v][hf][2 * rp], m[v][hf][2 * rp + 1], mm[v]);
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const f32x2 z = e == 0 ? pk_add2(pk_add2(mm[0], mm[1]), mm[2]) : pk_sub2(pk_sub2(mm[1], mm[2]), mm[3]);
            if (u == 0) o0[rp][e][hf] = z;
            if (u == 1) { o0[rp][e][hf] = pk_add2(o0[rp][e][hf], z); o1[rp][e][hf] = z; }
            if (u == 2) { o0[rp][e][hf] = pk_add2(o0[rp][e][hf], z); o1[rp][e][hf] = pk_sub2(o1[rp][e][hf], z); }
            if (u == 3) o1[rp][e][hf] = pk_sub2(o1[rp][e][hf], z);
          }
        }
    };
    // output row oy leaves: ReLU / mask, store, sign words, the c1 weight gradient's MFMAs
    auto emit_row = [&](int oy, const f32x2 (&o)[2][2][2], const unsigned (&mw)[8], float (&pend)[16], int& yso) {
      yso = oy * pitch;
      const char* xa[2];
#pragma unroll
      for (int nh = 0; nh < 2; ++nh) {
        const char* in_ring = xring + ((oy + xky[nh]) & 3) * C4::SLOTB + xlane[nh];
        xa[nh] = (t16 + 16 * nh >= 27) ? smem + W2_XBASE + WPB * W2_XRINGB : in_ring;
      }
      unsigned keep[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) keep[i] = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          float ov[2];
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) {
            float v = o[r >> 1][e][hf][r & 1];
            if (EPI == EPI_BIAS_RELU_BITS) v = (v > 0.f) ? v : 0.f;      // one compare serves the ReLU and the sign ballot
            if (MASKED) v = __builtin_bit_cast(float, __builtin_bit_cast(int, v) & __builtin_amdgcn_sbfe((int)mw[2 * r + e], (unsigned)(t16 + 16 * hf), 1u));
            ov[hf] = v;
            pend[(2 * r + e) * 2 + hf] = v;      // stored from inside the MFMA block (store_pending)
          }
          if (W1) {
            const float b0 = *(const float*)(xa[0] + (2 * r + e) * 16), b1 = *(const float*)(xa[1] + (2 * r + e) * 16);
            wacc[0][0] = DD_MFMA16(ov[0], b0, wacc[0][0]);
            wacc[0][1] = DD_MFMA16(ov[0], b1, wacc[0][1]);
            wacc[1][0] = DD_MFMA16(ov[1], b0, wacc[1][0]);
            wacc[1][1] = DD_MFMA16(ov[1], b1, wacc[1][1]);
          }
          if (EPI == EPI_BIAS_RELU_BITS) {
            const unsigned long long b0 = __ballot(ov[0] > 0.f), b1 = __ballot(ov[1] > 0.f);
            const int G = (lane & 31) >> 3;
            keep[2 * r + e] = (unsigned)((b0 >> (16 * G)) & 0xffffull) | ((unsigned)((b1 >> (16 * G)) & 0xffffull) << 16);
          }
        }
      }
      if (EPI == EPI_BIAS_RELU_BITS) {
        const int P = lane & 31, sel = P & 7;
        unsigned word = keep[0];
#pragma unroll
        for (int i = 1; i < 8; ++i) word = (sel == i) ? keep[i] : word;
        __builtin_amdgcn_raw_buffer_store_b32(word, bors, boff, oy * pitchb, 0);
      }
    };

    // Output element (2r+e, hf) of this lane: pixel x0 + 8 q4 + 2r + e, channel t16 + 16 hf.  A 64-lane dword store costs the wave
    // ~16 issue cycles in the vector block and nothing behind an MFMA (the matrix pipe is busy for 32): the stores of a row are
    // issued one per MFMA.  (The compiler does not see them; it can only over-wait for its own loads because of that.)
    auto store_pending = [&](int i, const float (&pend)[16], int yso) {
      if (i & 1) asm volatile("buffer_store_dword %0, %1, %2, %3 offen offset:64 nt" : : "v"(pend[i]), "v"(pst[i >> 1]), "s"(yrs), "s"(yso) : "memory");
      else asm volatile("buffer_store_dword %0, %1, %2, %3 offen nt" : : "v"(pend[i]), "v"(pst[i >> 1]), "s"(yrs), "s"(yso) : "memory");
    };
    f32x4 R0[2][4], R1[2][4], R2[2][4], R3[2][4];      // x-stage results of four input rows
    f32x4 vq[4], uq[2][4][2];                          // V row of the current stage; U vectors of the current / next stage (AGPRs)
    unsigned m1w[8];                                   // sign words of output row 2tr+1 (loaded in stage 7, used in the next stage 1)
    f32x4 xpre[2][C4::NLOAD];
#pragma unroll
    for (int i = 0; i < 8; ++i) m1w[i] = 0;
    row_load(2 * r0 - 1, R0);
    row_load(2 * r0, R1);
    row_load(2 * r0 + 1, R2);
    row_load(2 * r0 + 2, R3);
    if (W1) {
#pragma unroll
      for (int d = 0; d < 2; ++d) {      // image rows 2 r0 - 1, 2 r0 into the ring; 2 r0 + 1, 2 r0 + 2 follow in the first pass
        f32x4 t4[C4::NLOAD];
        load_row<4, 1>(x4b, H, W, 2 * r0 - 1 + d, gx0, lane, t4);
        store_row<4, 1, false>(xring + ((2 * r0 + d) & 3) * C4::SLOTB, xspill, lane, t4);
      }
      load_row<4, 1>(x4b, H, W, 2 * r0 + 1, gx0, lane, xpre[0]);
      load_row<4, 1>(x4b, H, W, 2 * r0 + 2, gx0, lane, xpre[1]);
    }
    xstage(R0, R0);
    xstage(R1, R1);
    xstage(R2, R2);
    uread(0, 0, uq[0]);
    float pfv[4] = {0.f, 0.f, 0.f, 0.f};
    int oy_prev = H;      // nothing to emit in the first pass

    // One tile-row.  A0 .. A3 = the register rows holding input rows 2tr-1 .. 2tr+2; A0 is refilled with row 2tr+3 and A1 with
    // row 2tr+4 (the next tile-row's r = 2, 3).  mp = sign words of the previous tile-row's second output row, mn = this one's.
    auto step = [&](int tr, f32x4 (&A0)[2][4], f32x4 (&A1)[2][4], f32x4 (&A2)[2][4], f32x4 (&A3)[2][4]) {
      f32x2 o0[2][2][2];
      unsigned m0w[8];
      float pend[16];      // the outputs of a row between the vector block that forms them and their stores
      int yso;
#pragma unroll
      for (int st = 0; st < 8; ++st) {
        const int u = st >> 1, g = st & 1;
        __builtin_amdgcn_sched_barrier(0);
        ystage(u, g, A0, A1, A2, A3, vq);
        // ---- work for other stages / tile-rows ----
        if (st == 0) transform_row(3, o0);                       // the previous tile-row's last position row (o0 untouched)
        if (st == 1) {
          emit_row(oy_prev, o1, m1w, pend, yso);
          row_load(2 * tr + 3, A0);                              // A0 is dead: V(u = 0, g = 1) has just been formed
        }
        if (st == 2) {
          if (pf_rows) {
            pfacc += pfv[0] + pfv[1] + pfv[2] + pfv[3];      // the previous tile-row's (landed long ago; keeps them alive)
#pragma unroll
            for (int q = 0; q < 4; ++q) pfv[q] = dd_bload1(xrs, pfoff + (q & 1) * 64, (2 * (tr + pf_rows) + 3 + (q >> 1)) * pitch);
          }
          transform_row(0, o0);
          if (W1) {
            store_row<4, 1, false>(xring + ((2 * tr + 2) & 3) * C4::SLOTB, xspill, lane, xpre[0]);
            store_row<4, 1, false>(xring + ((2 * tr + 3) & 3) * C4::SLOTB, xspill, lane, xpre[1]);
          }
        }
        if (st == 3) {
          xstage(A3, A3);                                        // input row 2tr+2, in flight since the previous tile-row's stage 7
          if (W1) {
            load_row<4, 1>(x4b, H, W, 2 * tr + 3, gx0, lane, xpre[0]);
            load_row<4, 1>(x4b, H, W, 2 * tr + 4, gx0, lane, xpre[1]);
          }
        }
        if (st == 4) transform_row(1, o0);
        if (st == 5) {
          xstage(A0, A0);                                        // input row 2tr+3, in flight since stage 1
          if (MASKED) mask_load(2 * tr, m0w);
        }
        if (st == 6) transform_row(2, o0);
        if (st == 7) {
          emit_row(2 * tr, o0, m0w, pend, yso);
          if (MASKED) mask_load(2 * tr + 1, m1w);
          row_load(2 * tr + 4, A1);                              // A1 is dead: V(u = 3, g = 1) has just been formed
        }
        // ---- this stage's 32 MFMAs: back to back in a region of their own.  Every switch between vector and matrix
        // instructions costs the wave ~5 cycles on top of the instructions themselves (tools/ubench/mfma_issue.hip: 48.7
        // cycles per MFMA with two v_pk_add_f32 behind each, 43.5 with 64 behind 32) and with one wave per SIMD nothing
        // overlaps anyway; written as volatile asm because the scheduler interleaves whatever it is allowed to move.
        // (Operands: V was formed at the top of the stage, U has arrived by u_wait(), the accumulators are read a stage later.)
        __builtin_amdgcn_sched_barrier(0);
        u_wait(uq[st & 1]);
        const f32x4(&vv)[4] = vq;
        const f32x4(&uu)[4][2] = uq[st & 1];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
              f32x4& acc = accr[u & 1][v][hf];
              if (g == 0 && j == 0) {
                // the first MFMA of an accumulator takes a literal zero -- or, at position (1,1), the bias: A^T e11 A = all
                // ones, so a constant in M[1][1] reaches all four outputs of the tile once
                if (EPI == EPI_BIAS_RELU_BITS && u == 1 && v == 1)
                  asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %3" : "=a"(acc) : "v"(vv[v][j]), "a"(uu[v][hf][j]), "a"(hf ? bias1 : bias0));
                else
                  asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, 0" : "=a"(acc) : "v"(vv[v][j]), "a"(uu[v][hf][j]));
              } else {
                asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+a"(acc) : "v"(vv[v][j]), "a"(uu[v][hf][j]));
              }
              // behind the MFMA, for free: the next stage's U vectors (one read each behind the first eight), a row's stores
              const int i = (j * 4 + v) * 2 + hf;
              if (i < 8) uread1((st + 1) & 1, ((st + 1) & 7) >> 1, i >> 1, i & 1, uq[(st + 1) & 1][i >> 1][i & 1]);
              if (!W1 && (st == 1 || st == 7) && i >= 8 && i < 24) store_pending(i - 8, pend, yso);
            }
        __builtin_amdgcn_sched_barrier(0);
      }
      oy_prev = 2 * tr + 1;
    };

    int tr = r0;
    for (;;) {
      step(tr, R0, R1, R2, R3);
      if (++tr >= r1) break;
      step(tr, R2, R3, R0, R1);
      if (++tr >= r1) break;
    }
    {      // the column's last output row
      f32x2 unused[2][2][2];
      float pend[16];
      int yso;
      transform_row(3, unused);
      emit_row(oy_prev, o1, m1w, pend, yso);
      if (!W1)
#pragma unroll
        for (int q = 0; q < 16; ++q) store_pending(q, pend, yso);
    }
  }
  asm volatile("" : : "v"(pfacc));      // the prefetched words must not be optimised away
  if (W1) {
    const long gw = (long)blockIdx.x * WPB + wave;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
      for (int nh = 0; nh < 2; ++nh)
#pragma unroll
        for (int i = 0; i < 4; ++i) w1part[((gw * 2 + hf) * 2 + nh) * 256 + i * 64 + lane] = wacc[hf][nh][i];
  }
}

// Reduce of conv_wino2_fwd<EPI_RELU_BITS_W1>'s per-wave dW1 partials ([wave][half][column half][reg][lane]) in a fixed order and
// scatter to OIHW [32][3][3][3] + bias [32]: a block owns 8 elements, 32 thread groups share the waves.
__global__ __launch_bounds__(256) void conv_w1_reduce(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db,
                                                      int nw) {
  __shared__ float red[32][8];
  const int el = threadIdx.x & 7, g = threadIdx.x >> 3;
  const int e = blockIdx.x * 8 + el;      // < 1024
  float s0 = 0.f, s1 = 0.f;
  int w = g;
  for (; w + 32 < nw; w += 64) {
    s0 += part[(long)w * 1024 + e];
    s1 += part[(long)(w + 32) * 1024 + e];
  }
  if (w < nw) s0 += part[(long)w * 1024 + e];
  red[g][el] = s0 + s1;
  __syncthreads();
  if (g != 0) return;
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) v += red[i][el];
  const int l = e & 63, reg = (e >> 6) & 3, nh = (e >> 8) & 1, hf = e >> 9;
  const int co = 16 * hf + 4 * (l >> 4) + reg, col = 16 * nh + (l & 15);
  if (col < 27) {
    const int tap = col / 3, ci = col - 3 * tap;
    dw[(co * 3 + ci) * 9 + tap] = v;
  } else if (col == 27) {
    db[co] = v;
  }
}

// U image for conv_wino2_fwd: packed[((((4u+v)*2 + half)*2 + g)*64 + lane)*4 + j] = (G Weff G^T)[u][v] of
// Weff[co = (lane&15) + 16*half][ci = 8*(lane>>4) + 4g + j]; kind as conv_wino_pack_kernel.
__global__ void conv_wino2_pack_kernel(const float* __restrict__ w, float* __restrict__ p, int kind) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= WINO2_UFLOATS) return;
  const int j = idx & 3, lane = (idx >> 2) & 63, g = (idx >> 8) & 1, hf = (idx >> 9) & 1, pos = idx >> 10;
  const int u = pos >> 2, v = pos & 3;
  const int co = (lane & 15) + 16 * hf, ci = 8 * (lane >> 4) + 4 * g + j;
  float t[3][3];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
      t[ky][kx] = kind == 0 ? w[((long)co * 32 + ci) * 9 + ky * 3 + kx] : w[((long)ci * 32 + co) * 9 + (2 - ky) * 3 + (2 - kx)];
  float rowt[3];      // x-direction transform of each tap row
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    if (v == 0) rowt[ky] = t[ky][0];
    else if (v == 1) rowt[ky] = 0.5f * ((t[ky][0] + t[ky][1]) + t[ky][2]);
    else if (v == 2) rowt[ky] = 0.5f * ((t[ky][0] - t[ky][1]) + t[ky][2]);
    else rowt[ky] = t[ky][2];
  }
  float out;
  if (u == 0) out = rowt[0];
  else if (u == 1) out = 0.5f * ((rowt[0] + rowt[1]) + rowt[2]);
  else if (u == 2) out = 0.5f * ((rowt[0] - rowt[1]) + rowt[2]);
  else out = rowt[2];
  p[idx] = out;
}

// Weight gradient by the 2-D form F(3x3, 2x2): per 2x2 tile of dy and its 4x4 input patch
//   S[u][v] += (G g G^T)[u][v] (x) (B^T d B)[u][v],    dW = A^T S A   (A^T = [[1,1,1,0],[0,1,-1,0],[0,1,1,1]]),
// 16 accumulators of 32x32 over K = tiles: 128 MFMAs per 2 output rows x 32 pixels instead of 192 (1-D) or 288 (direct).
// A = transformed dy tile (lane = output channel, four 4-byte loads per tile straight from HBM), B = transformed patch
// (lane = input channel, sixteen ds_read_b32 per tile from a plain 4-slot ring), k-step = the tile pair (2s, 2s+1) on
// the two half-waves.  One wave per SIMD (256 accumulator registers): the operands of tile s+1 are transformed into
// their own registers while tile s's 16 MFMAs execute, its patch reads are issued a tile earlier still.
constexpr int W2W_STAGE4 = 65 * 64;      // float4s per staging area of the final in-LDS reduction (64 KB of sums + the bias row)
template <int WPB>
__global__ __launch_bounds__(WPB * 64) void conv_wino2_wgrad(const float* __restrict__ x, const float* __restrict__ dy,
                                                             float* __restrict__ part, float* __restrict__ bpart, int B,
                                                             int H, int W, int nstrips) {
  using C = StripCfg<32, 1>;
  constexpr int RINGB = 4 * C::SLOTB + C::SPILLB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  char* ring = smem + wave * RINGB;
  char* spill = ring + 4 * C::SLOTB;
  const int h = lane >> 5, n = lane & 31;
  const int gw = blockIdx.x * WPB + wave;
  const int HT = (H + 1) / 2;

  f32x16 acc[16];
#pragma unroll
  for (int p = 0; p < 16; ++p)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[p][r] = 0.f;
  float bsum = 0.f;

  long idx, end;
  dd_range((long)B * nstrips * HT, gw, gridDim.x * WPB, idx, end);
  while (idx < end) {
    const long col = idx / HT;
    const int r0 = (int)(idx - col * HT);
    const int r1 = (int)min((long)HT, r0 + (end - idx));
    idx += r1 - r0;
    const int b = (int)(col / nstrips), x0 = (int)(col % nstrips) * 32;
    const float* xb = x + (long)b * H * W * 32;
    const float* dyb = dy + (long)b * H * W * 32;
    const int gx0 = x0 - 1;
    const int aoff = ((x0 + 2 * h) * 32 + n) * 4;   // tile 2s+h = pixels x0 + 4s + 2h, +1: + 512 bytes per s, + 128 for the odd pixel
    // Descriptors: base = the image, the row in the scalar offset, num_records = the END of that row -- the range check adds the
    // scalar offset to the lane offset (tools/ubench/soffset_probe.hip), so a pixel right of the row is out of range and one
    // left of it (a negative lane offset) too.  One multiply, one add and one select per row instead of a 64-bit base + row *
    // pitch with its 16-bit split.
    const int pitch = W * 128;
    int roff[C::NLOAD];      // this lane's 16-byte chunks of a ring row (the idle lanes of the last group: out of range)
#pragma unroll
    for (int q = 0; q < C::NLOAD; ++q) {
      const int c = lane + 64 * q;
      roff[q] = (c < C::NCH) ? (gx0 + c / C::CHUNKS) * C::PXB + (c % C::CHUNKS) * 16 : -16;
    }
    auto row_loadq = [&](int iy, int q, f32x4& d) {      // chunk group q of input row iy
      const bool ok = (iy >= 0) && (iy < H);
      const int so = ok ? iy * pitch : 0;
      d = dd_bload4<DD_AUX_NT>(dd_rsrc(xb, ok ? so + pitch : 0), roff[q], so);
    };

#pragma unroll
    for (int d = 0; d < 4; ++d) {      // input rows 2*r0 - 1 .. 2*r0 + 2; slot of row iy = (iy + 1) & 3
      f32x4 t[C::NLOAD];
      const int iy = 2 * r0 - 1 + d;
#pragma unroll
      for (int q = 0; q < C::NLOAD; ++q) row_loadq(iy, q, t[q]);
      store_row<32, 1, false>(ring + ((iy + 1) & 3) * C::SLOTB, spill, lane, t);
    }
    // dy rows 2tr, 2tr+1 of the strip: g[a][e][s]
    auto load_dy1 = [&](int tr, int s8, f32x2 (&g)[2][8]) {      // g[e][s] = (row 2tr, row 2tr+1) of the tile's column e: tile s8's four
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int oy = 2 * tr + a;
        const bool ok = (tr < r1) && (oy < H);       // rows past the range belong to the next wave: read zeros
        const int so = ok ? oy * pitch : 0;
        const __amdgpu_buffer_rsrc_t as = dd_rsrc(dyb, ok ? so + pitch : 0);
        g[0][s8][a] = dd_bload1<DD_AUX_NT>(as, aoff + s8 * 512, so);
        g[1][s8][a] = dd_bload1<DD_AUX_NT>(as, aoff + s8 * 512 + 128, so);
      }
    };
    f32x2 ga[2][8], gb[2][8];      // dy of the current / next tile-row, alternating (no register moves)
#pragma unroll
    for (int s8 = 0; s8 < 8; ++s8) load_dy1(r0, s8, ga);

    auto step = [&](int tr, const f32x2 (&gc)[2][8], f32x2 (&gn)[2][8]) {
      f32x4 pre[2][C::NLOAD];

      const char* rb[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) rb[r] = ring + ((2 * tr + r) & 3) * C::SLOTB + n * 4;      // slot of input row 2*tr - 1 + r
      float dq[2][4][4];          // patches of tile s+1 / s+2 (reads in flight)
      float aq[2][16], bq[2][16];   // transformed operands of tile s / s+1
      auto rd = [&](int s8, float (&d)[4][4]) {
        const int poff = (2 * (2 * s8 + h)) * 128;      // ring pixel 2t of tile t = 2s + h
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) d[r][c] = *(const float*)(rb[r] + poff + c * 128);
      };
      auto tf = [&](int s8, const float (&d)[4][4], float (&av)[16], float (&bv)[16]) {
        // packed fp32 throughout (the vector ALUs are the matrix ALUs: every instruction here is matrix time lost).
        // x stage on register pairs (c0,c1) / (c2,c3) with a broadcast operand, y stage pairwise over c.
        f32x2 wl[4], wh[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const f32x2 lo = {d[r][0], d[r][1]}, hi = {d[r][2], d[r][3]};
          asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(wl[r]) : "v"(lo), "v"(hi));                // d0 - d2, d1 + d2
          asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(wh[r]) : "v"(hi), "v"(lo));  // d2 - d1, d3 - d1
        }
        const f32x2 bl[4] = {pk_sub2(wl[0], wl[2]), wl[1] + wl[2], pk_sub2(wl[2], wl[1]), pk_sub2(wl[3], wl[1])};
        const f32x2 bh[4] = {pk_sub2(wh[0], wh[2]), wh[1] + wh[2], pk_sub2(wh[2], wh[1]), pk_sub2(wh[3], wh[1])};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          bv[u * 4 + 0] = bl[u].x;
          bv[u * 4 + 1] = bl[u].y;
          bv[u * 4 + 2] = bh[u].x;
          bv[u * 4 + 3] = bh[u].y;
        }
        // dy tile (pairs over the tile's two rows), WITHOUT the halves of G = [[1,0],[.5,.5],[.5,-.5],[0,1]]: position
        // (u,v) carries the factor (1,2,2,1)[u] * (1,2,2,1)[v], taken out again (exactly) in conv_wino2_wgrad_reduce_b.
        const f32x2 g0 = gc[0][s8], g1 = gc[1][s8];
        const f32x2 gr[4] = {g0, g0 + g1, pk_sub2(g0, g1), g1};
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          f32x2 sd;      // (row0 + row1, row0 - row1)
          asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(sd) : "v"(gr[v]));
          av[0 * 4 + v] = gr[v].x;
          av[1 * 4 + v] = sd.x;
          av[2 * 4 + v] = sd.y;
          av[3 * 4 + v] = gr[v].y;
        }
        bsum += av[5];                              // (1,1) position = g00 + g01 + g10 + g11: the tile's bias contribution
      };
      rd(0, dq[0]);
      rd(1, dq[1]);
      tf(0, dq[0], aq[0], bq[0]);
      // Per tile: a block of vector work (the next tile's transform), then the 16 MFMAs with everything that is not a vector
      // instruction issued behind them -- the LDS reads of the tile after next, this tile-row's share of the global loads for the
      // next one, the ring writes.  A memory instruction costs the wave 8-40 issue cycles inside the vector block and nothing
      // behind an MFMA (64 cycles of matrix pipe each; tools/ubench/mfma_issue.hip), and every switch between vector and matrix
      // instructions costs ~5 more.
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8) {
        __builtin_amdgcn_sched_barrier(0);
        if (s8 + 1 < 8) tf(s8 + 1, dq[(s8 + 1) & 1], aq[(s8 + 1) & 1], bq[(s8 + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        if (s8 + 2 < 8) rd(s8 + 2, dq[s8 & 1]);                      // dq[s8&1] held tile s8: already transformed
        load_dy1(tr + 1, s8, gn);
#pragma unroll
        for (int q = 2 * s8; q < 2 * s8 + 2; ++q)      // the ring rows of the next tile-row: out by tile 2, written to LDS in tiles 6 and 7
          if (q < C::NLOAD) {
            row_loadq(2 * tr + 3, q, pre[0][q]);
            row_loadq(2 * tr + 4, q, pre[1][q]);
          }
        if (s8 == 6) store_row<32, 1, false>(ring + ((2 * tr + 4) & 3) * C::SLOTB, spill, lane, pre[0]);      // every patch read of this
        if (s8 == 7) store_row<32, 1, false>(ring + ((2 * tr + 5) & 3) * C::SLOTB, spill, lane, pre[1]);      // tile-row is out (tile 7's: s8 = 5)
#pragma unroll
        for (int p = 0; p < 16; ++p) acc[p] = DD_MFMA(aq[s8 & 1][p], bq[s8 & 1][p], acc[p]);
#pragma unroll
        for (int p = 0; p < 16; ++p) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // MFMA
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // DS read
          __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);      // VMEM read
          __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);      // DS write
          __builtin_amdgcn_sched_group_barrier(0x004, 2, 0);      // SALU
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    int tr = r0;
    do {      // pairs of tile-rows; a trailing odd one sees zero dy (no contribution)
      step(tr, ga, gb);
      step(tr + 1, gb, ga);
      tr += 2;
    } while (tr < r1);
  }

  // The workgroup's four partials are added in LDS, ((w0 + w1) + (w2 + w3)), before anything goes to HBM: 16 MB of
  // partials instead of 67 (the reduce kernel reads them beside the overlapped optimizer pass, at a fraction of the
  // HBM rate).  Two 65 KB staging areas over the rings, which nobody reads any more.  The accumulators only ever flow OUT of
  // their registers: waves 1 and 3 store theirs, waves 0 and 2 add theirs on top with LDS float adds (one contributor per
  // address and phase: w1 + w0 is the same number whoever arrives first, so the result stays bit-reproducible), then all 256
  // threads add the two areas and write the block's partial.  (Reading partial sums back INTO the 256 accumulators under
  // wave-uniform branches, as this epilogue first did, made the register allocator spill 48 registers to scratch.)
  static_assert(WPB == 4, "conv_wino2_wgrad: the in-LDS reduction is written for four waves");
  const int lane_e = dd_fresh_lane();                          // the epilogue's own: no lane-derived register crosses the tile loop
  float* stage = (float*)((f32x4*)smem + (wave >> 1) * W2W_STAGE4 + lane_e);      // [chunk = 4p + r/4][lane] float4, + one row for the bias sums
  __syncthreads();
  if (wave & 1) {
#pragma unroll
    for (int p = 0; p < 16; ++p)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        *(f32x4*)(stage + (4 * p + c) * 256) = f32x4{acc[p][4 * c], acc[p][4 * c + 1], acc[p][4 * c + 2], acc[p][4 * c + 3]};
    *(f32x4*)(stage + 64 * 256) = f32x4{bsum, 0.f, 0.f, 0.f};
  }
  __syncthreads();
  if (!(wave & 1)) {
#pragma unroll
    for (int p = 0; p < 16; ++p)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        __hip_atomic_fetch_add(stage + (4 * p + (r >> 2)) * 256 + (r & 3), acc[p][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(stage + 64 * 256, bsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  {
    const f32x4* sa = (const f32x4*)smem;
    const f32x4* sb = sa + W2W_STAGE4;
    const int tid_e = lane_e + 64 * wave;
    float* out = part + (long)blockIdx.x * 256 * 64;
    for (int i = tid_e; i < 64 * 64; i += WPB * 64) {      // float4 i = chunk * 64 + lane holds rows 4 chunk .. + 3 of lane's column
      const f32x4 a = sa[i], b = sb[i];
      const int chunk = i >> 6, ln = i & 63;
#pragma unroll
      for (int k = 0; k < 4; ++k) out[(chunk * 4 + k) * 64 + ln] = a[k] + b[k];
    }
    if (tid_e < 64) bpart[(long)blockIdx.x * 64 + tid_e] = sa[64 * 64 + tid_e].x + sb[64 * 64 + tid_e].x;
  }
}

// Second stage of conv_wino2_wgrad, in two launches (one block per accumulator row would leave 17 blocks to read 64 MB):
//  a) 256 blocks = (position p, chunk c of the waves): fixed-order sum over the chunk's partials.  A wave's partial of
//     one position is 16 rows x 64 lanes = 4 KB contiguous, read as 256 float4 (the first version read one 256-byte
//     row per wave, 64 KB apart: 0.57 TB/s) -> tsum[c][p][r][64]
//  b) one block per register row r (+ one for the bias): sum of the 16 chunks, output transform A^T S A, scatter to OIHW.
constexpr int W2R_CHUNKS = 16;
// 256-thread blocks (and 64-thread ones in reduce_b): these run on a side stream beside resident kernels that hold most wave
// slots of every CU -- a 1024-thread block then waits for a whole CU's worth of them (measured: 1.3 ms in the queue).
__global__ __launch_bounds__(256) void conv_wino2_wgrad_reduce_a(const float* __restrict__ part, float* __restrict__ tsum, int nw) {
  const int f = threadIdx.x;
  const int p = blockIdx.x & 15, c = blockIdx.x >> 4;
  const int per = (nw + W2R_CHUNKS - 1) / W2R_CHUNKS;
  const int w0 = c * per, w1 = min(nw, w0 + per);
  const f32x4* src = (const f32x4*)part + (long)p * 256 + f;
  f32x4 s[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  int w = w0;
  for (; w + 3 < w1; w += 4) {
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] += src[(long)(w + i) * 4096];
  }
  for (int i = 0; w < w1; ++w, ++i) s[i] += src[(long)w * 4096];
  ((f32x4*)tsum)[((long)c * 16 + p) * 256 + f] = (s[0] + s[1]) + (s[2] + s[3]);
}

// The output transform runs as running sums with coefficients 0 / +-1 in the order of the closed forms ((t0 + t1) + t2, t1 - t2,
// (t1 + t2) + t3), one column v at a time.  (Rounds 3-4 kept this kernel at 40 registers with every loop rolled so that it fitted beside
// the c2 data gradient's 464; that kernel now holds 475 and nothing fits beside it, and since round 5 the weight gradient this launch
// reduces is the LAST conv kernel of the step, so the launch is the step's tail: its loads are batched per column instead.)
__global__ __launch_bounds__(64) void conv_wino2_wgrad_reduce_b(const float* __restrict__ tsum, const float* __restrict__ bpart,
                                                                float* __restrict__ dw, float* __restrict__ db, int nw) {
  const int l = threadIdx.x;
  const int r = blockIdx.x;   // accumulator register row, or 16 for the bias
  if (r == 16) {
    // s[i] = the partials w = i, i + 4, ... in order, as the four-way loop this replaces -- with 64 loads in flight instead of 4 (the
    // bias block was the long pole of the launch: nw / 4 dependent round trips, 34 us at the tail of the step)
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    const int full = nw & ~3;
#pragma unroll
    for (int i = 0; i < 4; ++i) dd_sum_strided(s[i], bpart + (long)i * 64 + l, 256, full / 4);
    for (int w = full, i = 0; w < nw; ++w, ++i) s[i] += bpart[(long)w * 64 + l];
    const float t = (s[0] + s[1]) + (s[2] + s[3]);
    const float other = __shfl_xor(t, 32);
    if (l < 32) db[l] = t + other;
    return;
  }
  float out[3][3];
#pragma unroll
  for (int a = 0; a < 9; ++a) out[a / 3][a % 3] = 0.f;
#pragma unroll 1
  for (int v = 0; v < 4; ++v) {
    float z[3] = {0.f, 0.f, 0.f};      // z[ky] = A^T[ky][u] t[u][v]
    // the 4 x 16 chunk sums of this column are requested together (one memory round trip per column instead of four); each t[u] is still
    // the sum of its 16 chunks in chunk order
    float tv[4][W2R_CHUNKS];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int c = 0; c < W2R_CHUNKS; ++c) tv[u][c] = tsum[(((long)c * 16 + (u * 4 + v)) * 16 + r) * 64 + l];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float t = 0.f;
#pragma unroll
      for (int c = 0; c < W2R_CHUNKS; ++c) t += tv[u][c];
      // the halves of G left out of conv_wino2_wgrad's dy transform (powers of two: exact)
      t = t * ((u == 1 || u == 2) ? 0.5f : 1.f) * ((v == 1 || v == 2) ? 0.5f : 1.f);
      z[0] += (u < 3 ? 1.f : 0.f) * t;
      z[1] += (u == 1 ? 1.f : u == 2 ? -1.f : 0.f) * t;
      z[2] += (u > 0 ? 1.f : 0.f) * t;
    }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {      // dW[ky][kx] = z[ky][v] A[v][kx]
      out[ky][0] += (v < 3 ? 1.f : 0.f) * z[ky];
      out[ky][1] += (v == 1 ? 1.f : v == 2 ? -1.f : 0.f) * z[ky];
      out[ky][2] += (v > 0 ? 1.f : 0.f) * z[ky];
    }
  }
  const int o = dd_acc_row(r, l), jj = l & 31;
  float* dst = dw + ((long)o * 32 + jj) * 9;
#pragma unroll
  for (int a = 0; a < 9; ++a) dst[a] = out[a / 3][a % 3];
}

// The kernels here address a whole image through one buffer descriptor, the row in the scalar offset; 2^30 stands for "outside" (FAR)
int require_30bit_image(const dd_conv_desc* d, const char* who) {
  DD_REQUIRE((long)d->height * d->width * 128 < (1L << 30), DD_ERR_UNSUPPORTED, "%s: image of %d x %d pixels: the kernel addresses an image with 30-bit offsets",
             who, d->height, d->width);
  return 0;
}

template <int EPI>
int launch_wino2(const float* x, const float* up, const float* bias, const unsigned* bits_in, float* y, unsigned* bits_out,
                 const dd_conv_desc* d, hipStream_t st, const float* x4 = nullptr, float* w1part = nullptr, int* nw_out = nullptr) {
  using C = StripCfg<32, 1>;
  using C4 = StripCfg<4, 1>;
  constexpr int WPB = 4;
  const int nstrips = (d->width + 31) / 32;
  // Register-row kernels by default.  DD_WINO2_RING=1: the LDS-ring form everywhere, DD_WINO2_RING_W1=1: for the fused data
  // gradient only (A/B; DESIGN.md 3.1c: beside the optimizer pass the choice depends on how that pass is launched -- adam_stream_grid, csrc/dd_adam.h).
  static const bool ring_env = getenv("DD_WINO2_RING") != nullptr;
  static const bool ring_w1 = getenv("DD_WINO2_RING_W1") != nullptr;
  const bool ring = ring_env || (EPI == EPI_RELU_BITS_W1 && ring_w1);
  if (int rc = require_30bit_image(d, "conv_wino2")) return rc;
  const size_t lds = (size_t)WINO2_UFLOATS * 4 + (ring ? (size_t)WPB * (4 * C::SLOTB + C::SPILLB) : 0) +
                     (EPI == EPI_RELU_BITS_W1 ? (size_t)WPB * (4 * C4::SLOTB + C4::SPILLB) + 128 : 0);
  const int grid = resident_grid(d, (long)d->batch * nstrips * ((d->height + 1) / 2), WPB, 1);
  if (nw_out) *nw_out = grid * WPB;
  if (int rc = dd_allow_lds(ring ? (const void*)conv_wino2_fwd<EPI, WPB> : (const void*)conv_wino2r_fwd<EPI, WPB>, lds)) return rc;
  // rows of the next tile-row are pulled into L2 a tile-row ahead (in the step: forward 1.195 -> 1.163 ms against no prefetch)
  constexpr int pf_rows = 1;
  auto kring = conv_wino2_fwd<EPI, WPB>;
  auto kreg = conv_wino2r_fwd<EPI, WPB>;
  if (ring) hipLaunchKernelGGL(kring, dim3(grid), dim3(WPB * 64), lds, st, x, up, bias, bits_in, y, bits_out, d->batch, d->height, d->width, nstrips, x4, w1part);
  else hipLaunchKernelGGL(kreg, dim3(grid), dim3(WPB * 64), lds, st, x, up, bias, bits_in, y, bits_out, d->batch, d->height, d->width, nstrips, x4, w1part, pf_rows);
  DD_LAUNCH_CHECK("conv_wino2_fwd");
  return 0;
}

int wino2_wgrad_grid(const dd_conv_desc* d) {
  return resident_grid(d, (long)d->batch * ((d->width + 31) / 32) * ((d->height + 1) / 2), 4, 1);
}

// Workspace of the weight gradient: `grid` partials of 16 accumulators (one per WORKGROUP: its four waves are added in LDS), their
// bias rows, then conv_wino2_wgrad_reduce_a's chunk sums.  bytes() holds 4 * DD_NUM_CU partials, four times the largest grid.
struct Wino2WgradWs {
  static constexpr int64_t PART = 16 * 1024, BPART = 64, TSUM = W2R_CHUNKS * 16 * 1024;      // floats
  float *part, *bpart, *tsum;
  Wino2WgradWs(void* workspace, int grid) : part((float*)workspace), bpart(part + grid * PART), tsum(bpart + grid * BPART) {}
  static int64_t bytes() { return ((int64_t)4 * DD_NUM_CU * (PART + BPART) + TSUM) * 4; }
};

}  // namespace

extern "C" {

int64_t dd_conv_wino2_packed_floats(const dd_conv_desc* d) {
  return is_c2(d) ? WINO2_UFLOATS : -1;
}

int dd_conv_wino2_pack(const float* w_oihw, float* packed, const dd_conv_desc* d, int32_t kind, void* stream) {
  if (int rc = require_c2(d, w_oihw && packed, "conv_wino2_pack")) return rc;
  DD_REQUIRE(kind == 0 || kind == 1, DD_ERR_BAD_ARG, "conv_wino2_pack: kind %d (0 forward, 1 data gradient)", kind);
  hipLaunchKernelGGL(conv_wino2_pack_kernel, dim3((WINO2_UFLOATS + 255) / 256), dim3(256), 0, (hipStream_t)stream, w_oihw, packed, kind);
  DD_LAUNCH_CHECK("conv_wino2_pack");
  return 0;
}

int dd_conv_wino2_fwd_relu_bits(const float* x, const float* packed, const float* bias, float* y, uint32_t* relu_bits,
                                const dd_conv_desc* d, void* stream) {
  if (int rc = require_c2(d, x && packed && bias && y && relu_bits, "conv_wino2_fwd_relu_bits")) return rc;
  return launch_wino2<EPI_BIAS_RELU_BITS>(x, packed, bias, nullptr, y, relu_bits, d, (hipStream_t)stream);
}

int dd_conv_wino2_dgrad_relu_bits(const float* dy, const float* packed, const uint32_t* relu_bits, float* dx,
                                  const dd_conv_desc* d, void* stream) {
  if (int rc = require_c2(d, dy && packed && relu_bits && dx, "conv_wino2_dgrad_relu_bits")) return rc;
  return launch_wino2<EPI_RELU_BITS>(dy, packed, nullptr, relu_bits, dx, nullptr, d, (hipStream_t)stream);
}

int64_t dd_conv_wino2_dgrad_w1_workspace_bytes(const dd_conv_desc* d) {
  return is_c2(d) ? (int64_t)4 * DD_NUM_CU * 1024 * 4 : -1;      // one 32 x 32 partial per wave
}

int dd_conv_wino2_dgrad_w1(const float* dy, const float* packed, const uint32_t* relu_bits, const float* x_nhwc4, float* dw1_oihw,
                           float* dbias1, void* workspace, int64_t workspace_bytes, const dd_conv_desc* d, void* stream) {
  if (int rc = require_c2(d, dy && packed && relu_bits && x_nhwc4 && dw1_oihw && dbias1 && workspace, "conv_wino2_dgrad_w1")) return rc;
  DD_REQUIRE(workspace_bytes >= dd_conv_wino2_dgrad_w1_workspace_bytes(d), DD_ERR_WORKSPACE, "conv_wino2_dgrad_w1: workspace %ld < %ld bytes",
             (long)workspace_bytes, (long)dd_conv_wino2_dgrad_w1_workspace_bytes(d));
  int nw = 0;
  if (int rc = launch_wino2<EPI_RELU_BITS_W1>(dy, packed, nullptr, relu_bits, nullptr, nullptr, d, (hipStream_t)stream, x_nhwc4,
                                              (float*)workspace, &nw))
    return rc;
  hipLaunchKernelGGL(conv_w1_reduce, dim3(128), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, dw1_oihw, dbias1, nw);
  DD_LAUNCH_CHECK("conv_w1_reduce");
  return 0;
}

int64_t dd_conv_wino2_wgrad_workspace_bytes(const dd_conv_desc* d) {
  return is_c2(d) ? Wino2WgradWs::bytes() : -1;
}

int dd_conv_wino2_wgrad_partials(const float* x, const float* dy, void* workspace, int64_t workspace_bytes, const dd_conv_desc* d,
                                 void* stream) {
  if (int rc = require_c2(d, x && dy && workspace, "conv_wino2_wgrad")) return rc;
  DD_REQUIRE(workspace_bytes >= Wino2WgradWs::bytes(), DD_ERR_WORKSPACE, "conv_wino2_wgrad: workspace %ld < %ld bytes",
             (long)workspace_bytes, (long)Wino2WgradWs::bytes());
  if (int rc = require_30bit_image(d, "conv_wino2_wgrad")) return rc;
  constexpr int WPB = 4;
  const int nstrips = (d->width + 31) / 32;
  const int grid = wino2_wgrad_grid(d);
  const Wino2WgradWs ws(workspace, grid);
  auto k = conv_wino2_wgrad<WPB>;
  const size_t lds = max((size_t)WPB * (4 * StripCfg<32, 1>::SLOTB + StripCfg<32, 1>::SPILLB), (size_t)2 * W2W_STAGE4 * 16);
  if (int rc = dd_allow_lds((const void*)k, lds)) return rc;
  hipLaunchKernelGGL(k, dim3(grid), dim3(WPB * 64), lds, (hipStream_t)stream, x, dy, ws.part, ws.bpart, d->batch, d->height, d->width, nstrips);
  DD_LAUNCH_CHECK("conv_wino2_wgrad");
  return 0;
}

int dd_conv_wino2_wgrad_finish(void* workspace, int64_t workspace_bytes, float* dw_oihw, float* dbias, const dd_conv_desc* d,
                               void* stream) {
  if (int rc = require_c2(d, workspace && dw_oihw && dbias, "conv_wino2_wgrad_finish")) return rc;
  DD_REQUIRE(workspace_bytes >= Wino2WgradWs::bytes(), DD_ERR_WORKSPACE, "conv_wino2_wgrad_finish: workspace %ld < %ld bytes",
             (long)workspace_bytes, (long)Wino2WgradWs::bytes());
  hipStream_t st = (hipStream_t)stream;
  const int nw = wino2_wgrad_grid(d);
  const Wino2WgradWs ws(workspace, nw);
  hipLaunchKernelGGL(conv_wino2_wgrad_reduce_a, dim3(256), dim3(256), 0, st, ws.part, ws.tsum, nw);
  DD_LAUNCH_CHECK("conv_wino2_wgrad_reduce_a");
  hipLaunchKernelGGL(conv_wino2_wgrad_reduce_b, dim3(17), dim3(64), 0, st, ws.tsum, ws.bpart, dw_oihw, dbias, nw);
  DD_LAUNCH_CHECK("conv_wino2_wgrad_reduce_b");
  return 0;
}

int dd_conv_wino2_wgrad(const float* x, const float* dy, float* dw_oihw, float* dbias, void* workspace, int64_t workspace_bytes,
                        const dd_conv_desc* d, void* stream) {
  DD_REQUIRE(dw_oihw && dbias, DD_ERR_BAD_ARG, "conv_wino2_wgrad: NULL pointer");
  if (int rc = dd_conv_wino2_wgrad_partials(x, dy, workspace, workspace_bytes, d, stream)) return rc;
  return dd_conv_wino2_wgrad_finish(workspace, workspace_bytes, dw_oihw, dbias, d, stream);
}

}  // extern "C"

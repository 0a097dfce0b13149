// SUPERSEDED by conv_wino2.inc (like it, included at the end of conv3x3.hip): reached only through ops.WINOGRAD_2D = False, and pinned by the tests.
// Winograd F(2,3) along x for the 32 -> 32 stride-1 layer (c2 forward and its data gradient): two adjacent output
// pixels share four transformed inputs, so a 3-tap row costs 4 multiplies instead of 6 -- 192 instead of 288
// matrix-core cycles per pixel pair, in exact fp32 arithmetic (the transforms are adds and one halving):
//   inputs   d0..d3 (pixels 2t-1 .. 2t+2)      v = (d0-d2, d1+d2, d2-d1, d1-d3)
//   weights  g0..g2 (kx = 0..2, per ky)        u = (g0, (g0+g1+g2)/2, (g0-g1+g2)/2, g2)
//   outputs  y(2t) = m0+m1+m2,  y(2t+1) = m1-m2-m3     with m_p = sum over ky, ci of v_p * u_p
// A wave still owns 32 output pixels = 16 pairs; the GEMM tile is 16 (pairs) x 16 (channels) x 4 (input channels) on
// v_mfma_f32_16x16x4_f32 (same flop rate as the 32x32x2 form), 4 positions x 2 channel halves = 8 accumulators of
// 4 registers, issued round-robin (the 16x16 form has a 40-cycle dependent latency on a 32-cycle issue).  Lane
// (pair t = lane&15, q = lane>>4) transforms input channels 8q..8q+7 of its own pair in registers, so the A operand
// never goes back to LDS; U (48 KB) sits in LDS next to the eight 3-slot rings (13.5 KB each): 159.7 of 160 KB.
// Rest of the machinery (ring, prefetch, ranges, buffer addressing) is conv_strip_fwd's (conv3x3.hip; the ring: dd_conv_strip.h).
namespace {

constexpr int WINO_UFLOATS = 3 * 4 * 2 * 2 * 64 * 4;      // [ky][pos][half][chunk][lane][4]

template <int EPI, int WPB>   // EPI_BIAS_RELU_BITS (forward) or EPI_RELU_BITS (data gradient)
__global__ __launch_bounds__(WPB * 64) void conv_wino_fwd(const float* __restrict__ x, const float* __restrict__ up,
                                                          const float* __restrict__ bias, const unsigned* __restrict__ bits_in,
                                                          float* __restrict__ y, unsigned* __restrict__ bits_out, int B, int H,
                                                          int W, int nstrips) {
  using C = StripCfg<32, 1>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  {
    f32x4* ul4 = (f32x4*)smem;
    const f32x4* ug4 = (const f32x4*)up;
    for (int i = tid; i < WINO_UFLOATS / 4; i += WPB * 64) ul4[i] = ug4[i];
  }
  __syncthreads();
  char* ring = smem + WINO_UFLOATS * 4 + wave * C::WAVEB;
  char* spill = ring + 3 * C::SLOTB;
  const f32x4* ul = (const f32x4*)smem;
  const int t16 = lane & 15, q4 = lane >> 4;
  const float bv0 = (EPI == EPI_BIAS_RELU_BITS) ? bias[t16] : 0.f, bv1 = (EPI == EPI_BIAS_RELU_BITS) ? bias[16 + t16] : 0.f;

  long idx, end;
  dd_range((long)B * nstrips * H, blockIdx.x * WPB + wave, gridDim.x * WPB, idx, end);
  while (idx < end) {
    const long col = idx / H;
    const int y0 = (int)(idx - col * H);
    const int y1 = (int)min((long)H, y0 + (end - idx));
    idx += y1 - y0;
    const int b = (int)(col / nstrips), x0 = (int)(col % nstrips) * 32;
    const float* xb = x + (long)b * H * W * 32;
    const int gx0 = x0 - 1;

#pragma unroll
    for (int d = 0; d < 3; ++d) {
      f32x4 t[C::NLOAD];
      const int iy = y0 - 1 + d;
      load_row<32, 1>(xb, H, W, iy, gx0, lane, t);
      store_row<32, 1, true>(ring + ((iy + 1) % 3) * C::SLOTB, spill, lane, t);
    }

    for (int yy = y0; yy < y1; ++yy) {
      f32x4 pre[C::NLOAD];
      load_row<32, 1>(xb, H, W, yy + 2, gx0, lane, pre);
      const long opix = (long)(b * H + yy) * W;
      unsigned mw[8];
      if (EPI == EPI_RELU_BITS) {   // sign words of this lane's 8 output pixels: pairs 4q..4q+3 = pixels x0 + 8q .. +7
        const __amdgpu_buffer_rsrc_t ms = dd_rsrc(bits_in + opix, W * 4);
#pragma unroll
        for (int i = 0; i < 8; ++i)   // one dword each: every word is range-checked by itself at a ragged row end
          mw[i] = __builtin_amdgcn_raw_buffer_load_b32(ms, (x0 + 8 * q4 + i) * 4, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);

      f32x4 acc[4][2];
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) acc[p][hf] = f32x4{0.f, 0.f, 0.f, 0.f};

      // 6 groups (tap row ky, channel quad g) of 12 reads (4 input pixels + 8 U vectors) + 32 MFMAs; the reads of the
      // next group are issued before the MFMAs of the current one
      f32x4 dbuf[2][4], ubuf[2][4][2];
      auto rd = [&](int it, f32x4 (&d)[4], f32x4 (&u)[4][2]) {
        const int ky = it >> 1, g = it & 1;
        const char* rowb = ring + ((yy + ky) % 3) * C::SLOTB;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int px = 2 * t16 + c;
          d[c] = *(const f32x4*)(rowb + px * 128 + (((2 * q4 + g) ^ swz<32>(px)) << 4));
        }
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) u[p][hf] = ul[((((ky * 4 + p) * 2 + hf) * 2 + g) * 64) + lane];
      };
      // the input transform of a group runs while the PREVIOUS group's MFMAs execute and lands in its own registers: an
      // MFMA never waits for a VALU result, a VALU write never waits for an MFMA that has not read its operand yet
      f32x4 vbuf[2][4];
      auto tf = [&](const f32x4 (&d)[4], f32x4 (&v)[4]) {
        v[0] = pk_sub4(d[0], d[2]);
        v[1] = pk_add4(d[1], d[2]);
        v[2] = pk_sub4(d[2], d[1]);
        v[3] = pk_sub4(d[1], d[3]);
      };
      rd(0, dbuf[0], ubuf[0]);
      tf(dbuf[0], vbuf[0]);
#pragma unroll
      for (int it = 0; it < 6; ++it) {
        if (it + 1 < 6) {
          rd(it + 1, dbuf[(it + 1) & 1], ubuf[(it + 1) & 1]);
          tf(dbuf[(it + 1) & 1], vbuf[(it + 1) & 1]);
        }
        __builtin_amdgcn_sched_barrier(0);
        const f32x4(&u)[4][2] = ubuf[it & 1];
        const f32x4(&v)[4] = vbuf[it & 1];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) acc[p][hf] = DD_MFMA16(v[p][j], u[p][hf][j], acc[p][hf]);
        __builtin_amdgcn_sched_barrier(0);
      }

      store_row<32, 1, true>(ring + ((yy + 3) % 3) * C::SLOTB, spill, lane, pre);

      // output transform + epilogue: lane = channel t16 (+16 per half), register r = pair 4q + r
      const __amdgpu_buffer_rsrc_t ys = dd_rsrc(y + opix * 32, W * 128);
      unsigned keep[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) keep[i] = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {          // the pair's even / odd pixel
          const int opx = x0 + 2 * (4 * q4 + r) + e;
          float o[2];
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) {
            const float m0 = acc[0][hf][r], m1 = acc[1][hf][r], m2 = acc[2][hf][r], m3 = acc[3][hf][r];
            float v = e == 0 ? (m0 + m1) + m2 : (m1 - m2) - m3;
            if (EPI == EPI_BIAS_RELU_BITS) v = fmaxf(v + (hf ? bv1 : bv0), 0.f);
            if (EPI == EPI_RELU_BITS) {
              v = ((mw[2 * r + e] >> (t16 + 16 * hf)) & 1u) ? v : 0.f;
            }
            o[hf] = v;
            dd_bstore1<DD_AUX_NT>(ys, (opx * 32 + t16 + 16 * hf) * 4, v);
          }
          if (EPI == EPI_BIAS_RELU_BITS) {
            // ballot bit L = (o > 0) of lane L = (channel L&15, pair group L>>4): 16 channel bits of 4 different pixels
            const unsigned long long b0 = __ballot(o[0] > 0.f), b1 = __ballot(o[1] > 0.f);
            // lane P (< 32) keeps the word of strip pixel P = 2*(4G + r) + e
            const int G = (lane & 31) >> 3;
            const unsigned w = (unsigned)((b0 >> (16 * G)) & 0xffffull) | ((unsigned)((b1 >> (16 * G)) & 0xffffull) << 16);
            keep[2 * r + e] = w;
          }
        }
      }
      if (EPI == EPI_BIAS_RELU_BITS) {
        const int P = lane & 31, sel = P & 7;          // P = 8G + 2r + e  ->  keep index 2r + e = P & 7
        unsigned word = keep[0];
#pragma unroll
        for (int i = 1; i < 8; ++i) word = (sel == i) ? keep[i] : word;
        const __amdgpu_buffer_rsrc_t bs = dd_rsrc(bits_out + opix, W * 4);
        __builtin_amdgcn_raw_buffer_store_b32(word, bs, (lane < 32) ? (x0 + P) * 4 : -16, 0, 0);
      }
    }
  }
}

// Weight gradient of the same layer by F(3,2) along x (the transpose of the algorithm above): per tile of two
// adjacent output pixels the three taps' products  dW_k += g_j * x_{j+k}  (j = 0,1; k = 0..2) are
//   dW_k = A^T[k][:] . ( (G g) * (B^T d) ),   G g = (g0, (g0+g1)/2, (g0-g1)/2, g1),   B^T d = (d0-d2, d1+d2, d2-d1, d3-d1)
// and the sum over tiles commutes with A^T, so the kernel keeps 3 (ky) x 4 (position) accumulators S_p of 32 x 32
// over K = tiles -- 96 instead of 144 MFMAs per 32 pixels -- and the reduce kernel applies
//   dW_0 = S0+S1+S2,  dW_1 = S1-S2,  dW_2 = S1+S2+S3     once at the end.
// GEMM view as in conv_wgrad: A = G g (lane = output channel, straight from HBM), B = B^T d (lane = input channel,
// four ds_read_b32 per tile and tap row), k-step = the tile pair (2s, 2s+1) on the two half-waves.
template <int WPB>
__global__ __launch_bounds__(WPB * 64) void conv_wino_wgrad(const float* __restrict__ x, const float* __restrict__ dy,
                                                            float* __restrict__ part, float* __restrict__ bpart, int B,
                                                            int H, int W, int nstrips) {
  using C = StripCfg<32, 1>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  char* ring = smem + wave * C::WAVEB;
  char* spill = ring + 3 * C::SLOTB;
  const int h = lane >> 5, n = lane & 31;
  const int gw = blockIdx.x * WPB + wave;

  f32x16 acc[3][4];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ky][p][r] = 0.f;
  float bsum = 0.f;

  long idx, end;
  dd_range((long)B * nstrips * H, gw, gridDim.x * WPB, idx, end);
  while (idx < end) {
    const long col = idx / H;
    const int y0 = (int)(idx - col * H);
    const int y1 = (int)min((long)H, y0 + (end - idx));
    idx += y1 - y0;
    const int b = (int)(col / nstrips), x0 = (int)(col % nstrips) * 32;
    const float* xb = x + (long)b * H * W * 32;
    const float* dyb = dy + (long)b * H * W * 32;
    const int gx0 = x0 - 1;
    const int aoff = ((x0 + 2 * h) * 32 + n) * 4;   // tile 2s+h = pixels x0 + 4s + 2h, +1: + 512 bytes per s, + 128 for the odd pixel

#pragma unroll
    for (int d = 0; d < 3; ++d) {
      f32x4 t[C::NLOAD];
      const int iy = y0 - 1 + d;
      load_row<32, 1>(xb, H, W, iy, gx0, lane, t);
      store_row<32, 1, false>(ring + ((iy + 1) % 3) * C::SLOTB, spill, lane, t);
    }
    // One wave per SIMD: whatever is not an MFMA must slip into the shadow of one, or the pipe idles.  So the row step
    //  * keeps THREE rotating register groups (dy in use / rows arriving / rows just requested): no register moves;
    //  * runs the 24 (tap row, tile pair) groups tap-row-major, so the ring slot of the oldest input row is free after
    //    the first 8 groups and the arriving row is written into it in the middle of the MFMA stream;
    //  * issues the next group's 21 loads one per MFMA group instead of in a burst at the row boundary.
    // group(t) = input row t+2 and dy row t+1, i.e. what output row t+1 adds.
    struct Group {
      f32x4 xrow[C::NLOAD];
      float d0[8], d1[8];
    };
    auto issue_part = [&](int t, Group& f, int part) {       // part 0..7: dy pair s8 = part; parts 8..12: x chunks
      if (part < 8) {
        const bool ok = (t + 1 < y1);                        // dy rows past the range belong to the next wave: read zeros
        const __amdgpu_buffer_rsrc_t as = dd_rsrc(dyb + (long)(ok ? t + 1 : 0) * W * 32, ok ? W * 128 : 0);
        f.d0[part] = dd_bload1<DD_AUX_NT>(as, aoff + part * 512);
        f.d1[part] = dd_bload1<DD_AUX_NT>(as, aoff + part * 512 + 128);
      } else {
        const int i = part - 8;
        const int iy = t + 2;
        const bool rowok = (iy >= 0) && (iy < H);
        const __amdgpu_buffer_rsrc_t rs = dd_rsrc(xb + (long)(rowok ? iy : 0) * W * 32, rowok ? W * 128 : 0);
        const int c = lane + 64 * i;
        const int q = c / C::CHUNKS, ch = c % C::CHUNKS;
        f.xrow[i] = dd_bload4<DD_AUX_NT>(rs, (c < C::NCH) ? ((gx0 + q) * C::PXB + ch * 16) : -16);
      }
    };
    auto step = [&](int yy, const Group& prev, Group& cur, Group& nxt) {
      const char* rb[3];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) rb[ky] = ring + ((yy + ky) % 3) * C::SLOTB + n * 4;
      float a1[8], a2[8];
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8) {
        a1[s8] = 0.5f * (prev.d0[s8] + prev.d1[s8]);
        a2[s8] = 0.5f * (prev.d0[s8] - prev.d1[s8]);
        bsum += prev.d0[s8] + prev.d1[s8];
      }
      // reads run two groups ahead, the input transform one group ahead, each in its own registers: an MFMA must never
      // wait for a VALU result, nor a VALU write for an MFMA that has not read its operand yet
      float dq[3][4], vq[2][4];
      auto rd = [&](int it, float (&d)[4]) {
        const char* p = rb[it >> 3] + (2 * (2 * (it & 7) + h)) * 128;      // ring pixel 2t of tile t = 2s + h
        d[0] = *(const float*)p;
        d[1] = *(const float*)(p + 128);
        d[2] = *(const float*)(p + 256);
        d[3] = *(const float*)(p + 384);
      };
      auto tf = [&](const float (&d)[4], float (&v)[4]) {
        v[0] = d[0] - d[2];
        v[1] = d[1] + d[2];
        v[2] = d[2] - d[1];
        v[3] = d[3] - d[1];
      };
      rd(0, dq[0]);
      rd(1, dq[1]);
      tf(dq[0], vq[0]);
#pragma unroll
      for (int it = 0; it < 24; ++it) {
        const int ky = it >> 3, s8 = it & 7;
        if (it + 2 < 24) rd(it + 2, dq[(it + 2) % 3]);
        if (it + 1 < 24) tf(dq[(it + 1) % 3], vq[(it + 1) & 1]);
        if (it < 13) issue_part(yy + 1, nxt, it);            // next group's loads, one (pair) per MFMA group
        __builtin_amdgcn_sched_barrier(0);
        const float(&v)[4] = vq[it & 1];
        acc[ky][0] = DD_MFMA(prev.d0[s8], v[0], acc[ky][0]);
        acc[ky][1] = DD_MFMA(a1[s8], v[1], acc[ky][1]);
        acc[ky][2] = DD_MFMA(a2[s8], v[2], acc[ky][2]);
        acc[ky][3] = DD_MFMA(prev.d1[s8], v[3], acc[ky][3]);
        __builtin_amdgcn_sched_barrier(0);
        if (it == 15) {   // tap row 0 (the oldest input row) was read by groups 0..7 and tap-row-1 reads (8..15) are out too
          store_row<32, 1, false>(ring + ((yy + 3) % 3) * C::SLOTB, spill, lane, cur.xrow);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    };
    Group ga, gb, gc;
    {   // dy row y0 (group y0-1's dy half) and group y0, synchronously enough: the loop waits for them where it uses them
      const __amdgpu_buffer_rsrc_t as = dd_rsrc(dyb + (long)y0 * W * 32, W * 128);
#pragma unroll
      for (int s8 = 0; s8 < 8; ++s8) {
        ga.d0[s8] = dd_bload1<DD_AUX_NT>(as, aoff + s8 * 512);
        ga.d1[s8] = dd_bload1<DD_AUX_NT>(as, aoff + s8 * 512 + 128);
      }
#pragma unroll
      for (int part = 0; part < 13; ++part) issue_part(y0, gb, part);
    }
    __builtin_amdgcn_sched_barrier(0);
    int yy = y0;
    do {                                      // triples of rows; rows past the range see zero dy (no contribution)
      step(yy, ga, gb, gc);
      step(yy + 1, gb, gc, ga);
      step(yy + 2, gc, ga, gb);
      yy += 3;
    } while (yy < y1);
  }

#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int r = 0; r < 16; ++r) part[((((long)gw * 3 + ky) * 4 + p) * 16 + r) * 64 + lane] = acc[ky][p][r];
  bpart[(long)gw * 64 + lane] = bsum;
}

// Second stage: fixed-order sums of the per-wave partials S_p (one block per (ky, register) row), then the output
// transform and the scatter to OIHW.  Block 48 reduces the bias partials.
__global__ __launch_bounds__(1024) void conv_wino_wgrad_reduce(const float* __restrict__ part, const float* __restrict__ bpart,
                                                               float* __restrict__ dw, float* __restrict__ db, int nw) {
  constexpr int G = 16;
  __shared__ float red[4][G][64];
  const int l = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int row = blockIdx.x;   // ky*16 + r, or 48 for the bias
  if (row == 48) {
    float s0 = 0.f;
    for (int w = g; w < nw; w += G) s0 += bpart[(long)w * 64 + l];
    red[0][g][l] = s0;
    __syncthreads();
    if (g != 0) return;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < G; ++i) s += red[0][i][l];
    const float other = __shfl_xor(s, 32);
    if (l < 32) db[l] = s + other;
    return;
  }
  const int ky = row >> 4, r = row & 15;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int w = g; w < nw; w += G) {
#pragma unroll
    for (int p = 0; p < 4; ++p) s[p] += part[((((long)w * 3 + ky) * 4 + p) * 16 + r) * 64 + l];
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) red[p][g][l] = s[p];
  __syncthreads();
  if (g != 0) return;
  float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int i = 0; i < G; ++i) t[p] += red[p][i][l];
  const int o = dd_acc_row(r, l), j = l & 31;
  float* out = dw + ((long)o * 32 + j) * 9 + ky * 3;
  out[0] = (t[0] + t[1]) + t[2];
  out[1] = t[1] - t[2];
  out[2] = (t[1] + t[2]) + t[3];
}

// U image for conv_wino_fwd: packed[((((ky*4 + p)*2 + half)*2 + g)*64 + lane)*4 + j] = u_p of the taps
// Weff[co = (lane&15) + 16*half][ci = 8*(lane>>4) + 4g + j][ky][0..2];  kind 0: Weff = W (forward);
// kind 1: Weff[co][ci][ky][kx] = W[ci][co][2-ky][2-kx] (stride-1 data gradient).
__global__ void conv_wino_pack_kernel(const float* __restrict__ w, float* __restrict__ p, int kind) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= WINO_UFLOATS) return;
  const int j = idx & 3, lane = (idx >> 2) & 63, g = (idx >> 8) & 1, hf = (idx >> 9) & 1, pos = (idx >> 10) & 3, ky = idx >> 12;
  const int co = (lane & 15) + 16 * hf, ci = 8 * (lane >> 4) + 4 * g + j;
  float t[3];
#pragma unroll
  for (int kx = 0; kx < 3; ++kx)
    t[kx] = kind == 0 ? w[((long)co * 32 + ci) * 9 + ky * 3 + kx] : w[((long)ci * 32 + co) * 9 + (2 - ky) * 3 + (2 - kx)];
  float u;
  if (pos == 0) u = t[0];
  else if (pos == 1) u = 0.5f * ((t[0] + t[1]) + t[2]);
  else if (pos == 2) u = 0.5f * ((t[0] - t[1]) + t[2]);
  else u = t[2];
  p[idx] = u;
}

template <int EPI>
int launch_wino(const float* x, const float* up, const float* bias, const unsigned* bits_in, float* y, unsigned* bits_out,
                const dd_conv_desc* d, hipStream_t st) {
  using C = StripCfg<32, 1>;
  constexpr int WPB = 8;
  const int nstrips = (d->width + 31) / 32;
  const size_t lds = (size_t)WINO_UFLOATS * 4 + (size_t)WPB * C::WAVEB;
  const int grid = resident_grid(d, (long)d->batch * nstrips * d->height, WPB, 1);
  auto k = conv_wino_fwd<EPI, WPB>;
  if (int rc = dd_allow_lds((const void*)k, lds)) return rc;
  hipLaunchKernelGGL(k, dim3(grid), dim3(WPB * 64), lds, st, x, up, bias, bits_in, y, bits_out, d->batch, d->height, d->width, nstrips);
  DD_LAUNCH_CHECK("conv_wino_fwd");
  return 0;
}

}  // namespace

extern "C" {

int64_t dd_conv_wino_packed_floats(const dd_conv_desc* d) {
  return is_c2(d) ? WINO_UFLOATS : -1;
}

int dd_conv_wino_pack(const float* w_oihw, float* packed, const dd_conv_desc* d, int32_t kind, void* stream) {
  if (int rc = require_c2(d, w_oihw && packed, "conv_wino_pack")) return rc;
  DD_REQUIRE(kind == 0 || kind == 1, DD_ERR_BAD_ARG, "conv_wino_pack: kind %d (0 forward, 1 data gradient)", kind);
  hipLaunchKernelGGL(conv_wino_pack_kernel, dim3((WINO_UFLOATS + 255) / 256), dim3(256), 0, (hipStream_t)stream, w_oihw, packed, kind);
  DD_LAUNCH_CHECK("conv_wino_pack");
  return 0;
}

int64_t dd_conv_wino_wgrad_workspace_bytes(const dd_conv_desc* d) {
  return is_c2(d) ? (int64_t)4 * DD_NUM_CU * ((int64_t)12 * 1024 + 64) * 4 : -1;      // one 4-wave workgroup per CU, 12 accumulators per wave
}

int dd_conv_wino_wgrad(const float* x, const float* dy, float* dw_oihw, float* dbias, void* workspace, int64_t workspace_bytes,
                       const dd_conv_desc* d, void* stream) {
  if (int rc = require_c2(d, x && dy && dw_oihw && dbias && workspace, "conv_wino_wgrad")) return rc;
  DD_REQUIRE(workspace_bytes >= dd_conv_wino_wgrad_workspace_bytes(d), DD_ERR_WORKSPACE, "conv_wino_wgrad: workspace %ld < %ld bytes",
             (long)workspace_bytes, (long)dd_conv_wino_wgrad_workspace_bytes(d));
  hipStream_t st = (hipStream_t)stream;
  constexpr int WPB = 4;
  const int nstrips = (d->width + 31) / 32;
  const int grid = resident_grid(d, (long)d->batch * nstrips * d->height, WPB, 1);
  const int nw = grid * WPB;
  float* part = (float*)workspace;
  float* bpart = part + (size_t)nw * 12 * 1024;
  auto k = conv_wino_wgrad<WPB>;
  const size_t lds = (size_t)WPB * StripCfg<32, 1>::WAVEB;
  if (int rc = dd_allow_lds((const void*)k, lds)) return rc;
  hipLaunchKernelGGL(k, dim3(grid), dim3(WPB * 64), lds, st, x, dy, part, bpart, d->batch, d->height, d->width, nstrips);
  DD_LAUNCH_CHECK("conv_wino_wgrad");
  hipLaunchKernelGGL(conv_wino_wgrad_reduce, dim3(49), dim3(1024), 0, st, part, bpart, dw_oihw, dbias, nw);
  DD_LAUNCH_CHECK("conv_wino_wgrad_reduce");
  return 0;
}

int dd_conv_wino_fwd_relu_bits(const float* x, const float* packed, const float* bias, float* y, uint32_t* relu_bits,
                               const dd_conv_desc* d, void* stream) {
  if (int rc = require_c2(d, x && packed && bias && y && relu_bits, "conv_wino_fwd_relu_bits")) return rc;
  return launch_wino<EPI_BIAS_RELU_BITS>(x, packed, bias, nullptr, y, relu_bits, d, (hipStream_t)stream);
}

int dd_conv_wino_dgrad_relu_bits(const float* dy, const float* packed, const uint32_t* relu_bits, float* dx,
                                 const dd_conv_desc* d, void* stream) {
  if (int rc = require_c2(d, dy && packed && relu_bits && dx, "conv_wino_dgrad_relu_bits")) return rc;
  return launch_wino<EPI_RELU_BITS>(dy, packed, nullptr, relu_bits, dx, nullptr, d, (hipStream_t)stream);
}

}  // extern "C"

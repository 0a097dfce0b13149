// What conv3x3.hip (direct strip kernels), conv_wino.inc (F(2,3) along x) and conv_wino2.inc (F(2x2,3x3)) share (internal): the epilogue codes, the LDS
// ring's geometry and row loaders, the packed adds of the Winograd transforms, the host checks of a dd_conv_desc.  No kernel; all in an anonymous namespace.
#pragma once
#include "dd_common.h"

namespace {

// internal epilogues on top of the public DD_EPI_* ones: the ReLU sign travels as ONE BIT per activation
// (a uint32 per 32-channel pixel) instead of being re-read from the 128-byte fp32 pixel by the backward kernels
constexpr int EPI_BIAS_RELU_BITS = 5;   // y = relu(conv + bias), bits[pixel] = mask of (y > 0) over the 32 channels
constexpr int EPI_RELU_BITS = 6;        // y = conv * bit(channel) of bits[pixel]
// Conv -> BatchNorm2d -> ReLU variant (reference components_v2.py:43-46): the conv writes the PRE-normalisation value
// and gathers the batch statistics in its epilogue; the normalise + ReLU is applied by whoever READS the tensor
// (next conv's row loader, pool, mask tests) from a per-channel (scale, shift), so the activation is never rewritten.
constexpr int EPI_BIAS_STATS = 7;       // u = conv + bias; per-channel (n, mean, M2) of the wave's u -> stats[wave][128] (bn2d.hip)
constexpr int EPI_RELU_MASK_AFF = 8;    // y = conv * (mask*m_scale[c] + m_shift[c] > 0)
constexpr int EPI_RELU_BITS_W1 = 9;     // conv_wino2_fwd only: as EPI_RELU_BITS, but y is not stored -- it feeds the 3 -> 32 layer's weight gradient in place

// per-channel affine tables handed to the kernels: [0:32) input scale, [32:64) input shift, [64:96) mask scale, [96:128) mask shift

template <int CIN, int S>
struct StripCfg {
  static constexpr int PXB = CIN * 4;        // bytes per pixel
  static constexpr int CHUNKS = CIN / 4;     // 16-byte chunks per pixel
  static constexpr int NPX = 32 * S + 2;     // input pixels a 32-wide output strip touches (+1 spare for S=2)
  static constexpr int SLOTB = NPX * PXB;    // one ring slot = one input row of the strip
  static constexpr int NCH = NPX * CHUNKS;
  static constexpr int NLOAD = (NCH + 63) / 64;
  static constexpr int SPILLB = (NLOAD * 64 - NCH) * 16;  // landing zone of the idle lanes of the last chunk group
  static constexpr int WAVEB = 3 * SLOTB + SPILLB;        // LDS per wave: 3-slot ring + landing zone
  static constexpr int KGROUPS = (CIN == 32) ? 36 : 5;   // groups of 4 MFMA k-steps
  static constexpr int WFLOATS = KGROUPS * 64 * 4;
};

// XOR swizzle of the 16-byte chunk index inside a 128-byte pixel so that the ds_read_b128 of 16
// consecutive pixels (one lane group) covers all 64 banks: pixels q and q+1 differ in address bit 7,
// (q>>1)&7 spreads the other 8 pixel pairs over the 8 chunk positions.
template <int CIN>
__device__ __forceinline__ int swz(int q) {
  return CIN == 32 ? ((q >> 1) & 7) : 0;
}

// Row iy of image `img` ([H][W][CIN] floats): pixels gx0 .. gx0+NPX-1 into registers (zeros outside the image).
template <int CIN, int S>
__device__ __forceinline__ void load_row(const float* __restrict__ img, int H, int W, int iy, int gx0, int lane,
                                         f32x4 (&r)[StripCfg<CIN, S>::NLOAD]) {
  using C = StripCfg<CIN, S>;
  const bool rowok = (iy >= 0) && (iy < H);
  const __amdgpu_buffer_rsrc_t rs = dd_rsrc(img + (long)(rowok ? iy : 0) * W * CIN, rowok ? W * C::PXB : 0);
#pragma unroll
  for (int i = 0; i < C::NLOAD; ++i) {
    const int c = lane + 64 * i;
    const int q = c / C::CHUNKS, ch = c % C::CHUNKS;
    // a negative pixel index gives a huge unsigned offset: out of range -> zero, like the pixels right of the image
    const int off = (c < C::NCH) ? ((gx0 + q) * C::PXB + ch * 16) : -16;
    r[i] = dd_bload4<DD_AUX_NT>(rs, off);
  }
}

// The same with ONE multiply, add and select per row instead of a 64-bit base + row * pitch and the 16-bit split of the address:
// base = the image, the row in the scalar offset, num_records = the END of that row.  gfx950 adds the scalar offset in the range
// check (tools/ubench/soffset_probe.hip), so a pixel right of the row is out of range and one left of it (a negative lane offset) too.
template <int CIN, int S>
__device__ __forceinline__ void load_row_img(const float* __restrict__ img, int H, int W, int iy, int gx0, int lane,
                                             f32x4 (&r)[StripCfg<CIN, S>::NLOAD]) {
  using C = StripCfg<CIN, S>;
  const bool rowok = (iy >= 0) && (iy < H);
  const int so = rowok ? iy * W * C::PXB : 0;
  const __amdgpu_buffer_rsrc_t rs = dd_rsrc(img, rowok ? so + W * C::PXB : 0);
#pragma unroll
  for (int i = 0; i < C::NLOAD; ++i) {
    const int c = lane + 64 * i;
    const int q = c / C::CHUNKS, ch = c % C::CHUNKS;
    const int off = (c < C::NCH) ? ((gx0 + q) * C::PXB + ch * 16) : -16;
    r[i] = dd_bload4<DD_AUX_NT>(rs, off, so);
  }
}

// Registers -> ring slot.  Every lane writes (no exec-masked branch that would drag the matching load and a
// full vmcnt(0) wait into it): the lanes of the last, partial chunk group land in the wave's `spill` zone.
template <int CIN, int S, bool SWZ>
__device__ __forceinline__ void store_row(char* slot, char* spill, int lane,
                                          const f32x4 (&r)[StripCfg<CIN, S>::NLOAD]) {
  using C = StripCfg<CIN, S>;
#pragma unroll
  for (int i = 0; i < C::NLOAD; ++i) {
    const int c = lane + 64 * i;
    const int q = c / C::CHUNKS, ch = c % C::CHUNKS;
    char* dst = slot + q * C::PXB + ((ch ^ (SWZ ? swz<CIN>(q) : 0)) << 4);
    if (64 * (i + 1) > C::NCH) dst = (c < C::NCH) ? dst : spill + (c - C::NCH) * 16;
    *(f32x4*)dst = r[i];
  }
}

// Same, for a tensor stored PRE-BatchNorm: in-image pixels become relu(v * scale + shift) on their way into the ring;
// padding stays zero (it pads the normalised activation).  A lane's chunks all cover channels 4*(lane&7)..+3
// (64*i is a multiple of the 8 chunks per pixel), so it carries one (scale, shift) quad.
template <int S, bool SWZ>
__device__ __forceinline__ void store_row_aff(char* slot, char* spill, int lane, const f32x4 (&r)[StripCfg<32, S>::NLOAD],
                                              bool rowok, int gx0, int W, f32x4 sc, f32x4 sh) {
  using C = StripCfg<32, S>;
#pragma unroll
  for (int i = 0; i < C::NLOAD; ++i) {
    const int c = lane + 64 * i;
    const int q = c / C::CHUNKS, ch = c % C::CHUNKS;
    char* dst = slot + q * C::PXB + ((ch ^ (SWZ ? swz<32>(q) : 0)) << 4);
    if (64 * (i + 1) > C::NCH) dst = (c < C::NCH) ? dst : spill + (c - C::NCH) * 16;
    const bool in = rowok && (gx0 + q >= 0) && (gx0 + q < W);
    f32x4 v = r[i];
    v.x = in ? fmaxf(v.x * sc.x + sh.x, 0.f) : 0.f;
    v.y = in ? fmaxf(v.y * sc.y + sh.y, 0.f) : 0.f;
    v.z = in ? fmaxf(v.z * sc.z + sh.z, 0.f) : 0.f;
    v.w = in ? fmaxf(v.w * sc.w + sh.w, 0.f) : 0.f;
    *(f32x4*)dst = v;
  }
}

// Packed fp32 add / subtract on 4-channel vectors: the fp32 matrix and vector instructions share the ALUs, so every VALU
// instruction beside the MFMAs costs matrix time; v_pk_add_f32 does two lanes' worth per issue.  (hipcc selects it for
// a 2-vector add but splits a subtract into scalars, hence the explicit form with the negate modifiers.)
__device__ __forceinline__ f32x2 pk_sub2(f32x2 a, f32x2 b) {
  f32x2 r;
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ f32x2 pk_add2(f32x2 a, f32x2 b) {      // always packed (hipcc splits a 2-vector add whose operands are not register pairs yet)
  f32x2 r;
  asm("v_pk_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ f32x4 pk_add4a(f32x4 a, f32x4 b) {
  const f32x2 lo = pk_add2(f32x2{a.x, a.y}, f32x2{b.x, b.y}), hi = pk_add2(f32x2{a.z, a.w}, f32x2{b.z, b.w});
  return f32x4{lo.x, lo.y, hi.x, hi.y};
}
__device__ __forceinline__ f32x4 pk_add4(f32x4 a, f32x4 b) {
  const f32x2 lo = f32x2{a.x, a.y} + f32x2{b.x, b.y}, hi = f32x2{a.z, a.w} + f32x2{b.z, b.w};
  return f32x4{lo.x, lo.y, hi.x, hi.y};
}
__device__ __forceinline__ f32x4 pk_sub4(f32x4 a, f32x4 b) {
  f32x2 lo, hi;
  const f32x2 alo = {a.x, a.y}, ahi = {a.z, a.w}, blo = {b.x, b.y}, bhi = {b.z, b.w};
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(lo) : "v"(alo), "v"(blo));
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(hi) : "v"(ahi), "v"(bhi));
  return f32x4{lo.x, lo.y, hi.x, hi.y};
}

int check_desc(const dd_conv_desc* d) {
  DD_REQUIRE(d != nullptr, DD_ERR_BAD_ARG, "conv: NULL descriptor");
  DD_REQUIRE(d->batch > 0 && d->height > 0 && d->width > 0, DD_ERR_BAD_ARG, "conv: non-positive size");
  DD_REQUIRE(d->ksize == 3 && d->pad == 1, DD_ERR_UNSUPPORTED, "conv: only k3 p1 is implemented (got k%d p%d)", d->ksize, d->pad);
  DD_REQUIRE(d->stride == 1 || d->stride == 2, DD_ERR_UNSUPPORTED, "conv: stride %d", d->stride);
  DD_REQUIRE(d->cout == 32, DD_ERR_UNSUPPORTED, "conv: Cout %d (only 32)", d->cout);
  DD_REQUIRE((d->cin_real == 32 && d->cin_store == 32) || (d->cin_real == 3 && d->cin_store == 4), DD_ERR_UNSUPPORTED,
             "conv: Cin %d stored as %d (supported: 32/32, 3/4)", d->cin_real, d->cin_store);
  DD_REQUIRE(!(d->cin_real == 3 && d->stride == 2), DD_ERR_UNSUPPORTED, "conv: Cin 3 with stride 2");
  DD_REQUIRE((long)d->width * 128 < (1L << 31), DD_ERR_UNSUPPORTED, "conv: row too long for a 32-bit buffer descriptor");
  return 0;
}

// Workgroups launched = workgroups resident: `per_cu` blocks on each CU (bounded by the LDS ring + registers
// of the instantiation), fewer when the problem has fewer wave-sized pieces.  rows_per_task (a testing / tuning
// knob, never changes results) asks for at least that many rows per wave, i.e. fewer and longer ranges.
int resident_grid(const dd_conv_desc* d, long row_tiles, int wpb, int per_cu) {
  long blocks = (long)dd_cu_budget_internal() * per_cu;
  if (d->rows_per_task > 0) blocks = min(blocks, max(1L, row_tiles / d->rows_per_task / wpb));
  return (int)max(1L, min(blocks, (row_tiles + wpb - 1) / wpb));
}

// The first checks of every Winograd entry point, in the order their errors are reported: descriptor, its own pointers (`pointers` = all non-NULL), layer.
int require_c2(const dd_conv_desc* d, bool pointers, const char* who) {
  if (int rc = check_desc(d)) return rc;
  DD_REQUIRE(pointers, DD_ERR_BAD_ARG, "%s: NULL pointer", who);
  DD_REQUIRE(d->cin_real == 32 && d->stride == 1, DD_ERR_UNSUPPORTED, "conv_wino: only the 32 -> 32 stride-1 layer");
  return 0;
}

// For the size functions, which answer -1 for any other descriptor (a bad one leaves check_desc's message).
bool is_c2(const dd_conv_desc* d) { return check_desc(d) == 0 && d->cin_real == 32 && d->stride == 1; }

}  // namespace

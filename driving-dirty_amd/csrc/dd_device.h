// Device-side primitives shared by the gfx950 kernels: the one definition of everything two kernel files would otherwise each
// spell for themselves (vector types, matrix-core wrappers, range-checked buffer access, the work split, bf16 rounding, the LDS
// transpose read, the workgroup barriers).  All of it is forced inline: moving a primitive here changes no kernel's machine code.
// Included through dd_common.h.
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// D(32x32) += A(32x2) * B(2x32), exact fp32 (v_mfma_f32_32x32x2_f32, 64 cycles / SIMD).
// lane l supplies A[row = l&31][k = l>>5] and B[k = l>>5][col = l&31];
// D register r of lane l is D[row = (r&3) + 8*(r>>2) + 4*(l>>5)][col = l&31].
#define DD_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
// D(16x16) += A(16x4) * B(4x16), exact fp32 (v_mfma_f32_16x16x4_f32, 32 cycles / SIMD): a lane holds 4 rows of one column.
#define DD_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
// D(32x32) += A(32x16) * B(16x32), bf16 operands (8 per lane: k = 8*(l>>5) .. +7), fp32 accumulation; D laid out as DD_MFMA's.
#define DD_MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

// Row of accumulator register r (DD_MFMA, DD_MFMA_BF16) in the lanes of wave half h = lane >> 5.  Kernels that already hold h use the
// first form: the compiler selects other instructions for the same value when it meets the shift of the lane id again.
__device__ __forceinline__ int dd_acc_row_half(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
__device__ __forceinline__ int dd_acc_row(int r, int lane) { return dd_acc_row_half(r, lane >> 5); }

// The lane id, recomputed where it is needed: a `volatile` asm is neither hoisted nor shared, so code after a long MFMA loop
// (an epilogue's addresses, the next tile's fill plan) does not keep lane-derived registers alive across that loop -- which is
// what the register allocator otherwise spills to scratch in kernels that use the whole register file.
__device__ __forceinline__ int dd_fresh_lane() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// Raw buffer access: the descriptor (wave-uniform base + byte count) makes the hardware range-check every lane:
// an out-of-range load returns zeros, an out-of-range store is dropped.  A negative offset is a huge unsigned
// one, i.e. out of range.  Used for zero padding and ragged edges without branches, and as a guard against faults.
constexpr int DD_RSRC_FLAGS = 0x00020000;      // fourth descriptor word: 32-bit data format (raw dword access), no stride, no swizzle
__device__ __forceinline__ __amdgpu_buffer_rsrc_t dd_rsrc(const void* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, DD_RSRC_FLAGS);
}
// The same descriptor as four words (an inline-asm "s" operand): base, num_records = bytes, flags.
__device__ __forceinline__ i32x4 dd_rsrc_words(const void* base, int bytes) {
  const unsigned long a = (unsigned long)base;
  return i32x4{(int)(unsigned)a, (int)(unsigned)((a >> 32) & 0xffff), bytes, DD_RSRC_FLAGS};
}

// One 4-, 8- or 16-byte element T per lane at byte offset `off` (per lane) + `soff` (wave-uniform, counted in the range check).
// AUX is the cache hint of the instruction: 0 = none, DD_AUX_NT = non-temporal, for streams that are touched once.
constexpr int DD_AUX_NT = 2;
template <typename T, int AUX = 0>
__device__ __forceinline__ T dd_bload(__amdgpu_buffer_rsrc_t r, int off, int soff = 0) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8 || sizeof(T) == 16, "dd_bload: 4, 8 or 16 bytes per lane");
  if constexpr (sizeof(T) == 16) return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b128(r, off, soff, AUX));
  else if constexpr (sizeof(T) == 8) return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b64(r, off, soff, AUX));
  else return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b32(r, off, soff, AUX));
}
template <int AUX = 0, typename T>
__device__ __forceinline__ void dd_bstore(__amdgpu_buffer_rsrc_t r, int off, T v, int soff = 0) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8 || sizeof(T) == 16, "dd_bstore: 4, 8 or 16 bytes per lane");
  if constexpr (sizeof(T) == 16) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, off, soff, AUX);
  else if constexpr (sizeof(T) == 8) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, off, soff, AUX);
  else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, off, soff, AUX);
}
// the fp32 forms by name
template <int AUX = 0>
__device__ __forceinline__ f32x4 dd_bload4(__amdgpu_buffer_rsrc_t r, int off, int soff = 0) { return dd_bload<f32x4, AUX>(r, off, soff); }
template <int AUX = 0>
__device__ __forceinline__ float dd_bload1(__amdgpu_buffer_rsrc_t r, int off, int soff = 0) { return dd_bload<float, AUX>(r, off, soff); }
template <int AUX = 0>
__device__ __forceinline__ void dd_bstore1(__amdgpu_buffer_rsrc_t r, int off, float v) { dd_bstore<AUX>(r, off, v); }

// Batch statistics without the cancellation of sum(v^2) - sum(v)^2/n: the moments of a set of values ABOUT A PIVOT p close to them
// (the first value a lane meets): n, s = sum(v - p), q = sum((v - p)^2).  A lane gathers them in fp32 -- the terms are of the size
// of the spread, whatever the offset of the values -- and everything behind the lane's loop is done in fp64: two sets merge by
// moving the second onto the first's pivot (with d = p_b - p_a: s_b' = s_b + n_b d, q_b' = q_b + d (2 s_b + n_b d), exact algebra,
// no division), and mean = p + s/n, M2 = sum((v - mean)^2) = q - s^2/n lose nothing, since |s/n| is of the size of the spread too.
// Merged in this form, (n, mean, M2) sets combine exactly as by Chan's pairwise formula.  An empty set is n = 0 with finite entries.
struct DdMoments {
  double n, p, s, q;
};
__device__ __forceinline__ void dd_moments_merge(DdMoments& a, const DdMoments& b) {
  if (a.n == 0.0) a.p = b.p;      // a.s == a.q == 0: the union takes b's pivot
  const double d = b.p - a.p;
  a.s += b.s + b.n * d;
  a.q += b.q + d * (2.0 * b.s + b.n * d);
  a.n += b.n;
}
__device__ __forceinline__ void dd_moments_finish(const DdMoments& a, double& mean, double& m2) {
  const double r = a.n > 0.0 ? a.s / a.n : 0.0;
  mean = a.n > 0.0 ? a.p + r : 0.0;
  m2 = fmax(a.q - a.s * r, 0.0);
}

// The contiguous range [idx, end) of `total` work items owned by piece `i` of `n` equal pieces (for the row tiles of the convolutions:
// piece = global wave, idx = column * rows + row).  A piece past the end of the work gets the empty range idx == end.
__device__ __forceinline__ void dd_range(long total, int i, int n, long& idx, long& end) {
  const long per = (total + n - 1) / n;
  idx = (long)i * per;
  end = idx + per < total ? idx + per : total;
  if (idx > end) idx = end;
}

// The entry t of a launch table that this workgroup works on: first[t] <= blockIdx.x < first[t + 1], where first[] holds the running
// sum of the entries' workgroup counts (the multi-tensor launches: dd_adam.h, gradnorm.hip).  A linear walk: a table has 48 entries.
template <int N>
__device__ __forceinline__ int dd_table_entry(const int (&first)[N], int count) {
  int t = 0;
  while (t + 1 < count && (int)blockIdx.x >= first[t + 1]) ++t;
  return t;
}

// bf16 <-> fp32.  Every kernel rounds through dd_pack_bf16 (v_cvt_pk_bf16_f32: round to nearest even, NaN stays NaN), which is
// what the bf16 contract of the oracle assumes.
__device__ __forceinline__ unsigned dd_pack_bf16(float lo, float hi) {      // two bf16 in one word, `lo` in the low half
  return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){lo, hi}, bf16x2));
}
__device__ __forceinline__ float dd_bf16_lo(unsigned u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float dd_bf16_hi(unsigned u) { return __builtin_bit_cast(float, u & 0xffff0000u); }
__device__ __forceinline__ unsigned dd_bf16_round_bits(float x) { return dd_pack_bf16(x, 0.f) << 16; }      // the bf16 nearest x, as an fp32 pattern

// LDS transpose read (ds_read_b64_tr_b16): per 16-lane group a block of 4 rows x 16 consecutive bf16; lane 4q+p of the group
// supplies the address of row q, elements 4p..4p+3; lane e receives element e of the four rows.  dd_join: two reads = one MFMA operand.
__device__ __forceinline__ s16x4 dd_tr_read(const char* p) {
  typedef s16x4 __attribute__((address_space(3))) * lds_s16x4_ptr;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)p);
}
__device__ __forceinline__ bf16x8 dd_join(s16x4 a, s16x4 b) {
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for every outstanding vector-memory operation
// (vmcnt(0)): in the dilated kernels that would drain the weight fragments requested a tap row ahead at every chunk boundary -- a
// full L2 round trip with all 8 waves of the workgroup idle (measured: ~3k cycles per chunk, 12 % of up_conv_1's forward).  For
// kernels that read nothing from global memory that they wrote, and whose LDS is not filled by DMA (or that count vmcnt themselves).
__device__ __forceinline__ void dd_barrier_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// Barrier behind LDS-DMA fills: they must have landed (vmcnt) before the barrier publishes the buffer; the LDS reads of this step
// are done (lgkmcnt).
__device__ __forceinline__ void dd_barrier_dma() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// sigmoid(z) and softplus(-|z|) = log1p(exp(-|z|)) from the hardware transcendentals (v_exp_f32 / v_log_f32 / v_rcp_f32,
// 1 ulp each) instead of libm's expf + log1pf + IEEE divisions: 145 -> ~25 instructions per element, which is what
// made the loss pass compute-bound (87 us for 184 MB).  log1p(e) = log(u) * e / (u - 1) with u = fl(1 + e) undoes the
// rounding of 1 + e (u - 1 is exact); one Newton step refines the reciprocal.
// Accuracy against fp64 (tests/_element_ref.py derives the bounds from an fp32 model of this formula with correctly rounded
// primitives; tests/test_gpu_element_range.py holds the kernels to them and prints what they use of each; DESIGN.md 3.4f has the
// figures): sigmoid for z >= 0 within 3 x 2^-24 ABSOLUTE, and bit for bit the correctly rounded reciprocal of u wherever u is
// determined -- that is what the Newton step buys; the absolute bound holds without it. For z < 0, and for the softplus, the
// error is RELATIVE and grows with |z|: within (|z| + 11) 2^-24 and (|z| + 12) 2^-24 on the tested logits, below 2^-126 flushed
// to zero. The |z| is the rounding of the exponent -|z| log2(e) -- half an ulp of it is up to 2^-24 |z| of e -- plus 0.22 |z|
// for the rounded constant: so "within 1 ulp" holds in the absolute sense only, and a logit past |z| = 40 whose exponent rounds
// the wrong way just above 64 can need 1.22 |z| + 3.
// Here because it is the ONE sigmoid of the dense head: dd_sigmoid, the BCE pass (dense.hip) and dd_linear_sigmoid_gt (linear.hip) all
// take theirs from it, so their probabilities agree bit for bit.
__device__ __forceinline__ void dd_sigmoid_softplus(float z, float& sig, float& l1p) {
  const float e = __builtin_amdgcn_exp2f(-fabsf(z) * 1.4426950408889634f);      // in [0, 1]; flushes to 0 below 2^-126
  const float u = 1.f + e, d = u - 1.f;
  float r = __builtin_amdgcn_rcpf(u);
  r = fmaf(r, fmaf(-u, r, 1.f), r);
  sig = z >= 0.f ? r : e * r;
  l1p = d == 0.f ? e : (__builtin_amdgcn_logf(u) * 0.6931471805599453f) * (e * __builtin_amdgcn_rcpf(d));
}

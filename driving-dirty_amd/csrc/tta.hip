// Mirror test-time averaging (include/dd_tta.h; csrc/libdd_tta.so, a library of its own):
//   dd_tta_mean_prob   mean[b,r,c] = 0.5f * (P(a[b,r,c]) + P(m[b,h-1-r,c]))   -> fp32 [B,h,w]
//   dd_tta_mean_gt     mean > tau                                            -> bytes [B,h,w]; the mean never reaches memory
// Pure streaming: every input element is read once, every output element written once, no LDS, no atomics, a bounded grid with a
// grid-stride loop.  The kernel is picked by the SHAPE alone (never by an address); all of them compute an element through the one
// function `tta_mean`, so the same bits:
//   w % 16 == 0 (the byte form; 800)   16 consecutive columns per lane: four 16-byte loads from each input, ONE 16-byte store
//   w %  4 == 0                        4 consecutive columns per lane: one 16-byte load from each input; a 16-byte store (fp32) or a
//                                      4-byte store (bytes)
//   otherwise                          one element per lane
// A group of columns never crosses a row (w is a multiple of the group), so the mirrored row's group is consecutive too, and with
// 16-byte aligned operands every row of w % 4 == 0 floats starts on a 16-byte boundary.  Each lane clamps the groups past the end
// to the last one and issues all loads of its kUnroll groups before the first use: eight 16-byte loads (or eight scalar ones) in
// flight per lane.
#include "dd_common.h"

#include "../../include/dd_tta.h"

#pragma clang fp contract(off)      // P(a) + P(m) is ONE rounded add: the product that ends the sigmoid (e * r) is not fused into it

namespace {

template <bool LOGITS>
__device__ __forceinline__ float tta_prob(float z) {
  if constexpr (!LOGITS) return z;
  float sig, l1p;
  dd_sigmoid_softplus(z, sig, l1p);      // the dense head's one sigmoid; the softplus half is dead code here
  return sig;
}

// THE per-element function of every kernel below
template <bool LOGITS>
__device__ __forceinline__ float tta_mean(float a, float m) { return 0.5f * (tta_prob<LOGITS>(a) + tta_prob<LOGITS>(m)); }

// element offset of the mirrored partner of element offset `i` = (b * h + r) * w + c: (b * h + h - 1 - r) * w + c.  All below 2^31.
__device__ __forceinline__ unsigned mirrored(unsigned i, unsigned h, unsigned w) {
  const unsigned row = i / w, b = row / h;
  return i + ((2 * b + 1) * h - 1 - 2 * row) * w;      // row' - row = (b h + h - 1 - r) - (b h + r), r = row - b h; wraps as it should
}

// COLS consecutive columns per lane, COLS in {4, 16}, w % COLS == 0.  GT: bytes (mean > tau), else fp32 (COLS == 4 only).
template <bool LOGITS, int COLS, bool GT>
__global__ __launch_bounds__(256) void tta_vec_kernel(const float* __restrict__ a, const float* __restrict__ m, float tau,
                                                      void* __restrict__ out, unsigned groups, unsigned h, unsigned w) {
  static_assert(GT || COLS == 4, "the fp32 form stores four columns per lane");
  constexpr int kVec = COLS / 4, kUnroll = 8 / (2 * kVec) < 1 ? 1 : 8 / (2 * kVec);      // 4 groups of 4 columns, 1 group of 16
  const unsigned stride = gridDim.x * blockDim.x;
  for (unsigned g0 = blockIdx.x * blockDim.x + threadIdx.x; g0 < groups; g0 += stride * kUnroll) {
    f32x4 va[kUnroll][kVec], vm[kUnroll][kVec];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const unsigned i = min(g0 + u * stride, groups - 1) * COLS;      // past the end: the last group again, loaded and not stored
      const unsigned im = mirrored(i, h, w);
#pragma unroll
      for (int v = 0; v < kVec; ++v) {
        va[u][v] = *(const f32x4*)(a + i + 4 * v);
        vm[u][v] = *(const f32x4*)(m + im + 4 * v);
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const unsigned g = g0 + u * stride;
      if (g >= groups) continue;
      if constexpr (GT) {
        unsigned word[kVec];
#pragma unroll
        for (int v = 0; v < kVec; ++v) {
          word[v] = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) word[v] |= (tta_mean<LOGITS>(va[u][v][j], vm[u][v][j]) > tau ? 1u : 0u) << (8 * j);
        }
        if constexpr (COLS == 16) ((u32x4*)out)[g] = u32x4{word[0], word[1], word[2], word[3]};
        else ((unsigned*)out)[g] = word[0];
      } else {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = tta_mean<LOGITS>(va[u][0][j], vm[u][0][j]);
        ((f32x4*)out)[g] = o;
      }
    }
  }
}

// any w: one element per lane, four in flight
template <bool LOGITS, bool GT>
__global__ __launch_bounds__(256) void tta_scalar_kernel(const float* __restrict__ a, const float* __restrict__ m, float tau,
                                                         void* __restrict__ out, unsigned total, unsigned h, unsigned w) {
  constexpr int kUnroll = 4;
  const unsigned stride = gridDim.x * blockDim.x;
  for (unsigned i0 = blockIdx.x * blockDim.x + threadIdx.x; i0 < total; i0 += stride * kUnroll) {
    float va[kUnroll], vm[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const unsigned i = min(i0 + u * stride, total - 1);
      va[u] = a[i];
      vm[u] = m[mirrored(i, h, w)];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const unsigned i = i0 + u * stride;
      if (i >= total) continue;
      const float mean = tta_mean<LOGITS>(va[u], vm[u]);
      if constexpr (GT) ((unsigned char*)out)[i] = mean > tau ? 1 : 0;
      else ((float*)out)[i] = mean;
    }
  }
}

int grid_for(long items, int per_lane_iter) {
  const long lanes = (items + per_lane_iter - 1) / per_lane_iter;
  return (int)min((lanes + 255) / 256, (long)DD_NUM_CU * 8);
}

bool overlaps(const void* p, long p_bytes, const void* q, long q_bytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)q_bytes && b < a + (uintptr_t)p_bytes;
}

// by the SHAPE alone
template <bool GT, bool LOGITS>
void launch_shape(const float* a, const float* m, float tau, void* out, long total, int h, int w, hipStream_t st) {
  if constexpr (GT) {
    if (w % 16 == 0) {
      hipLaunchKernelGGL((tta_vec_kernel<LOGITS, 16, true>), dim3(grid_for(total / 16, 1)), dim3(256), 0, st, a, m, tau, out,
                         (unsigned)(total / 16), (unsigned)h, (unsigned)w);
      return;
    }
  }
  if (w % 4 == 0)
    hipLaunchKernelGGL((tta_vec_kernel<LOGITS, 4, GT>), dim3(grid_for(total / 4, 4)), dim3(256), 0, st, a, m, tau, out,
                       (unsigned)(total / 4), (unsigned)h, (unsigned)w);
  else
    hipLaunchKernelGGL((tta_scalar_kernel<LOGITS, GT>), dim3(grid_for(total, 4)), dim3(256), 0, st, a, m, tau, out, (unsigned)total,
                       (unsigned)h, (unsigned)w);
}

template <bool GT>
int launch_mean(const char* who, const float* a, const float* m, float tau, void* out, int batch, int h, int w, int from_logits,
                void* stream) {
  DD_REQUIRE(a && m && out, DD_ERR_BAD_ARG, "%s: NULL pointer", who);
  DD_REQUIRE(batch > 0 && h > 0 && w > 0, DD_ERR_BAD_ARG, "%s: non-positive size (batch %d, %d x %d)", who, batch, h, w);
  const long total = (long)batch * h * w;
  DD_REQUIRE(total < (1L << 31), DD_ERR_UNSUPPORTED, "%s: [%d,%d,%d] is too large (batch * h * w must stay below 2^31)", who, batch, h, w);
  DD_REQUIRE(from_logits == 0 || from_logits == 1, DD_ERR_BAD_ARG, "%s: from_logits = %d is neither 0 (probabilities) nor 1 (logits)", who,
             from_logits);
  DD_REQUIRE((((uintptr_t)a | (uintptr_t)m | (uintptr_t)out) & 15) == 0, DD_ERR_BAD_ARG, "%s: a, m and out must be 16-byte aligned", who);
  const long out_bytes = total * (GT ? 1 : 4);
  DD_REQUIRE(!overlaps(out, out_bytes, a, total * 4) && !overlaps(out, out_bytes, m, total * 4), DD_ERR_BAD_ARG,
             "%s: out overlaps an input: the row reversal cannot be done in place", who);
  if (from_logits) launch_shape<GT, true>(a, m, tau, out, total, h, w, (hipStream_t)stream);
  else launch_shape<GT, false>(a, m, tau, out, total, h, w, (hipStream_t)stream);
  DD_LAUNCH_CHECK(who);
  return 0;
}

}  // namespace

extern "C" {

int dd_tta_mean_prob(const float* a, const float* m, float* out, int32_t batch, int32_t h, int32_t w, int32_t from_logits,
                     void* stream) {
  return launch_mean<false>("tta_mean_prob", a, m, 0.f, out, batch, h, w, from_logits, stream);
}

int dd_tta_mean_gt(const float* a, const float* m, float tau, unsigned char* out, int32_t batch, int32_t h, int32_t w,
                   int32_t from_logits, void* stream) {
  return launch_mean<true>("tta_mean_gt", a, m, tau, out, batch, h, w, from_logits, stream);
}

}  // extern "C"

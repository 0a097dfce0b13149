// dd_ts_hist: the road-map threat score at EVERY threshold k / bins from one pass over the probabilities.
//
// TS(tau) = TP / (P + T - TP) counts elements only, so a histogram of the probabilities split by the target (2 x (bins + 1)
// integers) holds the whole curve: suffix sums give TP and P at each threshold (ops.ts_curve).  Integer adds commute, so the
// result does not depend on scheduling, and the histograms of a validation epoch's batches add up in one buffer.
#include "dd_common.h"

namespace {

constexpr int kMaxBins = 1024;
constexpr int kHistBlocks = 1024;
// LDS copies of the histogram, lane l counts into copy l % copies: a trained head's probabilities pile up in the two end bins, and
// lanes that add to one LDS word are served one after the other.  As many copies as 16 KB holds.
constexpr int kHistWords = 4128;      // 8 copies x 2 x 257 slots (bins = 256) = 4112; 2 x 2 x 1025 (bins = 1024) = 4100
int hist_copies(int bins) { return max(1, min(8, 2048 / bins)); }

// slot = j + 1 with j = ceil(p * bins) - 1 clamped to [-1, bins - 1]; bins is a power of two, so the product is exact and
// slot > k <=> p > k / bins in fp32.  Every comparison with a NaN is false: slot 0.
__device__ __forceinline__ int ts_slot(float p, float fbins, int bins) {
  const float c = ceilf(p * fbins);
  return c >= fbins ? bins : (c > 0.f ? (int)c : 0);
}

template <typename TT>
__device__ __forceinline__ unsigned target_bits4(const TT* t, long i);      // bit e: element e of quad i is non-zero
template <>
__device__ __forceinline__ unsigned target_bits4<float>(const float* t, long i) {
  const f32x4 v = ((const f32x4*)t)[i];
  return (v.x != 0.f) | (v.y != 0.f) << 1 | (v.z != 0.f) << 2 | (v.w != 0.f) << 3;
}
template <>
__device__ __forceinline__ unsigned target_bits4<unsigned char>(const unsigned char* t, long i) {
  const unsigned w = ((const unsigned*)t)[i];
  return ((w & 0xff) != 0) | ((w & 0xff00) != 0) << 1 | ((w & 0xff0000) != 0) << 2 | ((w >> 24) != 0) << 3;
}

template <typename TT>
__global__ __launch_bounds__(256) void ts_hist_kernel(const float* __restrict__ prob, const TT* __restrict__ target, long n4, int bins,
                                                      int copies, unsigned long long* __restrict__ hist) {
  __shared__ unsigned h[kHistWords];
  const int slots = bins + 1, words = 2 * slots;
  for (int i = threadIdx.x; i < copies * words; i += 256) h[i] = 0;
  __syncthreads();
  unsigned* mine = h + (threadIdx.x % copies) * words;
  const float fbins = (float)bins;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 p = ((const f32x4*)prob)[i];
    const unsigned t = target_bits4<TT>(target, i);
#pragma unroll
    for (int e = 0; e < 4; ++e) atomicAdd(mine + ((t >> e) & 1) * slots + ts_slot(p[e], fbins, bins), 1u);
  }
  __syncthreads();
  for (int s = threadIdx.x; s < words; s += 256) {
    unsigned long long c = 0;
    for (int r = 0; r < copies; ++r) c += h[r * words + s];
    if (c) atomicAdd(hist + s, c);
  }
}

}  // namespace

extern "C" int dd_ts_hist(const float* prob, const void* target, int32_t target_dtype, int64_t n, int32_t bins, int64_t* hist, void* stream) {
  DD_REQUIRE(prob && target && hist, DD_ERR_BAD_ARG, "ts_hist: NULL pointer");
  DD_REQUIRE(bins >= 2 && bins <= kMaxBins && (bins & (bins - 1)) == 0, DD_ERR_UNSUPPORTED, "ts_hist: bins = %d must be a power of two in [2, %d]",
             bins, kMaxBins);
  // a workgroup counts its share in 32-bit LDS words: at most n / kHistBlocks + 1024 elements
  DD_REQUIRE(n > 0 && n % 4 == 0 && n <= ((int64_t)1 << 40), DD_ERR_UNSUPPORTED, "ts_hist: n = %ld must be a positive multiple of 4, at most 2^40", (long)n);
  DD_REQUIRE(target_dtype == DD_TARGET_F32 || target_dtype == DD_TARGET_U8, DD_ERR_UNSUPPORTED, "ts_hist: unknown target dtype %d", target_dtype);
  const bool f32 = target_dtype == DD_TARGET_F32;
  DD_REQUIRE((uintptr_t)prob % 16 == 0 && (uintptr_t)target % (f32 ? 16 : 4) == 0 && (uintptr_t)hist % 8 == 0, DD_ERR_BAD_ARG, "ts_hist: misaligned buffer");
  const long n4 = n / 4;
  const dim3 grid((unsigned)min((n4 + 255) / 256, (long)kHistBlocks));
  unsigned long long* out = (unsigned long long*)hist;
  if (f32)
    hipLaunchKernelGGL(ts_hist_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, prob, (const float*)target, n4, bins, hist_copies(bins), out);
  else
    hipLaunchKernelGGL(ts_hist_kernel<unsigned char>, grid, dim3(256), 0, (hipStream_t)stream, prob, (const unsigned char*)target, n4, bins,
                       hist_copies(bins), out);
  DD_LAUNCH_CHECK("ts_hist");
  return 0;
}

// Weight averaging (include/dd_ema.h; csrc/libdd_ema.so, a library of its own):
//   dd_ema_update_ptrs   e' = fmaf(alpha, w - e, e) over a table of (average, parameter) tensors
//   dd_ema_swap_ptrs     a <-> b as 32-bit words over a table of tensor pairs
// Pure streaming, ONE kernel family for the whole table: the table (a slice of at most kTableMax tensors) travels in the kernel
// arguments with a prefix `first[]` of piece counts, the way dd_adam.h passes ADAM_TABLE_MAX quadruples.  The work is the flat list of
// kChunk-element pieces of all tensors of the slice; workgroup b takes pieces b, b + grid, ... of a grid capped at 8 workgroups per
// CU.  The piece index depends on the workgroup alone, so the table is read with scalar loads from the kernel arguments and the
// search for a piece's tensor costs no vector work: a binary search for the first piece, then a step forward only when a piece
// leaves the current tensor (the pieces of a workgroup ascend).
// A piece inside a tensor's whole 16-byte vectors is four 16-byte loads per lane from each buffer, all issued before the first use,
// and four 16-byte stores; a tensor's last piece guards each vector and ends with the scalar tail of its n % 4 elements.  Both
// paths compute an element by the one function `ema_elem`.  No LDS, no atomics.
// Loads and stores are the non-temporal form, as dd_adam_step's (dd_adam.h): every byte is touched once per call, a plain or a
// non-temporal store both leave the XCD's L2 at the same rate (neither is a write-through), and nothing reads e' again before the
// next step's 1.3 GB have gone through the caches.
#include <algorithm>
#include <math.h>
#include <vector>

#include "dd_common.h"

#include "../../include/dd_ema.h"

#pragma clang fp contract(off)      // w - e is ONE rounded subtract; the fused multiply-add below is written out, not left to the compiler

namespace {

constexpr int kChunk = DD_EMA_CHUNK, kTableMax = DD_EMA_TABLE_MAX, kThreads = 256, kUnroll = kChunk / (4 * kThreads);
static_assert(kUnroll * 4 * kThreads == kChunk && kUnroll >= 1, "a piece is a whole number of 16-byte vectors per lane");

struct EmaTable {
  unsigned* a[kTableMax];              // update: the averages (written); swap: one side
  unsigned* b[kTableMax];              // update: the parameters (read only); swap: the other side
  unsigned n[kTableMax];               // elements, < 2^31
  int first[kTableMax + 1];            // pieces in front of tensor t; first[count] = pieces of the launch, < 2^26
  int count;
};

// THE per-element function of the update
__device__ __forceinline__ float ema_elem(float e, float w, float alpha) {
  const float d = w - e;
  return d == 0.f ? e : __builtin_fmaf(alpha, d, e);      // e == w keeps e's bits (fmaf(alpha, +0, -0) would be +0)
}

__device__ __forceinline__ unsigned ema_word(unsigned e, unsigned w, float alpha) {
  return __float_as_uint(ema_elem(__uint_as_float(e), __uint_as_float(w), alpha));
}

template <bool SWAP>
__device__ __forceinline__ void piece_vec(u32x4* __restrict__ pa, u32x4* __restrict__ pb, u32x4 va, u32x4 vb, float alpha) {
  if constexpr (SWAP) {
    __builtin_nontemporal_store(vb, pa);
    __builtin_nontemporal_store(va, pb);
  } else {
    u32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = ema_word(va[j], vb[j], alpha);
    __builtin_nontemporal_store(o, pa);
  }
}

template <bool SWAP>
__global__ __launch_bounds__(kThreads) void ema_kernel(EmaTable tab, float alpha) {
  const int pieces = tab.first[tab.count];
  int t = 0;
  {      // the tensor of this workgroup's first piece: first[t] <= blockIdx.x < first[t + 1]
    int hi = tab.count;
    while (hi - t > 1) {
      const int mid = (t + hi) >> 1;
      if (tab.first[mid] <= (int)blockIdx.x) t = mid; else hi = mid;
    }
  }
  for (int c = blockIdx.x; c < pieces; c += gridDim.x) {
    while (c >= tab.first[t + 1]) ++t;      // c < pieces = first[count]: stops at t < count
    unsigned* __restrict__ a = tab.a[t];
    unsigned* __restrict__ b = tab.b[t];
    const unsigned n = tab.n[t], n4 = n & ~3u;
    const unsigned off = (unsigned)(c - tab.first[t]) * kChunk;      // < n < 2^31
    const unsigned i0 = off + 4 * threadIdx.x;                       // < 2^31 + kChunk: no wrap
    if (off + kChunk <= n4) {      // the same in every lane: a whole piece of whole vectors
      u32x4 va[kUnroll], vb[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        va[u] = __builtin_nontemporal_load((const u32x4*)(a + i0 + u * 4 * kThreads));
        vb[u] = __builtin_nontemporal_load((const u32x4*)(b + i0 + u * 4 * kThreads));
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u)
        piece_vec<SWAP>((u32x4*)(a + i0 + u * 4 * kThreads), (u32x4*)(b + i0 + u * 4 * kThreads), va[u], vb[u], alpha);
    } else {                       // the tensor's last piece: every vector guarded, then the n % 4 tail
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const unsigned i = i0 + u * 4 * kThreads;
        if (i < n4) {              // i and n4 are multiples of 4: i + 4 <= n4
          const u32x4 va = __builtin_nontemporal_load((const u32x4*)(a + i));
          const u32x4 vb = __builtin_nontemporal_load((const u32x4*)(b + i));
          piece_vec<SWAP>((u32x4*)(a + i), (u32x4*)(b + i), va, vb, alpha);
        }
      }
      const unsigned i = n4 + threadIdx.x;      // n4 >= off: the tail belongs to this, the last piece
      if (i < n) {
        const unsigned ea = a[i], eb = b[i];
        if constexpr (SWAP) {
          a[i] = eb;
          b[i] = ea;
        } else {
          a[i] = ema_word(ea, eb, alpha);
        }
      }
    }
  }
}

struct Span {
  uintptr_t lo, hi;
  int side, tensor;
};

// 0, or the refusal.  `what_a` / `what_b`: the operands' names in the header
int check_tables(const char* who, const char* what_a, const char* what_b, const void* const* a, const void* const* b,
                 const int64_t* counts, int32_t tensors) {
  DD_REQUIRE(a, DD_ERR_BAD_ARG, "%s: %s is NULL", who, what_a);
  DD_REQUIRE(b, DD_ERR_BAD_ARG, "%s: %s is NULL", who, what_b);
  DD_REQUIRE(counts, DD_ERR_BAD_ARG, "%s: counts is NULL", who);
  DD_REQUIRE(tensors >= 1, DD_ERR_BAD_ARG, "%s: tensors = %d, at least one is needed", who, tensors);
  std::vector<Span> spans;
  spans.reserve(2 * (size_t)tensors);
  for (int t = 0; t < tensors; ++t) {
    DD_REQUIRE(counts[t] >= 1 && counts[t] < (1LL << 31), DD_ERR_BAD_ARG, "%s: counts[%d] = %lld is outside [1, 2^31)", who, t,
               (long long)counts[t]);
    DD_REQUIRE(a[t], DD_ERR_BAD_ARG, "%s: %s[%d] is NULL", who, what_a, t);
    DD_REQUIRE(b[t], DD_ERR_BAD_ARG, "%s: %s[%d] is NULL", who, what_b, t);
    DD_REQUIRE(((uintptr_t)a[t] & 15) == 0, DD_ERR_BAD_ARG, "%s: %s[%d] is not 16-byte aligned", who, what_a, t);
    DD_REQUIRE(((uintptr_t)b[t] & 15) == 0, DD_ERR_BAD_ARG, "%s: %s[%d] is not 16-byte aligned", who, what_b, t);
    const uintptr_t bytes = (uintptr_t)counts[t] * 4;
    spans.push_back({(uintptr_t)a[t], (uintptr_t)a[t] + bytes, 0, t});
    spans.push_back({(uintptr_t)b[t], (uintptr_t)b[t] + bytes, 1, t});
  }
  // no buffer of one table overlaps a buffer of the other: by ascending start, a span that begins in front of the furthest end seen
  // so far on the OTHER side overlaps the span that end belongs to
  std::sort(spans.begin(), spans.end(), [](const Span& x, const Span& y) { return x.lo < y.lo; });
  uintptr_t end[2] = {0, 0};
  int owner[2] = {-1, -1};
  for (const Span& s : spans) {
    const int other = 1 - s.side;
    if (owner[other] >= 0 && s.lo < end[other]) {
      const int ta = s.side == 0 ? s.tensor : owner[other], tb = s.side == 0 ? owner[other] : s.tensor;
      return dd_fail(DD_ERR_BAD_ARG, "%s: %s[%d] overlaps %s[%d]", who, what_a, ta, what_b, tb);
    }
    if (owner[s.side] < 0 || s.hi > end[s.side]) {
      end[s.side] = s.hi;
      owner[s.side] = s.tensor;
    }
  }
  return 0;
}

template <bool SWAP>
int launch_tables(const char* who, void* const* a, void* const* b, const int64_t* counts, int32_t tensors, float alpha,
                  void* stream) {
  for (int32_t base = 0; base < tensors; base += kTableMax) {      // consecutive slices of the table, one launch each
    EmaTable tab;
    tab.count = std::min<int32_t>(kTableMax, tensors - base);
    int pieces = 0;
    for (int i = 0; i < tab.count; ++i) {
      tab.a[i] = (unsigned*)a[base + i];
      tab.b[i] = (unsigned*)b[base + i];
      tab.n[i] = (unsigned)counts[base + i];
      tab.first[i] = pieces;
      pieces += (int)((counts[base + i] + kChunk - 1) / kChunk);      // <= 2^19 each, kTableMax of them
    }
    for (int i = tab.count; i < kTableMax; ++i) {      // never read; kept defined
      tab.a[i] = tab.b[i] = nullptr;
      tab.n[i] = 0;
      tab.first[i + 1] = 0;
    }
    tab.first[tab.count] = pieces;
    const int grid = std::min(pieces, DD_NUM_CU * 8);
    hipLaunchKernelGGL(ema_kernel<SWAP>, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, tab, alpha);
    DD_LAUNCH_CHECK(who);
  }
  return 0;
}

}  // namespace

extern "C" {

int dd_ema_update_ptrs(float* const* ema_ptrs, const float* const* param_ptrs, const int64_t* counts, int32_t tensors, float alpha,
                       void* stream) {
  const int rc = check_tables("ema_update_ptrs", "ema_ptrs", "param_ptrs", (const void* const*)ema_ptrs, (const void* const*)param_ptrs,
                              counts, tensors);
  if (rc) return rc;
  DD_REQUIRE(alpha >= 0.f && alpha <= 1.f, DD_ERR_BAD_ARG, "ema_update_ptrs: alpha = %g is outside [0, 1]", (double)alpha);      // a NaN fails both
  if (alpha == 0.f) return 0;      // every e keeps its bits, whatever w holds (the header): nothing to launch
  return launch_tables<false>("ema_update_ptrs", (void* const*)ema_ptrs, (void* const*)param_ptrs, counts, tensors, alpha, stream);
}

int dd_ema_swap_ptrs(float* const* a_ptrs, float* const* b_ptrs, const int64_t* counts, int32_t tensors, void* stream) {
  const int rc = check_tables("ema_swap_ptrs", "a_ptrs", "b_ptrs", (const void* const*)a_ptrs, (const void* const*)b_ptrs, counts, tensors);
  if (rc) return rc;
  return launch_tables<true>("ema_swap_ptrs", (void* const*)a_ptrs, (void* const*)b_ptrs, counts, tensors, 0.f, stream);
}

}  // extern "C"

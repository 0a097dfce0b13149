// Shared helpers for the gfx950 kernels of the hot path (internal; the public ABI is include/dd_hotpath.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/dd_hotpath.h"
#include "dd_device.h"

#define DD_NUM_CU 256

int dd_fail(int code, const char* fmt, ...);
int dd_adam_blocks_internal();  // persistent workgroups per CU of dd_adam_step / dd_adam_step_rankb: dd_set_adam_blocks_per_cu
int dd_adam_spare_internal();   // compute units dd_adam_step_rankb leaves free of its workgroups: dd_set_adam_spare_cus
int dd_cu_budget_internal();   // compute units the resident-grid (persistent) kernels may fill: dd_set_cu_budget
// Before launching `kernel` with `bytes` of dynamic LDS: raises its limit (64 KB by default) once per kernel and host thread (runtime.hip).
int dd_allow_lds(const void* kernel, size_t bytes);

#define DD_REQUIRE(cond, code, ...)            \
  do {                                         \
    if (!(cond)) return dd_fail(code, __VA_ARGS__); \
  } while (0)

#define DD_LAUNCH_CHECK(what)                                                        \
  do {                                                                               \
    hipError_t e_ = hipGetLastError();                                               \
    if (e_ != hipSuccess) return dd_fail(DD_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e_)); \
  } while (0)

static inline int dd_conv_out(int in, int stride) { return (in + 2 - 3) / stride + 1; }

// grid of a grid-stride kernel of 256 lanes over n items: one lane per item, at most 8 workgroups per compute unit
static inline int dd_grid_for(long n) { return (int)min((n + 255) / 256, (long)DD_NUM_CU * 8); }

// The collate hands a batch over as a TUPLE of per-sample tensors (collate_fn = tuple(zip(*batch)), helper.py:22-23).  Kernels read
// them where they lie through a table of base pointers passed BY VALUE in the kernel arguments (no device-side table, no torch.stack
// copy), 64 samples per launch.
template <typename T>
struct DdPtrTable {
  const T* p[64];
  __device__ const T* sample(int b) const { return p[b]; }
  __device__ long first(int) const { return 0; }      // an entry points at its sample's first element (camera_gather.hip: view)
};

// Walks `batch` pointers in chunks of 64: each chunk's table is filled (unused entries null), its entries checked for null on the
// host ("<who>: null <what> pointer"), and `launch(table, b0, nb)` called for samples b0 .. b0 + nb - 1 (it offsets its outputs by b0 samples), then checked.
template <typename T, typename Launch>
int dd_for_each_chunk(const char* who, const char* what, const T* const* ptrs, int batch, Launch launch) {
  for (int b0 = 0; b0 < batch; b0 += 64) {
    const int nb = min(64, batch - b0);
    DdPtrTable<T> tab;
    for (int i = 0; i < 64; ++i) tab.p[i] = i < nb ? ptrs[b0 + i] : nullptr;
    for (int i = 0; i < nb; ++i) DD_REQUIRE(tab.p[i] != nullptr, DD_ERR_BAD_ARG, "%s: null %s pointer", who, what);
    launch(tab, b0, nb);
    DD_LAUNCH_CHECK(who);
  }
  return 0;
}

// s += p[0] + p[stride] + ... (n terms), left to right -- the order, and so the bits, of the plain loop -- with SIXTEEN loads in flight:
// the second stages of the weight / bias gradients add a few hundred per-workgroup partials per output element, and written as
// `for (w...) s += part[w * stride]` each add waited for its own load: 50-60 us of memory latency per launch for a few KB of output
// (round 5: 0.49 ms of the box-head step in ten such launches).
template <typename Acc>
__device__ __forceinline__ void dd_sum_strided(Acc& s, const float* __restrict__ p, long stride, int n) {
  for (int i = 0; i < n; i += 16) {
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = p[(long)min(i + j, n - 1) * stride];      // unconditional (a guarded load is a branch per load): past the end, the last term again, not added
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (i + j < n) s += (Acc)v[j];
  }
}

// dconv_t.hip: the input-aligned forward of the dilated transposed layers; false = not one of its layers, nothing launched.
bool dd_dconv_desc_ok(const dd_gconv_desc* d);      // dconv.hip: the eligibility test of dd_dconv_fwd, for its two specialised launchers
bool dd_dconv_tfwd_launch(const float* x, const float* packed, const float* bias, float* y, const dd_gconv_desc* d, int epilogue,
                          int wp_bytes, hipStream_t st);
bool dd_dconv_tfwd8_launch(const float* x, const float* packed, const float* bias, float* y, const dd_gconv_desc* d, int epilogue,
                           hipStream_t st);      // dconv_t.hip: up_conv_4's forward, four tap columns per column tile
bool dd_dconv_gfwd_launch(const float* x, const float* packed, const float* bias, const float* mask, float* y, const dd_gconv_desc* d,
                          int epilogue, int wp_bytes, hipStream_t st);
// dconv_m.hip: gather form with several output rows per workgroup (rows that are not a whole number of 8 m-tiles); false = not one of its layers.
bool dd_dconv_mfwd_launch(const float* x, const float* packed, const float* bias, const float* mask, float* y, const dd_gconv_desc* d,
                          int epilogue, int wp_bytes, hipStream_t st);
bool dd_dconv_mfwd_launch_colsum(const float* x, const float* packed, const float* bias, const float* mask, float* y, const dd_gconv_desc* d,
                                 int epilogue, int wp_bytes, hipStream_t st, float* colsum_part);
void dd_dconv_colsum_reduce_launch(const float* part, float* out, int nblocks, int cout, hipStream_t st);
bool dd_dconv_mwin_takes(const dd_gconv_desc* d, int epilogue, bool has_mask, bool has_bias);

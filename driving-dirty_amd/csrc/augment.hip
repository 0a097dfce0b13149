// Train-time augmentation next to the 6-view gather (include/dd_augment.h; csrc/libdd_augment.so, a library of its own):
//   dd_aug_views_u8_ptrs / dd_aug_views_ptrs   left/right mirror of the rig + per-view gain/bias + view blanking -> fp32 [B,6,3,H,W]
//   dd_aug_masks_u8_ptrs                       the road masks under the same mirror (rows reversed)          -> bytes [B,h,w]
// HBM-bound byte shuffling, as camera_gather.hip's gathers: every output byte is written once, 16 bytes per lane for the views.
// The output is cut into groups of four consecutive fp32, so the 16-byte store does not depend on W % 4 (the cameras' W = 306 is
// no multiple of 4): a group may cross a row, and each of its four elements finds its own source.  Two kernels per input type,
// picked by the SHAPE alone (never by an address), both through the one per-element function `augment_value`, so the same bits:
//   H * W % 4 == 0 (the cameras' 256 x 306)  one workgroup column per (sample, view, channel) plane: flags, colour and the source
//                                            plane are wave-uniform (scalar loads), a group never leaves its plane;
//   otherwise                                groups of the FLAT [B,6,3,H,W] array, which may also cross planes, views and samples;
//                                            the last group of an element count that is no multiple of 4 is stored by element.
#include "dd_common.h"

#include "../../include/dd_augment.h"

#pragma clang fp contract(off)      // o = v * gain, THEN o + bias: two roundings, as the header states and the tests' reference computes

namespace {

constexpr int kChunk = 32;                       // samples per launch: 32 x (8 + 4 + 48) = 1920 bytes of kernel arguments
constexpr unsigned kFlagMirror = 1u;
constexpr unsigned kFlagsKnown = kFlagMirror | (0x3Fu << 8);

// pointers, flags and colours of one chunk, passed by value in the kernel arguments: no device-side table, no copy to wait for
struct AugTable {
  const void* p[kChunk];
  unsigned flags[kChunk];
  float color[kChunk][6][2];      // [sample][output view] = (gain, bias)
};

struct MaskTable {
  const unsigned char* p[kChunk];
  unsigned flags[kChunk];
};

__device__ __forceinline__ int mirror_view(int v) { return v + 2 - 2 * (v % 3); }      // {2,1,0,5,4,3}

__device__ __forceinline__ float load_value(const float* p, int v, int c, int y, int x, int H, int W) {
  return p[(((long)v * 3 + c) * H + y) * W + x];
}
__device__ __forceinline__ float load_value(const unsigned char* p, int v, int c, int y, int x, int H, int W) {
  return (float)p[(((long)v * H + y) * W + x) * 3 + c] / 255.0f;      // a true division: ToTensor's, as dd_stitch6_u8
}

// the colour of one value: (1, 0) moves it bit for bit; else two roundings and the clamp
__device__ __forceinline__ float augment_value(float val, float gain, float bias) {
  if (gain == 1.f && bias == 0.f) return val;
  val = val * gain;
  val = val + bias;
  return fminf(fmaxf(val, 0.f), 1.f);
}

// H * W % 4 == 0.  grid (x, 18, nb): blockIdx.z the sample, blockIdx.y the output plane 3 v + c, x strides over the plane's groups.
template <typename SrcT>
__global__ __launch_bounds__(256) void aug_views_plane_kernel(const AugTable t, float* __restrict__ out, int H, int W) {
  const int b = blockIdx.z, v = blockIdx.y / 3, c = blockIdx.y - 3 * v;
  const int plane = H * W, groups = plane / 4;
  const unsigned fl = t.flags[b];
  const bool blank = (fl >> (8 + v)) & 1u, mir = fl & kFlagMirror;
  const float gain = t.color[b][v][0], bias = t.color[b][v][1];
  const SrcT* src = (const SrcT*)t.p[b];
  const int sv = mir ? mirror_view(v) : v;
  f32x4* dst = (f32x4*)(out + ((long)b * 18 + blockIdx.y) * plane);
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (!blank) {      // a blanked view is +0.0f and is not read
      int y = (4 * g) / W, x = 4 * g - y * W;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] = augment_value(load_value(src, sv, c, y, mir ? W - 1 - x : x, H, W), gain, bias);
        if (++x == W) { x = 0; ++y; }      // y == H only behind the plane's last element, which ends a group
      }
    }
    dst[g] = f32x4{o[0], o[1], o[2], o[3]};
  }
}

template <typename SrcT>
__global__ __launch_bounds__(256) void aug_views_kernel(const AugTable t, float* __restrict__ out, int nb, int H, int W) {
  const int per_sample = 18 * H * W;
  const long total = (long)nb * per_sample;
  const long groups = (total + 3) / 4;
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
    const long i0 = 4 * g;
    const int n = (int)min(4L, total - i0);
    int b = (int)(i0 / per_sample);
    int r = (int)(i0 - (long)b * per_sample);
    int x = r % W; r /= W;
    int y = r % H; r /= H;
    int c = r % 3, v = r / 3;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < n) {
        const unsigned fl = t.flags[b];
        if (!((fl >> (8 + v)) & 1u)) {      // a blanked view is +0.0f and is not read
          const bool mir = fl & kFlagMirror;
          o[j] = augment_value(load_value((const SrcT*)t.p[b], mir ? mirror_view(v) : v, c, y, mir ? W - 1 - x : x, H, W),
                               t.color[b][v][0], t.color[b][v][1]);
        }
        if (++x == W) {
          x = 0;
          if (++y == H) {
            y = 0;
            if (++c == 3) {
              c = 0;
              if (++v == 6) { v = 0; ++b; }
            }
          }
        }
      }
    }
    if (n == 4) {
      *(f32x4*)(out + i0) = f32x4{o[0], o[1], o[2], o[3]};
    } else {      // the last group of an element count that is no multiple of 4
      for (int j = 0; j < n; ++j) out[i0 + j] = o[j];
    }
  }
}

// four output bytes per lane, one 4-byte store; the source row is the mirrored one.  Where the four bytes lie in one row and the
// source address allows, one 4-byte load; else byte loads: the same bytes either way.
__global__ __launch_bounds__(256) void aug_masks_kernel(const MaskTable t, unsigned char* __restrict__ out, int nb, int h, int w) {
  const int per_sample = h * w;
  const long total = (long)nb * per_sample;
  const long groups = (total + 3) / 4;
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
    const long i0 = 4 * g;
    const int n = (int)min(4L, total - i0);
    int b = (int)(i0 / per_sample);
    int r = (int)(i0 - (long)b * per_sample);
    int x = r % w, y = r / w;
    if (n == 4 && x + 3 < w) {
      const unsigned char* src = t.p[b] + (long)((t.flags[b] & kFlagMirror) ? h - 1 - y : y) * w + x;
      if (((unsigned long)src & 3) == 0) {
        *(unsigned*)(out + i0) = *(const unsigned*)src;
        continue;
      }
    }
    unsigned word = 0;
    for (int j = 0; j < n; ++j) {
      const unsigned char byte = t.p[b][(long)((t.flags[b] & kFlagMirror) ? h - 1 - y : y) * w + x];
      word |= (unsigned)byte << (8 * j);
      if (++x == w) {
        x = 0;
        if (++y == h) { y = 0; ++b; }
      }
    }
    if (n == 4) {
      *(unsigned*)(out + i0) = word;
    } else {
      for (int j = 0; j < n; ++j) out[i0 + j] = (unsigned char)(word >> (8 * j));
    }
  }
}

int check_flags(const char* who, const uint32_t* flags, int batch) {
  for (int i = 0; i < batch; ++i)
    DD_REQUIRE((flags[i] & ~kFlagsKnown) == 0, DD_ERR_BAD_ARG, "%s: flags[%d] = 0x%x has a bit that means nothing (bit 0: mirror, bits 8..13: blank a view)",
               who, i, flags[i]);
  return 0;
}

template <typename SrcT>
int launch_views(const char* who, const SrcT* const* sample_ptrs, const uint32_t* flags, const float* color, float* out, int batch,
                 int height, int width, void* stream) {
  DD_REQUIRE(sample_ptrs && flags && color && out, DD_ERR_BAD_ARG, "%s: NULL pointer", who);
  DD_REQUIRE(batch > 0 && height > 0 && width > 0, DD_ERR_BAD_ARG, "%s: non-positive size (batch %d, %d x %d)", who, batch, height, width);
  DD_REQUIRE(18L * height * width < (1L << 31), DD_ERR_UNSUPPORTED, "%s: %d x %d views are too large (18 * H * W must stay below 2^31)", who,
             height, width);
  DD_REQUIRE(((uintptr_t)out & 15) == 0, DD_ERR_BAD_ARG, "%s: out must be 16-byte aligned", who);
  if (int rc = check_flags(who, flags, batch)) return rc;
  for (int i = 0; i < batch; ++i) {
    DD_REQUIRE(sample_ptrs[i] != nullptr, DD_ERR_BAD_ARG, "%s: null sample pointer", who);
    DD_REQUIRE(((uintptr_t)sample_ptrs[i] & (sizeof(SrcT) - 1)) == 0, DD_ERR_BAD_ARG, "%s: sample %d is not aligned to its element", who, i);
  }
  const long per_sample = 18L * height * width;
  for (int b0 = 0; b0 < batch; b0 += kChunk) {      // kChunk x per_sample x 4 bytes is a multiple of 16: every chunk's output stays aligned
    const int nb = min(kChunk, batch - b0);
    AugTable tab;
    for (int i = 0; i < kChunk; ++i) {
      const int s = b0 + min(i, nb - 1);      // past the chunk's end: the last sample again, never read
      tab.p[i] = sample_ptrs[s];
      tab.flags[i] = flags[s];
      for (int k = 0; k < 12; ++k) tab.color[i][k / 2][k % 2] = color[(long)s * 12 + k];
    }
    if ((height * width) % 4 == 0) {      // by the shape alone: the two kernels compute every element by the same function
      const int groups = height * width / 4;
      hipLaunchKernelGGL(aug_views_plane_kernel<SrcT>, dim3(min((groups + 255) / 256, 32), 18, nb), dim3(256), 0, (hipStream_t)stream,
                         tab, out + b0 * per_sample, height, width);
    } else {
      hipLaunchKernelGGL(aug_views_kernel<SrcT>, dim3(dd_grid_for((nb * per_sample + 3) / 4)), dim3(256), 0, (hipStream_t)stream, tab,
                         out + b0 * per_sample, nb, height, width);
    }
    DD_LAUNCH_CHECK(who);
  }
  return 0;
}

}  // namespace

extern "C" {

int dd_aug_views_u8_ptrs(const unsigned char* const* sample_ptrs, const uint32_t* flags, const float* color, float* out,
                         int32_t batch, int32_t height, int32_t width, void* stream) {
  return launch_views<unsigned char>("aug_views_u8_ptrs", sample_ptrs, flags, color, out, batch, height, width, stream);
}

int dd_aug_views_ptrs(const float* const* sample_ptrs, const uint32_t* flags, const float* color, float* out, int32_t batch,
                      int32_t height, int32_t width, void* stream) {
  return launch_views<float>("aug_views_ptrs", sample_ptrs, flags, color, out, batch, height, width, stream);
}

int dd_aug_masks_u8_ptrs(const unsigned char* const* mask_ptrs, const uint32_t* flags, unsigned char* out, int32_t batch, int32_t h,
                         int32_t w, void* stream) {
  const char* who = "aug_masks_u8_ptrs";
  DD_REQUIRE(mask_ptrs && flags && out, DD_ERR_BAD_ARG, "%s: NULL pointer", who);
  DD_REQUIRE(batch > 0 && h > 0 && w > 0, DD_ERR_BAD_ARG, "%s: non-positive size (batch %d, %d x %d)", who, batch, h, w);
  DD_REQUIRE((long)h * w < (1L << 31), DD_ERR_UNSUPPORTED, "%s: %d x %d masks are too large (h * w must stay below 2^31)", who, h, w);
  DD_REQUIRE(((uintptr_t)out & 15) == 0, DD_ERR_BAD_ARG, "%s: out must be 16-byte aligned", who);
  if (int rc = check_flags(who, flags, batch)) return rc;
  for (int i = 0; i < batch; ++i) DD_REQUIRE(mask_ptrs[i] != nullptr, DD_ERR_BAD_ARG, "%s: null mask pointer", who);
  const long per_sample = (long)h * w;
  for (int b0 = 0; b0 < batch; b0 += kChunk) {      // kChunk x per_sample bytes is a multiple of 4: every chunk's 4-byte stores stay aligned
    const int nb = min(kChunk, batch - b0);
    MaskTable tab;
    for (int i = 0; i < kChunk; ++i) {
      const int s = b0 + min(i, nb - 1);
      tab.p[i] = mask_ptrs[s];
      tab.flags[i] = flags[s];
    }
    hipLaunchKernelGGL(aug_masks_kernel, dim3(dd_grid_for((nb * per_sample + 3) / 4)), dim3(256), 0, (hipStream_t)stream, tab,
                       out + b0 * per_sample, nb, h, w);
    DD_LAUNCH_CHECK(who);
  }
  return 0;
}

}  // extern "C"

// What the data pipeline hands over -> the NHWC4 image the conv kernels read, one thread per output pixel (HBM-bound byte shuffling:
// 12 or 3 bytes in, 16 or 8 bytes out).  The facts about the input format are stated here once:
//   input   fp32 views [6,3,H,W] per sample (autoencoder.py:53-57) or uint8 frames [6,H,W,3] as a JPEG decoder emits them, with
//           ToTensor's /255 (data_helper.py:63-68) fused in; a stacked batch or the collate's tuple (DdPtrTable, dd_common.h)
//   output  the wide six-view image in the order of wide_stitch_six_images (roadmap_bce_v2.py:53-64), fp32 or bf16, with the
//           masked-view task of BasicAE.six_to_one_task (autoencoder.py:59-73) optional; or one view with SpatialMappingCNN's
//           rot90 / flip applied
#include "dd_common.h"

namespace {

__constant__ int kViewOrder[6] = {0, 1, 2, 5, 4, 3};

// ---- where a sample's six views start: view `first(b) + view` of what `sample(b)` points at.  A stacked batch is one run of B x 6
// views; an entry of the collate's tuple (DdPtrTable) points at the sample itself.
template <typename T>
struct DenseBatch {
  const T* __restrict__ base;
  __device__ const T* sample(int) const { return base; }
  __device__ long first(int b) const { return (long)b * 6; }
};

// ---- the pixel source: the three values of pixel (y, x) of view `view` of sample b
struct Rgb {
  float c0, c1, c2;
};
template <typename T, template <typename> class Batch>
struct Pixels;

template <template <typename> class Batch>
struct Pixels<float, Batch> {      // fp32 planar [6,3,H,W]: three planes, each coalesced along x
  Batch<float> batch;
  __device__ Rgb load(int b, int view, int y, int x, int H, int W) const {
    const long plane = (long)H * W;
    const float* src = batch.sample(b) + ((batch.first(b) + view) * 3) * plane + (long)y * W + x;
    return Rgb{src[0], src[plane], src[2 * plane]};
  }
};

template <template <typename> class Batch>
struct Pixels<unsigned char, Batch> {      // uint8 [6,H,W,3]
  Batch<unsigned char> batch;
  __device__ Rgb load(int b, int view, int y, int x, int H, int W) const {
    const unsigned char* src = batch.sample(b) + (((batch.first(b) + view) * H + y) * W + x) * 3;
    // a true division, correctly rounded: bit for bit ToTensor's img.float().div(255) (x * (1/255.f) differs in the last place for
    // some of the 256 values)
    return Rgb{(float)src[0] / 255.0f, (float)src[1] / 255.0f, (float)src[2] / 255.0f};
  }
};

// ---- the store of wide-image pixel p = (b, y, xw): `make` turns the three values into the stored pixel (all zero bits = a blanked
// pixel in every format), `put` writes it.  `from(px)`: the same outputs px pixels on, a chunk's on the host.
struct StoreNhwc4 {      // NHWC4 fp32
  f32x4* __restrict__ nhwc4;
  static __device__ f32x4 make(Rgb v) { return f32x4{v.c0, v.c1, v.c2, 0.f}; }
  __device__ void put(long p, int, int, int, int, int, f32x4 v) const { nhwc4[p] = v; }
  StoreNhwc4 from(long px) const { return StoreNhwc4{nhwc4 + px}; }
};

struct StoreF32 {      // dd_stitch6's: NHWC4 and / or NCHW [B,3,H,6W] fp32; either may be null
  f32x4* __restrict__ nhwc4;
  float* __restrict__ nchw;
  static __device__ f32x4 make(Rgb v) { return f32x4{v.c0, v.c1, v.c2, 0.f}; }
  __device__ void put(long p, int b, int y, int xw, int H, int W6, f32x4 v) const {
    if (nhwc4) nhwc4[p] = v;
    if (nchw) {
      float* o = nchw + ((long)b * 3) * H * W6 + (long)y * W6 + xw;
      o[0] = v.x; o[(long)H * W6] = v.y; o[2L * H * W6] = v.z;
    }
  }
  StoreF32 from(long px) const { return StoreF32{nhwc4 ? nhwc4 + px : nullptr, nchw ? nchw + 3 * px : nullptr}; }
};

struct StoreBf16 {      // NHWC4 bf16: the one rounding, in dd_pack_bf16
  u32x2* __restrict__ nhwc4;
  static __device__ u32x2 make(Rgb v) { return u32x2{dd_pack_bf16(v.c0, v.c1), dd_pack_bf16(v.c2, 0.f)}; }
  __device__ void put(long p, int, int, int, int, int, u32x2 v) const { nhwc4[p] = v; }
  StoreBf16 from(long px) const { return StoreBf16{nhwc4 + px}; }
};

// ---- the wide image.  Wide slot `mask_slot` (-1: none) is blanked and, when `target` is given, its fp32 values -- before any rounding
// of the store, so the same bits in both precisions -- go to `target` [B,3,H,W].  MASK: whether the entry point has a masked view at
// all; where it has (every entry but dd_stitch6_ptrs and dd_stitch6_u8), mask_slot and target are run-time arguments.
template <bool MASK, typename Src, typename Store>
__global__ __launch_bounds__(256) void wide_image_kernel(const Src src, const Store out, float* __restrict__ target, int B, int H, int W,
                                                         int mask_slot) {
  const long npx = (long)B * H * 6 * W;
  const long plane = (long)H * W;
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < npx; p += (long)gridDim.x * blockDim.x) {
    const int xw = (int)(p % (6 * W));
    const int yy = (int)((p / (6 * W)) % H);
    const int b = (int)(p / ((long)6 * W * H));
    const int slot = xw / W, xx = xw - slot * W;
    const Rgb v = src.load(b, kViewOrder[slot], yy, xx, H, W);
    auto px = Store::make(v);
    if (MASK && slot == mask_slot) {
      if (target) {
        float* t = target + ((long)b * 3) * plane + (long)yy * W + xx;
        t[0] = v.c0; t[plane] = v.c1; t[2 * plane] = v.c2;
      }
      px = decltype(px){};
    }
    out.put(p, b, yy, xw, H, 6 * W, px);
  }
}

// ---- one view as NHWC4 fp32 with transform tf: 0 as it is, 1 rot90(k=1, dims [2,3]), 2 rot90(k=1, dims [3,2]), 3 flip([2,3])
template <typename Src>
__global__ __launch_bounds__(256) void single_view_kernel(const Src src, f32x4* __restrict__ out, int B, int H, int W, int view, int tf) {
  const int Ho = (tf == 1 || tf == 2) ? W : H, Wo = (tf == 1 || tf == 2) ? H : W;
  const long total = (long)B * Ho * Wo;
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const int j = (int)(p % Wo), i = (int)((p / Wo) % Ho);
    const int b = (int)(p / ((long)Wo * Ho));
    int ys, xs;
    if (tf == 0) { ys = i; xs = j; }
    else if (tf == 1) { ys = j; xs = W - 1 - i; }         // out[i][j] = in[j][W-1-i]
    else if (tf == 2) { ys = H - 1 - j; xs = i; }         // out[i][j] = in[H-1-j][i]
    else { ys = H - 1 - i; xs = W - 1 - j; }
    const Rgb v = src.load(b, view, ys, xs, H, W);
    out[p] = f32x4{v.c0, v.c1, v.c2, 0.f};
  }
}

// ---- host side: argument checks shared by the entry points of a kind, then one launch (stacked batch) or one per chunk (tuple)
template <bool MASK, typename Src, typename Store>
void launch_wide(Src src, Store out, float* target, int nb, int H, int W, int mask_slot, void* stream) {
  hipLaunchKernelGGL((wide_image_kernel<MASK, Src, Store>), dim3(dd_grid_for((long)nb * H * 6 * W)), dim3(256), 0, (hipStream_t)stream, src, out, target,
                     nb, H, W, mask_slot);
}

template <bool MASK = true, typename T, typename Store>
int wide_dense(const char* who, const T* views, Store out, bool has_out, float* target, int batch, int H, int W, int mask_slot, void* stream) {
  DD_REQUIRE(views && has_out && batch > 0 && H > 0 && W > 0, DD_ERR_BAD_ARG, "%s: bad argument", who);
  DD_REQUIRE(mask_slot >= -1 && mask_slot < 6, DD_ERR_BAD_ARG, "%s: mask_slot %d", who, mask_slot);
  launch_wide<MASK>(Pixels<T, DenseBatch>{{views}}, out, target, batch, H, W, mask_slot, stream);
  DD_LAUNCH_CHECK(who);
  return 0;
}

template <bool MASK = true, typename T, typename Store>
int wide_ptrs(const char* who, const T* const* sample_ptrs, Store out, bool has_out, float* target, int batch, int H, int W, int mask_slot,
              void* stream) {
  DD_REQUIRE(sample_ptrs && has_out && batch > 0 && H > 0 && W > 0, DD_ERR_BAD_ARG, "%s: bad argument", who);
  DD_REQUIRE(mask_slot >= -1 && mask_slot < 6, DD_ERR_BAD_ARG, "%s: mask_slot %d", who, mask_slot);
  return dd_for_each_chunk(who, "sample", sample_ptrs, batch, [&](const DdPtrTable<T>& tab, int b0, int nb) {
    launch_wide<MASK>(Pixels<T, DdPtrTable>{tab}, out.from((long)b0 * H * 6 * W), target ? target + (long)b0 * 3 * H * W : nullptr, nb, H, W, mask_slot,
                stream);
  });
}

template <typename Src>
void launch_view(Src src, float* out, int nb, int H, int W, int view, int transform, void* stream) {
  hipLaunchKernelGGL(single_view_kernel<Src>, dim3(dd_grid_for((long)nb * H * W)), dim3(256), 0, (hipStream_t)stream, src, (f32x4*)out, nb, H, W,
                     view, transform);
}

int view_args(const char* who, const void* src, const float* out, int batch, int H, int W, int view, int transform) {
  DD_REQUIRE(src && out && batch > 0 && H > 0 && W > 0, DD_ERR_BAD_ARG, "%s: bad argument", who);
  DD_REQUIRE(view >= 0 && view < 6 && transform >= 0 && transform <= 3, DD_ERR_BAD_ARG, "%s: view %d transform %d", who, view, transform);
  return 0;
}

template <typename T>
int view_ptrs(const char* who, const T* const* sample_ptrs, float* out, int batch, int H, int W, int view, int transform, void* stream) {
  if (int rc = view_args(who, sample_ptrs, out, batch, H, W, view, transform)) return rc;
  return dd_for_each_chunk(who, "sample", sample_ptrs, batch, [&](const DdPtrTable<T>& tab, int b0, int nb) {
    launch_view(Pixels<T, DdPtrTable>{tab}, out + (long)b0 * H * W * 4, nb, H, W, view, transform, stream);
  });
}

}  // namespace

extern "C" {

int dd_stitch6(const float* views, float* wide_nhwc4, float* wide_nchw, float* target, int32_t batch, int32_t height, int32_t width,
               int32_t mask_slot, void* stream) {
  DD_REQUIRE(views && (wide_nhwc4 || wide_nchw), DD_ERR_BAD_ARG, "stitch6: NULL pointer");
  DD_REQUIRE(batch > 0 && height > 0 && width > 0, DD_ERR_BAD_ARG, "stitch6: non-positive size");
  return wide_dense("stitch6", views, StoreF32{(f32x4*)wide_nhwc4, wide_nchw}, wide_nhwc4 || wide_nchw, target, batch, height, width, mask_slot,
                    stream);
}

int dd_stitch6_ptrs(const float* const* sample_ptrs, float* wide_nhwc4, int32_t batch, int32_t height, int32_t width, void* stream) {
  return wide_ptrs<false>("stitch6_ptrs", sample_ptrs, StoreNhwc4{(f32x4*)wide_nhwc4}, wide_nhwc4, nullptr, batch, height, width, -1, stream);
}

int dd_stitch6_u8(const unsigned char* frames, float* wide_nhwc4, int32_t batch, int32_t height, int32_t width, void* stream) {
  return wide_dense<false>("stitch6_u8", frames, StoreNhwc4{(f32x4*)wide_nhwc4}, wide_nhwc4, nullptr, batch, height, width, -1, stream);
}

int dd_stitch6_u8_ptrs(const unsigned char* const* sample_ptrs, float* wide_nhwc4, float* target, int32_t batch, int32_t height,
                       int32_t width, int32_t mask_slot, void* stream) {
  return wide_ptrs("stitch6_u8_ptrs", sample_ptrs, StoreNhwc4{(f32x4*)wide_nhwc4}, wide_nhwc4, target, batch, height, width, mask_slot,
                   stream);
}

int dd_stitch6_bf16_masked(const float* views, uint16_t* wide_nhwc4, float* target, int32_t batch, int32_t height, int32_t width,
                           int32_t mask_slot, void* stream) {
  return wide_dense("stitch6_bf16", views, StoreBf16{(u32x2*)wide_nhwc4}, wide_nhwc4, target, batch, height, width, mask_slot, stream);
}

int dd_stitch6_bf16(const float* views, uint16_t* wide_nhwc4, int32_t batch, int32_t height, int32_t width, void* stream) {
  return dd_stitch6_bf16_masked(views, wide_nhwc4, nullptr, batch, height, width, -1, stream);
}

int dd_stitch6_bf16_ptrs_masked(const float* const* sample_ptrs, uint16_t* wide_nhwc4, float* target, int32_t batch, int32_t height,
                                int32_t width, int32_t mask_slot, void* stream) {
  return wide_ptrs("stitch6_bf16_ptrs", sample_ptrs, StoreBf16{(u32x2*)wide_nhwc4}, wide_nhwc4, target, batch, height, width, mask_slot, stream);
}

int dd_stitch6_bf16_ptrs(const float* const* sample_ptrs, uint16_t* wide_nhwc4, int32_t batch, int32_t height, int32_t width,
                         void* stream) {
  return dd_stitch6_bf16_ptrs_masked(sample_ptrs, wide_nhwc4, nullptr, batch, height, width, -1, stream);
}

int dd_stitch6_bf16_u8_ptrs_masked(const unsigned char* const* sample_ptrs, uint16_t* wide_nhwc4, float* target, int32_t batch,
                                   int32_t height, int32_t width, int32_t mask_slot, void* stream) {
  return wide_ptrs("stitch6_bf16_u8_ptrs", sample_ptrs, StoreBf16{(u32x2*)wide_nhwc4}, wide_nhwc4, target, batch, height, width, mask_slot, stream);
}

int dd_stitch6_bf16_u8_ptrs(const unsigned char* const* sample_ptrs, uint16_t* wide_nhwc4, int32_t batch, int32_t height, int32_t width,
                            void* stream) {
  return dd_stitch6_bf16_u8_ptrs_masked(sample_ptrs, wide_nhwc4, nullptr, batch, height, width, -1, stream);
}

int dd_view_to_nhwc4(const float* views, float* out, int32_t batch, int32_t height, int32_t width, int32_t view, int32_t transform,
                     void* stream) {
  if (int rc = view_args("view_to_nhwc4", views, out, batch, height, width, view, transform)) return rc;
  launch_view(Pixels<float, DenseBatch>{{views}}, out, batch, height, width, view, transform, stream);
  DD_LAUNCH_CHECK("view_to_nhwc4");
  return 0;
}

int dd_view_to_nhwc4_ptrs(const float* const* sample_ptrs, float* out, int32_t batch, int32_t height, int32_t width, int32_t view,
                          int32_t transform, void* stream) {
  return view_ptrs("view_to_nhwc4_ptrs", sample_ptrs, out, batch, height, width, view, transform, stream);
}

int dd_view_to_nhwc4_u8_ptrs(const unsigned char* const* sample_ptrs, float* out, int32_t batch, int32_t height, int32_t width,
                             int32_t view, int32_t transform, void* stream) {
  return view_ptrs("view_to_nhwc4_u8_ptrs", sample_ptrs, out, batch, height, width, view, transform, stream);
}

}  // extern "C"

/* dd_augment.h -- C ABI of the train-time augmentation library (csrc/libdd_augment.so): the label-preserving left/right mirror
 * of the six-camera rig, per-view exposure jitter and view blanking, applied on the device next to the 6-view gather.
 *
 * An extension library of its own: include/dd_hotpath.h (DD_ABI_VERSION 4) is not touched by it.  The conventions are that
 * header's: plain pointers, sizes as int32, `stream` a hipStream_t passed as void* last, no allocation, no host synchronisation,
 * 0 on success and a DD_ERR_* code of dd_hotpath.h otherwise, the message through libdd_hotpath.so's dd_last_error() (this library
 * links against it).  Every declaration here is a launch function.
 *
 * All three are "ptrs" forms: `sample_ptrs` / `mask_ptrs` is a HOST array of `batch` DEVICE pointers, one per sample (a stacked
 * tensor is B such pointers too).  `flags` and `color` are HOST arrays; they travel, with the pointers, in the kernel arguments,
 * the batch cut into chunks of 32 samples (augment.CHUNK) by the launcher.  Any batch > 0 is served.
 *
 * flags[b]   bit 0: mirror sample b.  bit 8 + v: blank OUTPUT view v (all +0.0f).  Any other bit: refused (DD_ERR_BAD_ARG).
 * mirror     out[b,v,c,y,x] = in[b,M[v],c,y,W-1-x], M = {2,1,0,5,4,3}: front-left <-> front-right, back-left <-> back-right
 *            (data_helper.py:16-23), every frame reversed left to right.  Without the bit: M the identity, x as it is.
 * color      color[(b * 6 + v) * 2 + {0,1}] = (gain, bias) of OUTPUT view v.  gain == 1 && bias == 0: the value is moved bit for
 *            bit, no clamp.  Otherwise o = v * gain (rounded), o = o + bias (rounded), o = fminf(fmaxf(o, 0), 1).
 *            For uint8 input the value v is (float)byte / 255.0f, a true division (as dd_stitch6_u8).
 */
#ifndef DD_AUGMENT_H
#define DD_AUGMENT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per-sample uint8 frames [6,H,W,3] (any alignment) -> out fp32 [B,6,3,H,W] (16-byte aligned).  18 * H * W < 2^31. */
int dd_aug_views_u8_ptrs(const unsigned char* const* sample_ptrs, const uint32_t* flags, const float* color, float* out,
                         int32_t batch, int32_t height, int32_t width, void* stream);

/* The same from per-sample fp32 views [6,3,H,W] (4-byte aligned). */
int dd_aug_views_ptrs(const float* const* sample_ptrs, const uint32_t* flags, const float* color, float* out, int32_t batch,
                      int32_t height, int32_t width, void* stream);

/* Per-sample road masks [h,w] bytes (bool or uint8, any alignment) -> out bytes [B,h,w] (16-byte aligned), copied as they are.
 * Under the mirror row r <-> h-1-r: the bird's-eye frame has x forward along the columns and y to the LEFT along the rows
 * (helper.py:25-31).  Only bit 0 of flags[b] is read; the other bits are checked as above.  h * w < 2^31. */
int dd_aug_masks_u8_ptrs(const unsigned char* const* mask_ptrs, const uint32_t* flags, unsigned char* out, int32_t batch, int32_t h,
                         int32_t w, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DD_AUGMENT_H */

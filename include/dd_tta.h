/* dd_tta.h -- C ABI of the test-time averaging library (csrc/libdd_tta.so): the mean of a prediction made from the scene and of
 * the prediction made from its left/right mirror (dd_augment.h), reflected back, in one pass on the device.
 *
 * An extension library of its own, as dd_augment.h: include/dd_hotpath.h (DD_ABI_VERSION 4) and include/dd_augment.h are not
 * touched by it.  The conventions are dd_hotpath.h's: plain device pointers, sizes as int32, `stream` a hipStream_t passed as void*
 * last, no allocation, no host synchronisation, 0 on success and a DD_ERR_* code of dd_hotpath.h otherwise, the message through
 * libdd_hotpath.so's dd_last_error() (this library links against it).  Every declaration here is a launch function.
 *
 * THE SEMANTICS, stated once.  `a` (from the scene) and `m` (from the mirrored scene) are fp32 [batch,h,w]:
 *
 *     mean[b,r,c] = 0.5f * ( P(a[b,r,c]) + P(m[b,h-1-r,c]) )
 *
 * from_logits 0: P is the identity.  from_logits 1: P is the `sig` of dd_sigmoid_softplus (csrc/dd_device.h), the bits dd_sigmoid,
 * the BCE pass and dd_linear_sigmoid_gt produce.  Any other value is refused.  The sum is ONE rounded fp32 add (never fused with
 * the product inside P), the halving is exact.  The rows reverse because the bird's-eye frame has y to the left along the rows: the
 * reversal dd_aug_masks_u8_ptrs applies to a mirrored sample's road mask.  With an odd h the middle row pairs with itself.
 *
 * Operands: `a`, `m` and `out` are each 16-byte aligned (every torch allocation is); `out` overlaps neither `a` nor `m` (the row
 * reversal makes an in-place call wrong).  batch, h, w > 0 and batch * h * w < 2^31; any such shape is served.  The kernel is picked
 * by the shape alone (w % 16, w % 4), never by an address; every kernel computes an element by the same function.
 */
#ifndef DD_TTA_H
#define DD_TTA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* out fp32 [batch,h,w] = mean. */
int dd_tta_mean_prob(const float* a, const float* m, float* out, int32_t batch, int32_t h, int32_t w, int32_t from_logits,
                     void* stream);

/* out bytes [batch,h,w] = (mean > tau) as 0 / 1, strictly, tau as the fp32 it is handed as; a NaN mean is 0.  Neither the
 * probabilities nor the mean are written anywhere. */
int dd_tta_mean_gt(const float* a, const float* m, float tau, unsigned char* out, int32_t batch, int32_t h, int32_t w,
                   int32_t from_logits, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DD_TTA_H */

/* dd_ema.h -- C ABI of the weight-averaging library (csrc/libdd_ema.so): an exponential moving average (EMA) of a model's
 * parameters kept on the device, and the in-place exchange of the parameters with it.
 *
 * An extension library of its own, as dd_augment.h and dd_tta.h: include/dd_hotpath.h (DD_ABI_VERSION 4), include/dd_augment.h and
 * include/dd_tta.h are not touched by it.  The conventions are dd_hotpath.h's: plain device pointers, `stream` a hipStream_t passed
 * as void* last, no allocation, no host synchronisation, 0 on success and a DD_ERR_* code of dd_hotpath.h otherwise, the message
 * through libdd_hotpath.so's dd_last_error() (this library links against it).  Every declaration here is a launch function.
 *
 * Both are "ptrs" forms, as dd_aug_*_ptrs: `*_ptrs` are HOST arrays of `tensors` DEVICE pointers, `counts` a HOST array of
 * `tensors` element counts; tensor t of one table pairs with tensor t of the other and both have counts[t] fp32 elements.  The host
 * arrays are read before the function returns.
 *
 * THE SEMANTICS, stated once.
 *
 * UPDATE.  For every element, with e the average and w the parameter:
 *
 *     d  = w - e                 one rounded fp32 subtract
 *     e' = fmaf(alpha, d, e)     ONE rounding: the product is never rounded on its own
 *
 * `alpha` is the fp32 it is handed as and lies in [0, 1]; NaN or a value outside is refused.  Where d == 0 (e == w, signed zeros
 * included) e keeps its bits.  alpha == 0 leaves every e with the same bits, whatever w holds: the operands are checked and nothing
 * is launched.  Otherwise a NaN or an infinity in w reaches e' at that element and at no other.  w is never written.  Against the
 * exact e + alpha (w - e) an element errs by at most 1.5 * 2^-23 * max(|e|, |w|): 2^-24 |w - e| from the subtract, which alpha <= 1
 * does not grow, and 2^-24 |e'| from the fused multiply-add.
 *
 * SWAP.  The buffers a[t] and b[t] exchange their contents as 32-bit words: NaN payloads, signed zeros and denormals are
 * preserved, and two calls are the identity.
 *
 * OPERANDS.  tensors >= 1; every pointer non-NULL and 16-byte aligned (every torch allocation is) -- anything else is refused, and
 * the kernel is never picked by an address; every count >= 1 and < 2^31; no buffer of one table overlaps a buffer of the other.
 *
 * THE LAUNCHES.  The work is a flat list of pieces of DD_EMA_CHUNK elements across all tensors of a launch (a tensor's last piece
 * may be shorter), so a 120 M-element weight and a 16-element bias share one launch without imbalance; a capped grid strides over
 * the list.  The table travels in the kernel arguments, DD_EMA_TABLE_MAX tensors at most: a longer table is split into consecutive
 * slices of DD_EMA_TABLE_MAX tensors, one launch each, in table order on `stream`.  That is also how no launch indexes past int32:
 * a tensor has fewer than 2^31 / DD_EMA_CHUNK = 2^19 + 1 pieces, a launch therefore fewer than 2^26 (the piece index is an int32),
 * and an element is addressed by its offset inside its own tensor, below 2^31 + DD_EMA_CHUNK, held as an unsigned 32-bit number.
 */
#ifndef DD_EMA_H
#define DD_EMA_H

#include <stdint.h>

#define DD_EMA_CHUNK 4096     /* elements per piece: 256 lanes x 4 vectors of 16 bytes */
#define DD_EMA_TABLE_MAX 96   /* tensors per launch */

#ifdef __cplusplus
extern "C" {
#endif

/* ema_ptrs[t][i] = fmaf(alpha, param_ptrs[t][i] - ema_ptrs[t][i], ema_ptrs[t][i]) for i < counts[t], t < tensors. */
int dd_ema_update_ptrs(float* const* ema_ptrs, const float* const* param_ptrs, const int64_t* counts, int32_t tensors, float alpha,
                       void* stream);

/* a_ptrs[t][0 .. counts[t]) <-> b_ptrs[t][0 .. counts[t]) as 32-bit words, t < tensors. */
int dd_ema_swap_ptrs(float* const* a_ptrs, float* const* b_ptrs, const int64_t* counts, int32_t tensors, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DD_EMA_H */

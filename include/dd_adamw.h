/* dd_adamw.h -- C ABI of the decoupled-weight-decay library (csrc/libdd_adamw.so): torch.optim.AdamW's step as a mode of the
 * streaming Adam passes of dd_hotpath.h, and the pre-scale for the tensors whose update is dd_adam_step_rankb.
 *
 * An extension library of its own, as dd_augment.h, dd_tta.h, dd_ema.h and dd_rm_loss.h: include/dd_hotpath.h (DD_ABI_VERSION 4)
 * and the four other extension headers are not touched by it.  The conventions are dd_hotpath.h's: plain device pointers, `stream` a
 * hipStream_t passed as void* last, no allocation, no host synchronisation, 0 on success and a DD_ERR_* code of dd_hotpath.h
 * otherwise, the message through libdd_hotpath.so's dd_last_error() (this library links against it).  Every declaration here is a
 * launch function.  `dd_adam_tensor` is dd_hotpath.h's struct; no struct is added.
 *
 * THE SEMANTICS, stated once.  Per element of a decayed tensor
 *
 *     p1 = p * keep              ONE fp32 multiply, one rounding, never contracted into what follows
 *     (p', m', v') = the Adam element of csrc/dd_adam.h (adam_elem2 / adam_elem) on (p1, g, m, v), unchanged
 *
 * with keep = (float)(1.0 - (double)lr * (double)weight_decay), computed by the CALLER on the host in double and handed over as one
 * fp32.  That is torch.optim.AdamW's `param.mul_(1 - lr * weight_decay)` followed by its Adam update: with zero gradients and zero
 * moments one step gives p * keep bit for bit.  What follows from it:
 *
 *   - the decay is DECOUPLED: m and v never see it, they are the bits dd_adam_step gives for the same (g, m, v);
 *   - keep == 1.0f leaves p1's bits equal to p's (a signalling NaN alone is quieted), so the step is dd_adam_step's bit for bit;
 *   - dd_adamw_step and dd_adamw_step_multi give the bits of dd_decay followed by dd_adam_step / dd_adam_step_multi (and of a
 *     separate fp32 multiply by keep followed by them): the same element code runs on the same p1.
 *
 * keep lies in [0, 1]: a NaN, an infinity, a negative value (lr * weight_decay > 1 is not a decay) or one above 1 is refused.
 *
 * THE SCALE of the gradient, as in dd_adam_step / dd_adam_step_dev: `grad_scale_dev` NULL -> `grad_scale` by value; otherwise ONE
 * fp32 in device memory (4-byte aligned) that the kernel reads when it starts -- what dd_clip_scale wrote earlier on the stream --
 * and `grad_scale` is not used.  The two forms are two kernels with the same arithmetic: the same value gives the same bits.
 *
 * REFUSED on the host, before any device call, with a message: a NULL p / g / m / v (or table, or keep array, or table entry);
 * n <= 0 (a table entry: n outside [1, 2^30)); count <= 0; step < 1; a flat buffer that is not 16-byte aligned; a misaligned
 * grad_scale_dev; keep as above.
 */
#ifndef DD_ADAMW_H
#define DD_ADAMW_H

#include <stdint.h>

#include "dd_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

/* torch.optim.AdamW over one flat fp32 buffer: p, g, m, v of n elements, 16-byte aligned; step >= 1.  The streaming pass of
 * dd_adam_step with the multiply by `keep` in front of the element: the same 28 bytes per element, non-temporal 16-byte accesses,
 * the n % 4 tail by workgroup 0, one persistent grid sized by dd_set_adam_blocks_per_cu.  The by-value kernel needs no more vector
 * registers than dd_adam_step's (48): it runs beside the same conv kernels. */
int dd_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, int32_t step,
                  float grad_scale, const float* grad_scale_dev, float keep, void* stream);

/* The same for `count` small tensors in one launch, the twin of dd_adam_step_multi: `tensors` a HOST array, `keep` a HOST array of
 * one factor per tensor (1.0f: that tensor does not decay -- biases and BatchNorm vectors ride in the same launch); all share `step`.
 * 48 tensors per launch, one element per thread, any alignment.  Both arrays are read before the function returns. */
int dd_adamw_step_multi(const dd_adam_tensor* tensors, const float* keep, int32_t count, float lr, float beta1, float beta2, float eps,
                        int32_t step, float grad_scale, const float* grad_scale_dev, void* stream);

/* p[i] = p[i] * keep for i < n; p 16-byte aligned.  The pre-scale of a tensor whose update is dd_adam_step_rankb(_dev): launched on
 * the same stream directly in front of that pass it is ordered behind the backward's last read of the weight.  8 bytes per element,
 * non-temporal 16-byte accesses, four in flight per lane, the n % 4 tail by workgroup 0; the grid is capped as the Adam pass's
 * (dd_set_adam_blocks_per_cu) and leaves dd_set_adam_spare_cus compute units free, as the rank-B pass does.  Nothing past p[n - 1]
 * is read or written. */
int dd_decay(float* p, int64_t n, float keep, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DD_ADAMW_H */

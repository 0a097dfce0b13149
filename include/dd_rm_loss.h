/* dd_rm_loss.h -- C ABI of the road-map loss library (csrc/libdd_rm_loss.so): weighted BCE-with-logits plus the soft threat score on
 * the road-map head's LOGITS, the logit-domain counterpart of the dd_box_loss_* block of dd_hotpath.h.
 *
 * An extension library of its own, as dd_augment.h, dd_tta.h and dd_ema.h: include/dd_hotpath.h (DD_ABI_VERSION 4) and the three
 * other extension headers are not touched by it.  The conventions are dd_hotpath.h's: plain device pointers, `stream` a hipStream_t
 * passed as void* last, no allocation, no host synchronisation, 0 on success and a DD_ERR_* code of dd_hotpath.h otherwise, the
 * message through libdd_hotpath.so's dd_last_error() (this library links against it).  Every declaration here is a launch function:
 * there is no size query, the workspace size follows from DD_RM_LOSS_CHUNK (below).
 *
 * THE SEMANTICS, stated once.
 *
 * logits fp32 [batch][per_sample]; t the target of the same shape: fp32 in [0, 1] (target_kind 0, dd_hotpath.h's DD_TARGET_F32) or one
 * byte 0 / 1 per element (target_kind 1, DD_TARGET_U8: uint8 / bool).  Per element, with (sig, l1p) = dd_sigmoid_softplus(z) of
 * csrc/dd_device.h -- the bits dd_sigmoid, the BCE pass and dd_linear_sigmoid_gt produce --
 *
 *     sp_pos = max(z, 0) + l1p      softplus(z)  = -log(1 - sigmoid(z))
 *     sp_neg = max(-z, 0) + l1p     softplus(-z) = -log(sigmoid(z))
 *
 * and per sample b over its P = per_sample elements
 *
 *     T = sum t      S = sum sig      I = sum sig t      U = S + T - I
 *     A = sum t sp_neg                C = sum (1 - t) sp_pos
 *     w = pos_weight, or with pos_weight == DD_RM_POS_WEIGHT_AUTO the sample's own (P - T) / max(T, 1); a constant of the step
 *     L_bce = 1 / (B P) sum_b (w A + C)          = F.binary_cross_entropy_with_logits(z, t, pos_weight = w)
 *     L_ts  = 1 / B sum_b [1 - (I + eps) / (U + eps)]
 *     L     = bce_weight L_bce + ts_weight L_ts
 *     dL/dz = c1 (1 - t) p - c0 t (1 - p) + p (1 - p) [c3 (1 - t) - c2 t]          p = sig
 *             c0 = bce_weight w / (B P)        c1 = bce_weight / (B P)
 *             c2 = ts_weight / (B (U + eps))   c3 = ts_weight (I + eps) / (B (U + eps)^2)
 *
 * No log is clamped and nothing is divided by p or 1 - p: loss and gradient are finite for every finite logit.
 *
 * THE FORWARD (dd_rm_loss_fwd, dd_rm_loss_fwd_u8_ptrs): ONE pass over logits and target writes `probs` (fp32, the sig bits; may be
 * NULL) and, per workgroup, fp64 partials of the five sums into `workspace`; ONE small launch then adds the partials in a fixed order
 * and writes stats fp64 [batch][5] = {T, S, I, A, C}, coef fp32 [batch][4] = {c0, c1, c2, c3} and loss_out fp32 [3] = {L, L_bce, L_ts}.
 * No atomics: two calls on the same operands give the same bits.  Validation stops here.
 *
 * THE BACKWARD (dd_rm_loss_bwd, dd_rm_loss_bwd_u8_ptrs): dlogits = dL/dz * grad_scale from the SAVED PROBABILITIES of a forward call
 * (not from the logits: no transcendental), the same target and that call's coef.  One pass.
 *
 * THE `_u8_ptrs` FORMS take the target as a HOST array of `batch` DEVICE pointers, one contiguous byte mask of per_sample elements
 * per sample (the collate's tuple, as dd_bce_logits_u8_ptrs takes it), at most DD_RM_LOSS_TABLE_MAX of them: the table travels in
 * the kernel arguments and is read before the function returns.  They give the bits of the stacked byte target.
 *
 * THE WORK SPLIT.  A workgroup (256 threads) takes one piece of DD_RM_LOSS_CHUNK consecutive elements of ONE sample (a sample's last
 * piece may be shorter); a sample has ceil(per_sample / DD_RM_LOSS_CHUNK) pieces.  A thread adds its at most DD_RM_LOSS_CHUNK / 256 = 32
 * elements of each of the five sums in fp32 and then converts to fp64; everything after that -- the workgroup's sum, the partials,
 * the sample's totals, the losses -- is fp64.  So against exact summation of the element values a sum of non-negative terms errs
 * by at most (DD_RM_LOSS_CHUNK / 256) 2^-24 of itself.  16-byte loads and stores of fp32 (4 bytes of a byte mask beside them);
 * nothing is read or written past the end of an operand.
 *
 * OPERANDS.  batch >= 1 (any; at most DD_RM_LOSS_TABLE_MAX for the _u8_ptrs forms); per_sample a positive multiple of 4;
 * batch * per_sample <= 2^40.  workspace: at least 5 * 8 * batch * ceil(per_sample / DD_RM_LOSS_CHUNK) bytes, 8-byte aligned;
 * `workspace_bytes` is its size and a smaller one is refused.  logits, probs, dlogits, coef and an fp32 target 16-byte aligned, a byte
 * target (every mask of a table) 4-byte aligned, stats and workspace 8, loss_out 4.
 *
 * REFUSED on the host, before any device call, with a message: a NULL or misaligned buffer (probs alone may be NULL); a NULL table
 * entry or batch > DD_RM_LOSS_TABLE_MAX on a _u8_ptrs call; per_sample % 4 != 0 or a size outside the above (DD_ERR_UNSUPPORTED, as
 * an unknown target kind); pos_weight <= 0 that is not DD_RM_POS_WEIGHT_AUTO, or infinite; eps < 0 or a negative bce_weight /
 * ts_weight, or an infinite one; a NaN among the scalars; a workspace that is too small; probs overlapping logits (forward) and
 * dlogits overlapping probs (backward: the saved probabilities are what is left of the logits there).
 */
#ifndef DD_RM_LOSS_H
#define DD_RM_LOSS_H

#include <stdint.h>

#define DD_RM_LOSS_CHUNK 8192       /* elements per piece: 256 lanes x 8 vectors of 16 bytes; a multiple of 1024 */
#define DD_RM_LOSS_TABLE_MAX 64     /* per-sample mask pointers of a _u8_ptrs call */
#define DD_RM_POS_WEIGHT_AUTO (-1.0f)

#ifdef __cplusplus
extern "C" {
#endif

/* The forward on a stacked target.  target_kind: 0 fp32, 1 bytes. */
int dd_rm_loss_fwd(const float* logits, const void* target, int32_t target_kind, int32_t batch, int64_t per_sample, float pos_weight,
                   float bce_weight, float ts_weight, float ts_eps, float* probs, float* loss_out, double* stats, float* coef,
                   void* workspace, int64_t workspace_bytes, void* stream);

/* The forward on a HOST table of `batch` per-sample byte masks. */
int dd_rm_loss_fwd_u8_ptrs(const float* logits, const unsigned char* const* target_ptrs, int32_t batch, int64_t per_sample,
                           float pos_weight, float bce_weight, float ts_weight, float ts_eps, float* probs, float* loss_out, double* stats,
                           float* coef, void* workspace, int64_t workspace_bytes, void* stream);

/* dlogits = dL/dz * grad_scale from the probabilities and the coef of a forward call on the same target. */
int dd_rm_loss_bwd(const float* probs, const void* target, int32_t target_kind, int32_t batch, int64_t per_sample, const float* coef,
                   float grad_scale, float* dlogits, void* stream);

int dd_rm_loss_bwd_u8_ptrs(const float* probs, const unsigned char* const* target_ptrs, int32_t batch, int64_t per_sample,
                           const float* coef, float grad_scale, float* dlogits, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DD_RM_LOSS_H */

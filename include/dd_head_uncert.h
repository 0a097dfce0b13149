/* dd_head_uncert.h -- C ABI of the sampled road-map head's uncertainty (csrc/libdd_head_uncert.so): the head's Linear on S latents per
 * scene -- S dropout draws of the encoder's dense tail, as dd_head_mean.h -- and, in the SAME pass over the head's weight, what the
 * spread of the S probabilities says: the entropy of their mean, the mutual information between prediction and weights (BALD: the
 * draws disagree = model uncertainty; every draw says 0.5 = data uncertainty, entropy without mutual information), their variance, and
 * per-scene means of the three.  Neither logits nor probabilities of the single draws are written anywhere.
 *
 * An extension library of its own, as dd_head_mean.h: include/dd_hotpath.h (DD_ABI_VERSION 4) and the other extension headers are not
 * touched by it.  The conventions are dd_hotpath.h's: plain device pointers, sizes as int32, `stream` a hipStream_t passed as void*
 * last, no allocation, no host synchronisation, 0 on success and a DD_ERR_* code of dd_hotpath.h otherwise, the message through
 * libdd_hotpath.so's dd_last_error() (this library links against it).  The one declaration here is a launch function; the one
 * constant is the column block below.
 *
 * Operands.  `x` fp32 [scenes*samples, k], scene-major: row b*samples + s is draw s of scene b.  `w` fp32 [n, k], nn.Linear's
 * layout; `bias` fp32 [n] or NULL.  The maps `mean`, `entropy`, `mi`, `var`: fp32 [scenes, n] each, or NULL = not written.  `partials`
 * fp64 [ceil(n / DD_HEAD_UNCERT_BLOCK), scenes, 3] (the caller's workspace) and `scores` fp64 [scenes, 3]: both given, or both NULL.
 *
 * THE SEMANTICS, stated once.  With S = samples; everything in nats; every operation below is ONE rounded fp32 operation, nothing is
 * contracted into a fused multiply-add:
 *
 *     z[b,s,j], p[b,s,j], sum[b,j], mean[b,j]
 *                   exactly as dd_head_mean.h defines them: dd_linear_fwd's tiles and contraction order, the `sig` of
 *                   dd_sigmoid_softplus(z) (csrc/dd_device.h), adds in draw order, one multiply by (float)(1.0 / S).  `mean` has the
 *                   bits of dd_head_mean_prob.
 *     h[b,s,j]      = l1p + |z| * q, the entropy of ONE draw, taken from the LOGIT: l1p = log1p(exp(-|z|)) and q = sigmoid(-|z|), the
 *                   `l1p` and the `sig` of dd_sigmoid_softplus(-|z|).  It is softplus(z) - p z with the cancellation removed: finite
 *                   for every finite logit, ln 2 at 0, falling to 0 in both tails without a clamp.
 *     expected[b,j] = (h[b,0,j] + h[b,1,j] + ... + h[b,S-1,j]) * (float)(1.0 / S), added in draw order
 *     entropy[b,j]  = (-(m * ln m)) - ((1 - m) * ln(1 - m)) of m = mean[b,j]; a term whose factor is 0 is 0; 1 - m is one subtract;
 *                   ln is logf, good to 1 ulp
 *     mi[b,j]       = entropy - expected where that is positive, else 0 (in real arithmetic it is >= 0 by Jensen: only rounding is
 *                   removed; a NaN stays a NaN).  With S = 1 it is 0 * entropy: exact 0.
 *     var[b,j]      = ((p_0 - m)^2 + ... + (p_{S-1} - m)^2) * (float)(1.0 / S): the population variance, two passes, the squares
 *                   added in draw order.  Exact 0 at S = 1 (m = p_0 * 1.0f).
 *     scores[b]     = (sum_j entropy[b,j], sum_j mi[b,j], sum_j var[b,j]) / n in fp64.  The workgroup of column block i adds its
 *                   <= DD_HEAD_UNCERT_BLOCK columns of scene b, widened to fp64, in column order, into partials[i, b, :]; a finishing
 *                   launch adds the blocks in block order and divides by (double)n.  No atomics: the same bits on every run, and
 *                   whether or not any map is written.
 *
 * A NaN logit gives NaN in that pixel's maps and in that scene's scores, and nowhere else.
 *
 * Limits, those of dd_head_mean.h: 1 <= samples <= 64; k % 4 == 0 and k <= 512; any scenes > 0 and n > 0 with scenes * n < 2^31.
 * `x`, `w` and the maps are 16-byte aligned, `bias` 4-byte, `partials` and `scores` 8-byte.  No output overlaps an input or another
 * output.  A call that asks for no output at all (every map and `scores` NULL) is refused; `partials` without `scores`, or the
 * reverse, is refused.  A refused call writes nothing.
 *
 * A launch holds floor(64 / samples) scenes, at most 64 rows; more scenes run as further launches in stream order, and one finishing
 * launch follows when scores are asked for.  The kernel is picked by the shape (the rows of a launch) alone; which outputs are
 * written is an argument of it; an address never decides anything.
 */
#ifndef DD_HEAD_UNCERT_H
#define DD_HEAD_UNCERT_H

#include <stdint.h>

#define DD_HEAD_UNCERT_BLOCK 128

#ifdef __cplusplus
extern "C" {
#endif

int dd_head_uncert(const float* x, const float* w, const float* bias, float* mean, float* entropy, float* mi, float* var,
                   double* partials, double* scores, int32_t scenes, int32_t samples, int32_t n, int32_t k, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DD_HEAD_UNCERT_H */

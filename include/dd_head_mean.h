/* dd_head_mean.h -- C ABI of the sampled road-map head (csrc/libdd_head_mean.so): the head's Linear on S latents per scene -- S
 * dropout draws of the encoder's dense tail -- and the mean of the S probabilities, in ONE pass over the head's weight.  Neither
 * logits nor probabilities of the single draws are written anywhere.
 *
 * An extension library of its own, as dd_tta.h: include/dd_hotpath.h (DD_ABI_VERSION 4) and the other extension headers are not
 * touched by it.  The conventions are dd_hotpath.h's: plain device pointers, sizes as int32, `stream` a hipStream_t passed as void*
 * last, no allocation, no host synchronisation, 0 on success and a DD_ERR_* code of dd_hotpath.h otherwise, the message through
 * libdd_hotpath.so's dd_last_error() (this library links against it).  Every declaration here is a launch function.
 *
 * Operands.  `x` fp32 [scenes*samples, k], scene-major: row b*samples + s is draw s of scene b.  `w` fp32 [n, k], nn.Linear's
 * layout; `bias` fp32 [n] or NULL.  `out` [scenes, n].
 *
 * THE SEMANTICS, stated once.  With S = samples:
 *
 *     z[b,s,j]  = dd_linear_fwd's value for row b*S + s, column j: the same tiles, the same contraction order, so the same bits
 *                 (as dd_linear_sigmoid_gt's are)
 *     p[b,s,j]  = the `sig` of dd_sigmoid_softplus(z[b,s,j]) (csrc/dd_device.h): the dense head's one sigmoid
 *     sum[b,j]  = p[b,0,j], then + p[b,1,j], ... up to + p[b,S-1,j]: sequential fp32 adds in draw order, each ONE rounded add, never
 *                 fused with anything inside the sigmoid
 *     mean[b,j] = sum[b,j] * (float)(1.0 / S): one rounded multiply, exact for S = 1 (and for every power of two)
 *
 * Limits: 1 <= samples <= 64; k % 4 == 0 and k <= 512 (dd_linear_fwd walks such a contraction in one workgroup; a shape where it
 * would split K over workgroups is refused, as dd_linear_sigmoid_gt refuses it); any scenes > 0 and n > 0 with scenes * n < 2^31.
 * `x`, `w` and `out` are 16-byte aligned (every torch allocation is); `out` overlaps no input.  A refused call writes nothing.
 *
 * A launch holds floor(64 / samples) scenes, at most 64 rows; more scenes run as further launches in stream order: the weight is
 * streamed ceil(scenes / floor(64 / samples)) times, not `samples` times.  The kernel is picked by the shape alone (the rows of a
 * launch, n % 4, n % 16), never by an address.
 */
#ifndef DD_HEAD_MEAN_H
#define DD_HEAD_MEAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* out fp32 [scenes,n] = mean. */
int dd_head_mean_prob(const float* x, const float* w, const float* bias, float* out, int32_t scenes, int32_t samples, int32_t n,
                      int32_t k, void* stream);

/* out bytes [scenes,n] = (mean > tau) as 0 / 1, strictly, tau as the fp32 it is handed as; a NaN mean is 0.  With samples = 1 byte
 * for byte dd_linear_sigmoid_gt's output.  Nothing else is written. */
int dd_head_mean_gt(const float* x, const float* w, const float* bias, float tau, unsigned char* out, int32_t scenes,
                    int32_t samples, int32_t n, int32_t k, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DD_HEAD_MEAN_H */

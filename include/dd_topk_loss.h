/* dd_topk_loss.h -- C ABI of the bootstrapped road-map loss library (csrc/libdd_topk_loss.so): BCE-with-logits averaged over each
 * sample's K HARDEST pixels (bootstrapped cross-entropy, Wu et al. 2016), with an exact per-sample selection -- the K-th largest of
 * per_sample values -- made on the device, without a host round trip.
 *
 * An extension library of its own, as dd_rm_loss.h and dd_consistency.h: include/dd_hotpath.h (DD_ABI_VERSION 4) and the other
 * extension headers are not touched by it.  The conventions are dd_hotpath.h's: plain device pointers, `stream` a hipStream_t passed as
 * void* last, no allocation, no host synchronisation, 0 on success and a DD_ERR_* code of dd_hotpath.h otherwise, the message through
 * libdd_hotpath.so's dd_last_error() (this library links against it).  Every declaration here is a launch function: there is no size
 * query, the workspace size follows from the constants below.
 *
 * THE SEMANTICS, stated once.
 *
 * z fp32 [batch][per_sample], the logits; t one byte per element, 0 or 1 (uint8 / bool; a non-zero byte counts as 1), stacked
 * [batch][per_sample] (dd_topk_bce) or as a HOST array of `batch` DEVICE pointers to per-sample masks (dd_topk_bce_u8_ptrs: the
 * collate's tuple, with the conventions of dd_rm_loss_fwd_u8_ptrs, at most DD_TOPK_TABLE_MAX entries; the table travels in the kernel
 * arguments and is read before the function returns).  keep = K, an integer in 1 .. per_sample, the same for every sample.
 *
 *     margin   u_i = t_i ? -z_i : z_i            a sign flip: exact.  The per-pixel loss softplus(u_i) is strictly increasing in u, so
 *                                                the K pixels with the largest loss are the K pixels with the largest margin
 *     key(u)   the order-preserving uint32 image of u's bits (bits ^ 0x80000000 for a clear sign bit, ~bits for a set one), -0
 *              taken as +0 first.  EVERY comparison is made on keys: denormal margins order correctly whatever the float mode
 *     tau_b    the K-th largest margin of sample b, exact
 *     S_b      = { i : key(u_i) >= key(tau_b) }      ties at tau_b are all kept
 *     n_b      = |S_b| >= K, exact
 *     sp_i     = max(u_i, 0) + l1p_i,   (sig_i, l1p_i) = dd_sigmoid_softplus(z_i) of csrc/dd_device.h, the bits every other loss here uses
 *     L        = (1 / B) sum_b (1 / n_b) sum_{i in S_b} sp_i
 *     L_all    = 1 / (B P) sum_b sum_i sp_i           the plain mean BCE-with-logits, from the same pass
 *     dL/dz_i  = grad_scale (sig_i - t_i) / (B n_b)   for i in S_b, and exactly 0.0f elsewhere
 *
 * Nothing is divided by p or 1 - p and no log is clamped: loss and gradient are finite for every finite logit.  Where the pixels of a
 * NaN logit land is unspecified (its key is some uint32 and is ordered as such); the call finishes and stays inside its operands.
 * keep == per_sample: tau_b is the sample's minimum, every pixel is kept, the selection launches are skipped and L = L_all.
 *
 * OUTPUTS.  probs fp32 [batch][per_sample], the sig bits, written for EVERY element, selected or not; may be NULL.  dlogits fp32
 * [batch][per_sample], every element written (a zero where not selected); may be NULL: the no-gradient form, a compile-time branch of
 * the same kernel template, so both forms add the same terms in the same order and give the same bits of loss_out and stats.  loss_out
 * fp32 [2] = {L, L_all}.  stats fp64 [batch][4] = {n_b, sum_{S_b} sp, tau_b, sum_all sp}.
 *
 * THE SELECTION is a most-significant-digit radix select on the key, per sample: three digits of 11, 11 and 10 bits.  For each digit a
 * streaming pass over z and t counts, per workgroup in LDS, the digit's values among the elements whose higher digits equal the
 * prefix found so far, and adds its non-zero counts to the sample's histogram in the workspace with global INTEGER atomics (the call
 * zeroes the histograms on the same stream first); a small launch, one workgroup per sample, then walks the bins from the top until
 * the cumulative count reaches the remaining rank and writes the new prefix and the remaining rank to the sample's state block.  After
 * the last digit the state holds key(tau_b) and, from the counts alone, n_b = (K - r) + c (r the remaining rank inside the final
 * exact-key bin, c that bin's count), so the final pass knows 1 / (B n_b) before it starts.  Counts are integers: their accumulation
 * order cannot change them.  There are no floating-point atomics; every floating-point sum has a fixed order: two calls on the same
 * operands give the same bits of every output.
 *
 * THE WORK SPLIT.  A workgroup (256 threads) takes one piece of DD_TOPK_CHUNK consecutive elements of ONE sample (a sample's last piece
 * may be shorter); a sample has ceil(per_sample / DD_TOPK_CHUNK) pieces.  In the final pass a thread adds the sp of its at most
 * DD_TOPK_CHUNK / 256 = 32 elements in fp32 and then converts to fp64; everything after that is fp64.  16-byte loads and stores of
 * fp32, 4 bytes of mask beside them; nothing is read or written past the end of an operand.
 *
 * OPERANDS.  batch >= 1 (at most DD_TOPK_TABLE_MAX on the table form); per_sample a positive multiple of 4 below 2^31; batch *
 * per_sample <= 2^40; 1 <= keep <= per_sample; grad_scale finite.  workspace: at least
 *
 *     batch * (DD_TOPK_PIECE_BYTES * ceil(per_sample / DD_TOPK_CHUNK) + 4 * DD_TOPK_BINS + DD_TOPK_STATE_BYTES)
 *
 * bytes, 8-byte aligned; `workspace_bytes` is its size and a smaller one is refused.  logits, probs and dlogits 16-byte aligned, a
 * byte target (every mask of a table) 4-byte aligned, stats and workspace 8, loss_out 4.
 *
 * REFUSED on the host, before any device call, with a message: a NULL or misaligned buffer (probs and dlogits alone may be NULL); a
 * NULL table entry or batch > DD_TOPK_TABLE_MAX on the table form; per_sample % 4 != 0 or a size outside the above
 * (DD_ERR_UNSUPPORTED); keep outside 1 .. per_sample; a grad_scale that is not finite; a workspace that is too small; probs or dlogits
 * overlapping logits or each other.
 */
#ifndef DD_TOPK_LOSS_H
#define DD_TOPK_LOSS_H

#include <stdint.h>

#define DD_TOPK_CHUNK 8192          /* elements per piece: 256 lanes x 8 vectors of 16 bytes; a multiple of 1024 */
#define DD_TOPK_TABLE_MAX 64        /* per-sample mask pointers of a dd_topk_bce_u8_ptrs call */
#define DD_TOPK_BINS 5120           /* histogram counters per sample: 2048 + 2048 + 1024, the three digits */
#define DD_TOPK_PIECE_BYTES 24      /* per piece: two fp64 partial sums and the piece's smallest key */
#define DD_TOPK_STATE_BYTES 16      /* per sample: the key prefix, the remaining rank, n_b */

#ifdef __cplusplus
extern "C" {
#endif

/* The loss on a stacked byte target. */
int dd_topk_bce(const float* logits, const unsigned char* target, int32_t batch, int64_t per_sample, int64_t keep, float grad_scale,
                float* probs, float* dlogits, float* loss_out, double* stats, void* workspace, int64_t workspace_bytes, void* stream);

/* The loss on a HOST table of `batch` per-sample byte masks. */
int dd_topk_bce_u8_ptrs(const float* logits, const unsigned char* const* target_ptrs, int32_t batch, int64_t per_sample, int64_t keep,
                        float grad_scale, float* probs, float* dlogits, float* loss_out, double* stats, void* workspace,
                        int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DD_TOPK_LOSS_H */

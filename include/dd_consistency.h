/* dd_consistency.h -- C ABI of the consistency-loss library (csrc/libdd_consistency.so): the mirror consistency loss on pairs of the
 * road-map head's LOGITS -- a scene's map and the map of its left/right mirror, pulled together (the Pi-model's loss on two
 * stochastic views of one unlabelled sample, with the mirror's row reversal inside it).
 *
 * An extension library of its own, as dd_rm_loss.h and dd_tta.h: include/dd_hotpath.h (DD_ABI_VERSION 4) and the other extension
 * headers are not touched by it.  The conventions are dd_hotpath.h's: plain device pointers, `stream` a hipStream_t passed as void*
 * last, no allocation, no host synchronisation, 0 on success and a DD_ERR_* code of dd_hotpath.h otherwise, the message through
 * libdd_hotpath.so's dd_last_error() (this library links against it).  Every declaration here is a launch function: there is no size
 * query, the workspace size follows from DD_CONS_CHUNK (below).
 *
 * THE SEMANTICS, stated once.
 *
 * a fp32 [batch][h][w], the logits of the scenes; m fp32 [batch][h][w], the logits of the mirrored scenes.  The mirrored scene's map is
 * the scene's map with its rows reversed (dd_tta.h's convention): m'[b][r][c] = m[b][h-1-r][c].  P(z) is the dense head's one sigmoid
 * (dd_sigmoid_softplus of csrc/dd_device.h, the bits dd_tta_mean_prob takes).  With N = batch h w,
 *
 *     d        = P(a) - P(m')                                   per element
 *     Q_b      = sum_{r,c} d^2                                  per pair
 *     L        = (sum_b Q_b) / N
 *     D_b      = #{(r,c) : (a > 0) != (m' > 0)}                 taken on the logits: exact
 *     dL/da[b][r][c]     =  grad_scale 2 d p_a  (1 - p_a)  / N
 *     dL/dm[b][h-1-r][c] = -grad_scale 2 d p_m' (1 - p_m') / N
 *
 * The gradient goes through p (1 - p) only: nothing is divided, loss and gradient are finite for every finite logit.
 *
 * dd_cons_fwd: ONE pass over a and m writes, per workgroup, fp64 partials of Q and D into `workspace`; ONE small launch then adds the
 * partials in a fixed order and writes stats fp64 [batch][2] = {Q_b, D_b} and loss fp32 [1] = L.  dd_cons_fwd_grad: the same pass also
 * writes da and dm (each fp32 [batch][h][w], every element exactly once): it reads two maps and writes two, nothing is saved in
 * between.  One kernel template serves both: the two give the same bits of loss and stats.  No atomics: two calls on the same operands
 * give the same bits.
 *
 * THE WORK SPLIT.  A workgroup (256 threads) takes one piece of DD_CONS_CHUNK consecutive elements of ONE pair's a (a pair's last piece
 * may be shorter) and the elements of m they are compared with; a pair has ceil(h w / DD_CONS_CHUNK) pieces.  A thread adds the squares
 * of its at most DD_CONS_CHUNK / 256 = 16 elements in fp32 and counts its disagreements in an integer, then converts both to fp64;
 * everything after that -- the workgroup's sum, the partials, the pair's totals, the loss -- is fp64.
 *
 * TWO PATHS, the same arithmetic in the same order, so the same bits.  With w % 4 == 0 and a, m, da, dm all 16-byte aligned: 16-byte
 * loads and stores -- a vector of four columns never straddles a row, so the reversed row is a coalesced stream too.  Otherwise: 4-byte
 * loads and stores.  Nothing is read or written past the end of an operand on either path.
 *
 * OPERANDS.  batch >= 1, h >= 1, w >= 1; h w < 2^31; batch h w <= 2^40.  workspace: at least 2 * 8 * batch * ceil(h w / DD_CONS_CHUNK)
 * bytes, 8-byte aligned; `workspace_bytes` is its size and a smaller one is refused.  a, m, da, dm and loss 4-byte aligned, stats 8.
 *
 * REFUSED on the host, before any device call, with a message: a NULL or misaligned buffer; a size outside the above (a size the
 * kernels do not serve: DD_ERR_UNSUPPORTED); a grad_scale that is not finite; a workspace that is too small; da or dm overlapping a,
 * m or each other (the row reversal cannot be done in place).
 */
#ifndef DD_CONSISTENCY_H
#define DD_CONSISTENCY_H

#include <stdint.h>

#define DD_CONS_CHUNK 4096       /* elements per piece: 256 lanes x 4 vectors of 16 bytes; a multiple of 1024 */

#ifdef __cplusplus
extern "C" {
#endif

/* loss fp32 [1], stats fp64 [batch][2] = {Q_b, D_b}. */
int dd_cons_fwd(const float* a, const float* m, int32_t batch, int32_t h, int32_t w, float* loss, double* stats, void* workspace,
                int64_t workspace_bytes, void* stream);

/* The same, and da = dL/da * grad_scale, dm = dL/dm * grad_scale. */
int dd_cons_fwd_grad(const float* a, const float* m, int32_t batch, int32_t h, int32_t w, float grad_scale, float* da, float* dm,
                     float* loss, double* stats, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DD_CONSISTENCY_H */

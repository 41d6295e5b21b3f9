/* The Lovasz-Softmax loss and the Lovasz hinge (Berman, Triki, Blaschko, CVPR 2018), the convex Lovasz extension of the Jaccard loss,
 * on a stable segmented device sort: the entries of liblmnet_hip.so behind lm_net_amd.loss.LovaszLoss and lovasz_ranks.  Every other
 * criterion of the package is a surrogate for something else (CE, Dice, focal and BCE are regional, the distance-map losses train
 * against HD95); this one trains against the mIoU column itself.  These symbols are listed in lm_net_amd.hip.SYMBOLS_LOVASZ, a list of
 * its own that lm_net_amd.hip.load checks next to hip.EXPORTS; tests/test_lovasz_cpu.py checks it against this header and ties the
 * three device entries to tests/test_guard_lovasz_gpu.py.  Plain arguments only: no struct, no ABI bump.
 *
 * DEFINITIONS.  A SEGMENT is the set of elements one Lovasz extension is taken over.  per_image == 0 (Berman's default): one segment
 *   per scored class, the P = B * H * W pixels of the batch, element index i = b * H * W + y * W + x, segment s = kk (the kk-th scored
 *   class in ascending order).  per_image != 0: one segment per (image, class), P = H * W, s = b * nk + kk.  S segments in all.
 *   Softmax head (C >= 2, target a label map [B, H, W]): p = softmax(z) over all C classes; a pixel is VALID when its label is in
 *      [0, C), everything else is void.  For a scored class k: fg_i = [label_i == k], e_i = |fg_i - p_k(i)| in fp32.
 *   Sigmoid head (target planes [B, C, H, W]): Berman's hinge on each scored plane; an element is valid when its target is 0 or 1;
 *      s_i = 2 t_i - 1, e_i = 1 - z_i s_i, fg_i = t_i.  The hinge enters later as relu(e).
 *   ORDER.  The valid elements of a segment are ranked by e descending, TIES BY ELEMENT INDEX ASCENDING; void elements take the ranks
 *      after the last valid one, by index ascending.  A stable sort: the order is a function of the inputs alone.  The 32-bit key of a
 *      valid element is ~bits(e) & 0x7fffffff for e >= 0 (-0 is stored as +0) and bits(e) for e < 0 -- descending float order as
 *      ascending unsigned order; void is 0xffffffff, which no finite e produces.
 *   COEFFICIENT.  G: the valid foreground elements of the segment; n_r, m_r: the foreground and background elements among ranks
 *      0 .. r (integers, from an integer scan).  Berman's lovasz_grad (jaccard[r] - jaccard[r - 1]) in closed form:
 *           foreground at rank r:  g_r = 1 / (G + m_r)
 *           background at rank r:  g_r = (G - n_r) / ((G + m_r - 1) (G + m_r))
 *           G == 0:                g_0 = 1, every other g_r = 0
 *      no difference of nearly equal numbers and no float scan.  Void ranks get g = 0.
 *   SEGMENT LOSS.  Softmax head: L_s = sum_r e_(r) g_r.  Sigmoid head: L_s = sum_r relu(e_(r)) g_r.
 *   REDUCTION.  A GROUP is the nk segments of one image (per_image) or of the batch.  present != 0 (Berman's classes="present"): the
 *      mean over the group's segments with G > 0; present == 0: the mean over all nk.  Then the mean over the groups.  The weight of
 *      a segment is w_s = 1 / (n_group * groups), 0 for a segment left out.  A SEGMENT WITHOUT A VALID ELEMENT CONTRIBUTES 0 AND AN
 *      AVERAGE OVER NO SEGMENT IS 0 with an all-zero gradient, never NaN (a deliberate difference from torch); the gradient is +0 at
 *      every void position.
 *   GRADIENT.  dL/de_i = w_s g_rank(i), times [e_i > 0] under the hinge: this is `coef`.  Softmax head: de/dp_k = -1 on foreground and
 *      +1 on background (the subgradient taken at e = 0 too), dz_j = p_j (d_j - sum_k p_k d_k) over the scored classes.  Sigmoid head:
 *      dz_i = -s_i coef_i.
 *
 * LIMITS.  B >= 1, 1 <= C <= 64 (C == 1 only for a sigmoid head), H, W >= 1, B * C * H * W < 2^31; 1 <= S <= 65535, P >= 1,
 * S * P < 2^31.
 *
 * NO FLOAT ATOMICS ANYWHERE: the counts are integer atomics, the sums go through fixed slots in a fixed order, so two calls are
 * bit-identical in either deterministic mode, loss and gradient.  NO KERNEL WAITS ON ANOTHER BLOCK (no look-back, no flag, no grid
 * barrier); every loop of every kernel is bounded by the tile size, the block count of a segment or the class count.  Every argument
 * error is rejected before any HIP call (LMN_E_BADARG and lmn_last_error, messages "lovasz_order: ...", "lovasz_fwd: ...",
 * "lovasz_bwd: ...").  Not recorded by plans.                                                                                      */
#ifndef LMNET_LOVASZ_H
#define LMNET_LOVASZ_H
#include "../lmnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMN_LOVASZ_TILE 2048         /* elements of a segment one block of the sort sorts per digit pass */
#define LMN_LOVASZ_SCAN_THREADS 64   /* threads of the block that scans one digit row of the [digit][block] table */
#define LMN_LOVASZ_MAX_SEGMENTS 65535
#define LMN_LOVASZ_LABELS_U8 0       /* target_kind */
#define LMN_LOVASZ_LABELS_I64 1
#define LMN_LOVASZ_SOFTMAX 0         /* head */
#define LMN_LOVASZ_SIGMOID 1
#define LMN_LOVASZ_SUMS_WORDS 4      /* sums: [0] segments with a non-zero weight (int32)  [1] L (float)  [2] scale (float)  [3] 0 */

/* bytes of `workspace` for S segments of P elements, exactly, nb = ceil(P / LMN_LOVASZ_TILE): two key and two payload buffers
 * (uint32 [S, P] each), the digit table (uint32 [S, 256, nb]) and the digit totals (uint32 [S, 256]), the foreground counts and
 * the partial sums of the tiles (int32 and float [S, nb]) and the segment losses (float [S]), each rounded up to 256 bytes.  Host
 * arithmetic; -1 and lmn_last_error outside 1 <= S <= 65535, P >= 1, S * P < 2^31. */
int64_t lmn_lovasz_workspace(int S, int64_t P);

/* The stable ascending sort of S segments of P keys each: perm[s][r] (int32 [S, P]) is the in-segment index of the r-th smallest key
 * of segment s, ties by index ascending.  keys (uint32 [S, P]) is not modified.  An LSD radix sort of (key, index) pairs over four
 * 8-bit digits, grid.y = segment; after one zero fill each digit pass is three launches: the digit histogram of every tile (and the
 * segment's digit totals, integer atomics), an exclusive scan of the segment's [digit][block] table, one wave per digit row, and a
 * scatter that ranks inside a tile by wave ballots and per-wave offsets in LDS. */
int lmn_lovasz_order(const uint32_t* keys, int S, int64_t P, void* workspace, int64_t ws_bytes, int32_t* perm, lmn_stream_t stream);

/* loss[0] = scale * L under one head (LMN_LOVASZ_SOFTMAX: target is a label map [B, H, W]; LMN_LOVASZ_SIGMOID: target is planes
 * [B, C, H, W]) of target_kind; all pointers device.  The scored classes are the set bits of class_mask (bits >= C clear, at least
 * one set), nk of them; S = nk, P = B * H * W, or S = B * nk, P = H * W with per_image.
 *   workspace  at least lmn_lovasz_workspace(S, P) bytes, ws_bytes its size
 *   errors     fp32 [S, P], 0 at a void element        perm    int32 [S, P], the order above
 *   counts     int32 [S, 2]: valid elements and G      coef    fp32 [B, nk, H, W]: dL/de of every element at its own position
 *   sums       LMN_LOVASZ_SUMS_WORDS words of 4 bytes, read by lmn_lovasz_bwd;  scale: finite
 * Launches on `stream`: a zero fill, the keys, the thirteen launches of the sort, the foreground counts of the tiles, the coefficients
 * (coef and perm through the sorted payload, the partial sums of e g into fixed slots), a one-block finish. */
int lmn_lovasz_fwd(const float* logits, const void* target, int target_kind, int head, int per_image, int present, float scale, int B,
                   int C, int H, int W, uint64_t class_mask, void* workspace, int64_t ws_bytes, float* errors, int32_t* perm,
                   int32_t* counts, float* coef, void* sums, float* loss, lmn_stream_t stream);

/* dlogits (fp32 [B, C, H, W], every element written) = gscale[0] * d loss / d logits from the coef and sums of lmn_lovasz_fwd on the
 * same arguments; gscale: one device float, or NULL for 1.  One pointwise launch. */
int lmn_lovasz_bwd(const float* logits, const void* target, int target_kind, int head, int B, int C, int H, int W, uint64_t class_mask,
                   const float* coef, const void* sums, const float* gscale, float* dlogits, lmn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

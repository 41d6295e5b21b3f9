/* The region-overlap losses -- soft Dice, soft Jaccard, Tversky / focal Tversky (Salehi et al. 2017; Abraham and Khan 2019) and the
 * generalized Dice loss (Sudre et al. 2017) -- per batch or per image, under a softmax or a sigmoid head: the entries of
 * liblmnet_hip.so behind lm_net_amd.loss.RegionLoss and region_sums.  The fused criteria (lmn_segloss*, lmn_sigloss*) carry one form
 * of this family, the batch-level Dice with a squared denominator; every other member is a function of the same per-(group, class)
 * sums, so one kernel family covers them at one read of logits and labels per pass.  These symbols are listed in
 * lm_net_amd.hip.SYMBOLS_REGION, a list of its own that lm_net_amd.hip.load checks next to hip.EXPORTS; tests/test_region_cpu.py
 * checks it against this header and ties the two device entries to tests/test_guard_region_gpu.py.  Plain arguments only: no struct,
 * no ABI bump.
 *
 * DEFINITIONS.  Logits are fp32 [B, C, H, W].
 *   Softmax head (2 <= C <= 64, target a uint8 or int64 label map [B, H, W]): p = softmax(z) over all C classes, t = [label == k];
 *      a pixel is VALID when its label lies in [0, C).
 *   Sigmoid head (1 <= C <= 64, target planes [B, C, H, W] of uint8 or int64): p = sigmoid(z_k), t the target element; an element is
 *      VALID when its target is 0 or 1.
 *   GROUPS.  A group is one image (per_image != 0, G = B) or the whole batch (G = 1).
 *   SCORED CLASSES.  The set bits of class_mask (bits >= C clear, at least one set), nk of them, in ascending order.
 *   SUMS over the valid elements of group g and scored class k:  I = sum p t,  P1 = sum p,  P2 = sum p^2  (fp32; P2 only under
 *      LMN_REGION_SQUARED, 0 otherwise),  T = sum t  and  N = #valid  (int32 from integer atomics: exact in either mode).
 *      FP = P1 - I,  FN = T - I,  s = smooth >= 0,  D = P2 + T (LMN_REGION_SQUARED) or P1 + T (LMN_REGION_LINEAR).
 *   RATIO.
 *      LMN_REGION_DICE      R = (2 I + s) / (D + s)
 *      LMN_REGION_JACCARD   R = (I + s) / (D - I + s)
 *      LMN_REGION_TVERSKY   R = (I + s) / (I + alpha FP + beta FN + s),  alpha, beta >= 0;  linear only
 *      LMN_REGION_GDICE     one ratio per group, R_g = (2 sum_k v_k I_k + s) / (sum_k v_k (P1_k + T_k) + s);  linear only, weight must be
 *                           NULL, every class of the group gets L_gk = L_g.  v_k = 1 / T_k^2; a class with T_k = 0 takes the largest
 *                           finite v of its group (MONAI's rule), 0 when the group has none.  v depends on the target only: a
 *                           constant of the gradient.
 *   EDGE RULES.  A DENOMINATOR THAT IS EXACTLY 0 GIVES R = 1 (this needs s = 0): the loss is 0 and its coefficients are 0.
 *      With u = 1 - R:  exponent == 1: L = u;  otherwise L = u^exponent for u > 0 and L = 0 WITH A ZERO DERIVATIVE FOR u <= 0, which
 *      keeps a saturated plane (p rounded to exactly 1 or 0 in fp32) from producing an infinite gradient.  exponent in (0, 8];
 *      Abraham and Khan's focal Tversky at gamma = 4/3 is exponent = 0.75.
 *   LOSS.  loss = scale / (G nk) * sum_g sum_k w_k L_gk,  w an optional fp32 weight per scored class (NULL: 1).  All G groups count
 *      in the mean; a group without a valid element has L = 0 by the rules above.  The loss is never NaN.
 *   GRADIENT.  For a valid element d_k = a_gk t + b_gk + c_gk p with a = d loss / dI, b = d loss / dP1, c = 2 d loss / dP2 (they
 *      carry scale, w_k and 1 / (G nk)): `coef` [G, nk, 3].  Softmax head: dz_j = p_j (d_j - sum_k p_k d_k) over the scored classes,
 *      d = 0 for an unscored class.  Sigmoid head: dz = p (1 - p) d, +0 on an unscored plane.  EVERY VOID POSITION GETS GRADIENT +0 in
 *      every class (the package's standing difference from torch).
 *   IDENTITIES.  tversky(alpha = beta = 0.5, s) = linear dice(2 s);  tversky(alpha = beta = 1, s) = linear jaccard(s);  dice, squared,
 *      per batch, smooth 1e-5 with weight w is the Dice term of lmn_segloss_ex_fwd.
 *   The per-sample Dice of the reference's offical_DiceLoss is B times the per-image squared form at smooth = 1 ONLY WITHOUT VOID
 *      LABELS: its denominator sums the squared probabilities over every pixel, valid or not, and that quirk is not reproduced.
 *
 * LIMITS.  1 <= B <= 65535, 1 <= C <= 64 (C == 1 only under the sigmoid head), H, W >= 1, B * C * H * W < 2^31.
 *
 * REDUCTION.  Ordinary mode: one float atomic per block and sum.  Deterministic mode (lmn_set_deterministic): every block writes its
 * partial sums to a slot of `workspace` and the finish kernel adds the slots of a group in block order, so loss, per_class, coef and
 * dlogits are bit-identical from call to call.  T and N are integer atomics in both modes.  Every argument error is rejected before
 * any HIP call (LMN_E_BADARG and lmn_last_error, messages "region_workspace: ...", "region_fwd: ...", "region_bwd: ...").  Not
 * recorded by plans.                                                                                                              */
#ifndef LMNET_REGION_H
#define LMNET_REGION_H
#include "../lmnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMN_REGION_DICE 0            /* kind */
#define LMN_REGION_JACCARD 1
#define LMN_REGION_TVERSKY 2
#define LMN_REGION_GDICE 3
#define LMN_REGION_LINEAR 0          /* denominator */
#define LMN_REGION_SQUARED 1
#define LMN_REGION_SOFTMAX 0         /* head */
#define LMN_REGION_SIGMOID 1
#define LMN_REGION_LABELS_U8 0       /* target_kind */
#define LMN_REGION_LABELS_I64 1
#define LMN_REGION_MAX_BATCH 65535

/* bytes of `workspace`, exactly: the deterministic-mode slots, fp32 [B, nbx, nk, 3] rounded up to 256 bytes, nbx the blocks of the
 * sums pass per image (softmax head) or per plane (sigmoid head) -- a function of head, B, C and H * W alone.  Host arithmetic; -1
 * and lmn_last_error outside the limits above. */
int64_t lmn_region_workspace(int head, int B, int C, int H, int W, uint64_t class_mask);

/* loss[0] = the loss above; all pointers device.
 *   weight     fp32 [nk] or NULL             workspace  lmn_region_workspace bytes (ws_bytes its size); read and written in
 *                                                       deterministic mode only, may be NULL otherwise
 *   sums       fp32 [G, nk, 3]: I, P1, P2    counts     int32 [G, nk, 2]: T, N
 *   coef       fp32 [G, nk, 3]: a, b, c      per_class  fp32 [G, nk]: L_gk, unweighted and unscaled
 * Launches on `stream`: a zero fill of sums and counts, the sums pass, a one-block finish in fp64.  The sums pass: softmax heads
 * with C in {2, 3, 4, 8} run register-resident templates, any other C stages the pixel's logits in LDS; grid.y is the image, so a
 * block never mixes two images and per_image only changes the slot a block adds to.  Sigmoid heads run one grid row per scored
 * (image, class) plane, four elements per lane with 16-byte loads when H * W % 4 == 0 and the bases are aligned, one otherwise.  The
 * instances without P2 serve LMN_REGION_LINEAR. */
int lmn_region_fwd(const float* logits, const void* target, int target_kind, int head, int kind, int denominator, int per_image,
                   float alpha, float beta, float smooth, float exponent, float scale, int B, int C, int H, int W, uint64_t class_mask,
                   const float* weight, void* workspace, int64_t ws_bytes, float* sums, int32_t* counts, float* coef, float* per_class,
                   float* loss, lmn_stream_t stream);

/* dlogits (fp32 [B, C, H, W], every element written) = gscale[0] * d loss / d logits from the coef of lmn_region_fwd on the same
 * arguments; gscale: one device float, or NULL for 1.  One pointwise launch. */
int lmn_region_bwd(const float* logits, const void* target, int target_kind, int head, int per_image, int B, int C, int H, int W,
                   uint64_t class_mask, const float* coef, const float* gscale, float* dlogits, lmn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

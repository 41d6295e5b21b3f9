/* Dense signed Euclidean distance maps of label masks and the two losses built on them: the entries of liblmnet_hip.so behind
 * lm_net_amd.loss.distance_maps, BoundaryLoss and HausdorffDTLoss.  Every other criterion of the package is regional (CE, Dice,
 * focal); these two train against what the HD95 column of SurfaceDistanceMeter reports.  Elsewhere the maps come from
 * scipy.ndimage.distance_transform_edt inside the data loader; here the label map a step sees is made on the device (DeviceAugment)
 * and the thresholded prediction exists only mid-step, so the transform runs on the device too.  These symbols are listed in
 * lm_net_amd.hip.SYMBOLS_DISTMAP, a list of its own that lm_net_amd.hip.load checks next to hip.EXPORTS; tests/test_distmap_cpu.py
 * checks it against this header and ties the three device entries to tests/test_guard_distmap_gpu.py.  Plain arguments only: no
 * struct, no ABI bump.
 *
 * DEFINITIONS.  For one (sample, class) plane with mask M over the H x W pixels, sd2 is the SIGNED SQUARED Euclidean distance between
 * pixel centres:
 *      x outside M:  sd2(x) = +min over q in M      of |x - q|^2
 *      x inside M:   sd2(x) = -min over q outside M of |x - q|^2
 *   The pixels outside the image are neither.  IF M IS EMPTY OR M IS THE WHOLE IMAGE, THE PLANE IS ALL 0 and flagged
 *   (LMN_DISTMAP_FLAG_EMPTY / LMN_DISTMAP_FLAG_FULL); an ordinary plane has no 0 in it.  This is a deliberate difference from scipy,
 *   whose distance_transform_edt returns arbitrary numbers for a mask without a zero; the empty-mask rule is Kervadec's own
 *   `if posmask.any()`.  Elsewhere rint((edt(M) + edt(~M))^2) == |sd2|.
 *   |sd2| <= 2 * 1023^2 < 2^24: every value is an exact int32 AND exactly representable in fp32, which is why the integer square is
 *   what is stored: sqrtf of it in the loss kernels is correctly rounded and identical from run to run.
 *   Masks.  From a label map (int64 or uint8 [B, H, W]): the mask of class k is label == k; a label >= C (or negative) belongs to no
 *   class.  From logits [B, C, H, W], mode softmax: expf(z_k - logsumexp(z)) > threshold in fp32; mode sigmoid: z_k > threshold (a
 *   logit: 0 for the probability 0.5).
 *   The scored classes K are the set bits of class_mask, nk of them, in ascending order.
 *
 *   Boundary term (Kervadec et al., MIDL 2019).  phi_k(x) = sqrtf(sd2) outside the target mask, -(sqrtf(-sd2) - 1) inside
 *      (one_hot2dist: edt(neg) * neg - (edt(pos) - 1) * pos), 0 on a flagged plane.  L_b = (1 / N) sum_valid sum_{k in K} p_k phi_k.
 *   Hausdorff term (Karimi and Salcudean, TMI 2019).  With the target map sd2_g and the map sd2_p of the thresholded prediction (a
 *      constant of the step: no gradient flows through it), w_k(x) = |sd2_p|^(alpha / 2) + |sd2_g|^(alpha / 2) -- for alpha == 2 the
 *      integer sum converted once, no powf --  L_h = (1 / N) sum_valid sum_{k in K} (p_k - g_k)^2 w_k, g_k the 0 / 1 target.
 *   Heads.  Softmax: p = softmax(z) over all C classes, target a label map, valid pixels are those with a label in [0, C), N = valid
 *      pixels * nk; dL/dz_j = p_j ([j in K] dL/dp_j - sum_{k in K} p_k dL/dp_k).  Sigmoid: p_k = sigmoid(z_k), target planes
 *      [B, C, H, W], a valid element is one whose target is 0 or 1 (lmnet_sigmoid.h), N = valid elements of the scored planes.
 *   N = 0 GIVES THE LOSS 0 AND AN ALL-ZERO GRADIENT, never NaN (torch's mean of nothing is NaN); the gradient is +0 at every void pixel.
 *   Parity with MONAI's HausdorffDTLoss / Kervadec's repository is not pinned by the tests (neither is a dependency); these formulas are.
 *
 * LIMITS.  1 <= B, 1 <= C <= 64 (C == 1 only for a sigmoid head), 2 <= H, W <= 1024, B * nk * H * W < 2^31 (and B * C * H * W < 2^31
 * for the loss entries).
 *
 * lmn_dist_map uses integer arithmetic only (the thresholding of logits aside) and no float atomics: two calls are bit-identical in
 * either deterministic mode.  The loss sums use a float atomic per block in ordinary mode and fixed-order slots in deterministic mode
 * (lmn_set_deterministic), like the other losses.  Every loop of every kernel is bounded by a side length or the class count.
 * Every argument error is rejected before any HIP call (LMN_E_BADARG and lmn_last_error, messages "dist_map: ...",
 * "dist_loss_fwd: ...", "dist_loss_bwd: ...").  Not recorded by plans.                                                             */
#ifndef LMNET_DISTMAP_H
#define LMNET_DISTMAP_H
#include "../lmnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMN_DISTMAP_MAX_SIDE 1024
#define LMN_DISTMAP_LABELS_U8 0      /* label_kind / target_kind */
#define LMN_DISTMAP_LABELS_I64 1
#define LMN_DISTMAP_SOFTMAX 0        /* mode of lmn_dist_map from logits; head of the loss entries */
#define LMN_DISTMAP_SIGMOID 1
#define LMN_DISTMAP_FLAG_EMPTY 1     /* flags: 0 an ordinary mask */
#define LMN_DISTMAP_FLAG_FULL 2
#define LMN_DISTMAP_BOUNDARY 0       /* term of the loss entries */
#define LMN_DISTMAP_HAUSDORFF 1
#define LMN_DISTMAP_SUMS_WORDS 4     /* sums: [0] N (uint32)  [1] the sum (float)  [2] scale / N, 0 when N = 0 (float)  [3] 0 */

/* bytes of `workspace` lmn_dist_map needs for B samples x nk classes of H x W pixels, exactly: the masks (uint8 [B * nk, H, W]), the
 * column distances (uint16, the same shape) and the mask sizes (int32 [B * nk]), each rounded up to 256 bytes.  Host arithmetic;
 * -1 and lmn_last_error outside B >= 1, 1 <= nk <= 64, 2 <= H, W <= 1024, B * nk * H * W < 2^31. */
int64_t lmn_dist_workspace(int B, int nk, int H, int W);

/* sd2 (int32 [B, nk, H, W]) and flags (int32 [B, nk]) of the masks of the classes of class_mask (bits >= C must be clear, at least one
 * set).  EXACTLY ONE of logits (fp32 [B, C, H, W]) and labels ([B, H, W] of label_kind) is given, the other is NULL.  From labels,
 * threshold and mode are not read.  From logits: mode LMN_DISTMAP_SOFTMAX (C >= 2; threshold is a probability) or LMN_DISTMAP_SIGMOID
 * (threshold is a logit); the threshold must not be NaN.
 *   workspace  at least lmn_dist_workspace(B, nk, H, W) bytes (device), ws_bytes its size
 * Launches on `stream`: the masks; a column pass (64-row bit masks per lane: the vertical distance of every pixel to the nearest pixel
 * of OPPOSITE membership in its column, uint16, 32768 where the column has none); a row pass, one block per row, that holds the row's
 * two g^2 arrays in LDS (distance to the mask, distance to the complement: 8 KiB at W = 1024) and takes min_j (x - j)^2 + g^2(y, j)
 * scanning outwards from x until d^2 >= the best so far -- at most W - 1 steps per pixel. */
int lmn_dist_map(const float* logits, const void* labels, int label_kind, float threshold, int mode, int B, int C, int H, int W,
                 uint64_t class_mask, void* workspace, int64_t ws_bytes, int32_t* sd2, int32_t* flags, lmn_stream_t stream);

/* loss[0] = scale * L of one term (LMN_DISTMAP_BOUNDARY | LMN_DISTMAP_HAUSDORFF) under one head (LMN_DISTMAP_SOFTMAX: target is a
 * label map [B, H, W]; LMN_DISTMAP_SIGMOID: target is planes [B, C, H, W]) of target_kind; all pointers device.
 *   sd2_g   the target's map, int32 [B, nk, H, W] (lmn_dist_map); a flagged plane is all 0 there, which is all these entries need
 *   sd2_p   the prediction's map of the same shape: required for the Hausdorff term, NULL for the boundary term
 *   alpha   in (0, 8] (the weight stays finite in fp32), read by the Hausdorff term only;  scale: finite
 *   sums    LMN_DISTMAP_SUMS_WORDS words of 4 bytes, written here and read by lmn_dist_loss_bwd
 * Launches on `stream`: a zero fill, the per-block partial pass, a one-block finish. */
int lmn_dist_loss_fwd(const float* logits, const void* target, int target_kind, int head, int term, float alpha, float scale, int B,
                      int C, int H, int W, uint64_t class_mask, const int32_t* sd2_g, const int32_t* sd2_p, void* sums, float* loss,
                      lmn_stream_t stream);

/* dlogits (fp32 [B, C, H, W], every element written) = gscale[0] * d loss / d logits from the sums of lmn_dist_loss_fwd on the same
 * arguments; gscale: one device float, or NULL for 1.  One launch. */
int lmn_dist_loss_bwd(const float* logits, const void* target, int target_kind, int head, int term, float alpha, int B, int C, int H,
                      int W, uint64_t class_mask, const int32_t* sd2_g, const int32_t* sd2_p, const void* sums, const float* gscale,
                      float* dlogits, lmn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

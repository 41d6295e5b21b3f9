/* Hard pixels: the cross entropy of the K hardest elements of a group -- nnU-Net's top-k loss and OHEM (online hard example mining)
 * -- with K formed on the device and the K-th largest value found by an exact three-level radix select: the entries of
 * liblmnet_hip.so behind lm_net_amd.loss.HardPixelLoss and hard_pixel_values.  These symbols are listed in
 * lm_net_amd.hip.SYMBOLS_HARD, a list of its own that lm_net_amd.hip.load checks next to hip.EXPORTS; tests/test_hard_cpu.py checks
 * it against this header and ties the two device entries to tests/test_guard_hard_gpu.py.  Plain arguments only: no struct, no ABI
 * bump.
 *
 * ELEMENTS AND VALUES.  The logits z are fp32 [B, C, H, W]; w = weight (fp32 [C], finite, >= 0; NULL: all 1).
 *   LMN_HARD_SOFTMAX  `target`: a label map [B, H, W] (uint8 or int64).  An element is a pixel, VALID when its label y lies in [0, C);
 *                     l = w[y] * (logsumexp(z) - z[y]), the log-sum-exp max-subtracted.         values: fp32 [B, H, W]
 *   LMN_HARD_SIGMOID  `target`: planes [B, C, H, W].  An element is a (pixel, class) entry, VALID when its target t is 0 or 1;
 *                     l = w[c] * BCE_with_logits(z, t) = w[c] * softplus(t ? -z : z).            values: fp32 [B, C, H, W]
 *   THE STORED VALUE IS CLAMPED TO >= +0, so its raw bits are an order-preserving unsigned key (no sign-flip map); the value
 *   arithmetic is compiled without contraction, so an element gets the same bits from every kernel instance.  A VOID ELEMENT STORES
 *   -1: it sorts below every valid value and enters no histogram, count or sum.
 * GROUPS.  A group is the batch (G = 1) or, with per_image, one image (G = B); under the sigmoid head the classes of a group are pooled.
 * COUNT.  For a group with N valid elements, on the device:
 *   K = min(N, max(1, Kkeep, min_kept, Nhard)),   Kkeep = floor((double)keep * N)  (keep = 0: not given),
 *   Nhard = #{ l > cut } compared in fp32 on the stored values  (cut < 0: not given;  cut = (float)(-log(thresh)) is formed by the caller).
 * TERM AND TIE RULE.  tau = the K-th largest value of the group, n_gt = #{l > tau}, n_eq = #{l == tau}:
 *   term = (sum_{l > tau} l + (K - n_gt) * tau) / K          exactly the mean of the K largest values
 *   the gradient weight of an element is 1 / K where l > tau, (K - n_gt) / (n_eq * K) where l == tau, 0 elsewhere: TIED ELEMENTS AT
 *   THE CUTOFF SHARE THE REMAINING WEIGHT, the weights of a group sum to 1 and no ordering among ties exists.
 *   loss = scale / G * sum_g term_g;   d loss / d z = scale / G * weight_i * w * (softmax(z) - onehot)   (sigmoid: sigmoid(z) - t)
 * EDGE RULES.  A GROUP WITH N = 0 CONTRIBUTES 0 (its record is all 0).  The loss is never NaN for finite logits.  EVERY VOID POSITION
 *   AND EVERY UNSELECTED ELEMENT GETS GRADIENT +0.
 *
 * selection int32 [G, LMN_HARD_RECORD_WORDS]: N, K, n_gt, n_eq, the bits of tau.   terms fp32 [G]: term_g.   loss fp32 [1].
 *
 * LIMITS.  1 <= B <= 65535, 1 <= C <= 64 (C == 1 only under the sigmoid head), H, W >= 1, B * C * H * W < 2^31, and with per_image
 * B <= LMN_HARD_MAX_GROUPS (every group owns three histograms of the workspace).
 *
 * REDUCTION.  No float atomics anywhere: the count and the three histograms (the top 11, the middle 11 and the low 10 key bits) are
 * integer atomics, the sums go to per-block slots that one block adds in block order in fp64, so selection, terms, loss and dlogits
 * are BIT-IDENTICAL FROM CALL TO CALL whether lmn_set_deterministic is on or off.  Every argument error is rejected before any HIP
 * call (LMN_E_BADARG and lmn_last_error, messages "hard_workspace: ...", "hard_fwd: ...", "hard_bwd: ...").  Not recorded by plans. */
#ifndef LMNET_HARD_H
#define LMNET_HARD_H
#include "../lmnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMN_HARD_SOFTMAX 0           /* head */
#define LMN_HARD_SIGMOID 1
#define LMN_HARD_LABELS_U8 0         /* label_kind */
#define LMN_HARD_LABELS_I64 1
#define LMN_HARD_MAX_BATCH 65535
#define LMN_HARD_MAX_GROUPS 1024
#define LMN_HARD_RECORD_WORDS 5
#define LMN_HARD_BINS_HIGH 2048      /* bins of the first two levels (11 key bits each) */
#define LMN_HARD_BINS_LOW 1024       /* bins of the third level (10 key bits) */

/* bytes of `workspace`, exactly: per group uint32 [R * 2048 + 2048 + 1024] histograms -- the first one in R copies that the blocks of
 * the values pass spread their atomics over, R = 8 up to 8 groups, 4 up to 16, 2 up to 32, else 1 -- and int32 [16] partial counts of
 * Nhard (N is the total of the first histogram), rounded up to 256 bytes, then the fp64 slots of the sum pass, one per block,
 * [G, blocks] rounded up to 256 bytes -- a function of head, per_image, B, C and H * W alone.  Host arithmetic; -1 and lmn_last_error outside the limits above. */
int64_t lmn_hard_workspace(int head, int per_image, int B, int C, int H, int W);

/* All pointers device.  `workspace`: lmn_hard_workspace bytes (ws_bytes its size), 8-byte aligned, needed in either mode.  Writes
 * values (every element), selection, terms and loss.  keep in [0, 1], min_kept >= 0, cut (see COUNT); one of the three must be given.
 * Launches on `stream`: a zero fill of the histograms and counts; the values pass (softmax heads with C in {2, 3, 4, 8} run
 * register-resident templates, any other C reads the pixel's logits twice, the second time from the cache, grid.y is the image; sigmoid heads
 * run one grid row per (image, class) plane, four elements per lane with 16-byte loads when H * W % 4 == 0 and the bases are
 * aligned), which also counts Nhard and adds the first histogram from an LDS histogram per block; the second and the third
 * level, each block rescanning its group's previous table for K, the digit and the remaining rank; the sum pass; a one-block finish
 * in fp64.  No kernel waits for another block. */
int lmn_hard_fwd(const float* logits, const void* target, int label_kind, int head, int per_image, float keep, int64_t min_kept,
                 float cut, float scale, int B, int C, int H, int W, const float* weight, void* workspace, int64_t ws_bytes,
                 float* values, int32_t* selection, float* terms, float* loss, lmn_stream_t stream);

/* dlogits (fp32 [B, C, H, W], every element written) = gscale[0] * d loss / d logits from the values and the selection of
 * lmn_hard_fwd on the same arguments; gscale: one device float, or NULL for 1.  One pointwise launch: an element is classified by
 * comparing its SAVED value with tau, so forward and backward cannot disagree about the selection. */
int lmn_hard_bwd(const float* logits, const void* target, int label_kind, int head, int per_image, float scale, int B, int C, int H,
                 int W, const float* weight, const float* values, const int32_t* selection, const float* gscale, float* dlogits,
                 lmn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

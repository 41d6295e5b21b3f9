/* Soft targets: the criteria that read a distribution per pixel instead of an integer label -- cross entropy + Dice against given
 * probabilities or against the two-hot target of a Mixup batch, and the temperature-scaled Kullback-Leibler term of knowledge
 * distillation (Hinton et al. 2015) under a softmax or a sigmoid head -- and the batch mixer that makes Mixup / CutMix batches on the
 * device: the entries of liblmnet_hip.so behind lm_net_amd.loss.SoftSegLoss, DistillLoss and lm_net_amd.data.DeviceMix.  These symbols
 * are listed in lm_net_amd.hip.SYMBOLS_SOFT, a list of its own that lm_net_amd.hip.load checks next to hip.EXPORTS;
 * tests/test_soft_cpu.py checks it against this header and ties the three device entries to tests/test_guard_soft_gpu.py.  Plain
 * arguments only: no struct, no ABI bump.
 *
 * DEFINITIONS.  The student logits z are fp32 [B, C, H, W].  The target comes through one of four READERS:
 *   LMN_SOFT_PROBS         softmax head.  `target`: fp32 q [B, C, H, W], USED AS GIVEN (not renormalised, as torch).  A pixel is VALID
 *                          when every q_c of it is finite and >= 0 (NaN or -1 marks void).
 *   LMN_SOFT_PAIR          softmax head.  `ya`, `yb`: two label maps [B, H, W] of one kind (uint8 or int64), `lam`: fp32 [B] on the
 *                          device;  q = lam onehot(ya) + (1 - lam) onehot(yb), 1 - lam formed in fp32.  A pixel is VALID when both
 *                          labels lie in [0, C).
 *   LMN_SOFT_TEACHER_F32   softmax or sigmoid head.  `target`: teacher logits zt [B, C, H, W], fp32 or bf16, temperature T > 0.
 *   LMN_SOFT_TEACHER_BF16  Softmax: q = softmax(zt / T), p = softmax(z / T);  sigmoid: per element q = sigmoid(zt / T), p = sigmoid(z / T).
 *                          `ya`: NULL (everything is valid) or, softmax head, a label map [B, H, W]: a pixel is VALID when its label
 *                          lies in [0, C);  sigmoid head, target planes [B, C, H, W]: an element is VALID when its value is 0 or 1.
 *   All sums run over the valid pixels (elements under the sigmoid head); N is their count (int32 from integer atomics: exact).
 *
 * TERMS UNDER PROBS AND PAIR.  p = softmax(z), q' = (1 - eps) q + eps / C, w = w_ce, v = w_dice (NULL: all 1), s = smooth >= 0.
 *   ce   = -(1 / N) sum_pix sum_c w_c q'_c log p_c        F.cross_entropy(z, q, weight=w, label_smoothing=eps): torch's probability-
 *                                                          target form DIVIDES BY THE PIXEL COUNT, not by the weight sum
 *   dice = (1 / C) sum_c v_c (1 - (2 I_c + s) / (Z_c + Y_c + s)),  I_c = sum p_c q_c,  Z_c = sum p_c^2,  Y_c = sum q_c^2  (q unsmoothed:
 *          the reference's DiceLoss._dice_loss on a float target)
 *   loss = ce_scale ce + dice_scale dice;   terms = [loss, ce, dice]
 *   GRADIENT of the ce term: (p_k sum_c w_c q'_c - w_k q'_k) / N;  of the dice term: p_k (d_k - sum_c p_c d_c) with
 *          d_c = a_c q_c + c_c p_c,  a_c = d loss / dI_c,  c_c = 2 d loss / dZ_c.
 * TERM UNDER THE TEACHER READERS.
 *   kd   = T^2 / N * sum KL(q || p)   (a per-pixel mean -- per element under the sigmoid head, where KL is the Bernoulli divergence;
 *          torch's batchmean is not reproduced);   loss = scale kd  (scale travels in ce_scale);   terms = [loss, kd, 0]
 *   GRADIENT: scale T (p - q) / N.
 *   log q AND log p COME FROM THE SAME DEVICE FUNCTION -- a max-subtracted log-sum-exp under the softmax head, the softplus pair of the
 *   sigmoid point under the sigmoid head -- so teacher logits bitwise equal to the student's give loss exactly 0.0 and an all-zero
 *   gradient, and logits of +-100 stay finite.  0 * log 0 is 0.
 * EDGE RULES.  EVERY VOID POSITION GETS GRADIENT +0 in every class.  Without a valid pixel every term is 0 with a zero gradient,
 *   never NaN.  A DICE DENOMINATOR THAT IS EXACTLY 0 GIVES A RATIO OF 1 (this needs s = 0).
 *
 * coef fp32 [1 + 2 C]: coef[0] = ce_scale / N (teacher readers: scale T / N), 0 when N = 0; then a_c, c_c per class.
 * sums fp32 [1 + 3 C]: the ce (kd) sum, then I_c, Z_c, Y_c per class (teacher readers: sums[0] only).   counts int32 [1]: N.
 *
 * LIMITS.  1 <= B <= 65535, 1 <= C <= 64 (C == 1 only under the sigmoid head), H, W >= 1, B * C * H * W < 2^31.
 *
 * REDUCTION.  Ordinary mode: one float atomic per block and quantity.  Deterministic mode (lmn_set_deterministic): every block writes
 * its partial sums to a slot of `workspace` and the finish kernel adds the slots in block order, so terms, coef and dlogits are
 * bit-identical from call to call.  N is an integer atomic in both modes.  Every argument error is rejected before any HIP call
 * (LMN_E_BADARG and lmn_last_error, messages "soft_workspace: ...", "soft_fwd: ...", "soft_bwd: ...", "mix_batch: ...").  Not recorded
 * by plans.                                                                                                                        */
#ifndef LMNET_SOFT_H
#define LMNET_SOFT_H
#include "../lmnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMN_SOFT_PROBS 0             /* reader */
#define LMN_SOFT_PAIR 1
#define LMN_SOFT_TEACHER_F32 2
#define LMN_SOFT_TEACHER_BF16 3
#define LMN_SOFT_SOFTMAX 0           /* head */
#define LMN_SOFT_SIGMOID 1
#define LMN_SOFT_LABELS_U8 0         /* label_kind */
#define LMN_SOFT_LABELS_I64 1
#define LMN_SOFT_MAX_BATCH 65535
#define LMN_MIX_NONE 0               /* mode of a row of lmn_mix_batch */
#define LMN_MIX_MIXUP 1
#define LMN_MIX_CUTMIX 2
#define LMN_MIX_ROW_WORDS 8          /* int32 words of a row: partner, mode, lam, 1 - lam (fp32 bits), y0, x0, y1, x1 */

/* bytes of `workspace`, exactly: the deterministic-mode slots, one per block of the sums pass, fp32 [blocks, 1 + 3 C] (teacher
 * readers: [blocks, 1]) rounded up to 256 bytes -- a function of reader, head, B, C and H * W alone.  Host arithmetic; -1 and
 * lmn_last_error outside the limits above. */
int64_t lmn_soft_workspace(int reader, int head, int B, int C, int H, int W);

/* terms[0 .. 2] = the terms above; all pointers device.
 *   target     PROBS: q; teacher readers: zt; PAIR: NULL         ya, yb   see the readers (label_kind: their kind); yb PAIR only
 *   lam        fp32 [B], PAIR only                               w_ce, w_dice  fp32 [C] or NULL, PROBS and PAIR only
 *   workspace  lmn_soft_workspace bytes (ws_bytes its size); read and written in deterministic mode only, may be NULL otherwise
 * Launches on `stream`: a zero fill of sums and counts, the sums pass, a one-block finish in fp64.  The sums pass: softmax heads with
 * C in {2, 3, 4, 8} run register-resident templates, any other C stages the pixel's logits and target in LDS; grid.y is the image.
 * Sigmoid heads run one grid row per (image, class) plane, four elements per lane with 16-byte loads when H * W % 4 == 0 and the
 * bases are aligned, one otherwise.  bf16 teacher logits are loaded four to a lane (8 bytes) when H * W % 4 == 0 and the bases are aligned, under either head. */
int lmn_soft_fwd(const float* logits, int reader, int head, const void* target, const void* ya, const void* yb, int label_kind,
                 const float* lam, float temperature, float eps, float smooth, float ce_scale, float dice_scale, int B, int C, int H,
                 int W, const float* w_ce, const float* w_dice, void* workspace, int64_t ws_bytes, float* sums, int32_t* counts,
                 float* coef, float* terms, lmn_stream_t stream);

/* dlogits (fp32 [B, C, H, W], every element written) = gscale[0] * d loss / d logits from the coef of lmn_soft_fwd on the same
 * arguments; gscale: one device float, or NULL for 1.  One pointwise launch. */
int lmn_soft_bwd(const float* logits, int reader, int head, const void* target, const void* ya, const void* yb, int label_kind,
                 const float* lam, float temperature, float eps, int B, int C, int H, int W, const float* w_ce, const float* coef,
                 const float* gscale, float* dlogits, lmn_stream_t stream);

/* Mixup / CutMix of a device batch, out of place, one pass: x fp32 [B, Cin, H, W], y [B, H, W] of label_kind.  `rows`: HOST int32
 * [B, LMN_MIX_ROW_WORDS], checked and copied into the device buffer rows_dev (the same words) ahead of the launch.  Per sample b:
 *   LMN_MIX_NONE    x_out = x[b], ya = yb = y[b], lam_out = 1
 *   LMN_MIX_MIXUP   x_out = lam x[b] + (1 - lam) x[partner], evaluated UNFUSED as fadd(fmul(lam, a), fmul(1 - lam, b)) with the row's
 *                   fp32 1 - lam (which must equal 1.0f - lam), so contraction cannot change a bit;  ya = y[b], yb = y[partner],
 *                   lam_out = lam
 *   LMN_MIX_CUTMIX  inside the box [y0, y1) x [x0, x1) pixels AND labels come from the partner, outside from b;  ya = yb,
 *                   lam_out = 1: a hard label map, void labels included
 * yb_out may be NULL when no row is a mixup row.  A partner row is read while its own row is written: x_out must not overlap x, nor
 * ya_out / yb_out overlap y.  Limits: 1 <= B <= 65535, 1 <= Cin <= 64, B * Cin * H * W < 2^31, 0 <= lam <= 1, 0 <= y0 <= y1 <= H,
 * 0 <= x0 <= x1 <= W.  Loads of x are 16 bytes when W % 4 == 0 and the bases are aligned. */
int lmn_mix_batch(const float* x, const void* y, int label_kind, const int32_t* rows, int32_t* rows_dev, int B, int Cin, int H, int W,
                  float* x_out, void* ya_out, void* yb_out, float* lam_out, lmn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

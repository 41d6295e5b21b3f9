/* Sigmoid heads: a per-class binary loss (BCE + Dice + focal) and thresholded tp / fp / fn / tn statistics for one-logit (binary) and
 * multi-label models: the entries of liblmnet_hip.so behind lm_net_amd.SigmoidSegLoss, lm_net_amd.SigmoidStatsMeter and
 * lm_net_amd.metrics.sigmoid_labels.  One header per feature: these symbols are listed in lm_net_amd.hip.SYMBOLS_SIGMOID, which
 * lm_net_amd.hip.HEADERS files under this header's name, and the guard manifest (tests/guard.py) ties them to
 * tests/test_guard_sigmoid_gpu.py.
 *
 * Logits are fp32 NCHW [B, C, HW] with C in [1, 64]; the target has the same shape and is uint8 (target_kind LMN_SIG_T_U8) or int64
 * (LMN_SIG_T_I64).  Every class has its own logit plane and its own target plane; classes may overlap.  An element (b, c, i) is VALID
 * when its target is 0 or 1; every other value (255, -100, a stray 7, ...) is void for that element alone: it adds to no sum and
 * receives a gradient of +0.  For C = 1, [B, HW] is the same memory.
 *
 * Limits of every entry: B >= 1, 1 <= HW < 2^31, B * C <= 65535 (one grid row per plane), B * HW < 2^31 (the per-class counts are
 * 32-bit).                                                                                                                         */
#ifndef LMNET_SIGMOID_H
#define LMNET_SIGMOID_H
#include "lmnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMN_SIG_T_U8 0
#define LMN_SIG_T_I64 1

/* 4-byte word counts of the two device workspaces of the loss entries, for C classes                                               */
#define LMN_SIG_SUMS_WORDS(C) (6 * (C))    /* [k][C]: N_c and Y_c (uint32), then I_c, Z_c, the bce sum and the focal sum (float)      */
#define LMN_SIG_COEF_FLOATS(C) (4 * (C))   /* [k][C]: the backward coefficients the forward entry leaves for the backward entry       */

/* The scalar parameters of the loss (HOST memory, read before the entry returns).                                                  */
typedef struct {
  float smooth;          /* the Dice smoothing term (utils/loss.py:185 uses 1e-5), >= 0                                              */
  float bce_scale;       /* factors of the three terms, each >= 0; a term with factor 0 is exactly 0                                 */
  float dice_scale;
  float focal_scale;     /* 0: the focal term is off and the kernels do no focal arithmetic                                          */
  float focal_gamma;     /* >= 0; 0 gives the modulating factor 1 exactly                                                            */
  float focal_alpha;     /* <= 1; negative: no alpha weighting                                                                       */
  int32_t target_kind;   /* LMN_SIG_T_U8 or LMN_SIG_T_I64                                                                            */
  int32_t _pad[9];       /* fixed size: 64 bytes                                                                                     */
} lmn_sig_param_t;
int lmn_sizeof_sig_param(void);

/* loss4[0..3] = total, bce, dice, focal (device, each term already scaled; total is their sum).  With p = sigmoid(z), N_c the number
 * of valid elements of class c, N = sum_c N_c, and per-class device vectors w_bce, pos_weight, w_dice [C]:
 *   bce   = bce_scale * (1 / N) sum_c w_bce[c] sum_valid [pos_weight[c] t softplus(-z) + (1 - t) softplus(z)]
 *           -- F.binary_cross_entropy_with_logits(z, t, weight, pos_weight), mean over the valid elements, weights per class;
 *   dice  = dice_scale * (1 / C) sum_c w_dice[c] (1 - (2 I_c + smooth) / (Z_c + Y_c + smooth)),
 *           I_c = sum_valid p t, Z_c = sum_valid p^2, Y_c = sum_valid t
 *           -- DiceLoss._dice_loss(sigmoid(z[:, c]), t[:, c], ignore_c) weighted and averaged as DiceLoss.forward (utils/loss.py:183-206);
 *   focal = focal_scale * sum_c (1 / N_c) sum_valid a_t (1 - q_t)^gamma bce(z, t),  q_t and a_t as in lmnet_loss.h
 *           -- FocalLoss.forward (utils/loss.py:126-148), each class's mean restricted to its valid elements.
 * Deliberate difference from torch: with N = 0 the bce term and its gradient are 0, and a class with N_c = 0 adds 0 to the focal term;
 * no NaN reaches the step.
 * sums [LMN_SIG_SUMS_WORDS(C) words] and coef [LMN_SIG_COEF_FLOATS(C)] are device workspaces; coef feeds the backward entry.
 * Three launches (a clear of sums, the plane sums, a one-block finish).  A block works on one (b, c) plane only; a lane takes four
 * consecutive elements with 16-byte loads when HW % 4 == 0 and the logits are 16-byte aligned (and the target 4-byte aligned for
 * uint8, 16-byte for int64), one element otherwise.  The two counts are integer atomics; deterministic mode (see lmnet_hip.h) adds
 * the float partials in a fixed order and gives bit-identical results from run to run.  Argument errors (null pointer, C outside
 * [1, 64], a negative scale, smooth or gamma, alpha above 1, an unknown target_kind, sizes beyond the limits above) are rejected
 * before any HIP call.                                                                                                             */
int lmn_sigloss_fwd(const float* logits, const void* target, const float* w_bce, const float* pos_weight, const float* w_dice, int B,
                    int C, int64_t HW, const lmn_sig_param_t* param, void* sums, float* coef, float* loss4, lmn_stream_t stream);

/* dlogits [B, C, HW] = gscale[0] * d total / d logits (gscale: device scalar, NULL means 1) from the coef of the forward entry called
 * with the same logits, target, weights and parameters.  One read of logits and target, one write of dlogits; void elements are
 * written as +0.                                                                                                                   */
int lmn_sigloss_bwd(const float* logits, const void* target, const float* pos_weight, const float* coef, const float* gscale, int B,
                    int C, int64_t HW, const lmn_sig_param_t* param, float* dlogits, lmn_stream_t stream);

/* An element is predicted ON when z >= logit_threshold, compared in fp32 (the host passes log(thr / (1 - thr)), exactly 0 at
 * thr = 0.5): get_stats(sigmoid(z), t, mode = "binary" | "multilabel", threshold = thr) of utils/functional.py:61-219 away from
 * rounding ties.  At least one output is given:
 *   stats      int64 [B][C][4], OVERWRITTEN: tp, fp, fn, tn over the valid elements of that (image, class) plane, so the four sum to
 *              the plane's valid count; needs a target;
 *   labels_out uint8 [B, C, HW], 0 or 1: the thresholded prediction of every element, void or not; target may be NULL.
 * Integer arithmetic only (wave ballots, one integer atomic per block and counter): exact, and identical from call to call.          */
int lmn_sigmoid_stats(const float* logits, const void* target, int target_kind, float logit_threshold, int B, int C, int64_t HW,
                      int64_t* stats, uint8_t* labels_out, lmn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

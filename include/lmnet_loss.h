/* Void (ignore) labels in the training loss, a focal term, and per-image tp / fp / fn / tn statistics: the entries of
 * liblmnet_hip.so behind lm_net_amd.SegLoss(ignore_index=..., focal_scale=...), lm_net_amd.FocalLoss and lm_net_amd.ImageStatsMeter.
 * One header per feature: these symbols are listed in lm_net_amd.hip.SYMBOLS_LOSS, which lm_net_amd.hip.HEADERS files under this
 * header's name, and the guard manifest (tests/guard.py) ties them to tests/test_guard_loss_gpu.py.
 *
 * A pixel is VALID when its label y lies in [0, C); every other label is void: ignore_index (which must lie outside [0, C), e.g. the
 * 255 of VOC2012 or torch's -100) and any other out-of-range value alike, in line with the confusion entry of lmnet_hip.h, which
 * drops such labels.  A void pixel adds to no sum of any term and receives a zero gradient in every class.                         */
#ifndef LMNET_LOSS_H
#define LMNET_LOSS_H
#include "lmnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* float counts of the two device workspaces of the loss entries, for C classes                                                     */
#define LMN_LOSS_SUMS_FLOATS(C) (4 + 3 * (C))   /* S_w, NLL sum, smoothing sum, focal sum, then I_c, Z_c, Y_c                          */
#define LMN_LOSS_COEF_FLOATS(C) (4 + 2 * (C))   /* the backward coefficients the forward entry leaves for the backward entry           */

/* The scalar parameters of the loss (HOST memory, read before the entry returns).                                                  */
typedef struct {
  int64_t ignore_index;   /* the void label; read when has_ignore != 0, and then required to lie outside [0, C)                      */
  int32_t has_ignore;     /* 0: no ignore_index (labels outside [0, C) are void all the same)                                        */
  float label_smoothing;  /* eps of the cross entropy, in [0, 1]                                                                     */
  float smooth;           /* the Dice smoothing term (utils/loss.py:185 uses 1e-5), >= 0                                             */
  float ce_scale;         /* factors of the three terms, each >= 0; a term with factor 0 is exactly 0                                */
  float dice_scale;
  float focal_scale;      /* 0: the focal term is off and the kernels do no sigmoid work                                             */
  float focal_gamma;      /* >= 0; 0 gives the modulating factor 1 exactly                                                           */
  float focal_alpha;      /* <= 1; negative: no alpha weighting (as torchvision.ops.sigmoid_focal_loss)                              */
  int32_t _pad[6];        /* fixed size: 64 bytes                                                                                    */
} lmn_loss_param_t;
int lmn_sizeof_loss_param(void);

/* loss4[0..3] = total, ce, dice, focal (device, each term already scaled; total is their sum) of fp32 NCHW logits [B, C, HW] and
 * int64 labels [B, HW], C in [2, 64].  With p = softmax over classes, N_v the number of valid pixels, S_w = sum_valid w_ce[y]:
 *   ce    = ce_scale * [(1 - eps) sum_valid w_y (-log p_y) + (eps / C) sum_valid sum_c w_c (-log p_c)] / S_w
 *           -- F.cross_entropy(weight, label_smoothing, ignore_index), mean reduction (train.py:157 with void labels);
 *   dice  = dice_scale * (1 / C) sum_c w_dice[c] (1 - (2 I_c + smooth) / (Z_c + Y_c + smooth)),
 *           I_c = sum_valid p_c t_c, Z_c = sum_valid p_c^2, Y_c = sum_valid t_c
 *           -- DiceLoss.forward with its `ignore` mask (utils/loss.py:183-206);
 *   focal = focal_scale * sum_c (1 / N_v) sum_valid a_t (1 - q_t)^gamma bce(z_c, t_c),  q = sigmoid(z_c), q_t = q t + (1 - q)(1 - t),
 *           a_t = alpha t + (1 - alpha)(1 - t), or 1 when alpha < 0
 *           -- FocalLoss.forward (utils/loss.py:126-148: a per-class sigmoid focal loss, mean over pixels) restricted to valid pixels.
 * Deliberate difference from torch: when N_v = 0 (or S_w = 0) ce and focal are 0 with a zero gradient, not NaN; with every pixel
 * void the total is finite and the gradient is all zero.
 * sums [LMN_LOSS_SUMS_FLOATS(C)] and coef [LMN_LOSS_COEF_FLOATS(C)] are device workspaces; coef feeds the backward entry.
 * Three launches (a clear of sums, the batch sums, a one-block finish); C in {2, 3, 4, 8} run register-resident templates, other counts
 * stage the logits in LDS.  Deterministic mode (see lmnet_hip.h) gives bit-identical results from run to run.  Argument errors
 * (null pointer, C outside [2, 64], ignore_index inside [0, C), eps outside [0, 1], a negative scale, smooth or gamma, alpha above 1)
 * are rejected before any HIP call.                                                                                                */
int lmn_segloss_ex_fwd(const float* logits, const int64_t* target, const float* w_ce, const float* w_dice, int B, int C, int64_t HW,
                       const lmn_loss_param_t* param, float* sums, float* coef, float* loss4, lmn_stream_t stream);

/* dlogits [B, C, HW] = gscale[0] * d total / d logits (gscale: device scalar, NULL means 1) from the coef of the forward entry called
 * with the same logits, labels, weights and parameters.  One read of logits and labels, one write of dlogits; void pixels are
 * written as +0 in every class.                                                                                                    */
int lmn_segloss_ex_bwd(const float* logits, const int64_t* target, const float* w_ce, const float* coef, const float* gscale, int B,
                       int C, int64_t HW, const lmn_loss_param_t* param, float* dlogits, lmn_stream_t stream);

/* stats [B][C][4] (int64, OVERWRITTEN) = tp, fp, fn, tn per image and class, over the image's valid pixels -- get_stats in
 * mode "multiclass" with ignore_index (utils/functional.py:61-201) -- so that tp + fp + fn + tn is the image's valid-pixel count
 * for every class.  Exactly one prediction is given: fp32 logits [B, C, HW] (arg-max, first maximum wins) or a uint8 label map
 * [B, HW] whose values >= C mean "no class" (such a pixel is a false negative of its label and a true negative elsewhere).
 * Integer arithmetic only: exact, and identical from call to call.  A block never mixes two images.  HW < 2^31, B <= 65535.         */
int lmn_image_stats(const float* logits, const uint8_t* pred_labels, const int64_t* target, int B, int C, int64_t HW, int has_ignore,
                    int64_t ignore_index, int64_t* stats, lmn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

/* Parameter groups, gradient clipping, the loss-scale skip and weight averaging (EMA) for the one-launch AdamW: the entries of
 * liblmnet_hip.so behind lm_net_amd.optim.FusedAdamW(groups, max_norm=..., skip_nonfinite=..., ema_decay=...) and its GradScaler
 * protocol.  These symbols are listed in lm_net_amd.hip.SYMBOLS_OPTIM, a list of its own that lm_net_amd.hip.load checks next to
 * hip.EXPORTS; tests/test_optim_cpu.py checks it against this header and ties the two entries that write device memory to their guard
 * test, tests/test_guard_optim_gpu.py.
 *
 * Two entries per step, both over the flat parameter layout of lm_net_amd.LM_Net (n floats, n % 4 == 0):
 *   lmn_optim_prepare   a deterministic reduction over the flat gradient that leaves a 16-word CONTROL BLOCK on the device;
 *   lmn_adamw_step_ex   lmn_adamw_step of lmnet_hip.h, reading that block: nothing about a step is decided on the host, so the pair
 *                       can sit inside a captured graph, and a step that must be skipped costs no synchronisation.
 * The flat buffers are cut into QUADS of four floats.  qgroup [n / 4] (uint8, device) names the parameter group of every quad; the
 * layout keeps every parameter 16-byte aligned, so a quad never straddles two parameters (padding quads belong to their parameter's
 * group; their gradient is zero).                                                                                                   */
#ifndef LMNET_OPTIM_H
#define LMNET_OPTIM_H
#include "../lmnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMN_OPTIM_MAX_GROUPS 16
#define LMN_OPTIM_GRID_CAP 1024      /* blocks of the reduction (256 lanes, one quad per lane and iteration): the cap of the losses  */

/* flags of lmn_optim_param_t                                                                                                        */
#define LMN_OPTIM_SKIP_NONFINITE 1   /* a non-finite gradient value, or an incoming found_inf, skips the step                         */
#define LMN_OPTIM_NORM 2             /* run the reduction (norm and non-finite count); required by max_norm > 0 and by the skip flag  */

/* words (4 bytes each) of the control block                                                                                         */
#define LMN_OPTIM_CTRL_WORDS 16
#define LMN_OPTIM_SKIP 0             /* uint32: 1 when this step is skipped                                                           */
#define LMN_OPTIM_STEP 1             /* uint32: steps taken (step += !skip)                                                           */
#define LMN_OPTIM_SKIPPED 2          /* uint32: steps skipped (skipped += skip)                                                       */
#define LMN_OPTIM_GRAD_NORM 3        /* float: L2 norm of the unscaled gradient of the non-frozen groups, before clipping             */
#define LMN_OPTIM_INV_SCALE 4        /* float: 1 / grad_scale[0], or 1                                                                */
#define LMN_OPTIM_COEF 5             /* float: min(1, max_norm / (grad_norm + 1e-6)) -- torch.nn.utils.clip_grad_norm_ -- or 1        */
#define LMN_OPTIM_INV_BC1 6          /* float: 1 / (1 - beta1^step) for the new step count                                            */
#define LMN_OPTIM_INV_SQRT_BC2 7     /* float: 1 / sqrt(1 - beta2^step)                                                               */
#define LMN_OPTIM_NONFINITE 8        /* uint32: non-finite gradient values counted by this call (frozen groups are not counted)      */

/* The workspace (device, 4-byte words, ZEROED once by the caller before the first step; it carries the step counts from call to
 * call), with G = min(ceil(n / 1024), LMN_OPTIM_GRID_CAP) blocks of the reduction:
 *   [0, G)                  float   block partials of the sum of squares
 *   [G, 2G)                 uint32  block counts of non-finite values
 *   [2G, 2G + 16)                   the control block
 *   [2G + 16, 2G + 16 + 64) float   the group table [LMN_OPTIM_MAX_GROUPS][4]: lr, weight_decay, frozen (!= 0), spare -- written
 *                                   by the CALLER (lm_net_amd.optim refreshes it from pinned memory when a group's lr changes)
 * lmn_optim_workspace returns that word count (0 for n <= 0).                                                                       */
int64_t lmn_optim_workspace(int64_t n);
#define LMN_OPTIM_GROUP_WORDS (4 * LMN_OPTIM_MAX_GROUPS)

/* The scalar parameters shared by the two entries (HOST memory, read before the entry returns).  The betas are doubles so that the
 * bias corrections 1 - beta^step formed on the device are those lm_net_amd.optim forms on the host for lmn_adamw_step.             */
#define LMN_OPTIM_PARAM_BYTES 64
typedef struct {
  double beta1, beta2;    /* in [0, 1)                                                                                               */
  float eps;              /* > 0                                                                                                     */
  float max_norm;         /* <= 0: no clipping                                                                                       */
  float ema_decay;        /* < 0: no EMA; else in [0, 1]                                                                             */
  int32_t flags;          /* LMN_OPTIM_*                                                                                             */
  int32_t n_groups;       /* 1 .. LMN_OPTIM_MAX_GROUPS; every qgroup value must be below it                                          */
  int32_t _pad[7];        /* fixed size: LMN_OPTIM_PARAM_BYTES; lm_net_amd.hip.load compares its mirror with the export below  */
} lmn_optim_param_t;
int lmn_sizeof_optim_param(void);

/* Pass 1 (with LMN_OPTIM_NORM): G blocks, grid-stride, 16-byte loads; each block sums g^2 over the quads whose group is not frozen
 * and counts the values x with !(|x| <= FLT_MAX), reduces per wave, then per block in a fixed order, and writes one partial and one
 * count with plain stores -- no float atomics: the result is bit-identical from run to run in both determinism modes.
 * Pass 2: one block adds the partials in a fixed order in double precision, reads grad_scale[0] and found_inf[0] (device floats, either
 * may be NULL: the two tensors torch.amp.GradScaler hangs on an optimizer) and writes the control block.  Without LMN_OPTIM_NORM pass 1
 * is not launched: grad_norm = 0, coef = 1 and nothing skips the step (found_inf is honoured under LMN_OPTIM_SKIP_NONFINITE only).
 * Argument errors (null pointer, n % 4, n_groups outside 1..16, a beta outside [0, 1), eps <= 0, ema_decay above 1, clipping or the
 * skip flag without LMN_OPTIM_NORM) are rejected before any HIP call.                                                               */
int lmn_optim_prepare(const float* g, int64_t n, const uint8_t* qgroup, const lmn_optim_param_t* param, float* ws,
                      const float* grad_scale, const float* found_inf, lmn_stream_t stream);

/* One AdamW step from the control block lmn_optim_prepare left in ws.  Every lane reads the block; with skip set it returns without
 * a store: p, m, v and ema stay bit-identical (and prepare has not advanced the count).  Otherwise, per quad of group k:
 *   gu = g * inv_scale;  ge = gu * coef          (the multiplication order of unscale followed by clip)
 *   p *= 1 - lr_k * wd_k;  m = b1 m + (1 - b1) ge;  v = b2 v + (1 - b2) ge^2;  p -= (lr_k / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
 *   ema = d * ema + (1 - d) * p                  (ema may be NULL; required when ema_decay >= 0)
 * A quad of a frozen group is neither read past its group byte nor stored.  g is READ-ONLY: the gradient buffer is NOT unscaled or
 * clipped in place (unlike GradScaler.unscale_ and clip_grad_norm_), so p.grad still holds the scaled, unclipped values afterwards. */
int lmn_adamw_step_ex(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const uint8_t* qgroup,
                      const lmn_optim_param_t* param, const float* ws, lmn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

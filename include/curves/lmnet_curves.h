/* Threshold sweeps of a prediction: the entries of liblmnet_hip.so behind lm_net_amd.metrics.CurveMeter (ROC, precision-recall, AUROC,
 * average precision, the best threshold of any thresholded metric).  They stand in for the `AUROC` of the reference's torchmetrics
 * collection (train.py:29) and for running lmn_sigmoid_stats once per threshold.  These symbols are listed in
 * lm_net_amd.hip.SYMBOLS_CURVES, a list of its own that lm_net_amd.hip.load checks next to hip.EXPORTS; tests/test_curves_cpu.py
 * checks it against this header and ties the entry that writes device memory to its guard test, tests/test_guard_curves_gpu.py.
 *
 * The device counts, the host sums: one launch gives, per (image, class) plane, a histogram of the scores of the positive and of the
 * negative elements over the bins a table of thresholds cuts.  Integer counting only, no float atomics: the result does not depend on
 * the order of arrival, two calls are bit-identical in either deterministic mode, and a brute-force count on the host equals it
 * number for number.
 *
 * BIN RULE.  edges[0 .. n_edges) is non-decreasing fp32 (+-inf allowed).  The bin of an element with score s is
 *     b = #{k : s >= edges[k]},   0 <= b <= n_edges,
 * every comparison made in fp32 against the table itself (an upper-bound search; no arithmetic on s such as floor(s * n)).  A NaN
 * score gives b = 0: the element is predicted off at every threshold, the rule of lmn_sigmoid_stats.  "Predicted on at threshold k"
 * is b >= k + 1, so tp / fp at every threshold are suffix sums of the two histograms.                                              */
#ifndef LMNET_CURVES_H
#define LMNET_CURVES_H
#include "../lmnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMN_CURVE_MAX_EDGES 1024
#define LMN_CURVE_MAX_CLASSES 64

#define LMN_CURVE_RAW 0              /* score_kind: the score is the value itself (logits against logit edges, probability maps
                                        against probability edges: the host decides what the table holds)                        */
#define LMN_CURVE_SOFTMAX 1          /* the score of class c at a pixel is expf(z_c - L), L = m + logf(sum_j expf(z_j - m)),
                                        m = max_j z_j over the pixel's C logits (2 <= C <= 64); no S - e_c, so no cancellation.
                                        A pixel with a NaN or infinite logit has NaN scores where L is: bin 0                     */

#define LMN_CURVE_PLANES 0           /* target_form: the target has the size of `values`; 1: positive, 0: negative, else void     */
#define LMN_CURVE_LABELS 1           /* a label map [B, HW]; positive for class c where label == c, a label outside [0, C) makes
                                        the pixel void for every class                                                            */

#define LMN_CURVE_T_U8 0             /* target_kind: uint8 or int64 elements, for both forms                                      */
#define LMN_CURVE_T_I64 1

/* bytes of `workspace`: 0 for LMN_CURVE_RAW, 4 * B * HW (the per-pixel L) for LMN_CURVE_SOFTMAX; -1 on an unknown score_kind or
 * sizes beyond the limits below.  Host arithmetic.                                                                                 */
int64_t lmn_curve_workspace(int score_kind, int B, int64_t HW);

/* hist[B, C, 2, n_edges + 1] (int64, zeroed and overwritten): hist[b, c, 1, :] counts the valid elements of plane (b, c) that belong
 * to class c by the bin of their score, hist[b, c, 0, :] those that do not; void elements are counted nowhere, so the sum of a
 * plane's 2 (n_edges + 1) cells is its valid count.
 *   values     fp32 [B, C, HW], contiguous (device)
 *   target     LMN_CURVE_PLANES: [B, C, HW]; LMN_CURVE_LABELS: [B, HW]; elements of target_kind (device)
 *   edges      fp32 [n_edges], non-decreasing (device; not checked), 1 <= n_edges <= LMN_CURVE_MAX_EDGES
 *   workspace  lmn_curve_workspace bytes (device), written only for LMN_CURVE_SOFTMAX; may be NULL for LMN_CURVE_RAW
 * Limits: 1 <= C <= 64 (2 <= C for LMN_CURVE_SOFTMAX), B * C <= 65535, HW >= 1, B * HW < 2^31.
 * Argument errors (null pointer, an unknown kind or form, n_edges, C, a missing workspace, the limits) are rejected before any HIP
 * call.                                                                                                                            */
int lmn_curve_hist(const float* values, const void* target, int target_kind, int target_form, int score_kind, const float* edges,
                   int n_edges, int B, int C, int64_t HW, void* workspace, int64_t* hist, lmn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

/* Per-lesion detection and panoptic quality of a label VOLUME: the entries of liblmnet_hip.so behind lm_net_amd.metrics.LesionMeter.
 * The lesion-wise column of a results table -- how many target lesions were found, how many predicted lesions are false alarms,
 * lesion-wise F1, panoptic quality -- which a caller otherwise takes through .cpu() and scipy.ndimage.label for every validation
 * case.  The pooled meters cannot give it: a voxel-wise Dice of 0.9 says nothing about a missed 30-voxel lesion.  What these entries
 * add to lmn_cc3d_label of include/volpost/lmnet_volpost.h is the JOIN between the components of the prediction and those of the
 * target.  These symbols are listed in lm_net_amd.hip.SYMBOLS_LESION, a list of its own that lm_net_amd.hip.load checks next to
 * hip.EXPORTS; tests/test_lesion_cpu.py checks it against this header and ties lmn_lesion_match to its guard test in
 * tests/test_guard_lesion_gpu.py.  Plain arguments only: no struct, no ABI bump.
 *
 * DEFINITIONS.  For one case Lp (prediction) and Lt (target) are uint8 label volumes [D, H, W]; a 2D image is a one-slice case.  A
 * value >= C is read as 0 on BOTH sides, so void target voxels are background for these entries.
 *   Lesions.  For each scored class k, the lesions are the components of Lp == k (side 0, sizes n_p) and of Lt == k (side 1, sizes
 *      n_g) under `connectivity` 6, 18 or 26 (scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3)): the components of
 *      lmn_cc3d_label.  The root of a lesion is its smallest linear voxel index (z * H + y) * W + x; the root identifies the lesion
 *      and, through the label of that voxel, its class.
 *   Pairs.  For every pair (p, g) of lesions of the same class that share a voxel, n_pg is the number of shared voxels.
 *   Detection by overlap (parameters overlap = tau in [0, 1], min_size >= 0).  Components with fewer than min_size voxels are dropped
 *      from both sides, and their pairs go with them.  o_g = sum_p n_pg, o_p = sum_g n_pg.  g is detected iff o_g >= 1 and
 *      o_g >= tau n_g; p is a hit iff o_p >= 1 and o_p >= tau n_p (both comparisons in float64).  det_tp = detected targets,
 *      det_fn = |G| - det_tp, det_fp = predictions that are no hit; sensitivity = det_tp / |G|, precision = (|P| - det_fp) / |P|,
 *      f1 = 2 s p / (s + p), 0 when s + p = 0; a ratio is nan where its denominator is 0.
 *   Matching by IoU (parameter iou = theta in [0.5, 1)).  (p, g) is matched iff n_pg / (n_p + n_g - n_pg) > theta; the match is
 *      unique because theta >= 0.5.  tp, fp = |P| - tp, fn = |G| - tp; sq = sum IoU / tp, rq = tp / (tp + fp / 2 + fn / 2),
 *      pq = sq rq: 0 when tp = 0 and the denominator is positive, nan when there are no lesions on either side.
 *      lesion_dice = sum over matched pairs of 2 n_pg / (n_p + n_g), divided by tp + fp + fn: in the spirit of the BraTS lesion-wise
 *      Dice, without its dilation; it is not that challenge's code.
 * The entries produce the exact integers n_p, n_g and n_pg; the formulas run on the host (lm_net_amd.metrics.lesion_metrics).
 *
 * RECORDS.  A component record is key = side << 40 | class << 32 | root with its size; a pair record is key = root_p << 32 | root_g
 * with its count n_pg.  Keys are below 2^62; an unused slot holds LMN_LESION_EMPTY = -1 (all bits set), which no key can take, and a
 * size or count of 0.  THE SLOT A RECORD LANDS IN DEPENDS ON ARRIVAL ORDER; THE SET OF RECORDS DOES NOT: two calls on one input give
 * the same records, possibly in other slots.  A caller that needs bit-identical tensors sorts by key (LesionMeter.close_case does).
 *
 * LIMITS.  1 <= D <= 1024, 2 <= H, W <= 1024, 2 <= C <= 64: D * H * W <= 2^30, so a voxel index, a size and a count are int32.
 *
 * Integer arithmetic and integer atomics only.  No kernel waits for another thread or block: every probe loop is bounded by the slot
 * count.  Every argument error is rejected before any HIP call (LMN_E_BADARG and lmn_last_error, messages "lesion_match: ...").  Not
 * recorded by plans.                                                                                                               */
#ifndef LMNET_LESION_H
#define LMNET_LESION_H
#include "../lmnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMN_LESION_MAX_SIDE 1024
#define LMN_LESION_MIN_SLOTS 64
#define LMN_LESION_MAX_SLOTS 4194304
#define LMN_LESION_NCTRL 4

/* bytes of `workspace` lmn_lesion_match needs for a D x H x W volume, exactly: the roots and the sizes of both labellings, four int32
 * arrays [D, H, W], each rounded up to 256 bytes.  Host arithmetic; -1 and lmn_last_error outside 1 <= D <= 1024, 2 <= H, W <= 1024. */
int64_t lmn_lesion_workspace(int D, int H, int W);

/* ONE case: pred = Lp and target = Lt (uint8 [D, H, W], device, read only).
 *   1. Both volumes are labelled with lmn_cc3d_label under `connectivity` (6, 18 or 26) into `workspace`.
 *   2. comp_keys (int64 [max_components]) / comp_sizes (int32 [max_components]), device: one record per lesion of a class of
 *      class_mask on either side (bit k set: class k is scored; bit 0 and bits >= C must be clear).
 *   3. pair_keys (int64 [pair_slots]) / pair_counts (int32 [pair_slots]), device: the open-addressing table of the pairs; pair_slots
 *      is a power of two in [64, 2^22].
 *   4. ctrl (int32 [4], device): the lesions found (which may exceed max_components: the records beyond the capacity are not
 *      written), the pairs stored, the pair INSERTIONS that found the table full (an insertion carries the shared voxels of one pair
 *      seen by one block; 0 means that every n_pg is complete), and 0.
 * The entry initialises every output itself (keys to LMN_LESION_EMPTY, sizes, counts and ctrl to 0).
 *   workspace  at least lmn_lesion_workspace(D, H, W) bytes (device), ws_bytes its size
 * Launches on `stream`: the two labellings, then one pass over the voxels that appends the component records (one ballot per record
 * kind, one atomic add per wave on ctrl[0]) and fills the pair table: the voxels where prediction and target agree on a scored class
 * are reduced per wave and per block in a small table in LDS first, so that two full masks do not send every voxel's atomic to one
 * word; a global insertion is linear probing with a 64-bit compare-and-swap (EMPTY -> key) and an atomic add on the count.        */
int lmn_lesion_match(const uint8_t* pred, const uint8_t* target, int D, int H, int W, int C, int connectivity, uint64_t class_mask,
                     void* workspace, int64_t ws_bytes, int64_t* comp_keys, int32_t* comp_sizes, int max_components, int64_t* pair_keys,
                     int32_t* pair_counts, int pair_slots, int32_t* ctrl, lmn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

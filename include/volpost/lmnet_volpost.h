/* 3D connected-component cleaning of a label VOLUME: the entries of liblmnet_hip.so behind lm_net_amd.post.VolumePostprocess.  The
 * standard output step of a CT pipeline -- keep the largest 3D component of an organ (the two largest for kidneys and lungs), drop
 * components below a volume, fill cavities -- which a caller otherwise takes through .cpu() and scipy.ndimage.label /
 * binary_fill_holes for every validation case, between two things that run on the device: the arg-max of the prediction and
 * lmn_volume_dist of include/volume/lmnet_volume.h.  lmn_post_clean of include/lmnet_hip.h cleans every slice as its own 2D sample,
 * which is wrong for a case: an organ's second island in a slice is joined to it through the neighbouring slices.  These symbols are
 * listed in lm_net_amd.hip.SYMBOLS_VOLPOST, a list of its own that lm_net_amd.hip.load checks next to hip.EXPORTS;
 * tests/test_volpost_cpu.py checks it against this header and ties the two entries that write device memory to their guard tests in
 * tests/test_guard_volpost_gpu.py.  Plain arguments only: no struct, no ABI bump.
 *
 * DEFINITIONS.  L0 is a uint8 label volume [D, H, W] with values in [0, C) (lmn_post_clean without cleaning writes one: arg-max,
 * first maximum wins, values outside [0, C) -> 0).
 *   1. Components: voxels joined by a path of `connectivity`-neighbour steps (6, 18 or 26: scipy.ndimage.generate_binary_structure(3,
 *      1 | 2 | 3)) through voxels of equal label; every label, 0 included, is partitioned.  A component's root is the smallest linear
 *      index (z * H + y) * W + x of its voxels.
 *   2. Cleaning, for each class k of class_mask: the keep_largest[k] largest components survive (all of them when that is 0; equal
 *      sizes: the smaller root first); among those, the ones with at least min_volume[k] voxels survive.  Voxels of the others
 *      become 0 -> L1.
 *   3. Holes, on L1: a component of label 0 under the DUAL connectivity (6 for 18 and 26, 26 for 6) with no voxel on any of the six
 *      faces of the volume and at most hole_limit voxels is a hole; its voxels take the label of the voxel at x - 1 of its root voxel
 *      (non-zero by construction) -> L2.  scipy.ndimage.binary_fill_holes(L1 > 0, generate_binary_structure(3, 1 or 3)) plus a
 *      labelling rule.  In a one-slice volume every voxel lies on a face: it has no holes.
 *   4. stats[k] = (components of class k in L0, components of class k that survive, voxels of class k in L2, holes filled for k = 0
 *      and 0 otherwise).
 *
 * LIMITS.  1 <= D <= 1024, 2 <= H, W <= 1024, 2 <= C <= 64: D * H * W <= 2^30, so a voxel index and a component size are int32
 * (a byte offset is not: the entries do their pointer arithmetic in 64 bits).
 *
 * Integer arithmetic and integer atomics only: two calls on one input are bit-identical, in either deterministic mode.  No kernel
 * waits for another block.  Every argument error is rejected before any HIP call (LMN_E_BADARG and lmn_last_error).  Not recorded by
 * plans.                                                                                                                           */
#ifndef LMNET_VOLPOST_H
#define LMNET_VOLPOST_H
#include "../lmnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMN_VOLPOST_MAX_SIDE 1024
#define LMN_VOLPOST_MAX_KEEP 4
#define LMN_VOLPOST_NSTAT 4

/* bytes of `workspace` lmn_volpost_clean needs for a D x H x W volume, exactly: L1 (1 byte per voxel), the roots and the sizes of a
 * labelling (int32 each), one bit per voxel for "this root's component touches a face", and 64 x 4 selection words of 8 bytes; each
 * of the five arrays rounded up to 256 bytes.  Host arithmetic; -1 and lmn_last_error outside the limits above.                    */
int64_t lmn_volpost_workspace(int D, int H, int W);

/* Step 1 alone: the labelling of labels [D, H, W] (uint8, device, read only) under connectivity 6, 18 or 26 into roots and sizes
 * (int32 [D, H, W], device): roots = the root of the voxel's component, sizes = the component's voxel count at its root voxel and 0
 * elsewhere.  Every value of labels is partitioned as it stands (no range test).  No workspace.                                    */
int lmn_cc3d_label(const uint8_t* labels, int D, int H, int W, int connectivity, int32_t* roots, int32_t* sizes, lmn_stream_t stream);

/* Steps 1 - 4 of ONE case: labels = L0 (uint8 [D, H, W], device, read only; lmn_post_clean writes values in [0, C), and a value
 * >= C is read as 0 here) -> labels_out = L2 (uint8 [D, H, W], device, another buffer than labels) and stats (int32 [C][4], device,
 * zeroed and overwritten).
 *   class_mask     bit k set: class k is cleaned; bit 0 and bits >= C must be clear (background is never removed)
 *   keep_largest   HOST int32 [C]: keep_largest[k] in [0, 4], 0 = every component; 0 required outside class_mask
 *   min_volume     HOST int32 [C]: >= 0; read for the classes of class_mask
 *   hole_limit     >= 0; 0 = no hole filling (the second labelling is not launched)
 *   workspace      at least lmn_volpost_workspace(D, H, W) bytes (device), ws_bytes its size
 * The selection runs one pass per rank: max(keep_largest) passes, at most four.                                                   */
int lmn_volpost_clean(const uint8_t* labels, int D, int H, int W, int C, int connectivity, uint64_t class_mask,
                      const int32_t* keep_largest, const int32_t* min_volume, int hole_limit, void* workspace, int64_t ws_bytes,
                      uint8_t* labels_out, int32_t* stats, lmn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

/* Per-case 3D surface distances and overlap of a label VOLUME: the entries of liblmnet_hip.so behind
 * lm_net_amd.metrics.VolumeSurfaceMeter.  They stand in for medpy.metric.binary.dc, jc, hd, hd95, assd and ravd of a whole [D, H, W]
 * case with integer voxel pitches -- the per-case numbers of a CT results table -- which the reference's evaluate() prepares for and
 * never computes (utils/train_eval_utils.py:7 imports hausdorff_distance, :178-179 set up hausdorff_distance_list / rvd_list, :14-52
 * ravd / RVDEvaluator).  These symbols are listed in lm_net_amd.hip.SYMBOLS_VOLUME, a list of its own that lm_net_amd.hip.load checks
 * next to hip.EXPORTS; tests/test_volume_cpu.py checks it against this header and ties the two entries that write device memory to
 * their guard tests in tests/test_guard_volume_gpu.py.  Plain arguments only: no struct, no ABI bump.
 *
 * DEFINITIONS.  For class k, P = (pred == k), T = (target == k) over the whole volume.  The border of a mask is its voxels with a
 * 6-neighbour outside it; outside the volume counts as outside (scipy.ndimage.binary_erosion with generate_binary_structure(3, 1) and
 * border_value = 0, which medpy uses).  In a one-slice volume every mask voxel is therefore a border voxel.  With integer pitches
 * (kz, ky, kx) the squared distance of two voxels is the exact integer
 *     d2 = (kz dz)^2 + (ky dy)^2 + (kx dx)^2,
 * and D2(A -> B) is the d2 of every border voxel of A to the nearest border voxel of B.  A float pitch is out of scope: the caller
 * expresses the pitch in integer steps of a unit (3.0 x 0.78 x 0.78 mm = (50, 13, 13) steps of 0.06 mm) and scales the distances.
 *
 * LIMITS.  1 <= D <= 1024, 2 <= H, W <= 1024, 2 <= C <= 64, 1 <= nk <= 64, kz, ky, kx >= 1 and
 *     (kz (D - 1))^2 + (ky (H - 1))^2 + (kx (W - 1))^2 < 2^31,
 * so that every squared distance and every partial sum of one is an int32.
 *
 * Integer arithmetic and integer atomics only, apart from two float64 sums of sqrt(d2) formed in a fixed order: two calls on one
 * input are bit-identical, in either deterministic mode.  Every argument error is rejected before any HIP call (LMN_E_BADARG and
 * lmn_last_error).  Not recorded by plans.                                                                                         */
#ifndef LMNET_VOLUME_H
#define LMNET_VOLUME_H
#include "../lmnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMN_VOLUME_MAX_SIDE 1024
#define LMN_VOLUME_NSTAT_I 9
#define LMN_VOLUME_NSTAT_F 2

/* bytes of `workspace` lmn_volume_dist needs for nk classes of a D x H x W volume, exactly: per voxel, map and class a uint16 step
 * count along z, an int32 partial squared distance and an int32 result (20 bytes per voxel and class); per row (z, y), map and
 * class an int32 count and a uint8 flag; each of the five arrays rounded up to 256 bytes.  Host arithmetic; -1 and lmn_last_error
 * outside the limits above.                                                                                                        */
int64_t lmn_volume_workspace(int D, int H, int W, int nk);

/* Narrows n consecutive slices of a case to uint8 class ids (255 = no class) and writes them at slice z0 of the case buffers
 * lab_pred and lab_target (uint8 [D_cap, H, W], device): what medpy's callers do on the host with argmax(1).astype(np.uint8).
 * The prediction is EITHER pred_logits [n, C, H, W] fp32 (arg-max over C, first maximum wins, as lmn_confusion) OR pred_labels
 * [n, H, W] int64 (the other NULL); target [n, H, W] int64; values outside [0, C) belong to no class.  Writes slices
 * [z0, z0 + n) of both buffers and nothing else; requires 0 <= z0, 1 <= n, z0 + n <= D_cap <= 1024.  One kernel on `stream`.       */
int lmn_volume_labels(const float* pred_logits, const int64_t* pred_labels, const int64_t* target, int n, int C, int H, int W,
                      uint8_t* lab_pred, uint8_t* lab_target, int D_cap, int z0, lmn_stream_t stream);

/* Raw statistics of ONE case for the classes classes[0 .. nk) (HOST array of ids in [0, C)), from the uint8 label volumes
 * lab_pred / lab_target [D, H, W] (device, as lmn_volume_labels writes them; read only):
 *   stats_i [nk][9] int64 (device, zeroed and overwritten): |P|, |T|, border count of P, of T, max D2(P -> T), max D2(T -> P),
 *     D2[lo], D2[hi] of the pooled multiset D2(P -> T) U D2(T -> P) sorted ascending, lo = 95 (n - 1) / 100 (integer),
 *     hi = min(lo + 1, n - 1), n = its size (numpy's linear 95th percentile, medpy hd95), and |P n T| (medpy dc / jc);
 *   stats_f [nk][2] float64 (device): sum sqrt(D2(P -> T)), sum sqrt(D2(T -> P)) (medpy assd), each summed in a fixed order.
 * A class with |P| = 0 or |T| = 0 keeps its counts and gets 0 in the six distance fields (medpy raises there).
 *   workspace  at least lmn_volume_workspace(D, H, W, nk) bytes (device), ws_bytes its size
 * Four kernels on `stream`: steps to the nearest border voxel along z; the partial minimum along y, only in rows where the other
 * map has a border voxel; the minimum along x at the border voxels of the other map, written compacted per row; per class the
 * maxima, the sums and the two order statistics by a three-level radix select (11 + 10 + 10 bits).                                */
int lmn_volume_dist(const uint8_t* lab_pred, const uint8_t* lab_target, int D, int H, int W, int C, const int32_t* classes, int nk,
                    int kz, int ky, int kx, void* workspace, int64_t ws_bytes, int64_t* stats_i, double* stats_f, lmn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

/* The input side of a 3D case: intensity statistics of an int16 (or uint8) volume and the gather that turns it into the fp32 2.5D
 * batches the network reads -- the entries of liblmnet_hip.so behind lm_net_amd.data.VolumeSlicer.  These symbols are listed in
 * lm_net_amd.hip.SYMBOLS_SLICES, a list of its own that lm_net_amd.hip.load checks next to hip.EXPORTS; tests/test_slices_cpu.py
 * checks it against this header and ties the two device entries to tests/test_guard_slices_gpu.py.  Plain arguments only: no struct,
 * no ABI bump.
 *
 * DEFINITIONS.  A volume is [M, D, Hs, Ws] of int16 (LMN_SLICES_I16) or uint8 (LMN_SLICES_U8), M co-registered modalities.
 *   FOREGROUND of modality m: the voxels with v > foreground[m]; LMN_SLICES_NO_FOREGROUND admits every voxel.  It has n voxels.
 *   RECORD, eight int64 per modality:  n, sum v, sum v^2, min, max, v_lo, v_hi, 0  -- integer arithmetic throughout, so the record is
 *      exact and bit-identical from call to call (|sum v^2| <= 2^60 at the limits).  v_lo and v_hi are order statistics of the sorted
 *      foreground at RANK r = (q_ppm * (n - 1)) / 1000000 in 64-bit integer arithmetic, q_ppm = round(q_percent * 10^4) formed by
 *      the caller; q_lo_ppm = 0 and q_hi_ppm = 1000000 give min and max.  WITH n = 0 EVERY FIELD IS 0.
 *   NORM SPECS.  S rows (spec_mod[s] the modality, non-decreasing in s; spec_kind[s]); the finish forms the fp32 table row
 *      (lo, hi, a, b) of each in fp64 and rounds once:
 *         LMN_SLICES_WINDOW       lo = level - width / 2   hi = level + width / 2   a = lo      b = 1 / width
 *         LMN_SLICES_ZSCORE       lo = v_lo                hi = v_hi                a = mean    b = 1 / max(std, 1e-8)
 *         LMN_SLICES_PERCENTILE   lo = v_lo                hi = v_hi                a = v_lo    b = 1 / (v_hi - v_lo)
 *      mean and the population std are those of the UNCLIPPED foreground, from the integer sums (std^2 = (n sum v^2 - (sum v)^2) /
 *      n^2 with a 128-bit numerator: a constant volume has std = 0 exactly).  zscore: b = 0 WHEN n = 0.  percentile: b = 0 WHEN
 *      v_hi == v_lo.  The table is never NaN or infinite.
 *   CHANNELS.  K = 2 context + 1.  C = S * K <= 16; channel s * K + (dz + context) of output sample i reads source slice
 *      z[i] + dz * stride of modality spec_mod[s] -- so the order is modality, spec, dz.  LMN_SLICES_EDGE_REPLICATE clamps that index
 *      to [0, D); under LMN_SLICES_EDGE_ZERO an index outside [0, D) gives a plane that is 0 before gain and bias.  z[i] itself is
 *      clamped to [0, D) (it is device data).
 *   PARAMETER ROW of a sample, fp32 [8]:  m0 .. m5, gain, bias.  m is the INVERSE map from output pixel index to source pixel index;
 *      the caller forms it in fp64 (plain resize: sx = (x + 0.5) Ws / w - 0.5).  PINNED COORDINATE ARITHMETIC, no contraction:
 *         sx = __fadd_rn(__fadd_rn(__fmul_rn(m0, x), __fmul_rn(m1, y)), m2)      sy = the same on m3, m4, m5
 *         x0 = floorf(sx), fx = sx - x0 (exact), likewise y0, fy
 *      so that a float32 restatement takes the same floor at every pixel.
 *   IMAGE.  Bilinear over the taps (x0, y0) .. (x0 + 1, y0 + 1), read in the storage type and widened to fp32:
 *         top = fmaf(fx, v01 - v00, v00)   bot = fmaf(fx, v11 - v10, v10)   v = fmaf(fy, bot - top, top)
 *      LMN_SLICES_BORDER_REPLICATE clamps tap indices into the frame; under LMN_SLICES_BORDER_CONSTANT a tap outside the frame takes
 *      border_value[m], in raw units.  Then o = (min(max(v, lo), hi) - a) * b and o = o * gain + bias.  The specs of a modality share
 *      the interpolated v; coordinates and weights are formed once per pixel for all channels.
 *   LABEL.  Nearest, at floorf(__fadd_rn(s, 0.5f)) per axis -- the half-pixel rule (torch's nearest-exact), not cv2's, so that image
 *      and label move under one matrix -- with the same border rule and label_border; uint8 or int64 out.
 *
 * LIMITS.  1 <= D <= 1024, 2 <= Hs, Ws <= 1024, 1 <= M <= 4, 1 <= S, S * K <= 16, 0 <= context <= 7, 1 <= stride <= 1024,
 *   1 <= n <= 65535, 1 <= h, w <= 4096.
 *
 * Every argument error is rejected before any HIP call (LMN_E_BADARG and lmn_last_error, messages "slices_workspace: ...",
 * "slices_stats: ...", "slices_gather: ...").  Nothing synchronises; no kernel waits on another block.  Not recorded by plans.     */
#ifndef LMNET_SLICES_H
#define LMNET_SLICES_H
#include "../lmnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMN_SLICES_I16 0                 /* vol_kind */
#define LMN_SLICES_U8 1
#define LMN_SLICES_WINDOW 0              /* spec_kind */
#define LMN_SLICES_ZSCORE 1
#define LMN_SLICES_PERCENTILE 2
#define LMN_SLICES_EDGE_REPLICATE 0      /* edge: slices past the ends of the volume */
#define LMN_SLICES_EDGE_ZERO 1
#define LMN_SLICES_BORDER_REPLICATE 0    /* border: taps outside the frame */
#define LMN_SLICES_BORDER_CONSTANT 1
#define LMN_SLICES_LABELS_U8 0           /* label_kind of the output */
#define LMN_SLICES_LABELS_I64 1
#define LMN_SLICES_MAX_DEPTH 1024
#define LMN_SLICES_MAX_SIDE 1024
#define LMN_SLICES_MAX_MODALITIES 4
#define LMN_SLICES_MAX_CHANNELS 16
#define LMN_SLICES_MAX_CONTEXT 7
#define LMN_SLICES_MAX_OUT 4096
#define LMN_SLICES_MAX_BATCH 65535
#define LMN_SLICES_NSTAT 8
#define LMN_SLICES_NO_FOREGROUND (-32769)

/* bytes of the `workspace` of lmn_slices_stats, exactly: per modality the 64-bit sums (8), the coarse histogram over
 * (v + 32768) >> 6 (1024 counters of 32 bits), the two fine histograms (2 x 64) and the ranks and chosen bins (8 words), rounded up
 * to 256 bytes.  Host arithmetic; -1 and lmn_last_error outside the limits above. */
int64_t lmn_slices_workspace(int M, int D, int Hs, int Ws);

/* stats (device int64 [M, 8]) = the records above, table (device fp32 [S, 4]) = the normalisation rows.  foreground (int32 [M]),
 * spec_mod, spec_kind (int32 [S]) and spec_level, spec_width (double [S], read for LMN_SLICES_WINDOW rows; width > 0) are HOST arrays,
 * read before the entry returns.  Launches on `stream`: a zero fill of the workspace; a pass over the volume that accumulates n,
 * sum v, sum v^2, min and max per lane in int64, reduces per wave and issues one 64-bit integer atomic per block and quantity, and
 * counts the coarse histogram in LDS in the same pass; a one-block step that picks the coarse bin of each rank; a second pass that
 * counts the 64 values inside the two chosen bins; a one-block finish.  (Two levels because a 65536-bin histogram of 32-bit counters
 * does not fit the LDS of a CU.)  Equal values within a wave are reduced before the LDS atomic -- a case is often mostly one value --
 * and every counter has 32 bits. */
int lmn_slices_stats(const void* volume, int vol_kind, int M, int D, int Hs, int Ws, const int32_t* foreground, int q_lo_ppm,
                     int q_hi_ppm, int S, const int32_t* spec_mod, const int32_t* spec_kind, const double* spec_level,
                     const double* spec_width, void* workspace, int64_t ws_bytes, int64_t* stats, float* table, lmn_stream_t stream);

/* x (fp32 [n, S * K, h, w]) and / or y ([n, h, w], uint8 or int64 by label_kind) from the slices z (device int32 [n]) under the
 * parameter rows params (device fp32 [n, 8]).  Image mode: volume, table (device fp32 [S, 4], of lmn_slices_stats), spec_mod (HOST
 * int32 [S]), border_value (HOST fp32 [M]) and x are given; label mode: labels (device uint8 [D, Hs, Ws]) and y.  Either or both;
 * label-only mode (volume, table, spec_mod, border_value, x all NULL, S = 0) serves the way back to the source grid.  One launch: one grid
 * row per sample, so a block never mixes two samples; each lane owns four consecutive x with 16-byte stores when w % 4 == 0 and x is
 * 16-byte aligned, one x otherwise. */
int lmn_slices_gather(const void* volume, int vol_kind, const uint8_t* labels, int M, int D, int Hs, int Ws, const int32_t* z,
                      const float* params, int n, const float* table, int S, const int32_t* spec_mod, int context, int stride, int edge,
                      int border, const float* border_value, int label_border, int h, int w, float* x, void* y, int label_kind,
                      lmn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

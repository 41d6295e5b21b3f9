/* Tiled and flip-averaged inference on frames of any size: the entries of liblmnet_hip.so behind lm_net_amd.infer.TiledPredictor.
 * These symbols are listed in lm_net_amd.hip.SYMBOLS_TILES, a list of its own that lm_net_amd.hip.load checks next to hip.EXPORTS;
 * tests/test_tiles_cpu.py checks it against this header and ties the two entries that write device memory to their guard test,
 * tests/test_guard_tiles_gpu.py.
 *
 * GEOMETRY, per axis (image length L, tile t, stride s; all integers):
 *   V = max(L, t)                    the virtual length: an axis shorter than the tile is padded up to one tile
 *   p = (V - L) / 2                  padding before (the rest after); virtual coordinate v is source coordinate v - p
 *   n = ceil((V - t) / s) + 1        tiles
 *   start_i = min(i * s, V - t)      the last tile is pulled back to the edge: an axis of at least one tile is never padded
 * A source coordinate i outside [0, L) reads 0 (LMN_TILE_PAD_ZERO) or the reflection without the edge sample, continued with period
 * 2 (L - 1) (LMN_TILE_PAD_REFLECT: numpy.pad(mode="reflect") for any pad width; needs L >= 2).
 *
 * ENTRIES.  Every tile comes in n_flip mirrored copies: copy 0 is the identity, copy f > 0 is mirrored along the axes named by
 * flip[f] (LMN_TILE_FLIP_H: left-right, LMN_TILE_FLIP_V: up-down, both bits: both).  One image has E = n_y * n_x * n_flip entries
 * in the order [ty][tx][f]; images are outermost, so a batch has batch * E entries, numbered from 0.                              */
#ifndef LMNET_TILES_H
#define LMNET_TILES_H
#include "../lmnet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LMN_TILE_MIN 32              /* tile sides: multiples of 16 in [32, 1024] (the rule of LM_Net.forward and a cap)            */
#define LMN_TILE_MAX 1024
#define LMN_TILE_MAX_LEN 8192        /* image sides: 1 .. 8192                                                                      */
#define LMN_TILE_MAX_CLASSES 64      /* channels of the tile outputs lmn_tile_blend reads                                           */
#define LMN_TILE_MAX_FLIPS 4         /* the identity and at most three mirrors                                                      */

#define LMN_TILE_PAD_ZERO 0
#define LMN_TILE_PAD_REFLECT 1

#define LMN_TILE_FLIP_H 1
#define LMN_TILE_FLIP_V 2

#define LMN_TILE_AVG_LOGITS 0        /* g = identity                                                                                */
#define LMN_TILE_AVG_SOFTMAX 1       /* g = softmax over the channels of one tile pixel                                             */
#define LMN_TILE_AVG_SIGMOID 2       /* g = element-wise sigmoid                                                                    */

/* The geometry shared by the two entries (HOST memory, read before the entry returns).                                            */
#define LMN_TILE_PARAM_BYTES 96
typedef struct {
  int32_t batch;                 /* images, >= 1                                                                                     */
  int32_t channels;              /* lmn_tile_gather: channels of the source (>= 1); lmn_tile_blend: C of the tile outputs (1 .. 64) */
  int32_t height, width;         /* image size, 1 .. LMN_TILE_MAX_LEN each                                                           */
  int32_t tile_h, tile_w;
  int32_t stride_h, stride_w;    /* 1 .. tile                                                                                        */
  int32_t pad;                   /* LMN_TILE_PAD_*                                                                                   */
  int32_t n_flip;                /* 1 .. LMN_TILE_MAX_FLIPS                                                                          */
  int32_t flip[4];               /* flip[0] = 0; flip[f] in 1 .. 3, no value twice                                                   */
  int32_t average;               /* LMN_TILE_AVG_* (lmn_tile_blend only)                                                             */
  int32_t _pad[9];               /* fixed size: LMN_TILE_PARAM_BYTES; lm_net_amd.hip.load compares its mirror with the export below */
} lmn_tile_param_t;
int lmn_sizeof_tile_param(void);

/* tiles[count, channels, tile_h, tile_w] (fp32) = the entries first .. first + count - 1 of src[batch, channels, height, width]
 * (fp32): the source padded as above, cut at the tile's start and mirrored.  A pure copy, exact bit for bit: what the model is fed.
 * Argument errors (null pointer, a tile side that is no multiple of 16 in [32, 1024], a stride outside [1, tile], an image side
 * outside [1, 8192] or below 2 on a reflected axis shorter than the tile, an unknown pad mode or flip, count < 1 or first + count
 * past the entry count) are rejected before any HIP call.                                                                          */
int lmn_tile_gather(const float* src, const lmn_tile_param_t* param, int64_t first, int64_t count, float* tiles, lmn_stream_t stream);

/* map[batch, C, height, width] (fp32) from the tile outputs z[batch, n_y, n_x, n_flip, C, tile_h, tile_w] (fp32) and the separable
 * window w(y, x) = wy[y] wx[x] (fp32 tables of tile_h and tile_w positive values, indexed by the position inside the un-mirrored
 * tile).  A GATHER: one lane owns one pixel (b, Y, X), visits the tiles that cover it in the fixed order ty ascending, tx ascending,
 * f ascending, un-mirrors its tile-local coordinate for f and forms, per channel c,
 *     sum_{ty,tx,f} w * g(z[b,ty,tx,f,:,y,x])[c]  /  (n_flip * sum_{ty,tx} w)
 * in fp32, g by `average`.  No atomics, no cross-lane step: the order of a pixel's sum does not depend on the launch geometry and
 * two calls are bit-identical.  labels[batch, height, width] (uint8, may be NULL): the arg-max over c of the values just written,
 * lowest class on a tie (pred_common.h); it must be NULL for C == 1 and for LMN_TILE_AVG_SIGMOID.
 * Argument errors (those of lmn_tile_gather, C outside [1, 64], an unknown mode, labels where none are defined) are rejected before
 * any HIP call.                                                                                                                    */
int lmn_tile_blend(const float* z, const lmn_tile_param_t* param, const float* wy, const float* wx, float* map, uint8_t* labels,
                   lmn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

// The entries of include/tiles/lmnet_tiles.h: cut overlapping, optionally mirrored tiles out of a padded frame (lmn_tile_gather) and
// merge the model's tile outputs back into one full-size map under a separable window (lmn_tile_blend).  Both are bandwidth-bound
// and use no LDS: 256-lane blocks, one lane per element (gather) or per output pixel (blend), x fastest, so that a wave reads and
// writes whole row segments.  A tile start is an arbitrary integer after the pull-back and an `h` mirror reverses the lane order, so
// the loads are 4 bytes per lane: consecutive lanes still touch consecutive (ascending or descending) addresses.
// The blend is a GATHER: every output pixel sums the tiles that cover it in a fixed order in its own lane -- no atomics, no
// cross-lane step, nothing that depends on the launch geometry.  The arg-max of the labels is the one of pred_common.h.
#include <math.h>

#include "../../include/tiles/lmnet_tiles.h"
#include "loss_common.h"
#include "pred_common.h"

static_assert(sizeof(lmn_tile_param_t) == LMN_TILE_PARAM_BYTES, "lmn_tile_param_t: fixed size");

namespace {

// one axis of the geometry
struct TileAxis {
  int L, t, s;      // image length, tile, stride
  int V, p, n;      // virtual length max(L, t), padding before, tiles
};

struct TileGeo {
  TileAxis y, x;
  int B, C, F, pad;
  int flip[LMN_TILE_MAX_FLIPS];
};

inline TileAxis tile_axis(int L, int t, int s) {
  TileAxis a;
  a.L = L; a.t = t; a.s = s;
  a.V = L > t ? L : t;
  a.p = (a.V - L) / 2;
  a.n = (a.V - t + s - 1) / s + 1;
  return a;
}

__device__ __forceinline__ int tile_start(const TileAxis& a, int i) { return min(i * a.s, a.V - a.t); }

// reflection without the edge sample, continued with period 2 (L - 1); L >= 2
__device__ __forceinline__ int tile_reflect(int i, int L) {
  const int P = 2 * (L - 1);
  int m = i % P;
  if (m < 0) m += P;
  return m < L ? m : P - m;
}

// the tiles [lo, hi] of an axis that cover the virtual coordinate v (0 <= v < V): a contiguous, never empty run
__device__ __forceinline__ void tile_cover(const TileAxis& a, int v, int& lo, int& hi) {
  lo = v - a.t + 1 > 0 ? (v - a.t + a.s) / a.s : 0;      // smallest i with i * s + t > v
  lo = min(lo, a.n - 1);
  hi = v >= a.V - a.t ? a.n - 1 : v / a.s;               // the pulled-back last tile covers everything from V - t on
}

// grid.y walks the planes (entry, channel) of tiles[count, channels, th, tw] -- the entry is decoded once per block, in scalar
// registers -- and grid.x the th x tw elements of a plane with 32-bit arithmetic, x fastest
__global__ void __launch_bounds__(256) tile_gather_kernel(const float* __restrict__ src, TileGeo G, int64_t first, int64_t planes,
                                                          float* __restrict__ tiles) {
  const int th = G.y.t, tw = G.x.t, area = th * tw;
  for (int64_t pl = blockIdx.y; pl < planes; pl += gridDim.y) {
    const int ch = (int)(pl % G.C);
    int64_t e = first + pl / G.C;
    const int fl = G.flip[(int)(e % G.F)];
    e /= G.F;
    const int tx = (int)(e % G.x.n);
    e /= G.x.n;
    const int ty = (int)(e % G.y.n);
    const int b = (int)(e / G.y.n);
    const int y0 = tile_start(G.y, ty) - G.y.p, x0 = tile_start(G.x, tx) - G.x.p;
    const float* __restrict__ sp = src + ((int64_t)b * G.C + ch) * G.y.L * G.x.L;
    float* __restrict__ tp = tiles + pl * area;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < area; i += gridDim.x * 256) {
      const int y = i / tw, x = i - y * tw;
      int sy = y0 + ((fl & LMN_TILE_FLIP_V) ? th - 1 - y : y);
      int sx = x0 + ((fl & LMN_TILE_FLIP_H) ? tw - 1 - x : x);
      float v = 0.f;
      const bool inside = sy >= 0 && sy < G.y.L && sx >= 0 && sx < G.x.L;
      if (inside || G.pad == LMN_TILE_PAD_REFLECT) {
        if (!inside) {
          sy = tile_reflect(sy, G.y.L);
          sx = tile_reflect(sx, G.x.L);
        }
        v = sp[sy * G.x.L + sx];
      }
      tp[i] = v;
    }
  }
}

// One lane per output pixel (b, Y, X), X fastest; CB accumulators in registers.  C <= CB: one pass.  C > CB: passes over CB channels
// each (the softmax statistics of a tile pixel are formed again in every pass).
template <int CB, int MODE>
__global__ void __launch_bounds__(256) tile_blend_kernel(const float* __restrict__ z, TileGeo G, const float* __restrict__ wy,
                                                         const float* __restrict__ wx, int64_t pixels, float* map, uint8_t* labels) {
  const int H = G.y.L, W = G.x.L, th = G.y.t, tw = G.x.t, C = G.C, F = G.F;
  const int64_t hw = (int64_t)H * W, plane = (int64_t)th * tw;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * 256) {
    const int X = (int)(i % W);
    const int64_t r = i / W;
    const int Y = (int)(r % H), b = (int)(r / H);
    const int vy = Y + G.y.p, vx = X + G.x.p;
    int ylo, yhi, xlo, xhi;
    tile_cover(G.y, vy, ylo, yhi);
    tile_cover(G.x, vx, xlo, xhi);
    float* out = map + (int64_t)b * C * hw + (int64_t)Y * W + X;
    for (int c0 = 0; c0 < C; c0 += CB) {
      float acc[CB];
#pragma unroll
      for (int j = 0; j < CB; ++j) acc[j] = 0.f;
      float wsum = 0.f;
      for (int ty = ylo; ty <= yhi; ++ty) {
        const int ly = vy - tile_start(G.y, ty);
        if ((unsigned)ly >= (unsigned)th) continue;      // (never taken for tile_cover's run: keeps every address in bounds by construction)
        const float wyv = wy[ly];
        for (int tx = xlo; tx <= xhi; ++tx) {
          const int lx = vx - tile_start(G.x, tx);
          if ((unsigned)lx >= (unsigned)tw) continue;
          const float w = wyv * wx[lx];
          wsum += w;
          const int64_t e0 = (((int64_t)b * G.y.n + ty) * G.x.n + tx) * F;
          for (int f = 0; f < F; ++f) {
            const int fl = G.flip[f];
            const int zy = (fl & LMN_TILE_FLIP_V) ? th - 1 - ly : ly, zx = (fl & LMN_TILE_FLIP_H) ? tw - 1 - lx : lx;
            const float* zp = z + (e0 + f) * C * plane + (int64_t)zy * tw + zx;
            if (MODE == LMN_TILE_AVG_SOFTMAX) {
              float v[CB];
              float m = -INFINITY;
              if (C <= CB) {
#pragma unroll
                for (int j = 0; j < CB; ++j) {
                  v[j] = j < C ? zp[j * plane] : -INFINITY;
                  m = fmaxf(m, v[j]);
                }
              } else {
                for (int c = 0; c < C; ++c) m = fmaxf(m, zp[c * plane]);
#pragma unroll
                for (int j = 0; j < CB; ++j) v[j] = c0 + j < C ? zp[(c0 + j) * plane] : -INFINITY;
              }
              float s = 0.f;
              if (C <= CB) {
#pragma unroll
                for (int j = 0; j < CB; ++j) {
                  v[j] = __expf(v[j] - m);      // (exp(-inf) = 0 for the lanes past C)
                  s += v[j];
                }
              } else {
                for (int c = 0; c < C; ++c) s += __expf(zp[c * plane] - m);
#pragma unroll
                for (int j = 0; j < CB; ++j) v[j] = __expf(v[j] - m);
              }
              const float ws = w / s;
#pragma unroll
              for (int j = 0; j < CB; ++j) acc[j] = fmaf(ws, v[j], acc[j]);
            } else {
              float v[CB];      // (all loads of the entry first, then the arithmetic: the loads stay in flight together)
#pragma unroll
              for (int j = 0; j < CB; ++j) v[j] = c0 + j < C ? zp[(c0 + j) * plane] : 0.f;
#pragma unroll
              for (int j = 0; j < CB; ++j) {
                if (c0 + j < C) {      // (wave-uniform: no arithmetic for the accumulators past C)
                  if (MODE == LMN_TILE_AVG_SIGMOID) v[j] = __builtin_amdgcn_rcpf(1.f + __expf(-v[j]));
                  acc[j] = fmaf(w, v[j], acc[j]);
                }
              }
            }
          }
        }
      }
      const float den = (float)F * wsum;
#pragma unroll
      for (int j = 0; j < CB; ++j)
        if (c0 + j < C) out[(c0 + j) * hw] = acc[j] / den;
    }
    if (labels) labels[i] = (uint8_t)pred_argmax(out, C, hw);      // (this lane's own stores, read back in program order)
  }
}

// the argument checks shared by the two entries
int tile_check(const char* what, const lmn_tile_param_t* P) {
  LMN_REQUIRE(P->batch >= 1, "%s: batch=%d", what, P->batch);
  const int t[2] = {P->tile_h, P->tile_w}, s[2] = {P->stride_h, P->stride_w}, L[2] = {P->height, P->width};
  for (int a = 0; a < 2; ++a) {
    LMN_REQUIRE(t[a] % 16 == 0 && t[a] >= LMN_TILE_MIN && t[a] <= LMN_TILE_MAX, "%s: tile %dx%d: sides must be multiples of 16 in [%d, %d]",
                what, P->tile_h, P->tile_w, LMN_TILE_MIN, LMN_TILE_MAX);
    LMN_REQUIRE(s[a] >= 1 && s[a] <= t[a], "%s: stride %dx%d outside [1, tile]", what, P->stride_h, P->stride_w);
    LMN_REQUIRE(L[a] >= 1 && L[a] <= LMN_TILE_MAX_LEN, "%s: image %dx%d: sides must be in [1, %d]", what, P->height, P->width,
                LMN_TILE_MAX_LEN);
  }
  LMN_REQUIRE(P->pad == LMN_TILE_PAD_ZERO || P->pad == LMN_TILE_PAD_REFLECT, "%s: unknown pad mode %d", what, P->pad);
  for (int a = 0; a < 2; ++a)
    LMN_REQUIRE(P->pad != LMN_TILE_PAD_REFLECT || L[a] >= t[a] || L[a] >= 2, "%s: image %dx%d: a reflected axis needs length >= 2", what,
                P->height, P->width);
  LMN_REQUIRE(P->n_flip >= 1 && P->n_flip <= LMN_TILE_MAX_FLIPS, "%s: n_flip=%d not in [1, %d]", what, P->n_flip, LMN_TILE_MAX_FLIPS);
  LMN_REQUIRE(P->flip[0] == 0, "%s: flip[0]=%d: entry 0 is the identity", what, P->flip[0]);
  for (int f = 1; f < P->n_flip; ++f) {
    LMN_REQUIRE(P->flip[f] >= 1 && P->flip[f] <= 3, "%s: unknown flip %d", what, P->flip[f]);
    for (int k = 1; k < f; ++k) LMN_REQUIRE(P->flip[k] != P->flip[f], "%s: flip %d twice", what, P->flip[f]);
  }
  return 0;
}

TileGeo tile_geo(const lmn_tile_param_t* P) {
  TileGeo G;
  G.y = tile_axis(P->height, P->tile_h, P->stride_h);
  G.x = tile_axis(P->width, P->tile_w, P->stride_w);
  G.B = P->batch; G.C = P->channels; G.F = P->n_flip; G.pad = P->pad;
  for (int f = 0; f < LMN_TILE_MAX_FLIPS; ++f) G.flip[f] = f < P->n_flip ? P->flip[f] : 0;
  return G;
}

template <int MODE>
void tile_blend_launch(hipStream_t st, const float* z, const TileGeo& G, const float* wy, const float* wx, float* map, uint8_t* labels) {
  const int64_t pixels = (int64_t)G.B * G.y.L * G.x.L;
  const dim3 grid(loss_grid(pixels, 1 << 16)), block(256);
  if (G.C == 1) LMN_LAUNCH((tile_blend_kernel<1, MODE>), grid, block, 0, st, z, G, wy, wx, pixels, map, labels);
  else if (G.C == 2) LMN_LAUNCH((tile_blend_kernel<2, MODE>), grid, block, 0, st, z, G, wy, wx, pixels, map, labels);
  else if (G.C <= 4) LMN_LAUNCH((tile_blend_kernel<4, MODE>), grid, block, 0, st, z, G, wy, wx, pixels, map, labels);
  else if (G.C <= 8) LMN_LAUNCH((tile_blend_kernel<8, MODE>), grid, block, 0, st, z, G, wy, wx, pixels, map, labels);
  else LMN_LAUNCH((tile_blend_kernel<16, MODE>), grid, block, 0, st, z, G, wy, wx, pixels, map, labels);
}

}  // namespace

extern "C" {

int lmn_sizeof_tile_param(void) { return (int)sizeof(lmn_tile_param_t); }

int lmn_tile_gather(const float* src, const lmn_tile_param_t* param, int64_t first, int64_t count, float* tiles, lmn_stream_t stream) {
  LMN_REQUIRE(src && param && tiles, "tile_gather: null pointer");
  if (int rc = tile_check("tile_gather", param)) return rc;
  LMN_REQUIRE(param->channels >= 1, "tile_gather: channels=%d", param->channels);
  const TileGeo G = tile_geo(param);
  const int64_t entries = (int64_t)G.B * G.y.n * G.x.n * G.F;
  LMN_REQUIRE(first >= 0 && count >= 1 && first <= entries - count, "tile_gather: first=%lld, count=%lld: entries outside [0, %lld)", (long long)first,
              (long long)count, (long long)entries);
  const int64_t planes = count * G.C;
  // 16 elements per lane where the plane has them: the entry's decode (64-bit divisions) is paid once per block
  const dim3 grid(lmn_cdiv((int64_t)G.y.t * G.x.t, 16 * 256), (unsigned)(planes < 65535 ? planes : 65535));
  LMN_LAUNCH(tile_gather_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, G, first, planes, tiles);
  return lmn_launch_status("tile_gather");
}

int lmn_tile_blend(const float* z, const lmn_tile_param_t* param, const float* wy, const float* wx, float* map, uint8_t* labels,
                   lmn_stream_t stream) {
  LMN_REQUIRE(z && param && wy && wx && map, "tile_blend: null pointer");
  if (int rc = tile_check("tile_blend", param)) return rc;
  LMN_REQUIRE(param->channels >= 1 && param->channels <= LMN_TILE_MAX_CLASSES, "tile_blend: C=%d not in [1, %d]", param->channels,
              LMN_TILE_MAX_CLASSES);
  LMN_REQUIRE(param->average >= LMN_TILE_AVG_LOGITS && param->average <= LMN_TILE_AVG_SIGMOID, "tile_blend: unknown mode %d", param->average);
  LMN_REQUIRE(!labels || (param->channels >= 2 && param->average != LMN_TILE_AVG_SIGMOID),
              "tile_blend: labels are defined for C >= 2 and not for the sigmoid mode (C=%d, mode %d)", param->channels, param->average);
  const TileGeo G = tile_geo(param);
  hipStream_t st = (hipStream_t)stream;
  if (param->average == LMN_TILE_AVG_SOFTMAX) tile_blend_launch<LMN_TILE_AVG_SOFTMAX>(st, z, G, wy, wx, map, labels);
  else if (param->average == LMN_TILE_AVG_SIGMOID) tile_blend_launch<LMN_TILE_AVG_SIGMOID>(st, z, G, wy, wx, map, labels);
  else tile_blend_launch<LMN_TILE_AVG_LOGITS>(st, z, G, wy, wx, map, labels);
  return lmn_launch_status("tile_blend");
}

}  // extern "C"

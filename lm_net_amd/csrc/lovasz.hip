// The Lovasz-Softmax loss and the Lovasz hinge on a stable segmented radix sort (include/lovasz/lmnet_lovasz.h; lm_net_amd.loss.
// LovaszLoss, lovasz_ranks).  S segments of P elements each, grid.y = segment, a tile of LV_TILE elements per block.
//
//   1. lv_key_*_kernel    errors, 32-bit keys (descending float order as ascending unsigned, void = all ones) and payloads (the
//                         element index, bit 31: foreground); the counts of valid and foreground elements with integer atomics.
//   2. the sort           four 8-bit digit passes over (key, payload) pairs, three launches each:
//        lv_hist_kernel      the digit histogram of every tile into table[s][digit][block]; the digit totals of the segment into
//                            tot[s][digit] with integer atomics (zeroed before the first pass, and by the scatter for the next)
//        lv_scan_kernel      one wave per (digit, segment): the totals of the smaller digits (at most 255 loads) and then the
//                            exclusive scan of its own row of the table, in place -- the scan in [digit][block] order
//        lv_scatter_kernel   per tile, LV_ITEMS rounds of 256 consecutive elements: a lane finds the lanes of its wave with the same
//                            digit from 8 ballots, the waves' digit counts meet in LDS, the running digit offsets live in LDS.
//                            Elements of equal digit leave in the order they came: each pass is stable, so the whole sort is.
//   3. lv_fgcount_kernel  the foreground elements of every tile of the sorted order.
//   4. lv_coef_kernel     per tile: its base (the sum of the tiles before it: a loop over at most nb counts), the inclusive integer
//                         scan of fg by ballots, the closed-form coefficient, coef through perm, the tile's sum of e g into its slot.
//   5. lv_finish_kernel   one block: the segment losses (a wave per segment, fixed order), the weighted mean, loss and sums.
//   6. lv_bwd_*_kernel    one pointwise launch from coef and sums.
// No kernel waits on another block; every loop is bounded by LV_ITEMS, the block count nb of a segment or the class count.
#include "loss_common.h"
#include "../../include/lovasz/lmnet_lovasz.h"

#define LV_TILE LMN_LOVASZ_TILE
#define LV_THREADS 256
#define LV_ITEMS (LV_TILE / LV_THREADS)          // rounds of a tile in the scatter; ranks per lane of a wave's quarter in the coef pass
#define LV_WAVES (LV_THREADS / 64)
#define LV_VOID 0xffffffffu
#define LV_FG 0x80000000u
#define LV_SCAN_THREADS LMN_LOVASZ_SCAN_THREADS
static_assert(LV_SCAN_THREADS == 64 && LV_TILE % LV_THREADS == 0, "tile");
static_assert(LMN_LOVASZ_LABELS_U8 == LOSS_LABELS_U8 && LMN_LOVASZ_LABELS_I64 == LOSS_LABELS_I64 && LMN_LOVASZ_SOFTMAX == LOSS_SOFTMAX &&
              LMN_LOVASZ_SIGMOID == LOSS_SIGMOID, "loss_common.h reads the label kinds and heads of lmnet_lovasz.h");

namespace {

// descending float order as ascending unsigned order; -0 never reaches here (lv_canon)
__device__ __forceinline__ uint32_t lv_key(float e) {
  const uint32_t b = __float_as_uint(e);
  return (b & 0x80000000u) ? b : (~b & 0x7fffffffu);
}
__device__ __forceinline__ float lv_canon(float e) { return e + 0.f; }      // -0 -> +0

__device__ __forceinline__ unsigned lv_wave_incl_scan(unsigned v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = (unsigned)__shfl_up((int)v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

struct LvGeo {
  int64_t hw, P;
  uint64_t cmask;
  int B, C, nk, per_image, kind;
};
// segment and in-segment index of (image b, scored class kk, pixel pix)
__device__ __forceinline__ void lv_place(const LvGeo& g, int64_t b, int kk, int64_t pix, int& s, int64_t& i) {
  if (g.per_image) {
    s = (int)(b * g.nk + kk);
    i = pix;
  } else {
    s = kk;
    i = b * g.hw + pix;
  }
}
// the position in coef [B, nk, H, W] of element i of segment s
__device__ __forceinline__ int64_t lv_coef_off(const LvGeo& g, int s, int64_t i) {
  if (g.per_image) return (int64_t)s * g.P + i;
  const int64_t b = i / g.hw;
  return (b * g.nk + s) * g.hw + (i - b * g.hw);
}

// ------------------------------------------------------------------------------------------------------------------------ keys
// blockIdx.x = b * nbx + (block of 256 pixels of the image).  s_cnt: [0] the valid pixels, [1 + kk] the foreground pixels of class kk
__global__ __launch_bounds__(LV_THREADS) void lv_key_softmax_kernel(const float* __restrict__ logits, const void* __restrict__ target,
                                                                    LvGeo g, int nbx, float* __restrict__ errors,
                                                                    uint32_t* __restrict__ keys, uint32_t* __restrict__ pay,
                                                                    int32_t* __restrict__ counts) {
  __shared__ int s_cnt[65];
  if (threadIdx.x < 65) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t b = blockIdx.x / nbx;
  const int64_t pix = (int64_t)(blockIdx.x - b * nbx) * LV_THREADS + threadIdx.x;
  if (pix < g.hw) {
    const float* lg = logits + b * g.C * g.hw + pix;
    const int64_t yl = loss_label(target, g.kind, b * g.hw + pix);
    const bool valid = (uint64_t)yl < (uint64_t)g.C;
    float mx = -3.0e38f, den = 0.f;
    for (int c = 0; c < g.C; ++c) mx = fmaxf(mx, lg[c * g.hw]);
    for (int c = 0; c < g.C; ++c) den += expf(lg[c * g.hw] - mx);
    const float r = 1.f / den;
    if (valid) atomicAdd(&s_cnt[0], 1);
    int kk = 0;
    for (int c = 0; c < g.C; ++c) {
      if (!((g.cmask >> c) & 1)) continue;
      int s;
      int64_t i;
      lv_place(g, b, kk, pix, s, i);
      const bool fg = valid && yl == c;
      const float p = expf(lg[c * g.hw] - mx) * r;
      const float e = valid ? lv_canon(fabsf((fg ? 1.f : 0.f) - p)) : 0.f;
      const int64_t o = (int64_t)s * g.P + i;
      errors[o] = e;
      keys[o] = valid ? lv_key(e) : LV_VOID;
      pay[o] = (uint32_t)i | (fg ? LV_FG : 0u);
      if (fg) atomicAdd(&s_cnt[1 + kk], 1);
      ++kk;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < g.nk) {
    const int s = g.per_image ? (int)(b * g.nk + threadIdx.x) : (int)threadIdx.x;
    if (s_cnt[0]) atomicAdd(counts + 2 * s, s_cnt[0]);
    if (s_cnt[1 + threadIdx.x]) atomicAdd(counts + 2 * s + 1, s_cnt[1 + threadIdx.x]);
  }
}

// blockIdx.x = (b * nk + kk) * nbx + (block of 256 elements of the plane); cls: the scored planes in ascending order
__global__ __launch_bounds__(LV_THREADS) void lv_key_sigmoid_kernel(const float* __restrict__ logits, const void* __restrict__ target,
                                                                    LvGeo g, LossCls cls, int nbx, float* __restrict__ errors,
                                                                    uint32_t* __restrict__ keys, uint32_t* __restrict__ pay,
                                                                    int32_t* __restrict__ counts) {
  __shared__ int s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t plane = blockIdx.x / nbx;                 // b * nk + kk
  const int64_t b = plane / g.nk;
  const int kk = (int)(plane - b * g.nk);
  const int64_t pix = (int64_t)(blockIdx.x - plane * nbx) * LV_THREADS + threadIdx.x;
  int s;
  int64_t i;
  lv_place(g, b, kk, pix, s, i);
  bool valid = false, fg = false;
  if (pix < g.hw) {
    const int64_t src = (b * g.C + cls.id[kk]) * g.hw + pix;
    const int64_t t = loss_label(target, g.kind, src);
    valid = (uint64_t)t <= 1ull;
    fg = t == 1;
    const float z = logits[src];
    const float e = valid ? lv_canon(1.f - z * (fg ? 1.f : -1.f)) : 0.f;
    const int64_t o = (int64_t)s * g.P + i;
    errors[o] = e;
    keys[o] = valid ? lv_key(e) : LV_VOID;
    pay[o] = (uint32_t)i | (fg ? LV_FG : 0u);
  }
  const int nv = __popcll(__ballot(valid)), nf = __popcll(__ballot(fg));
  if ((threadIdx.x & 63) == 0) {
    if (nv) atomicAdd(&s_cnt[0], nv);
    if (nf) atomicAdd(&s_cnt[1], nf);
  }
  __syncthreads();
  if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(counts + 2 * s + threadIdx.x, s_cnt[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------------------------------ sort
// table[s][digit][block]; blockIdx.x = block, blockIdx.y = s
__global__ __launch_bounds__(LV_THREADS) void lv_hist_kernel(const uint32_t* __restrict__ keys, int64_t P, int nb, int shift,
                                                             uint32_t* __restrict__ table, uint32_t* __restrict__ tot) {
  __shared__ unsigned s_h[256];
  s_h[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t* k = keys + (int64_t)blockIdx.y * P;
  const int64_t t0 = (int64_t)blockIdx.x * LV_TILE;
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) {
    const int64_t i = t0 + j * LV_THREADS + threadIdx.x;
    if (i < P) atomicAdd(&s_h[(k[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  table[((int64_t)blockIdx.y * 256 + threadIdx.x) * nb + blockIdx.x] = s_h[threadIdx.x];
  if (s_h[threadIdx.x]) atomicAdd(tot + (int64_t)blockIdx.y * 256 + threadIdx.x, s_h[threadIdx.x]);
}

// blockIdx.x = digit, blockIdx.y = s; one wave.  The exclusive scan of the segment's table in [digit][block] order, in place: the
// row starts at the total of the smaller digits.
__global__ __launch_bounds__(LV_SCAN_THREADS) void lv_scan_kernel(uint32_t* __restrict__ table, const uint32_t* __restrict__ tot, int nb) {
  const int lane = threadIdx.x, d = blockIdx.x;
  const uint32_t* t = tot + (int64_t)blockIdx.y * 256;
  unsigned a = 0;
  for (int j = lane; j < d; j += 64) a += t[j];
  unsigned carry = loss_wave_sum(a);
  uint32_t* T = table + ((int64_t)blockIdx.y * 256 + d) * nb;
  for (int j0 = 0; j0 < nb; j0 += 64) {
    const int j = j0 + lane;
    const unsigned v = j < nb ? T[j] : 0u;
    const unsigned inc = lv_wave_incl_scan(v, lane);
    if (j < nb) T[j] = carry + inc - v;
    carry += (unsigned)__shfl((int)inc, 63, 64);
  }
}

// blockIdx.x = block, blockIdx.y = s.  pin NULL: the payload is the element index; kout NULL (the last pass): no keys written.
__global__ __launch_bounds__(LV_THREADS) void lv_scatter_kernel(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ pin,
                                                                int64_t P, int nb, int shift, const uint32_t* __restrict__ table,
                                                                uint32_t* __restrict__ tot, uint32_t* __restrict__ kout,
                                                                uint32_t* __restrict__ pout) {
  __shared__ unsigned s_off[256], s_wc[LV_WAVES][256];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t seg = (int64_t)blockIdx.y * P;
  s_off[threadIdx.x] = table[((int64_t)blockIdx.y * 256 + threadIdx.x) * nb + blockIdx.x];
  if (blockIdx.x == 0) tot[(int64_t)blockIdx.y * 256 + threadIdx.x] = 0u;      // (the scan is over: zero for the next pass's histogram)
#pragma unroll
  for (int w = 0; w < LV_WAVES; ++w) s_wc[w][threadIdx.x] = 0u;
  __syncthreads();
  const int64_t t0 = (int64_t)blockIdx.x * LV_TILE;
  for (int j = 0; j < LV_ITEMS; ++j) {
    const int64_t i = t0 + j * LV_THREADS + threadIdx.x;
    const bool live = i < P;
    const uint32_t key = live ? kin[seg + i] : 0u;
    const uint32_t pl = live ? (pin ? pin[seg + i] : (uint32_t)i) : 0u;
    const unsigned d = (key >> shift) & 255u;
    unsigned long long m = __ballot(live);                // the live lanes of this wave with the same digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bb = __ballot(live && bit);
      m &= bit ? bb : ~bb;
    }
    const unsigned rank = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    if (live && rank == 0) s_wc[wv][d] = (unsigned)__popcll(m);
    __syncthreads();
    if (live) {
      unsigned pos = s_off[d] + rank;
      for (int w = 0; w < wv; ++w) pos += s_wc[w][d];
      if ((int64_t)pos < P) {
        if (kout) kout[seg + pos] = key;
        pout[seg + pos] = pl;
      }
    }
    __syncthreads();
    {
      unsigned a = 0;
#pragma unroll
      for (int w = 0; w < LV_WAVES; ++w) {
        a += s_wc[w][threadIdx.x];
        s_wc[w][threadIdx.x] = 0u;
      }
      s_off[threadIdx.x] += a;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------- scan and coefficients
__global__ __launch_bounds__(LV_THREADS) void lv_fgcount_kernel(const uint32_t* __restrict__ pay, int64_t P, int nb, int32_t* __restrict__ bsum) {
  __shared__ int s_w[LV_WAVES];
  const uint32_t* p = pay + (int64_t)blockIdx.y * P;
  const int64_t t0 = (int64_t)blockIdx.x * LV_TILE;
  int a = 0;
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) {
    const int64_t r = t0 + j * LV_THREADS + threadIdx.x;
    a += __popcll(__ballot(r < P && (p[r] & LV_FG)));
  }
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) bsum[(int64_t)blockIdx.y * nb + blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// the weight of segment s in the loss: 1 / (segments averaged in its group * groups), 0 when it is left out.  At most nk steps.
__device__ __forceinline__ float lv_weight(const int32_t* __restrict__ counts, const LvGeo& g, int present, int s) {
  const int groups = g.per_image ? g.B : 1;
  int n = g.nk;
  if (present) {
    if (counts[2 * s + 1] <= 0) return 0.f;
    const int s0 = s / g.nk * g.nk;
    n = 0;
    for (int k = 0; k < g.nk; ++k) n += counts[2 * (s0 + k) + 1] > 0;
  }
  return 1.f / ((float)n * (float)groups);
}

// blockIdx.x = block (LV_TILE ranks of the sorted order), blockIdx.y = s; wave w walks ranks [w, w + 1) * LV_TILE / 4 of the tile
__global__ __launch_bounds__(LV_THREADS) void lv_coef_kernel(const uint32_t* __restrict__ pay, const float* __restrict__ errors,
                                                             const int32_t* __restrict__ counts, const int32_t* __restrict__ bsum,
                                                             LvGeo g, int nb, int present, int hinge, int32_t* __restrict__ perm,
                                                             float* __restrict__ coef, float* __restrict__ slot) {
  __shared__ int s_w[LV_WAVES], s_b[LV_WAVES];
  __shared__ float s_f[LV_WAVES], s_wt;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int s = blockIdx.y;
  const int64_t P = g.P, seg = (int64_t)s * P;
  const uint32_t* p = pay + seg;
  const int64_t w0 = (int64_t)blockIdx.x * LV_TILE + (int64_t)wv * (LV_TILE / LV_WAVES);
  // the foreground elements of the tiles before this one, and of this wave's part
  unsigned before = 0;
  for (int j = threadIdx.x; j < (int)blockIdx.x; j += LV_THREADS) before += (unsigned)bsum[(int64_t)s * nb + j];
  before = loss_wave_sum(before);
  int mine = 0;
#pragma unroll
  for (int j = 0; j < LV_ITEMS; ++j) {
    const int64_t r = w0 + j * 64 + lane;
    mine += __popcll(__ballot(r < P && (p[r] & LV_FG)));
  }
  if (lane == 0) {
    s_b[wv] = (int)before;
    s_w[wv] = mine;
  }
  if (threadIdx.x == 0) s_wt = lv_weight(counts, g, present, s);
  __syncthreads();
  int64_t carry = (int64_t)s_b[0] + s_b[1] + s_b[2] + s_b[3];
  for (int w = 0; w < wv; ++w) carry += s_w[w];
  const int64_t V = counts[2 * s], G = counts[2 * s + 1];
  const float wt = s_wt;
  float acc = 0.f;
  for (int j = 0; j < LV_ITEMS; ++j) {
    const int64_t r = w0 + j * 64 + lane;
    const bool live = r < P;
    const uint32_t pl = live ? p[r] : 0u;
    const bool fg = (pl & LV_FG) != 0u;
    const unsigned long long bal = __ballot(fg);
    const int64_t n = carry + __popcll(bal & (~0ull >> (63 - lane)));     // foreground among ranks 0 .. r
    carry += __popcll(bal);
    if (!live) continue;
    const int64_t idx = (int64_t)(pl & ~LV_FG);
    if (idx >= P) continue;                                               // (cannot happen: the payload is a permutation)
    const int64_t m = r + 1 - n;                                          // background among ranks 0 .. r (r < V: all valid)
    float gr = 0.f;
    if (r < V) {
      if (G == 0) gr = r == 0 ? 1.f : 0.f;
      else if (fg) gr = 1.f / (float)(G + m);
      else gr = (float)(G - n) / ((float)(G + m - 1) * (float)(G + m));
    }
    const float e = errors[seg + idx];
    const bool on = !hinge || e > 0.f;
    acc += on ? e * gr : 0.f;
    perm[seg + r] = (int32_t)idx;
    coef[lv_coef_off(g, s, idx)] = on ? wt * gr : 0.f;
  }
  acc = loss_wave_sum(acc);
  if (lane == 0) s_f[wv] = acc;
  __syncthreads();
  if (threadIdx.x == 0) slot[(int64_t)s * nb + blockIdx.x] = (s_f[0] + s_f[1]) + (s_f[2] + s_f[3]);
}

// one block.  segl[s]: the loss of segment s (a wave per segment, lanes strided over its nb slots, the fixed butterfly); then wave 0,
// lanes strided over the segments.  sums: [0] segments with a non-zero weight  [1] L  [2] scale  [3] 0
__global__ __launch_bounds__(LV_THREADS) void lv_finish_kernel(const float* __restrict__ slot, const int32_t* __restrict__ counts, LvGeo g,
                                                               int S, int nb, int present, float scale, float* __restrict__ segl,
                                                               uint32_t* __restrict__ sums, float* __restrict__ loss) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int s = wv; s < S; s += LV_WAVES) {
    float a = 0.f;
    for (int j = lane; j < nb; j += 64) a += slot[(int64_t)s * nb + j];
    a = loss_wave_sum(a);
    if (lane == 0) segl[s] = a;
  }
  __syncthreads();                                        // (one block: its own global writes are visible after the barrier)
  if (wv != 0) return;
  float a = 0.f;
  unsigned used = 0;
  for (int s = lane; s < S; s += 64) {
    const float w = lv_weight(counts, g, present, s);
    a += w * segl[s];
    used += w != 0.f;
  }
  a = loss_wave_sum(a);
  used = loss_wave_sum(used);
  if (lane == 0) {
    float* fs = reinterpret_cast<float*>(sums);
    sums[0] = used;
    fs[1] = a;
    fs[2] = scale;
    sums[3] = 0u;
    loss[0] = scale * a;
  }
}

// ------------------------------------------------------------------------------------------------------------------- backward
__global__ __launch_bounds__(LV_THREADS) void lv_bwd_softmax_kernel(const float* __restrict__ logits, const void* __restrict__ target, LvGeo g,
                                                                    const float* __restrict__ coef, const uint32_t* __restrict__ sums,
                                                                    const float* __restrict__ gscale, float* __restrict__ dlogits) {
  const float k = (gscale ? gscale[0] : 1.f) * reinterpret_cast<const float*>(sums)[2];
  const int64_t hw = g.hw, total = (int64_t)g.B * hw;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = idx / hw, pix = idx - b * hw;
    const float* lg = logits + b * g.C * hw + pix;
    float* d = dlogits + b * g.C * hw + pix;
    const int64_t yl = loss_label(target, g.kind, idx);
    if ((uint64_t)yl >= (uint64_t)g.C) {                  // void: +0 in every class
      for (int c = 0; c < g.C; ++c) d[c * hw] = 0.f;
      continue;
    }
    const float* cf = coef + b * g.nk * hw + pix;
    float mx = -3.0e38f, den = 0.f;
    for (int c = 0; c < g.C; ++c) mx = fmaxf(mx, lg[c * hw]);
    for (int c = 0; c < g.C; ++c) den += expf(lg[c * hw] - mx);
    const float r = 1.f / den;
    float gp = 0.f;                                       // sum_k p_k dL/dp_k over the scored classes
    int kk = 0;
    for (int c = 0; c < g.C; ++c) {
      if (!((g.cmask >> c) & 1)) continue;
      const float p = expf(lg[c * hw] - mx) * r;
      const float v = cf[kk * hw];
      gp += p * (c == yl ? -v : v);
      ++kk;
    }
    kk = 0;
    for (int c = 0; c < g.C; ++c) {
      const float p = expf(lg[c * hw] - mx) * r;
      float dp = 0.f;
      if ((g.cmask >> c) & 1) {
        const float v = cf[kk * hw];
        dp = c == yl ? -v : v;
        ++kk;
      }
      d[c * hw] = k * (p * (dp - gp));
    }
  }
}

__global__ __launch_bounds__(LV_THREADS) void lv_bwd_sigmoid_kernel(const void* __restrict__ target, LvGeo g, const float* __restrict__ coef,
                                                                    const uint32_t* __restrict__ sums, const float* __restrict__ gscale,
                                                                    float* __restrict__ dlogits) {
  const float k = (gscale ? gscale[0] : 1.f) * reinterpret_cast<const float*>(sums)[2];
  const int64_t hw = g.hw, total = (int64_t)g.B * g.C * hw;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t plane = idx / hw, pix = idx - plane * hw;
    const int64_t b = plane / g.C;
    const int c = (int)(plane - b * g.C);
    float d = 0.f;                                        // unscored plane, void element: +0
    if ((g.cmask >> c) & 1) {
      const int64_t t = loss_label(target, g.kind, idx);
      if ((uint64_t)t <= 1ull) {
        const int kk = __popcll(g.cmask & ((1ull << c) - 1ull));
        const float v = coef[(b * g.nk + kk) * hw + pix];
        d = k * (t == 1 ? -v : v);
      }
    }
    dlogits[idx] = d;
  }
}

// ------------------------------------------------------------------------------------------------------------------------ host
bool lv_dims_ok(int S, int64_t P) { return S >= 1 && S <= LMN_LOVASZ_MAX_SEGMENTS && P >= 1 && (int64_t)S * P < (1LL << 31); }
int64_t lv_nb(int64_t P) { return (P + LV_TILE - 1) / LV_TILE; }

struct LvWs {
  uint32_t *kA, *kB, *pA, *pB, *table, *tot;
  int32_t* bsum;
  float *slot, *segl;
  int64_t bytes;
};
LvWs lv_carve(void* ws, int S, int64_t P) {
  const int64_t nb = lv_nb(P), arr = lmn_up256((int64_t)S * P * 4), tab = lmn_up256((int64_t)S * 256 * nb * 4);
  const int64_t per = lmn_up256((int64_t)S * nb * 4), sg = lmn_up256((int64_t)S * 4), tt = lmn_up256((int64_t)S * 256 * 4);
  uint8_t* p = (uint8_t*)ws;
  LvWs w;
  w.kA = (uint32_t*)p;
  w.kB = (uint32_t*)(p + arr);
  w.pA = (uint32_t*)(p + 2 * arr);
  w.pB = (uint32_t*)(p + 3 * arr);
  w.table = (uint32_t*)(p + 4 * arr);
  w.tot = (uint32_t*)(p + 4 * arr + tab);
  w.bsum = (int32_t*)(p + 4 * arr + tab + tt);
  w.slot = (float*)(p + 4 * arr + tab + tt + per);
  w.segl = (float*)(p + 4 * arr + tab + tt + 2 * per);
  w.bytes = 4 * arr + tab + tt + 2 * per + sg;
  return w;
}

// the four digit passes: (k0, p0) -> ... -> pfinal; p0 NULL: the payload is the element index.  k0 is only read.
void lv_sort(hipStream_t st, const uint32_t* k0, const uint32_t* p0, int S, int64_t P, const LvWs& w, uint32_t* pfinal) {
  const int nb = (int)lv_nb(P);
  const dim3 grid(nb, S), blk(LV_THREADS);
  // pass 0 writes (kA, pA): fwd hands in (kB, pB), order the caller's keys; pass 1 may then overwrite (kB, pB)
  uint32_t* kbuf[2] = {w.kA, w.kB};
  uint32_t* pbuf[2] = {w.pA, w.pB};
  const uint32_t* kin = k0;
  const uint32_t* pin = p0;
  LMN_LAUNCH(loss_zero_kernel, dim3(loss_grid((int64_t)S * 256, 64)), dim3(256), 0, st, w.tot, (int64_t)S * 256);
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 8 * pass;
    uint32_t* kout = pass == 3 ? nullptr : kbuf[pass & 1];
    uint32_t* pout = pass == 3 ? pfinal : pbuf[pass & 1];
    LMN_LAUNCH(lv_hist_kernel, grid, blk, 0, st, kin, P, nb, shift, w.table, w.tot);
    LMN_LAUNCH(lv_scan_kernel, dim3(256, S), dim3(LV_SCAN_THREADS), 0, st, w.table, (const uint32_t*)w.tot, nb);
    LMN_LAUNCH(lv_scatter_kernel, grid, blk, 0, st, kin, pin, P, nb, shift, (const uint32_t*)w.table, w.tot, kout, pout);
    kin = kout;
    pin = pout;
  }
}

int lv_check(const char* what, int target_kind, int head, int B, int C, int H, int W, uint64_t class_mask) {
  LMN_REQUIRE(head == LMN_LOVASZ_SOFTMAX || head == LMN_LOVASZ_SIGMOID, "%s: unknown head %d", what, head);
  LMN_REQUIRE(B >= 1, "%s: B=%d < 1", what, B);
  if (int rc = loss_check_head(what, C, head == LMN_LOVASZ_SOFTMAX, class_mask, target_kind)) return rc;
  return loss_check_extent(what, B, C, H, W);
}

LvGeo lv_geo(int target_kind, int per_image, int B, int C, int H, int W, uint64_t class_mask) {
  LvGeo g;
  g.hw = (int64_t)H * W;
  g.P = per_image ? g.hw : (int64_t)B * g.hw;
  g.cmask = class_mask;
  g.B = B;
  g.C = C;
  g.nk = __builtin_popcountll(class_mask);
  g.per_image = per_image ? 1 : 0;
  g.kind = target_kind;
  return g;
}

}  // namespace

extern "C" {

int64_t lmn_lovasz_workspace(int S, int64_t P) {
  if (!lv_dims_ok(S, P)) {
    snprintf(g_lmn_err, sizeof(g_lmn_err), "lovasz_workspace: S=%d P=%lld outside 1 <= S <= %d, P >= 1, S * P < 2^31", S, (long long)P,
             LMN_LOVASZ_MAX_SEGMENTS);
    return -1;
  }
  return lv_carve(nullptr, S, P).bytes;
}

int lmn_lovasz_order(const uint32_t* keys, int S, int64_t P, void* workspace, int64_t ws_bytes, int32_t* perm, lmn_stream_t stream) {
  LMN_REQUIRE(keys && workspace && perm, "lovasz_order: null pointer");
  LMN_REQUIRE(lv_dims_ok(S, P), "lovasz_order: S=%d P=%lld outside 1 <= S <= %d, P >= 1, S * P < 2^31", S, (long long)P,
              LMN_LOVASZ_MAX_SEGMENTS);
  const LvWs w = lv_carve(workspace, S, P);
  LMN_REQUIRE(ws_bytes >= w.bytes, "lovasz_order: workspace of %lld bytes too small, %lld needed", (long long)ws_bytes, (long long)w.bytes);
  lv_sort((hipStream_t)stream, keys, nullptr, S, P, w, (uint32_t*)perm);
  return lmn_launch_status("lovasz_order");
}

int lmn_lovasz_fwd(const float* logits, const void* target, int target_kind, int head, int per_image, int present, float scale, int B,
                   int C, int H, int W, uint64_t class_mask, void* workspace, int64_t ws_bytes, float* errors, int32_t* perm,
                   int32_t* counts, float* coef, void* sums, float* loss, lmn_stream_t stream) {
  LMN_REQUIRE(logits && target && workspace && errors && perm && counts && coef && sums && loss, "lovasz_fwd: null pointer");
  if (int rc = lv_check("lovasz_fwd", target_kind, head, B, C, H, W, class_mask)) return rc;
  LMN_REQUIRE(loss_finite(scale), "lovasz_fwd: scale=%g is not finite", (double)scale);
  const LvGeo g = lv_geo(target_kind, per_image, B, C, H, W, class_mask);
  const int64_t S64 = per_image ? (int64_t)B * g.nk : g.nk;
  LMN_REQUIRE(S64 <= LMN_LOVASZ_MAX_SEGMENTS, "lovasz_fwd: %lld segments above %d", (long long)S64, LMN_LOVASZ_MAX_SEGMENTS);
  const int S = (int)S64;
  const int64_t P = g.P;
  const LvWs w = lv_carve(workspace, S, P);
  LMN_REQUIRE(ws_bytes >= w.bytes, "lovasz_fwd: workspace of %lld bytes too small, %lld needed", (long long)ws_bytes, (long long)w.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)lv_nb(P), nbx = lmn_cdiv(g.hw, LV_THREADS);
  LMN_LAUNCH(loss_zero_kernel, dim3(loss_grid(2 * (int64_t)S, 64)), dim3(256), 0, st, (uint32_t*)counts, 2 * (int64_t)S);
  if (head == LMN_LOVASZ_SOFTMAX) {
    LMN_LAUNCH(lv_key_softmax_kernel, dim3((unsigned)((int64_t)B * nbx)), dim3(LV_THREADS), 0, st, logits, target, g, nbx, errors, w.kB, w.pB, counts);
  } else {
    LossCls cls;
    loss_classes(class_mask, &cls);
    LMN_LAUNCH(lv_key_sigmoid_kernel, dim3((unsigned)((int64_t)B * g.nk * nbx)), dim3(LV_THREADS), 0, st, logits, target, g, cls, nbx, errors, w.kB,
               w.pB, counts);
  }
  lv_sort(st, w.kB, w.pB, S, P, w, w.pB);
  const dim3 grid(nb, S);
  LMN_LAUNCH(lv_fgcount_kernel, grid, dim3(LV_THREADS), 0, st, (const uint32_t*)w.pB, P, nb, w.bsum);
  LMN_LAUNCH(lv_coef_kernel, grid, dim3(LV_THREADS), 0, st, (const uint32_t*)w.pB, (const float*)errors, (const int32_t*)counts,
             (const int32_t*)w.bsum, g, nb, present ? 1 : 0, head == LMN_LOVASZ_SIGMOID ? 1 : 0, perm, coef, w.slot);
  LMN_LAUNCH(lv_finish_kernel, dim3(1), dim3(LV_THREADS), 0, st, (const float*)w.slot, (const int32_t*)counts, g, S, nb, present ? 1 : 0, scale,
             w.segl, (uint32_t*)sums, loss);
  return lmn_launch_status("lovasz_fwd");
}

int lmn_lovasz_bwd(const float* logits, const void* target, int target_kind, int head, int B, int C, int H, int W, uint64_t class_mask,
                   const float* coef, const void* sums, const float* gscale, float* dlogits, lmn_stream_t stream) {
  LMN_REQUIRE(logits && target && coef && sums && dlogits, "lovasz_bwd: null pointer");
  if (int rc = lv_check("lovasz_bwd", target_kind, head, B, C, H, W, class_mask)) return rc;
  const LvGeo g = lv_geo(target_kind, 0, B, C, H, W, class_mask);
  hipStream_t st = (hipStream_t)stream;
  if (head == LMN_LOVASZ_SOFTMAX) {
    LMN_LAUNCH(lv_bwd_softmax_kernel, dim3(loss_grid((int64_t)B * g.hw, 4096)), dim3(LV_THREADS), 0, st, logits, target, g, coef,
               (const uint32_t*)sums, gscale, dlogits);
  } else {
    LMN_LAUNCH(lv_bwd_sigmoid_kernel, dim3(loss_grid((int64_t)B * C * g.hw, 4096)), dim3(LV_THREADS), 0, st, target, g, coef, (const uint32_t*)sums,
               gscale, dlogits);
  }
  return lmn_launch_status("lovasz_bwd");
}

}  // extern "C"

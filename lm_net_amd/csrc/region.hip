// The region-overlap losses (include/region/lmnet_region.h): Dice, Jaccard, Tversky / focal Tversky and generalized Dice, per batch or
// per image, under a softmax or a sigmoid head.  Same structure as loss_ex.hip and sigmoid.hip: a sums pass, a one-block finish that
// writes the loss and the backward coefficients, a dlogits pass.
//   softmax head: templates for C in {2, 3, 4, 8}, general-C kernels that stage the logits in LDS; blockIdx.y is the image, so a
//                 block's partial sums belong to one image and per_image only changes the slot they are added to;
//   sigmoid head: blockIdx.y is the scored class, blockIdx.z the image, blockIdx.x strides over THAT plane only; four elements per
//                 lane when HW % 4 == 0 and the bases are aligned, one otherwise.
//   sums   fp32 [G, nk, 3]: I = sum p t, P1 = sum p, P2 = sum p^2 (SQ instances only)      counts int32 [G, nk, 2]: T = sum t, N = #valid
//   slots  fp32 [B, gridDim.x, nk, 3]: deterministic mode, one per block of the sums pass (P2 not written by the instances without it)
//   coef   fp32 [G, nk, 3]: a, b, c with d loss / dp_k = a t + b + c p
#include "loss_common.h"
#include "../../include/region/lmnet_region.h"
static_assert(LMN_REGION_LABELS_U8 == LOSS_LABELS_U8 && LMN_REGION_LABELS_I64 == LOSS_LABELS_I64 && LMN_REGION_SOFTMAX == LOSS_SOFTMAX &&
              LMN_REGION_SIGMOID == LOSS_SIGMOID, "loss_common.h reads the label kinds and heads of lmnet_region.h");

namespace {

constexpr int RG_CNT0 = 192;    // the first thread of a block that adds the integer counts (3 * LOSS_MAXC float sums come before it)

// where a block of the sums pass adds its partial sums
struct RgOut {
  float* sums;
  int32_t* counts;
  float* slots;   // deterministic mode, else NULL
  LossCls cls;
  int nk, per_image;
};

template <int KIND>
__device__ __forceinline__ int rg_label(const void* __restrict__ target, int64_t idx, int C) {   // the label, -1 void
  if constexpr (KIND == LMN_REGION_LABELS_U8) {
    const unsigned v = ((const uint8_t*)target)[idx];
    return v < (unsigned)C ? (int)v : -1;
  } else {
    const int64_t v = ((const int64_t*)target)[idx];
    return (uint64_t)v < (uint64_t)C ? (int)v : -1;
  }
}

// The block's sums of the softmax kernels leave through here: red_f[wave][f * C + c], red_u[wave][c] = T_c, red_n[wave] = N.  Thread
// kk * NF + f adds float sum f of scored class kk, thread RG_CNT0 + kk its two counts (integer atomics in either mode).
template <int NF>
__device__ __forceinline__ void rg_block_out(const RgOut& o, int C, int b, const float* red_f, int fstride, const unsigned* red_u,
                                             int ustride, const unsigned* red_n) {
  const int tid = threadIdx.x;
  const int g = o.per_image ? b : 0;
  if (tid < o.nk * NF) {
    const int kk = tid / NF, f = tid - kk * NF, c = o.cls.id[kk];
    const float v = red_f[f * C + c] + red_f[fstride + f * C + c] + red_f[2 * fstride + f * C + c] + red_f[3 * fstride + f * C + c];
    if (o.slots) o.slots[(((int64_t)b * gridDim.x + blockIdx.x) * o.nk + kk) * 3 + f] = v;
    else atomicAdd(o.sums + ((int64_t)g * o.nk + kk) * 3 + f, v);
  } else if (tid >= RG_CNT0 && tid - RG_CNT0 < o.nk) {
    const int kk = tid - RG_CNT0, c = o.cls.id[kk];
    const unsigned t = red_u[c] + red_u[ustride + c] + red_u[2 * ustride + c] + red_u[3 * ustride + c];
    const unsigned n = red_n[0] + red_n[1] + red_n[2] + red_n[3];
    int32_t* cn = o.counts + ((int64_t)g * o.nk + kk) * 2;
    if (t) atomicAdd(cn, (int32_t)t);
    if (n) atomicAdd(cn + 1, (int32_t)n);
  }
}

template <int C, bool SQ, int KIND>
__global__ __launch_bounds__(256) void rg_softmax_sums_kernel(const float* __restrict__ logits, const void* __restrict__ target,
                                                              int64_t hw, RgOut o) {
  constexpr int NF = SQ ? 3 : 2;
  float acc[NF * C];
  unsigned a_t[C], a_n = 0;
#pragma unroll
  for (int k = 0; k < NF * C; ++k) acc[k] = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) a_t[c] = 0;
  const int b = blockIdx.y;
  const float* lg = logits + (int64_t)b * C * hw;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
    float z[C], p[C];
#pragma unroll
    for (int c = 0; c < C; ++c) z[c] = lg[c * hw + i];     // (issued with the label load, not after it)
    const int y = rg_label<KIND>(target, (int64_t)b * hw + i, C);
    if (y < 0) continue;                                    // void: adds to no sum
    loss_softmax<C>(z, p);
    a_n += 1u;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const bool on = c == y;
      acc[c] += on ? p[c] : 0.f;
      acc[C + c] += p[c];
      if (SQ) acc[2 * C + c] += p[c] * p[c];
      a_t[c] += on ? 1u : 0u;
    }
  }
  __shared__ float red_f[4][NF * C];
  __shared__ unsigned red_u[4][C];
  __shared__ unsigned red_n[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NF * C; ++k) {
    const float v = loss_wave_sum(acc[k]);
    if (lane == 0) red_f[wv][k] = v;
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const unsigned v = loss_wave_sum(a_t[c]);
    if (lane == 0) red_u[wv][c] = v;
  }
  a_n = loss_wave_sum(a_n);
  if (lane == 0) red_n[wv] = a_n;
  __syncthreads();
  rg_block_out<NF>(o, C, b, &red_f[0][0], NF * C, &red_u[0][0], C, red_n);
}

// General class count: each wave stages the logits of its 64 pixels in LDS (tile [C][65], one global read per logit) and works in
// two phases per tile, as segloss_ex_sums_gen_kernel:
//   pixel phase  (lane = pixel): max and the softmax denominator of a valid pixel;
//   class phase  (lane = g * C + c, 64 / C pixel groups): the per-class sums over the tile's valid pixels.
// Every partial is summed in a fixed order, so the deterministic slots are bit-identical from run to run.
template <bool SQ, int KIND>
__global__ __launch_bounds__(256) void rg_softmax_sums_gen_kernel(const float* __restrict__ logits, const void* __restrict__ target, int C,
                                                                  int64_t hw, RgOut o) {
  constexpr int NF = SQ ? 3 : 2;
  extern __shared__ float rg_tile[];                   // [4 waves][C][LOSS_TILE_STRIDE]
  __shared__ float s_mx[4][64], s_ri[4][64];
  __shared__ int s_y[4][64];                           // label of the pixel, -1 void, -2 past the end of the image
  __shared__ float s_part[4][3][64];
  __shared__ unsigned s_partu[4][64];
  __shared__ float s_red[4][3 * LOSS_MAXC];
  __shared__ unsigned s_redu[4][LOSS_MAXC];
  __shared__ unsigned s_redn[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* tile = rg_tile + wv * C * LOSS_TILE_STRIDE;
  const int G = 64 / C, cc = lane % C, gg = lane / C;
  const int b = blockIdx.y;
  const float* lg = logits + (int64_t)b * C * hw;
  float a_pt = 0.f, a_p = 0.f, a_pp = 0.f;
  unsigned a_t = 0, a_n = 0;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < hw; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    int y = -2;
    float mx = -3.0e38f, ri = 0.f;
    if (i < hw) {
#pragma unroll 8
      for (int c = 0; c < C; ++c) {                    // (staged whatever the label: the loads go out with the label load)
        const float z = lg[c * hw + i];
        tile[c * LOSS_TILE_STRIDE + lane] = z;
        mx = fmaxf(mx, z);
      }
      y = rg_label<KIND>(target, (int64_t)b * hw + i, C);
      if (y >= 0) {
        float den = 0.f;
        for (int c = 0; c < C; ++c) den += __expf(tile[c * LOSS_TILE_STRIDE + lane] - mx);
        ri = 1.f / den;
        a_n += 1u;
      }
    }
    s_mx[wv][lane] = mx;
    s_ri[wv][lane] = ri;
    s_y[wv][lane] = y;
    __syncthreads();
    if (gg < G) {
      for (int p = gg; p < 64; p += G) {
        const int yp = s_y[wv][p];
        if (yp == -2) break;                           // (pixels past the end are the tail of the tile)
        if (yp < 0) continue;                          // void: adds to no sum
        const float pc = __expf(tile[cc * LOSS_TILE_STRIDE + p] - s_mx[wv][p]) * s_ri[wv][p];
        const bool on = yp == cc;
        a_pt += on ? pc : 0.f;
        a_p += pc;
        if (SQ) a_pp += pc * pc;
        a_t += on ? 1u : 0u;
      }
    }
    __syncthreads();
  }
  s_part[wv][0][lane] = a_pt;
  s_part[wv][1][lane] = a_p;
  s_part[wv][2][lane] = a_pp;
  s_partu[wv][lane] = a_t;
  a_n = loss_wave_sum(a_n);
  if (lane == 0) s_redn[wv] = a_n;
  __syncthreads();
  if (lane < C) {
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      float v = 0.f;
      for (int g = 0; g < G; ++g) v += s_part[wv][k][g * C + lane];
      s_red[wv][k * C + lane] = v;
    }
    unsigned u = 0;
    for (int g = 0; g < G; ++g) u += s_partu[wv][g * C + lane];
    s_redu[wv][lane] = u;
  }
  __syncthreads();
  rg_block_out<NF>(o, C, b, &s_red[0][0], 3 * LOSS_MAXC, &s_redu[0][0], LOSS_MAXC, s_redn);
}

template <bool VEC, bool SQ, int KIND>
__global__ __launch_bounds__(256) void rg_sigmoid_sums_kernel(const float* __restrict__ logits, const void* __restrict__ target, int C,
                                                              int64_t hw, RgOut o) {
  constexpr int E = VEC ? 4 : 1;
  constexpr int NF = SQ ? 3 : 2;
  const int kk = blockIdx.y, b = blockIdx.z, c = o.cls.id[kk];
  const int64_t plane = (int64_t)b * C + c;
  const float* lg = logits + plane * hw;
  const void* tg = (const uint8_t*)target + plane * hw * (KIND == LMN_REGION_LABELS_I64 ? 8 : 1);
  unsigned n_v = 0, n_y = 0;
  float a_i = 0.f, a_p = 0.f, a_pp = 0.f;
  const int64_t items = hw / E;                        // (VEC: hw % 4 == 0)
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < items; q += (int64_t)gridDim.x * 256) {
    float z[E];
    int t[E];
    loss_load_z<E>(lg, q * E, z);
    loss_load_t<KIND, E>(tg, q * E, t);
#pragma unroll
    for (int j = 0; j < E; ++j) {
      if (t[j] > 1) continue;                          // void: adds to no sum
      const float p = sig_point(z[j]).p;
      const bool on = t[j] == 1;
      n_v += 1u;
      n_y += on ? 1u : 0u;
      a_i += on ? p : 0.f;
      a_p += p;
      if (SQ) a_pp += p * p;
    }
  }
  __shared__ float red_f[4][3];
  __shared__ unsigned red_u[4][2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  n_v = loss_wave_sum(n_v);
  n_y = loss_wave_sum(n_y);
  a_i = loss_wave_sum(a_i);
  a_p = loss_wave_sum(a_p);
  if (SQ) a_pp = loss_wave_sum(a_pp);
  if (lane == 0) {
    red_u[wv][0] = n_y; red_u[wv][1] = n_v;
    red_f[wv][0] = a_i; red_f[wv][1] = a_p; red_f[wv][2] = a_pp;
  }
  __syncthreads();
  const int k = threadIdx.x, g = o.per_image ? b : 0;
  if (k < 2) {                                         // the counts: integer atomics, exact and order-independent in either mode
    const unsigned v = red_u[0][k] + red_u[1][k] + red_u[2][k] + red_u[3][k];
    if (v) atomicAdd(o.counts + ((int64_t)g * o.nk + kk) * 2 + k, (int32_t)v);
  } else if (k < 2 + NF) {
    const int f = k - 2;
    const float v = red_f[0][f] + red_f[1][f] + red_f[2][f] + red_f[3][f];
    if (o.slots) o.slots[(((int64_t)b * gridDim.x + blockIdx.x) * o.nk + kk) * 3 + f] = v;
    else atomicAdd(o.sums + ((int64_t)g * o.nk + kk) * 3 + f, v);
  }
}

struct RgFin {
  int kind, sq, G, nk, B, nbx, per_image, det;
  float alpha, beta, smooth, exponent, scale;
};

// L = f(u) and f'(u):  exponent == 1: u, 1;  otherwise u^e and e u^(e - 1) for u > 0, and 0, 0 for u <= 0
__device__ __forceinline__ void rg_power(double u, double ex, double& L, double& dL) {
  if (ex == 1.0) { L = u; dL = 1.0; }
  else if (u > 0.0) { L = pow(u, ex); dL = ex * pow(u, ex - 1.0); }
  else { L = 0.0; dL = 0.0; }
}

// One block.  Deterministic mode first folds the slots of every group into sums, in block order.  Then thread g % 256 takes group g:
// the ratios, the per-class losses and the backward coefficients in fp64; the 256 partial losses are added in thread order.
__global__ __launch_bounds__(256) void rg_finish_kernel(RgFin f, const float* __restrict__ slots, const float* __restrict__ weight,
                                                        float* __restrict__ sums, const int32_t* __restrict__ counts,
                                                        float* __restrict__ coef, float* __restrict__ per_class, float* __restrict__ loss) {
  __shared__ double s_part[256];
  const int nk = f.nk;
  if (f.det) {
    const int64_t row = (int64_t)nk * 3, total = (int64_t)f.G * row;
    const int64_t per = f.per_image ? f.nbx : (int64_t)f.B * f.nbx;
    for (int64_t e = threadIdx.x; e < total; e += 256) {
      const int64_t g = e / row, r = e - g * row;
      if (!f.sq && r % 3 == 2) continue;               // (P2 is not carried: its slots hold nothing, sums stays 0)
      const float* s = slots + (f.per_image ? g * per : 0) * row + r;
      double v = 0.0;
      for (int64_t j = 0; j < per; ++j) v += (double)s[j * row];
      sums[e] = (float)v;
    }
    __syncthreads();
  }
  const double s = f.smooth, ex = f.exponent, wn = (double)f.scale / ((double)f.G * nk);
  double part = 0.0;
  for (int g = threadIdx.x; g < f.G; g += 256) {
    const float* sg = sums + (int64_t)g * nk * 3;
    const int32_t* cg = counts + (int64_t)g * nk * 2;
    float* co = coef + (int64_t)g * nk * 3;
    float* pc = per_class + (int64_t)g * nk;
    if (f.kind == LMN_REGION_GDICE) {
      double vmax = 0.0;
      for (int k = 0; k < nk; ++k) {
        const double T = cg[2 * k];
        if (T > 0.0) vmax = fmax(vmax, 1.0 / (T * T));
      }
      double num = s, den = s;
      for (int k = 0; k < nk; ++k) {
        const double T = cg[2 * k], v = T > 0.0 ? 1.0 / (T * T) : vmax;
        num += 2.0 * v * (double)sg[3 * k];
        den += v * ((double)sg[3 * k + 1] + T);
      }
      const bool ok = den != 0.0;
      double L, dL;
      rg_power(ok ? 1.0 - num / den : 0.0, ex, L, dL);
      if (!ok) { L = 0.0; dL = 0.0; }
      for (int k = 0; k < nk; ++k) {
        const double T = cg[2 * k], v = T > 0.0 ? 1.0 / (T * T) : vmax;
        pc[k] = (float)L;
        co[3 * k] = ok ? (float)(-dL * wn * nk * 2.0 * v / den) : 0.f;   // (every class of the group carries L_g: nk of them)
        co[3 * k + 1] = ok ? (float)(dL * wn * nk * v * num / (den * den)) : 0.f;
        co[3 * k + 2] = 0.f;
      }
      part += wn * nk * L;
      continue;
    }
    for (int k = 0; k < nk; ++k) {
      const double I = sg[3 * k], P1 = sg[3 * k + 1], P2 = sg[3 * k + 2], T = cg[2 * k];
      const double D = (f.sq ? P2 : P1) + T;
      double num, den, rI, rP;                         // R = num / den;  dR/dI = rI (its direct part), dR/dP = rP, P = P2 or P1
      if (f.kind == LMN_REGION_DICE) {
        num = 2.0 * I + s; den = D + s;
        rI = 2.0 / den; rP = -num / (den * den);
      } else if (f.kind == LMN_REGION_JACCARD) {
        num = I + s; den = D - I + s;
        rI = 1.0 / den + num / (den * den); rP = -num / (den * den);
      } else {
        const double al = f.alpha, be = f.beta;
        num = I + s; den = I + al * (P1 - I) + be * (T - I) + s;
        rI = 1.0 / den - num * (1.0 - al - be) / (den * den); rP = -al * num / (den * den);
      }
      const bool ok = den != 0.0;
      double L, dL;
      rg_power(ok ? 1.0 - num / den : 0.0, ex, L, dL);
      if (!ok) { L = 0.0; dL = 0.0; rI = 0.0; rP = 0.0; }
      const double w = (weight ? (double)weight[k] : 1.0) * wn;
      pc[k] = (float)L;
      co[3 * k] = (float)(-dL * w * rI);
      co[3 * k + 1] = f.sq ? 0.f : (float)(-dL * w * rP);
      co[3 * k + 2] = f.sq ? (float)(-2.0 * dL * w * rP) : 0.f;
      part += w * L;
    }
  }
  s_part[threadIdx.x] = part;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = 0.0;
    for (int j = 0; j < 256; ++j) v += s_part[j];
    loss[0] = (float)v;
  }
}

// the coefficients of the C classes of group g, 0 for an unscored class
struct RgIn {
  const float* coef;
  LossCls cls;
  int nk, per_image;
};

template <int C, int KIND>
__global__ __launch_bounds__(256) void rg_softmax_bwd_kernel(const float* __restrict__ logits, const void* __restrict__ target, int64_t hw,
                                                             RgIn in, const float* __restrict__ gscale, float* __restrict__ dlogits) {
  const int b = blockIdx.y;
  float a[C], bq[C], cq[C];
#pragma unroll
  for (int c = 0; c < C; ++c) { a[c] = 0.f; bq[c] = 0.f; cq[c] = 0.f; }
  const float* co = in.coef + (int64_t)(in.per_image ? b : 0) * in.nk * 3;
  for (int kk = 0; kk < in.nk; ++kk) {
    const int k = in.cls.id[kk];
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (c == k) { a[c] = co[3 * kk]; bq[c] = co[3 * kk + 1]; cq[c] = co[3 * kk + 2]; }
  }
  const float gs = gscale ? gscale[0] : 1.f;
  const float* lg = logits + (int64_t)b * C * hw;
  float* dl = dlogits + (int64_t)b * C * hw;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
    float z[C], p[C];
#pragma unroll
    for (int c = 0; c < C; ++c) z[c] = lg[c * hw + i];     // (issued with the label load, not after it)
    const int y = rg_label<KIND>(target, (int64_t)b * hw + i, C);
    if (y < 0) {                                            // void: +0 in every class
#pragma unroll
      for (int c = 0; c < C; ++c) dl[c * hw + i] = 0.f;
      continue;
    }
    loss_softmax<C>(z, p);
    float d[C], dp = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      d[c] = (c == y ? a[c] : 0.f) + bq[c] + cq[c] * p[c];
      dp += d[c] * p[c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) dl[c * hw + i] = gs * (p[c] * (d[c] - dp));
  }
}

// dlogits of the general-C softmax head: one pixel per thread, its C logits staged in LDS ([C][256], one global read each), as
// segloss_ex_bwd_gen_kernel
template <int KIND>
__global__ __launch_bounds__(256) void rg_softmax_bwd_gen_kernel(const float* __restrict__ logits, const void* __restrict__ target, int C,
                                                                 int64_t hw, RgIn in, const float* __restrict__ gscale,
                                                                 float* __restrict__ dlogits) {
  extern __shared__ float rg_tile[];                   // [C][256]
  __shared__ float s_a[LOSS_MAXC], s_b[LOSS_MAXC], s_c[LOSS_MAXC];
  const int b = blockIdx.y;
  if (threadIdx.x < LOSS_MAXC) { s_a[threadIdx.x] = 0.f; s_b[threadIdx.x] = 0.f; s_c[threadIdx.x] = 0.f; }
  __syncthreads();
  if (threadIdx.x < in.nk) {
    const float* co = in.coef + ((int64_t)(in.per_image ? b : 0) * in.nk + threadIdx.x) * 3;
    const int k = in.cls.id[threadIdx.x];
    s_a[k] = co[0]; s_b[k] = co[1]; s_c[k] = co[2];
  }
  __syncthreads();
  float* z = rg_tile + threadIdx.x;
  const float gs = gscale ? gscale[0] : 1.f;
  const float* lg = logits + (int64_t)b * C * hw;
  float* dl = dlogits + (int64_t)b * C * hw;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
    float mx = -3.0e38f;
#pragma unroll 8
    for (int c = 0; c < C; ++c) {
      const float v = lg[c * hw + i];
      z[c * 256] = v;
      mx = fmaxf(mx, v);
    }
    const int y = rg_label<KIND>(target, (int64_t)b * hw + i, C);
    if (y < 0) {                                       // void: +0 in every class
#pragma unroll 8
      for (int c = 0; c < C; ++c) dl[c * hw + i] = 0.f;
      continue;
    }
    float den = 0.f;
    for (int c = 0; c < C; ++c) den += __expf(z[c * 256] - mx);
    const float r = 1.f / den;
    float dp = 0.f;
    for (int c = 0; c < C; ++c) {
      const float p = __expf(z[c * 256] - mx) * r;
      dp += ((c == y ? s_a[c] : 0.f) + s_b[c] + s_c[c] * p) * p;
    }
    for (int c = 0; c < C; ++c) {
      const float p = __expf(z[c * 256] - mx) * r;
      dl[c * hw + i] = gs * (p * ((c == y ? s_a[c] : 0.f) + s_b[c] + s_c[c] * p - dp));
    }
  }
}

// blockIdx.y: the class (every class: an unscored plane is written +0), blockIdx.z: the image
template <bool VEC, int KIND>
__global__ __launch_bounds__(256) void rg_sigmoid_bwd_kernel(const float* __restrict__ logits, const void* __restrict__ target, int C,
                                                             int64_t hw, RgIn in, uint64_t cmask, const float* __restrict__ gscale,
                                                             float* __restrict__ dlogits) {
  constexpr int E = VEC ? 4 : 1;
  const int c = blockIdx.y, b = blockIdx.z;
  const int64_t plane = (int64_t)b * C + c;
  const float* lg = logits + plane * hw;
  float* dl = dlogits + plane * hw;
  const void* tg = (const uint8_t*)target + plane * hw * (KIND == LMN_REGION_LABELS_I64 ? 8 : 1);
  const bool scored = (cmask >> c) & 1ull;
  float a = 0.f, bq = 0.f, cq = 0.f;
  if (scored) {
    const int kk = __popcll(cmask & ((1ull << c) - 1ull));
    const float* co = in.coef + ((int64_t)(in.per_image ? b : 0) * in.nk + kk) * 3;
    a = co[0]; bq = co[1]; cq = co[2];
  }
  const float gs = gscale ? gscale[0] : 1.f;
  const int64_t items = hw / E;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < items; q += (int64_t)gridDim.x * 256) {
    float d[E];
#pragma unroll
    for (int j = 0; j < E; ++j) d[j] = 0.f;            // void or unscored: +0
    if (scored) {
      float z[E];
      int t[E];
      loss_load_z<E>(lg, q * E, z);
      loss_load_t<KIND, E>(tg, q * E, t);
#pragma unroll
      for (int j = 0; j < E; ++j) {
        if (t[j] > 1) continue;
        const SigPoint s = sig_point(z[j]);
        d[j] = gs * (((t[j] == 1 ? a : 0.f) + bq + cq * s.p) * (s.p * s.omp));
      }
    }
    loss_store<E>(dl, q * E, d);
  }
}

// blocks of the sums pass per image (softmax head) or per plane (sigmoid head): a function of head, B, C and HW alone, so that
// lmn_region_workspace can state the slots exactly
inline int rg_nbx(int head, int B, int C, int64_t HW) {
  if (head == LMN_REGION_SOFTMAX) return loss_grid_per(HW, 1024, B);
  return loss_grid_per(HW % 4 == 0 ? HW / 4 : HW, 2048, (int64_t)B * C);
}

inline int64_t rg_ws_bytes(int head, int B, int C, int64_t HW, int nk) {
  return lmn_up256((int64_t)4 * B * rg_nbx(head, B, C, HW) * nk * 3);
}

int rg_check(const char* what, int target_kind, int head, int B, int C, int H, int W, uint64_t class_mask) {
  LMN_REQUIRE(head == LMN_REGION_SOFTMAX || head == LMN_REGION_SIGMOID, "%s: unknown head %d", what, head);
  LMN_REQUIRE(B >= 1 && B <= LMN_REGION_MAX_BATCH, "%s: B=%d not in [1, %d]", what, B, LMN_REGION_MAX_BATCH);
  if (int rc = loss_check_head(what, C, head == LMN_REGION_SOFTMAX, class_mask, target_kind)) return rc;
  return loss_check_extent(what, B, C, H, W);
}

}  // namespace

extern "C" {

int64_t lmn_region_workspace(int head, int B, int C, int H, int W, uint64_t class_mask) {
  if (rg_check("region_workspace", LMN_REGION_LABELS_U8, head, B, C, H, W, class_mask)) return -1;
  return rg_ws_bytes(head, B, C, (int64_t)H * W, __builtin_popcountll(class_mask));
}

int lmn_region_fwd(const float* logits, const void* target, int target_kind, int head, int kind, int denominator, int per_image,
                   float alpha, float beta, float smooth, float exponent, float scale, int B, int C, int H, int W, uint64_t class_mask,
                   const float* weight, void* workspace, int64_t ws_bytes, float* sums, int32_t* counts, float* coef, float* per_class,
                   float* loss, lmn_stream_t stream) {
  LMN_REQUIRE(logits && target && sums && counts && coef && per_class && loss, "region_fwd: null pointer");
  if (int rc = rg_check("region_fwd", target_kind, head, B, C, H, W, class_mask)) return rc;
  LMN_REQUIRE(kind >= LMN_REGION_DICE && kind <= LMN_REGION_GDICE, "region_fwd: unknown kind %d", kind);
  LMN_REQUIRE(denominator == LMN_REGION_LINEAR || denominator == LMN_REGION_SQUARED, "region_fwd: unknown denominator %d", denominator);
  LMN_REQUIRE(denominator == LMN_REGION_LINEAR || kind == LMN_REGION_DICE || kind == LMN_REGION_JACCARD,
              "region_fwd: the squared denominator exists for dice and jaccard only (kind %d)", kind);
  LMN_REQUIRE(alpha >= 0.f && beta >= 0.f && loss_finite(alpha) && loss_finite(beta), "region_fwd: alpha=%g, beta=%g must be finite and >= 0",
              (double)alpha, (double)beta);
  LMN_REQUIRE(smooth >= 0.f && loss_finite(smooth), "region_fwd: smooth=%g must be finite and >= 0", (double)smooth);
  LMN_REQUIRE(exponent > 0.f && exponent <= 8.f, "region_fwd: exponent=%g not in (0, 8]", (double)exponent);
  LMN_REQUIRE(loss_finite(scale), "region_fwd: scale=%g is not finite", (double)scale);
  LMN_REQUIRE(kind != LMN_REGION_GDICE || !weight, "region_fwd: generalized dice takes no class weight");
  const int64_t HW = (int64_t)H * W;
  const int nk = __builtin_popcountll(class_mask), nbx = rg_nbx(head, B, C, HW), G = per_image ? B : 1;
  const int64_t need = rg_ws_bytes(head, B, C, HW, nk);
  LMN_REQUIRE(workspace || !g_lmn_det, "region_fwd: deterministic mode needs the workspace");
  LMN_REQUIRE(!workspace || ws_bytes >= need, "region_fwd: workspace of %lld bytes too small, %lld needed", (long long)ws_bytes, (long long)need);
  hipStream_t st = (hipStream_t)stream;
  const bool sq = denominator == LMN_REGION_SQUARED;
  RgOut o;
  o.sums = sums;
  o.counts = counts;
  o.slots = g_lmn_det ? (float*)workspace : nullptr;
  loss_classes(class_mask, &o.cls);
  o.nk = nk;
  o.per_image = per_image ? 1 : 0;
  const int64_t words = (int64_t)G * nk;
  LMN_LAUNCH(loss_zero_kernel, dim3(loss_grid(3 * words, 64)), dim3(256), 0, st, (uint32_t*)sums, 3 * words);
  LMN_LAUNCH(loss_zero_kernel, dim3(loss_grid(2 * words, 64)), dim3(256), 0, st, (uint32_t*)counts, 2 * words);
  if (head == LMN_REGION_SOFTMAX) {
    const dim3 grid(nbx, B);
    LOSS_SWITCH_CT(C, LOSS_SWITCH_KIND(target_kind, LOSS_SWITCH_BOOL(SQ, sq, {
      if constexpr (CT > 0) {
        LMN_LAUNCH((rg_softmax_sums_kernel<CT, SQ, KIND>), grid, dim3(256), 0, st, logits, target, HW, o);
      } else {
        const size_t sh = (size_t)4 * C * LOSS_TILE_STRIDE * sizeof(float);
        if (sh > 48 * 1024) (void)hipFuncSetAttribute   /* (with the static arrays: past 64 KB in all) */
         ((const void*)rg_softmax_sums_gen_kernel<SQ, KIND>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
        LMN_LAUNCH((rg_softmax_sums_gen_kernel<SQ, KIND>), grid, dim3(256), sh, st, logits, target, C, HW, o);
      }
    })));
  } else {
    const bool vec = HW % 4 == 0 && lmn_aligned(logits, 16) && lmn_aligned(target, target_kind == LMN_REGION_LABELS_I64 ? 16 : 4);
    const dim3 grid(nbx, nk, B);
    LOSS_SWITCH_BOOL(SQ, sq, LOSS_SWITCH_KIND(target_kind, LOSS_SWITCH_BOOL(VEC, vec,
      LMN_LAUNCH((rg_sigmoid_sums_kernel<VEC, SQ, KIND>), grid, dim3(256), 0, st, logits, target, C, HW, o))));
  }
  const RgFin fin{kind, sq ? 1 : 0, G, nk, B, nbx, per_image ? 1 : 0, g_lmn_det ? 1 : 0, alpha, beta, smooth, exponent, scale};
  LMN_LAUNCH(rg_finish_kernel, dim3(1), dim3(256), 0, st, fin, (const float*)o.slots, weight, sums, (const int32_t*)counts, coef, per_class, loss);
  return lmn_launch_status("region_fwd");
}

int lmn_region_bwd(const float* logits, const void* target, int target_kind, int head, int per_image, int B, int C, int H, int W,
                   uint64_t class_mask, const float* coef, const float* gscale, float* dlogits, lmn_stream_t stream) {
  LMN_REQUIRE(logits && target && coef && dlogits, "region_bwd: null pointer");
  if (int rc = rg_check("region_bwd", target_kind, head, B, C, H, W, class_mask)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  RgIn in;
  in.coef = coef;
  loss_classes(class_mask, &in.cls);
  in.nk = __builtin_popcountll(class_mask);
  in.per_image = per_image ? 1 : 0;
  if (head == LMN_REGION_SOFTMAX) {
    const dim3 grid(loss_grid_per(HW, 4096, B), B);
    LOSS_SWITCH_CT(C, LOSS_SWITCH_KIND(target_kind, {
      if constexpr (CT > 0) {
        LMN_LAUNCH((rg_softmax_bwd_kernel<CT, KIND>), grid, dim3(256), 0, st, logits, target, HW, in, gscale, dlogits);
      } else {
        const size_t sh = (size_t)C * 256 * sizeof(float);   // (<= 64 KB of LDS at C = 64)
        LMN_LAUNCH((rg_softmax_bwd_gen_kernel<KIND>), grid, dim3(256), sh, st, logits, target, C, HW, in, gscale, dlogits);
      }
    }));
  } else {
    const bool vec = HW % 4 == 0 && lmn_aligned(logits, 16) && lmn_aligned(dlogits, 16) && lmn_aligned(target, target_kind == LMN_REGION_LABELS_I64 ? 16 : 4);
    const dim3 grid(loss_grid_per(vec ? HW / 4 : HW, 4096, (int64_t)B * C), C, B);
    LOSS_SWITCH_KIND(target_kind, LOSS_SWITCH_BOOL(VEC, vec, LMN_LAUNCH((rg_sigmoid_bwd_kernel<VEC, KIND>), grid, dim3(256), 0, st, logits, target, C, HW, in, class_mask, gscale, dlogits)));
  }
  return lmn_launch_status("region_bwd");
}

}  // extern "C"

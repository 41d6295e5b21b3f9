// The training loss with void labels and a focal term (include/lmnet_loss.h; that header's lmn_image_stats is in metrics.hip).
// Same structure as the loss of rows.hip: a sums pass, a one-block finish that writes the loss terms and the backward coefficients, a
// dlogits pass; templates for C in {2, 3, 4, 8}, general-C kernels that stage the logits in LDS.
//   sums: [0] S_w = sum_valid w_y   [1] sum_valid w_y*(-log p_y)   [2] sum_valid sum_c w_c*(-log p_c)   [3] focal sum
//         [4+c] I_c = sum_valid p_c*t_c   [4+C+c] Z_c = sum_valid p_c^2   [4+2C+c] Y_c = sum_valid t_c     (N_v = sum_c Y_c)
//   coef: [0] ce_scale*(1-eps)/S_w  [1] ce_scale*(eps/C)/S_w  [2] sum_c w_c  [3] focal_scale/N_v
//         [4+c] a_c  [4+C+c] b_c   with dL_dice/dp_c = a_c*t_c + b_c*p_c
// A pixel is valid when 0 <= y < C.  ignore_index lies outside [0, C) (checked by the entries), so that one unsigned compare covers
// it and every other out-of-range label.
#include "loss_common.h"
#include "../../include/lmnet_loss.h"

namespace {

template <int C, bool FOCAL>
__global__ __launch_bounds__(256) void segloss_ex_sums_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                              const float* __restrict__ wce, int B, int64_t hw, FocalK fk,
                                                              float* __restrict__ sums, int det) {
  constexpr int NS = 4 + 3 * C;
  float acc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = 0.f;
  float w[C];
#pragma unroll
  for (int c = 0; c < C; ++c) w[c] = wce[c];
  const int64_t total = (int64_t)B * hw;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = idx / hw, i = idx - b * hw;
    const float* lg = logits + b * C * hw + i;
    float z[C], p[C], lse;
#pragma unroll
    for (int c = 0; c < C; ++c) z[c] = lg[c * hw];         // (issued with the label load, not after it: one memory latency per pixel)
    const int64_t yl = target[idx];
    if ((uint64_t)yl >= (uint64_t)C) continue;             // void: adds to no sum
    const int y = (int)yl;
    loss_softmax<C>(z, p, lse);
    float sm = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float nlp = lse - z[c];  // -log p_c
      const float t = (c == y) ? 1.f : 0.f;
      sm += w[c] * nlp;
      acc[0] += t * w[c];
      acc[1] += t * w[c] * nlp;
      acc[4 + c] += p[c] * t;
      acc[4 + C + c] += p[c] * p[c];
      acc[4 + 2 * C + c] += t;
      if (FOCAL) acc[3] += focal_value(sig_point(z[c]), c == y, fk);
    }
    acc[2] += sm;
  }
  __shared__ float red[4][NS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const float v = loss_wave_sum(acc[k]);
    if (lane == 0) red[wv][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < NS)   // (deterministic mode: sums addresses slot copies [blocks][NS])
    lmn_red_add(sums + (det ? (int64_t)blockIdx.x * NS : 0) + threadIdx.x,
                red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x], det);
}

struct FinishK { float eps, smooth, ce_scale, dice_scale, focal_scale; };

// loss4 = total, ce, dice, focal.  N_v = 0 or S_w = 0: ce and focal are 0 and so are their coefficients (no NaN reaches the step).
__global__ void segloss_ex_finish_kernel(const float* __restrict__ sums, const float* __restrict__ wce, const float* __restrict__ wdice,
                                         int C, FinishK k, float* __restrict__ loss4, float* __restrict__ coef) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float Sw = sums[0];
  float dice = 0.f, wsum = 0.f, nv = 0.f;
  for (int c = 0; c < C; ++c) {
    const float I = sums[4 + c], Z = sums[4 + C + c], Y = sums[4 + 2 * C + c];
    const float num = 2.f * I + k.smooth, den = Z + Y + k.smooth;
    const bool ok = den > 0.f;                             // (smooth = 0 and no valid pixel: the class contributes nothing)
    dice += ok ? wdice[c] * (1.f - num / den) / C : 0.f;
    coef[4 + c] = ok ? k.dice_scale * (wdice[c] / C * (-2.f / den)) : 0.f;
    coef[4 + C + c] = ok ? k.dice_scale * (wdice[c] / C * (2.f * num / (den * den))) : 0.f;
    wsum += wce[c];
    nv += Y;
  }
  const bool ce_ok = Sw > 0.f, f_ok = nv > 0.f;
  const float ce = ce_ok ? k.ce_scale * (((1.f - k.eps) * sums[1] + (k.eps / C) * sums[2]) / Sw) : 0.f;
  const float focal = f_ok ? k.focal_scale * (sums[3] / nv) : 0.f;
  dice *= k.dice_scale;
  coef[0] = ce_ok ? k.ce_scale * (1.f - k.eps) / Sw : 0.f;
  coef[1] = ce_ok ? k.ce_scale * (k.eps / C) / Sw : 0.f;
  coef[2] = wsum;
  coef[3] = f_ok ? k.focal_scale / nv : 0.f;
  loss4[0] = ce + dice + focal;
  loss4[1] = ce;
  loss4[2] = dice;
  loss4[3] = focal;
}

template <int C, bool FOCAL>
__global__ __launch_bounds__(256) void segloss_ex_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                             const float* __restrict__ wce, const float* __restrict__ coef,
                                                             const float* __restrict__ gscale, int B, int64_t hw, FocalK fk,
                                                             float* __restrict__ dlogits) {
  float w[C], a[C], bq[C];
#pragma unroll
  for (int c = 0; c < C; ++c) { w[c] = wce[c]; a[c] = coef[4 + c]; bq[c] = coef[4 + C + c]; }
  const float k_nll = coef[0], k_sm = coef[1], wsum = coef[2], k_f = coef[3];
  const float gs = gscale ? gscale[0] : 1.f;
  const int64_t total = (int64_t)B * hw;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = idx / hw, i = idx - b * hw;
    float* d = dlogits + b * C * hw + i;
    const float* lg = logits + b * C * hw + i;
    float z[C], p[C], lse;
#pragma unroll
    for (int c = 0; c < C; ++c) z[c] = lg[c * hw];         // (issued with the label load, not after it)
    const int64_t yl = target[idx];
    if ((uint64_t)yl >= (uint64_t)C) {                     // void: zero gradient in every class
#pragma unroll
      for (int c = 0; c < C; ++c) d[c * hw] = 0.f;
      continue;
    }
    const int y = (int)yl;
    loss_softmax<C>(z, p, lse);
    float wy = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) wy = (c == y) ? w[c] : wy;
    float g[C], gp = 0.f;  // dice: dL/dp_c, then through the softmax Jacobian
#pragma unroll
    for (int c = 0; c < C; ++c) {
      g[c] = a[c] * ((c == y) ? 1.f : 0.f) + bq[c] * p[c];
      gp += g[c] * p[c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float t = (c == y) ? 1.f : 0.f;
      float v = k_nll * wy * (p[c] - t) + k_sm * (p[c] * wsum - w[c]) + p[c] * (g[c] - gp);
      if (FOCAL) v += k_f * focal_grad(sig_point(z[c]), c == y, fk);
      d[c * hw] = gs * v;
    }
  }
}

// General class count: each wave stages the logits of its 64 pixels in LDS (tile [C][65], one global read per logit) and works in
// two phases per tile, as segloss_sums_gen_kernel of rows.hip:
//   pixel phase  (lane = pixel): max, log-sum-exp, the three cross-entropy sums of a valid pixel;
//   class phase  (lane = g*C + c, G = 64/C pixel groups): the three per-class sums and the focal sum over the tile's valid pixels.
// Every partial is summed in a fixed order, so the deterministic slot copies are bit-identical from run to run.
template <bool FOCAL>
__global__ __launch_bounds__(256) void segloss_ex_sums_gen_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                                  const float* __restrict__ wce, int B, int C, int64_t hw, FocalK fk,
                                                                  float* __restrict__ sums, int det) {
  extern __shared__ float lx_tile[];                  // [4 waves][C][LOSS_TILE_STRIDE]
  __shared__ float s_lse[4][64];
  __shared__ int s_y[4][64];                          // label of the pixel, -1 void, -2 past the end of the batch
  __shared__ float s_part[4][3][64];
  __shared__ float s_red[4][4 + 3 * LOSS_MAXC];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* tile = lx_tile + wv * C * LOSS_TILE_STRIDE;
  const int G = 64 / C, cc = lane % C, gg = lane / C;
  float a_w = 0.f, a_nll = 0.f, a_sm = 0.f, a_f = 0.f, a_pt = 0.f, a_pp = 0.f, a_t = 0.f;
  const int64_t total = (int64_t)B * hw;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < total; base += (int64_t)gridDim.x * 256) {
    const int64_t idx = base + threadIdx.x;
    int y = -2;
    float lse = 0.f;
    if (idx < total) {
      const int64_t b = idx / hw, i = idx - b * hw;
      const float* lg = logits + b * C * hw + i;
      float mx = -3.0e38f;
#pragma unroll 8
      for (int c = 0; c < C; ++c) {                   // (staged whatever the label: the loads go out with the label load)
        const float z = lg[c * hw];
        tile[c * LOSS_TILE_STRIDE + lane] = z;
        mx = fmaxf(mx, z);
      }
      const int64_t yl = target[idx];
      y = ((uint64_t)yl < (uint64_t)C) ? (int)yl : -1;
      if (y >= 0) {
        float den = 0.f;
        for (int c = 0; c < C; ++c) den += __expf(tile[c * LOSS_TILE_STRIDE + lane] - mx);
        lse = mx + __logf(den);
        float sm = 0.f;
        for (int c = 0; c < C; ++c) sm += wce[c] * (lse - tile[c * LOSS_TILE_STRIDE + lane]);   // sum_c w_c * (-log p_c)
        a_sm += sm;
        const float wy = wce[y];
        a_w += wy;
        a_nll += wy * (lse - tile[y * LOSS_TILE_STRIDE + lane]);
      }
    }
    s_lse[wv][lane] = lse;
    s_y[wv][lane] = y;
    __syncthreads();
    if (gg < G) {
      for (int p = gg; p < 64; p += G) {
        const int yp = s_y[wv][p];
        if (yp == -2) break;                          // (pixels past the end are the tail of the tile)
        if (yp < 0) continue;                         // void: adds to no sum
        const float z = tile[cc * LOSS_TILE_STRIDE + p];
        const float pc = __expf(z - s_lse[wv][p]);
        const float t = (yp == cc) ? 1.f : 0.f;
        a_pt += pc * t;
        a_pp += pc * pc;
        a_t += t;
        if (FOCAL) a_f += focal_value(sig_point(z), yp == cc, fk);
      }
    }
    __syncthreads();
  }
  s_part[wv][0][lane] = a_pt;
  s_part[wv][1][lane] = a_pp;
  s_part[wv][2][lane] = a_t;
  a_w = loss_wave_sum(a_w);
  a_nll = loss_wave_sum(a_nll);
  a_sm = loss_wave_sum(a_sm);
  a_f = loss_wave_sum(a_f);
  if (lane == 0) { s_red[wv][0] = a_w; s_red[wv][1] = a_nll; s_red[wv][2] = a_sm; s_red[wv][3] = a_f; }
  __syncthreads();
  if (lane < C) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float v = 0.f;
      for (int g = 0; g < G; ++g) v += s_part[wv][k][g * C + lane];
      s_red[wv][4 + k * C + lane] = v;
    }
  }
  __syncthreads();
  const int NS = 4 + 3 * C;
  if (threadIdx.x < NS)   // (deterministic mode: sums addresses slot copies [blocks][NS])
    lmn_red_add(sums + (det ? (int64_t)blockIdx.x * NS : 0) + threadIdx.x,
                s_red[0][threadIdx.x] + s_red[1][threadIdx.x] + s_red[2][threadIdx.x] + s_red[3][threadIdx.x], det);
}

// dlogits of the general-C loss: one pixel per thread, its C logits staged in LDS ([C][256], one global read each); three passes
// over them (max / denominator, dice dot product, the write).
template <bool FOCAL>
__global__ __launch_bounds__(256) void segloss_ex_bwd_gen_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                                 const float* __restrict__ wce, const float* __restrict__ coef,
                                                                 const float* __restrict__ gscale, int B, int C, int64_t hw, FocalK fk,
                                                                 float* __restrict__ dlogits) {
  extern __shared__ float lx_tile[];                  // [C][256]
  float* z = lx_tile + threadIdx.x;
  const float k_nll = coef[0], k_sm = coef[1], wsum = coef[2], k_f = coef[3];
  const float* a = coef + 4;
  const float* bq = coef + 4 + C;
  const float gs = gscale ? gscale[0] : 1.f;
  const int64_t total = (int64_t)B * hw;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = idx / hw, i = idx - b * hw;
    float* d = dlogits + b * C * hw + i;
    const float* lg = logits + b * C * hw + i;
    float mx = -3.0e38f;
#pragma unroll 8
    for (int c = 0; c < C; ++c) {
      const float v = lg[c * hw];
      z[c * 256] = v;
      mx = fmaxf(mx, v);
    }
    const int64_t yl = target[idx];
    if ((uint64_t)yl >= (uint64_t)C) {                // void: zero gradient in every class
#pragma unroll 8
      for (int c = 0; c < C; ++c) d[c * hw] = 0.f;
      continue;
    }
    const int y = (int)yl;
    float den = 0.f;
    for (int c = 0; c < C; ++c) den += __expf(z[c * 256] - mx);
    const float r = 1.f / den;
    const float wy = wce[y];
    float gp = 0.f;
    for (int c = 0; c < C; ++c) {
      const float p = __expf(z[c * 256] - mx) * r;
      gp += (a[c] * ((c == y) ? 1.f : 0.f) + bq[c] * p) * p;
    }
    for (int c = 0; c < C; ++c) {
      const float zc = z[c * 256];
      const float p = __expf(zc - mx) * r;
      const float t = (c == y) ? 1.f : 0.f;
      float v = k_nll * wy * (p - t) + k_sm * (p * wsum - wce[c]) + p * (a[c] * t + bq[c] * p - gp);
      if (FOCAL) v += k_f * focal_grad(sig_point(zc), c == y, fk);
      d[c * hw] = gs * v;
    }
  }
}

// the argument checks shared by the two loss entries
int lx_check(const char* what, int B, int C, int64_t HW, const lmn_loss_param_t* p) {
  LMN_REQUIRE(B > 0 && HW > 0 && C >= 2 && C <= LOSS_MAXC, "%s: C=%d not in [2, %d]", what, C, LOSS_MAXC);
  LMN_REQUIRE(!p->has_ignore || p->ignore_index < 0 || p->ignore_index >= C, "%s: ignore_index=%lld inside [0, %d)", what,
              (long long)p->ignore_index, C);
  LMN_REQUIRE(p->label_smoothing >= 0.f && p->label_smoothing <= 1.f, "%s: label_smoothing=%g not in [0, 1]", what, (double)p->label_smoothing);
  if (int rc = loss_check_terms(what, "ce", p->smooth, p->ce_scale, p->dice_scale, p->focal_scale, p->focal_gamma, p->focal_alpha))
    return rc;
  return 0;
}

}  // namespace

extern "C" {

int lmn_sizeof_loss_param(void) { return (int)sizeof(lmn_loss_param_t); }

int lmn_segloss_ex_fwd(const float* logits, const int64_t* target, const float* w_ce, const float* w_dice, int B, int C, int64_t HW,
                       const lmn_loss_param_t* param, float* sums, float* coef, float* loss4, lmn_stream_t stream) {
  LMN_REQUIRE(logits && target && w_ce && w_dice && param && sums && coef && loss4, "segloss_ex_fwd: null pointer");
  if (int rc = lx_check("segloss_ex_fwd", B, C, HW, param)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool focal = param->focal_scale > 0.f;
  const int NS = LMN_LOSS_SUMS_FLOATS(C);
  const int grid = loss_grid((int64_t)B * HW, 1024);   // (the general form runs one 256-pixel tile per block and iteration)
  const FocalK fk{param->focal_gamma, param->focal_alpha};
  const FinishK fin{param->label_smoothing, param->smooth, param->ce_scale, param->dice_scale, param->focal_scale};
  LMN_LAUNCH(loss_zero_kernel, dim3(1), dim3(256), 0, st, (uint32_t*)sums, (int64_t)NS);
  float* sd = sums;
  if (g_lmn_det) {
    lmn_det_begin(st);
    sd = lmn_det_slots(st, (size_t)grid * NS);
    LMN_REQUIRE(sd, "segloss_ex_fwd: deterministic mode: no scratch");
  }
  LOSS_SWITCH_CT(C, LOSS_SWITCH_BOOL(FOCAL, focal, {
    if constexpr (CT > 0) {
      LMN_LAUNCH((segloss_ex_sums_kernel<CT, FOCAL>), dim3(grid), dim3(256), 0, st, logits, target, w_ce, B, HW, fk, sd, g_lmn_det);
    } else {
      const size_t sh = (size_t)4 * C * LOSS_TILE_STRIDE * sizeof(float);
      if (sh > 64 * 1024) (void)hipFuncSetAttribute((const void*)segloss_ex_sums_gen_kernel<FOCAL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
      LMN_LAUNCH((segloss_ex_sums_gen_kernel<FOCAL>), dim3(grid), dim3(256), sh, st, logits, target, w_ce, B, C, HW, fk, sd, g_lmn_det);
    }
  }));
  if (g_lmn_det) lmn_det_sum(st, sd, grid, NS, sums);
  LMN_LAUNCH(segloss_ex_finish_kernel, dim3(1), dim3(64), 0, st, sums, w_ce, w_dice, C, fin, loss4, coef);
  return lmn_launch_status("segloss_ex_fwd");
}

int lmn_segloss_ex_bwd(const float* logits, const int64_t* target, const float* w_ce, const float* coef, const float* gscale, int B,
                       int C, int64_t HW, const lmn_loss_param_t* param, float* dlogits, lmn_stream_t stream) {
  LMN_REQUIRE(logits && target && w_ce && coef && param && dlogits, "segloss_ex_bwd: null pointer");
  if (int rc = lx_check("segloss_ex_bwd", B, C, HW, param)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool focal = param->focal_scale > 0.f;
  const int grid = loss_grid((int64_t)B * HW, 4096);
  const FocalK fk{param->focal_gamma, param->focal_alpha};
  LOSS_SWITCH_CT(C, LOSS_SWITCH_BOOL(FOCAL, focal, {
    if constexpr (CT > 0) {
      LMN_LAUNCH((segloss_ex_bwd_kernel<CT, FOCAL>), dim3(grid), dim3(256), 0, st, logits, target, w_ce, coef, gscale, B, HW, fk, dlogits);
    } else {
      const size_t sh = (size_t)C * 256 * sizeof(float);   // (<= 64 KB of LDS at C = 64)
      LMN_LAUNCH((segloss_ex_bwd_gen_kernel<FOCAL>), dim3(grid), dim3(256), sh, st, logits, target, w_ce, coef, gscale, B, C, HW, fk, dlogits);
    }
  }));
  return lmn_launch_status("segloss_ex_bwd");
}

}  // extern "C"

// The entries of include/optim/lmnet_optim.h: a deterministic reduction over the flat gradient that leaves a control block on the device
// (lmn_optim_prepare) and the AdamW step that reads it (lmn_adamw_step_ex): parameter groups, gradient clipping, the loss-scale skip
// and weight averaging without a host decision.  Both are bandwidth-bound streams over quads of four floats: 256-lane blocks, one
// 16-byte load per lane, buffer and iteration; the only LDS is the block reduction's.  The wave sum and the capped grid are those of
// the losses (loss_common.h).
#include <float.h>
#include <math.h>

#include "../../include/optim/lmnet_optim.h"
#include "loss_common.h"

static_assert(sizeof(lmn_optim_param_t) == LMN_OPTIM_PARAM_BYTES, "lmn_optim_param_t: fixed size");

namespace {

// bit k: group k is frozen (table: [LMN_OPTIM_MAX_GROUPS][4] floats, uniform loads)
__device__ __forceinline__ unsigned optim_frozen_mask(const float* __restrict__ table, int n_groups) {
  unsigned f = 0u;
  for (int k = 0; k < n_groups; ++k) f |= (table[4 * k + 2] != 0.f ? 1u : 0u) << k;
  return f;
}

// pass 1: partial[b] = sum of g^2, counts[b] = number of non-finite values, over the quads of block b whose group is not frozen.
// Fixed order: lane (grid-stride, ascending), wave butterfly, the four waves ascending.  Plain stores, one per block.
__global__ void __launch_bounds__(256) optim_sumsq_kernel(const float* __restrict__ g, int64_t n4, const uint8_t* __restrict__ qgroup,
                                                          const float* __restrict__ table, int n_groups, float* __restrict__ partial,
                                                          uint32_t* __restrict__ counts) {
  const unsigned frozen = optim_frozen_mask(table, n_groups);
  float s = 0.f;
  unsigned c = 0u;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const unsigned k = qgroup[i] & (LMN_OPTIM_MAX_GROUPS - 1);
    if ((frozen >> k) & 1u) continue;
    const f32x4 x = ld4(g + 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s += x[j] * x[j];
      c += !(fabsf(x[j]) <= FLT_MAX) ? 1u : 0u;
    }
  }
  s = loss_wave_sum(s);
  c = loss_wave_sum(c);
  __shared__ float ss[4];
  __shared__ unsigned sc[4];
  if ((threadIdx.x & 63) == 0) {
    ss[threadIdx.x >> 6] = s;
    sc[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = ((ss[0] + ss[1]) + ss[2]) + ss[3];
    counts[blockIdx.x] = sc[0] + sc[1] + sc[2] + sc[3];
  }
}

struct FinishK { double beta1, beta2; float max_norm; int flags; };

// pass 2 (one block): the nb partials in double, lane t takes t, t + 256, ... ascending, then a fixed tree over the 256 lanes; lane 0
// writes the control block.  nb = 0: no reduction was run.
__global__ void __launch_bounds__(256) optim_finish_kernel(const float* __restrict__ partial, const uint32_t* __restrict__ counts, int nb,
                                                           FinishK K, const float* __restrict__ grad_scale,
                                                           const float* __restrict__ found_inf, uint32_t* __restrict__ ctrl) {
  __shared__ double sd[256];
  __shared__ unsigned sc[256];
  double d = 0.0;
  unsigned c = 0u;
  for (int i = threadIdx.x; i < nb; i += 256) {
    d += (double)partial[i];
    c += counts[i];
  }
  sd[threadIdx.x] = d;
  sc[threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sd[threadIdx.x] += sd[threadIdx.x + o];
      sc[threadIdx.x] += sc[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const unsigned nonfinite = sc[0];
  const float inv_scale = grad_scale ? (float)(1.0 / (double)grad_scale[0]) : 1.f;      // (GradScaler: scale.double().reciprocal().float())
  const bool inf_in = found_inf && found_inf[0] != 0.f;
  const bool skip = (K.flags & LMN_OPTIM_SKIP_NONFINITE) && (nonfinite != 0u || inf_in);
  const float gn = (float)(sqrt(sd[0]) * (double)inv_scale);
  const float coef = K.max_norm > 0.f ? fminf(1.f, K.max_norm / (gn + 1e-6f)) : 1.f;
  const uint32_t step = ctrl[LMN_OPTIM_STEP] + (skip ? 0u : 1u);
  const double t = (double)(step ? step : 1u);
  const float bc1 = (float)(1.0 - pow(K.beta1, t)), bc2 = (float)(1.0 - pow(K.beta2, t));
  ctrl[LMN_OPTIM_SKIP] = skip ? 1u : 0u;
  ctrl[LMN_OPTIM_STEP] = step;
  ctrl[LMN_OPTIM_SKIPPED] += skip ? 1u : 0u;
  ctrl[LMN_OPTIM_GRAD_NORM] = __float_as_uint(gn);
  ctrl[LMN_OPTIM_INV_SCALE] = __float_as_uint(inv_scale);
  ctrl[LMN_OPTIM_COEF] = __float_as_uint(coef);
  ctrl[LMN_OPTIM_INV_BC1] = __float_as_uint(1.f / bc1);
  ctrl[LMN_OPTIM_INV_SQRT_BC2] = __float_as_uint(1.f / sqrtf(bc2));
  ctrl[LMN_OPTIM_NONFINITE] = nonfinite;
}

// adamw_kernel of rows.hip (same arithmetic, same order) with the step's scalars read from the control block, lr / weight decay from
// the group table, gradients unscaled and clipped on the fly, frozen quads untouched and an optional EMA of the new parameters.
template <bool EMA>
__global__ void __launch_bounds__(256) adamw_ex_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, float* __restrict__ ema, int64_t n4,
                                                       const uint8_t* __restrict__ qgroup, const uint32_t* __restrict__ ctrl,
                                                       const float* __restrict__ table, int n_groups, float b1, float b2, float eps,
                                                       float d) {
  if (ctrl[LMN_OPTIM_SKIP] != 0u) return;
  const float inv_scale = __uint_as_float(ctrl[LMN_OPTIM_INV_SCALE]), coef = __uint_as_float(ctrl[LMN_OPTIM_COEF]);
  const float inv_bc1 = __uint_as_float(ctrl[LMN_OPTIM_INV_BC1]), inv_sqrt_bc2 = __uint_as_float(ctrl[LMN_OPTIM_INV_SQRT_BC2]);
  const unsigned frozen = optim_frozen_mask(table, n_groups);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned k = qgroup[i] & (LMN_OPTIM_MAX_GROUPS - 1);
    if ((frozen >> k) & 1u) continue;
    const float lr = table[4 * k], wd = table[4 * k + 1];
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i], mm = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
    const f32x4 gs = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 ee;
    if (EMA) ee = reinterpret_cast<f32x4*>(ema)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gu = gs[j] * inv_scale;
      const float ge = gu * coef;
      float x = pp[j] * (1.f - lr * wd);
      mm[j] = b1 * mm[j] + (1.f - b1) * ge;
      vv[j] = b2 * vv[j] + (1.f - b2) * ge * ge;
      const float denom = sqrtf(vv[j]) * inv_sqrt_bc2 + eps;
      pp[j] = x - (lr * inv_bc1) * (mm[j] / denom);
      if (EMA) ee[j] = d * ee[j] + (1.f - d) * pp[j];
    }
    reinterpret_cast<f32x4*>(p)[i] = pp;
    reinterpret_cast<f32x4*>(m)[i] = mm;
    reinterpret_cast<f32x4*>(v)[i] = vv;
    if (EMA) reinterpret_cast<f32x4*>(ema)[i] = ee;
  }
}

inline int optim_blocks(int64_t n) { return loss_grid(n / 4, LMN_OPTIM_GRID_CAP); }

// the argument checks shared by the two entries
int optim_check(const char* what, int64_t n, const lmn_optim_param_t* P) {
  LMN_REQUIRE(n > 0 && n % 4 == 0, "%s: n=%lld is not a positive multiple of 4", what, (long long)n);
  LMN_REQUIRE(P->n_groups >= 1 && P->n_groups <= LMN_OPTIM_MAX_GROUPS, "%s: n_groups=%d not in [1, %d]", what, P->n_groups,
              LMN_OPTIM_MAX_GROUPS);
  LMN_REQUIRE(P->beta1 >= 0.0 && P->beta1 < 1.0 && P->beta2 >= 0.0 && P->beta2 < 1.0, "%s: betas (%g, %g) outside [0, 1)", what, P->beta1,
              P->beta2);
  LMN_REQUIRE(P->eps > 0.f, "%s: eps=%g is not positive", what, (double)P->eps);
  LMN_REQUIRE(!(P->ema_decay > 1.f), "%s: ema_decay=%g above 1", what, (double)P->ema_decay);
  LMN_REQUIRE(!(P->max_norm > 0.f || (P->flags & LMN_OPTIM_SKIP_NONFINITE)) || (P->flags & LMN_OPTIM_NORM),
              "%s: clipping and the skip on non-finite values need LMN_OPTIM_NORM", what);
  return 0;
}

}  // namespace

extern "C" {

int lmn_sizeof_optim_param(void) { return (int)sizeof(lmn_optim_param_t); }

int64_t lmn_optim_workspace(int64_t n) {
  if (n <= 0) return 0;
  return 2 * (int64_t)optim_blocks(n) + LMN_OPTIM_CTRL_WORDS + LMN_OPTIM_GROUP_WORDS;
}

int lmn_optim_prepare(const float* g, int64_t n, const uint8_t* qgroup, const lmn_optim_param_t* param, float* ws,
                      const float* grad_scale, const float* found_inf, lmn_stream_t stream) {
  LMN_REQUIRE(g && qgroup && param && ws, "optim_prepare: null pointer");
  if (int rc = optim_check("optim_prepare", n, param)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int G = optim_blocks(n);
  float* partial = ws;
  uint32_t* counts = reinterpret_cast<uint32_t*>(ws) + G;
  uint32_t* ctrl = reinterpret_cast<uint32_t*>(ws) + 2 * G;
  const float* table = ws + 2 * G + LMN_OPTIM_CTRL_WORDS;
  const bool norm = (param->flags & LMN_OPTIM_NORM) != 0;
  if (norm) LMN_LAUNCH(optim_sumsq_kernel, dim3(G), dim3(256), 0, st, g, n / 4, qgroup, table, param->n_groups, partial, counts);
  const FinishK K{param->beta1, param->beta2, param->max_norm, param->flags};
  LMN_LAUNCH(optim_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, (const uint32_t*)counts, norm ? G : 0, K, grad_scale,
             found_inf, ctrl);
  return lmn_launch_status("optim_prepare");
}

int lmn_adamw_step_ex(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const uint8_t* qgroup,
                      const lmn_optim_param_t* param, const float* ws, lmn_stream_t stream) {
  LMN_REQUIRE(p && g && m && v && qgroup && param && ws, "adamw_step_ex: null pointer");
  if (int rc = optim_check("adamw_step_ex", n, param)) return rc;
  LMN_REQUIRE(!(param->ema_decay >= 0.f) || ema, "adamw_step_ex: ema_decay=%g without an EMA buffer", (double)param->ema_decay);
  hipStream_t st = (hipStream_t)stream;
  const int G = optim_blocks(n);
  const uint32_t* ctrl = reinterpret_cast<const uint32_t*>(ws) + 2 * G;
  const float* table = ws + 2 * G + LMN_OPTIM_CTRL_WORDS;
  const int grid = loss_grid(n / 4, 4096);      // (the grid of lmn_adamw_step)
  const float b1 = (float)param->beta1, b2 = (float)param->beta2;
  if (param->ema_decay >= 0.f)
    LMN_LAUNCH((adamw_ex_kernel<true>), dim3(grid), dim3(256), 0, st, p, g, m, v, ema, n / 4, qgroup, ctrl, table, param->n_groups, b1, b2,
               param->eps, param->ema_decay);
  else
    LMN_LAUNCH((adamw_ex_kernel<false>), dim3(grid), dim3(256), 0, st, p, g, m, v, (float*)nullptr, n / 4, qgroup, ctrl, table, param->n_groups,
               b1, b2, param->eps, 0.f);
  return lmn_launch_status("adamw_step_ex");
}

}  // extern "C"

// Sigmoid heads (include/lmnet_sigmoid.h): a per-class binary loss -- BCE + Dice + focal over independent logit planes -- and
// thresholded tp / fp / fn / tn statistics.  The classes are independent, so nothing is staged in LDS: blockIdx.y is the (b, c)
// plane, blockIdx.x strides over THAT plane only, and a block's partial sums belong to one class.  A lane takes four consecutive
// elements (one 16-byte load of logits, one 4-byte or two 16-byte loads of targets) when HW % 4 == 0 and the bases are aligned, one
// element otherwise; both forms handle the tail of a plane.
//   sums (4-byte words, [k][C]): [0] N_c = valid elements (uint32)   [1] Y_c = sum_valid t (uint32)   [2] I_c = sum_valid p t
//                                [3] Z_c = sum_valid p^2   [4] sum_valid pw_c t softplus(-z) + (1 - t) softplus(z)   [5] focal sum
//   coef (floats, [k][C]):       [0] a_c  [1] b_c  with dL_dice/dp = a_c t + b_c p   [2] bce_scale w_bce[c] / N   [3] focal_scale / N_c
#include "loss_common.h"
#include "../../include/lmnet_sigmoid.h"

static_assert(LMN_SIG_T_U8 == LOSS_LABELS_U8 && LMN_SIG_T_I64 == LOSS_LABELS_I64, "loss_common.h reads the target kinds of lmnet_sigmoid.h");

namespace {

constexpr int SG_NSUM = 6, SG_NFLT = 4;   // words per class in sums; the float ones among them (slot copies in deterministic mode)

template <int KIND, bool VEC, bool FOCAL>
__global__ __launch_bounds__(256) void sigloss_sums_kernel(const float* __restrict__ logits, const void* __restrict__ target,
                                                           const float* __restrict__ pos_weight, int C, int64_t hw, FocalK fk,
                                                           uint32_t* __restrict__ sums, float* __restrict__ slots) {
  constexpr int E = VEC ? 4 : 1;
  const int plane = blockIdx.y, c = plane % C;
  const float* lg = logits + (int64_t)plane * hw;
  const void* tg = (const uint8_t*)target + (int64_t)plane * hw * (KIND == LMN_SIG_T_I64 ? 8 : 1);
  const float pw = pos_weight[c];
  unsigned n_v = 0, n_y = 0;
  float a_i = 0.f, a_z = 0.f, a_b = 0.f, a_f = 0.f;
  const int64_t items = hw / E;                       // (VEC: hw % 4 == 0)
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < items; q += (int64_t)gridDim.x * 256) {
    float z[E];
    int t[E];
    loss_load_z<E>(lg, q * E, z);
    loss_load_t<KIND, E>(tg, q * E, t);
#pragma unroll
    for (int j = 0; j < E; ++j) {
      if (t[j] > 1) continue;                         // void: adds to no sum
      const SigPoint s = sig_point(z[j]);
      const bool on = t[j] == 1;
      n_v += 1u;
      n_y += on ? 1u : 0u;
      a_i += on ? s.p : 0.f;
      a_z += s.p * s.p;
      a_b += on ? pw * s.sp_neg : s.sp_pos;
      if (FOCAL) a_f += focal_value(s, on, fk);
    }
  }
  __shared__ float red_f[4][SG_NFLT];
  __shared__ unsigned red_u[4][2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  n_v = loss_wave_sum(n_v);
  n_y = loss_wave_sum(n_y);
  a_i = loss_wave_sum(a_i);
  a_z = loss_wave_sum(a_z);
  a_b = loss_wave_sum(a_b);
  if (FOCAL) a_f = loss_wave_sum(a_f);
  if (lane == 0) {
    red_u[wv][0] = n_v; red_u[wv][1] = n_y;
    red_f[wv][0] = a_i; red_f[wv][1] = a_z; red_f[wv][2] = a_b; red_f[wv][3] = a_f;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < 2) {                                        // the counts: integer atomics, exact and order-independent in either mode
    const unsigned v = red_u[0][k] + red_u[1][k] + red_u[2][k] + red_u[3][k];
    if (v) atomicAdd(sums + k * C + c, v);
  } else if (k < SG_NSUM && (FOCAL || k < SG_NSUM - 1)) {
    const int f = k - 2;
    const float v = red_f[0][f] + red_f[1][f] + red_f[2][f] + red_f[3][f];
    if (slots) {                                      // deterministic mode: slot (image, block) of the copies [B * gridDim.x][4][C]
      const int64_t s = (int64_t)(plane / C) * gridDim.x + blockIdx.x;
      slots[(s * SG_NFLT + f) * C + c] = v;
    } else {
      atomicAdd(reinterpret_cast<float*>(sums) + k * C + c, v);
    }
  }
}

struct SgFinishK { float smooth, bce_scale, dice_scale, focal_scale; };

// loss4 = total, bce, dice, focal.  N = 0: bce is 0 and so is its coefficient; N_c = 0: class c adds nothing to the focal term.
__global__ void sigloss_finish_kernel(const uint32_t* __restrict__ sums, const float* __restrict__ w_bce, const float* __restrict__ w_dice,
                                      int C, SgFinishK k, float* __restrict__ loss4, float* __restrict__ coef) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float* fs = reinterpret_cast<const float*>(sums);
  double n_all = 0.0;
  for (int c = 0; c < C; ++c) n_all += (double)sums[c];
  const float inv_n = n_all > 0.0 ? (float)(1.0 / n_all) : 0.f;
  float bce = 0.f, dice = 0.f, focal = 0.f;
  for (int c = 0; c < C; ++c) {
    const float Nc = (float)sums[c], Y = (float)sums[C + c], I = fs[2 * C + c], Z = fs[3 * C + c];
    const float num = 2.f * I + k.smooth, den = Z + Y + k.smooth;
    const bool ok = den > 0.f && k.dice_scale > 0.f;    // (smooth = 0 and no valid element: the class contributes nothing)
    dice += ok ? w_dice[c] * (1.f - num / den) / C : 0.f;
    coef[c] = ok ? k.dice_scale * (w_dice[c] / C * (-2.f / den)) : 0.f;
    coef[C + c] = ok ? k.dice_scale * (w_dice[c] / C * (2.f * num / (den * den))) : 0.f;
    const bool b_ok = k.bce_scale > 0.f && n_all > 0.0;
    bce += b_ok ? w_bce[c] * fs[4 * C + c] : 0.f;
    coef[2 * C + c] = b_ok ? k.bce_scale * w_bce[c] * inv_n : 0.f;
    const bool f_ok = k.focal_scale > 0.f && Nc > 0.f;
    focal += f_ok ? fs[5 * C + c] / Nc : 0.f;
    coef[3 * C + c] = f_ok ? k.focal_scale / Nc : 0.f;
  }
  bce = k.bce_scale > 0.f ? k.bce_scale * (bce * inv_n) : 0.f;
  dice = k.dice_scale > 0.f ? k.dice_scale * dice : 0.f;
  focal = k.focal_scale > 0.f ? k.focal_scale * focal : 0.f;
  loss4[0] = bce + dice + focal;
  loss4[1] = bce;
  loss4[2] = dice;
  loss4[3] = focal;
}

template <int KIND, bool VEC, bool FOCAL>
__global__ __launch_bounds__(256) void sigloss_bwd_kernel(const float* __restrict__ logits, const void* __restrict__ target,
                                                          const float* __restrict__ pos_weight, const float* __restrict__ coef,
                                                          const float* __restrict__ gscale, int C, int64_t hw, FocalK fk,
                                                          float* __restrict__ dlogits) {
  constexpr int E = VEC ? 4 : 1;
  const int plane = blockIdx.y, c = plane % C;
  const float* lg = logits + (int64_t)plane * hw;
  float* dl = dlogits + (int64_t)plane * hw;
  const void* tg = (const uint8_t*)target + (int64_t)plane * hw * (KIND == LMN_SIG_T_I64 ? 8 : 1);
  const float pw = pos_weight[c], a = coef[c], bq = coef[C + c], k_b = coef[2 * C + c], k_f = coef[3 * C + c];
  const float gs = gscale ? gscale[0] : 1.f;
  const int64_t items = hw / E;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < items; q += (int64_t)gridDim.x * 256) {
    float z[E], d[E];
    int t[E];
    loss_load_z<E>(lg, q * E, z);
    loss_load_t<KIND, E>(tg, q * E, t);
#pragma unroll
    for (int j = 0; j < E; ++j) {
      d[j] = 0.f;                                     // void: +0
      if (t[j] > 1) continue;
      const SigPoint s = sig_point(z[j]);
      const bool on = t[j] == 1;
      float v = ((on ? a : 0.f) + bq * s.p) * (s.p * s.omp);         // dice: dL/dp through p (1 - p)
      v += k_b * (on ? -pw * s.omp : s.p);                            // bce: -pw t (1 - p) + (1 - t) p
      if (FOCAL) v += k_f * focal_grad(s, on, fk);
      d[j] = gs * v;
    }
    loss_store<E>(dl, q * E, d);
  }
}

// tp / fp / fn / tn per (image, class) plane and the thresholded uint8 maps.  Every trip is taken by whole waves (the guard is part
// of the ballots), so lane 0 of a wave holds the wave's four counts: valid, predicted (among valid), labelled, true positive.
template <int KIND, bool VEC, bool HAS_T>
__global__ __launch_bounds__(256) void sigmoid_stats_kernel(const float* __restrict__ logits, const void* __restrict__ target, float thr,
                                                            int64_t hw, unsigned long long* __restrict__ stats,
                                                            uint8_t* __restrict__ labels_out) {
  constexpr int E = VEC ? 4 : 1;
  const int plane = blockIdx.y;
  const float* lg = logits + (int64_t)plane * hw;
  const void* tg = HAS_T ? (const void*)((const uint8_t*)target + (int64_t)plane * hw * (KIND == LMN_SIG_T_I64 ? 8 : 1)) : nullptr;
  uint8_t* lo = labels_out ? labels_out + (int64_t)plane * hw : nullptr;
  int n_v = 0, n_p = 0, n_l = 0, n_tp = 0;
  const int64_t items = hw / E;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < items; base += (int64_t)gridDim.x * 256) {
    const int64_t q = base + threadIdx.x;
    const bool in = q < items;
    float z[E];
    int t[E];
#pragma unroll
    for (int j = 0; j < E; ++j) { z[j] = 0.f; t[j] = 2; }
    if (in) {
      loss_load_z<E>(lg, q * E, z);
      if constexpr (HAS_T) loss_load_t<KIND, E>(tg, q * E, t);
    }
    uint32_t packed = 0;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const bool pred = z[j] >= thr;                  // fp32 compare (NaN: off)
      packed |= (pred ? 1u : 0u) << (8 * j);
      if constexpr (HAS_T) {
        const bool valid = in && t[j] <= 1, lab = in && t[j] == 1;
        n_v += __popcll(__ballot(valid));
        n_p += __popcll(__ballot(valid && pred));
        n_l += __popcll(__ballot(lab));
        n_tp += __popcll(__ballot(lab && pred));
      }
    }
    if (lo && in) {
      if constexpr (VEC) *reinterpret_cast<uint32_t*>(lo + q * 4) = packed;
      else lo[q] = (uint8_t)packed;
    }
  }
  if constexpr (HAS_T) {
    __shared__ int s_cnt[4][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { s_cnt[wv][0] = n_v; s_cnt[wv][1] = n_p; s_cnt[wv][2] = n_l; s_cnt[wv][3] = n_tp; }
    __syncthreads();
    if (threadIdx.x < 4) {                            // one integer atomic per block and counter
      int tot[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) tot[i] = s_cnt[0][i] + s_cnt[1][i] + s_cnt[2][i] + s_cnt[3][i];
      const int nv = tot[0], np = tot[1], nl = tot[2], tp = tot[3];
      const int out = threadIdx.x == 0 ? tp : threadIdx.x == 1 ? np - tp : threadIdx.x == 2 ? nl - tp : nv - np - nl + tp;
      if (out) atomicAdd(stats + (int64_t)plane * 4 + threadIdx.x, (unsigned long long)out);
    }
  }
}

int sg_check_sizes(const char* what, int B, int C, int64_t HW) {
  LMN_REQUIRE(C >= 1 && C <= LOSS_MAXC, "%s: C=%d not in [1, %d]", what, C, LOSS_MAXC);
  LMN_REQUIRE(B > 0 && HW > 0 && HW < (1LL << 31) && (int64_t)B * C <= 65535 && (int64_t)B * HW < (1LL << 31),
              "%s: B=%d, C=%d, HW=%lld (need B >= 1, 1 <= HW < 2^31, B * C <= 65535, B * HW < 2^31)", what, B, C, (long long)HW);
  return 0;
}

int sg_check(const char* what, int B, int C, int64_t HW, const lmn_sig_param_t* p) {
  if (int rc = sg_check_sizes(what, B, C, HW)) return rc;
  if (int rc = loss_check_terms(what, "bce", p->smooth, p->bce_scale, p->dice_scale, p->focal_scale, p->focal_gamma, p->focal_alpha))
    return rc;
  LMN_REQUIRE(p->target_kind == LMN_SIG_T_U8 || p->target_kind == LMN_SIG_T_I64, "%s: unknown target_kind %d", what, (int)p->target_kind);
  return 0;
}

}  // namespace

extern "C" {

int lmn_sizeof_sig_param(void) { return (int)sizeof(lmn_sig_param_t); }

int lmn_sigloss_fwd(const float* logits, const void* target, const float* w_bce, const float* pos_weight, const float* w_dice, int B,
                    int C, int64_t HW, const lmn_sig_param_t* param, void* sums, float* coef, float* loss4, lmn_stream_t stream) {
  LMN_REQUIRE(logits && target && w_bce && pos_weight && w_dice && param && sums && coef && loss4, "sigloss_fwd: null pointer");
  if (int rc = sg_check("sigloss_fwd", B, C, HW, param)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool focal = param->focal_scale > 0.f;
  const int kind = param->target_kind;
  const bool vec = HW % 4 == 0 && lmn_aligned(logits, 16) && lmn_aligned(target, kind == LMN_SIG_T_I64 ? 16 : 4);
  const int planes = B * C;
  const int gx = loss_grid_per(vec ? HW / 4 : HW, 2048, planes);
  const FocalK fk{param->focal_gamma, param->focal_alpha};
  const SgFinishK fin{param->smooth, param->bce_scale, param->dice_scale, param->focal_scale};
  LMN_LAUNCH(loss_zero_kernel, dim3(1), dim3(256), 0, st, (uint32_t*)sums, (int64_t)LMN_SIG_SUMS_WORDS(C));
  float* slots = nullptr;
  if (g_lmn_det) {
    lmn_det_begin(st);
    slots = lmn_det_slots(st, (size_t)B * gx * SG_NFLT * C);
    LMN_REQUIRE(slots, "sigloss_fwd: deterministic mode: no scratch");
  }
  LOSS_SWITCH_KIND(kind, LOSS_SWITCH_BOOL(VEC, vec, LOSS_SWITCH_BOOL(FOCAL, focal,
    LMN_LAUNCH((sigloss_sums_kernel<KIND, VEC, FOCAL>), dim3(gx, planes), dim3(256), 0, st, logits, target, pos_weight, C, HW, fk, (uint32_t*)sums, slots))));
  if (slots) lmn_det_sum(st, slots, B * gx, (int64_t)SG_NFLT * C, (float*)sums + 2 * C);
  LMN_LAUNCH(sigloss_finish_kernel, dim3(1), dim3(64), 0, st, (const uint32_t*)sums, w_bce, w_dice, C, fin, loss4, coef);
  return lmn_launch_status("sigloss_fwd");
}

int lmn_sigloss_bwd(const float* logits, const void* target, const float* pos_weight, const float* coef, const float* gscale, int B,
                    int C, int64_t HW, const lmn_sig_param_t* param, float* dlogits, lmn_stream_t stream) {
  LMN_REQUIRE(logits && target && pos_weight && coef && param && dlogits, "sigloss_bwd: null pointer");
  if (int rc = sg_check("sigloss_bwd", B, C, HW, param)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool focal = param->focal_scale > 0.f;
  const int kind = param->target_kind;
  const bool vec = HW % 4 == 0 && lmn_aligned(logits, 16) && lmn_aligned(dlogits, 16) && lmn_aligned(target, kind == LMN_SIG_T_I64 ? 16 : 4);
  const int planes = B * C;
  const int gx = loss_grid_per(vec ? HW / 4 : HW, 4096, planes);
  const FocalK fk{param->focal_gamma, param->focal_alpha};
  LOSS_SWITCH_KIND(kind, LOSS_SWITCH_BOOL(VEC, vec, LOSS_SWITCH_BOOL(FOCAL, focal,
    LMN_LAUNCH((sigloss_bwd_kernel<KIND, VEC, FOCAL>), dim3(gx, planes), dim3(256), 0, st, logits, target, pos_weight, coef, gscale, C, HW, fk, dlogits))));
  return lmn_launch_status("sigloss_bwd");
}

int lmn_sigmoid_stats(const float* logits, const void* target, int target_kind, float logit_threshold, int B, int C, int64_t HW,
                      int64_t* stats, uint8_t* labels_out, lmn_stream_t stream) {
  LMN_REQUIRE(logits, "sigmoid_stats: null pointer (logits)");
  LMN_REQUIRE(stats || labels_out, "sigmoid_stats: null pointer: at least one of stats and labels_out must be given");
  LMN_REQUIRE(!stats || target, "sigmoid_stats: null pointer: stats needs a target");
  LMN_REQUIRE(target_kind == LMN_SIG_T_U8 || target_kind == LMN_SIG_T_I64, "sigmoid_stats: unknown target_kind %d", target_kind);
  LMN_REQUIRE(logit_threshold == logit_threshold, "sigmoid_stats: logit_threshold is NaN");
  if (int rc = sg_check_sizes("sigmoid_stats", B, C, HW)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool has_t = stats != nullptr;                // (a target without stats is not read)
  const bool vec = HW % 4 == 0 && lmn_aligned(logits, 16) && (!has_t || lmn_aligned(target, target_kind == LMN_SIG_T_I64 ? 16 : 4)) &&
                   (!labels_out || lmn_aligned(labels_out, 4));
  const int planes = B * C;
  const int gx = loss_grid_per(vec ? HW / 4 : HW, 1024, planes);
  unsigned long long* so = (unsigned long long*)stats;
  if (has_t) {
    const int64_t words = (int64_t)planes * 8;
    LMN_LAUNCH(loss_zero_kernel, dim3(loss_grid(words, 64)), dim3(256), 0, st, (uint32_t*)stats, words);
    LOSS_SWITCH_KIND(target_kind, LOSS_SWITCH_BOOL(VEC, vec,
      LMN_LAUNCH((sigmoid_stats_kernel<KIND, VEC, true>), dim3(gx, planes), dim3(256), 0, st, logits, target, logit_threshold, HW, so, labels_out)));
  } else {
    LOSS_SWITCH_KIND(LOSS_LABELS_U8, LOSS_SWITCH_BOOL(VEC, vec,
      LMN_LAUNCH((sigmoid_stats_kernel<KIND, VEC, false>), dim3(gx, planes), dim3(256), 0, st, logits, target, logit_threshold, HW, so, labels_out)));
  }
  return lmn_launch_status("sigmoid_stats");
}

}  // extern "C"

// What the two loss sources, loss_ex.hip (softmax heads) and sigmoid.hip (sigmoid heads), compute the same way: the wave sum of their
// reductions, the sigmoid focal term and its derivative, the zero-fill of a reduction's start, the capped grid and the checks of the
// scalar parameters both param structs carry.  Everything else -- the sums and dlogits kernels, the two finish kernels (which treat
// dice_scale = 0 and the pixel counts differently on purpose) -- stays in its own file.  metrics.hip takes the zero fill and the grid.
// The three criteria, distmap.hip, lovasz.hip and region.hip, take the wave sum, the sigmoid point, the zero fill and the grid too,
// and share the front end of their entries: the class list of a
// class_mask (LossCls, loss_classes), the run-time-kind reader of a label (loss_label; region.hip's clamped, vectorised readers are its
// own) and the four argument rules on C, the head, class_mask and the label kind (loss_check_head).  Each keeps its own B, size and
// product rules, its kernels and the way it gets its deterministic slots.
#pragma once
#include "common.h"

namespace {

// what the headers of the three criteria name LMN_*_LABELS_U8 / _I64 and LMN_*_SOFTMAX / _SIGMOID: every source static_asserts it
constexpr int LOSS_LABELS_U8 = 0, LOSS_LABELS_I64 = 1, LOSS_SOFTMAX = 0, LOSS_SIGMOID = 1;

// the scored classes in ascending order; kernels take it by value
struct LossCls { uint8_t id[64]; };
// fills cls from a class_mask; the number of classes
inline int loss_classes(uint64_t class_mask, LossCls* cls) {
  int nk = 0;
  memset(cls, 0, sizeof(*cls));
  for (int c = 0; c < 64; ++c)
    if ((class_mask >> c) & 1) cls->id[nk++] = (uint8_t)c;
  return nk;
}

// a label or target element as int64 (a uint8 value is never negative); kind: LOSS_LABELS_*
__device__ __forceinline__ int64_t loss_label(const void* __restrict__ p, int kind, int64_t i) {
  return kind == LOSS_LABELS_I64 ? ((const int64_t*)p)[i] : (int64_t)((const uint8_t*)p)[i];
}

// the rules on the class count, the head, class_mask and the label kind that the entries of the three criteria share
inline int loss_check_head(const char* what, int C, bool softmax, uint64_t class_mask, int label_kind) {
  LMN_REQUIRE(C >= 1 && C <= 64, "%s: C=%d not in [1, 64]", what, C);
  LMN_REQUIRE(C >= 2 || !softmax, "%s: C=1 needs a sigmoid head (softmax over one class is constant)", what);
  const uint64_t all = C == 64 ? ~0ull : ((1ull << C) - 1);
  LMN_REQUIRE(class_mask != 0 && !(class_mask & ~all), "%s: class_mask is empty or names a class >= C=%d", what, C);
  LMN_REQUIRE(label_kind == LOSS_LABELS_U8 || label_kind == LOSS_LABELS_I64, "%s: unknown label kind %d", what, label_kind);
  return 0;
}

// 64-lane sum, butterfly m = 1 ... 32.  (lmn_wave_sum of common.h runs m = 32 ... 1 and rounds differently: the deterministic-mode
// results of the losses are pinned to this order.)
__device__ __forceinline__ float loss_wave_sum(float v) {
#pragma unroll
  for (int m = 1; m <= 32; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ unsigned loss_wave_sum(unsigned v) {
#pragma unroll
  for (int m = 1; m <= 32; m <<= 1) v += (unsigned)__shfl_xor((int)v, m, 64);
  return v;
}

// One softplus serves the sigmoid, both binary cross entropies and the focal factor: with e = exp(-|z|), l = log1p(e):
// softplus(z) = max(z, 0) + l = -log(1 - p),  softplus(-z) = max(-z, 0) + l = -log p,  p = sigmoid(z) = 1 / (1 + e) or e / (1 + e).
// No cancellation at large |z|, no overflow.
struct SigPoint { float p, omp, sp_pos, sp_neg; };   // p, 1 - p, softplus(z), softplus(-z)
__device__ __forceinline__ SigPoint sig_point(float z) {
  const float e = expf(-fabsf(z));
  const float l = log1pf(e);
  const float r = 1.f / (1.f + e);
  SigPoint s;
  s.p = z >= 0.f ? r : e * r;
  s.omp = z >= 0.f ? e * r : r;
  s.sp_pos = fmaxf(z, 0.f) + l;
  s.sp_neg = fmaxf(-z, 0.f) + l;
  return s;
}

struct FocalK { float gamma, alpha; };   // alpha < 0: no alpha weighting

// One class of the sigmoid focal loss at the point of logit z with target t (true: the element belongs to the class).  With q_t = p
// for t, 1 - p otherwise:  a_t (1 - q_t)^gamma bce,  bce = -log q_t,  log(1 - q_t) = -(the other softplus).  gamma = 0: exp(0) = 1
// exactly.
__device__ __forceinline__ float focal_value(const SigPoint& s, bool t, FocalK k) {
  const float bce = t ? s.sp_neg : s.sp_pos, l1 = -(t ? s.sp_pos : s.sp_neg);
  const float at = k.alpha < 0.f ? 1.f : (t ? k.alpha : 1.f - k.alpha);
  return at * expf(k.gamma * l1) * bce;
}
// d focal_value / dz = (2t - 1) a_t (1 - q_t)^gamma [-gamma q_t bce - (1 - q_t)]
__device__ __forceinline__ float focal_grad(const SigPoint& s, bool t, FocalK k) {
  const float bce = t ? s.sp_neg : s.sp_pos, l1 = -(t ? s.sp_pos : s.sp_neg);
  const float qt = t ? s.p : s.omp, omq = t ? s.omp : s.p;
  const float at = k.alpha < 0.f ? 1.f : (t ? k.alpha : 1.f - k.alpha);
  const float ds = at * expf(k.gamma * l1) * (-k.gamma * qt * bce - omq);
  return t ? ds : -ds;
}

// the zeroed start of a reduction (words of 4 bytes)
__global__ void loss_zero_kernel(uint32_t* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0u;
}

// blocks of 256 lanes for `work_items`, at least 1 and at most `cap`
inline int loss_grid(int64_t work_items, int64_t cap) {
  int64_t g = (work_items + 255) / 256;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// the checks of the scalar parameters lmn_loss_param_t and lmn_sig_param_t share; `first`: the name of the first term (ce / bce)
inline int loss_check_terms(const char* what, const char* first, float smooth, float first_scale, float dice_scale, float focal_scale,
                            float focal_gamma, float focal_alpha) {
  LMN_REQUIRE(smooth >= 0.f, "%s: smooth=%g is negative", what, (double)smooth);
  LMN_REQUIRE(first_scale >= 0.f && dice_scale >= 0.f && focal_scale >= 0.f, "%s: negative scale (%s %g, dice %g, focal %g)", what, first,
              (double)first_scale, (double)dice_scale, (double)focal_scale);
  LMN_REQUIRE(focal_gamma >= 0.f, "%s: focal_gamma=%g is negative", what, (double)focal_gamma);
  LMN_REQUIRE(focal_alpha <= 1.f, "%s: focal_alpha=%g above 1", what, (double)focal_alpha);
  return 0;
}

}  // namespace

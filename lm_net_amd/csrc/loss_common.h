// What the loss and criterion sources build their kernels and entries from, so that a new criterion copies none of it.
//   constants  LOSS_LABELS_* / LOSS_SOFTMAX / LOSS_SIGMOID (what every criterion header names its label kinds and heads),
//              LOSS_MAXC, LOSS_TILE_STRIDE
//   device     the readers of a plane (loss_load_t: targets as 0 / 1 / void, loss_load_z: logits or values, loss_store; four elements
//              per lane or one), loss_label (one label of a run-time kind), loss_softmax (a register column), loss_wave_sum (float,
//              unsigned, double: the butterfly the deterministic results are pinned to), sig_point / focal_value / focal_grad,
//              loss_zero_kernel
//   host       LossCls / loss_classes (the class list of a class_mask), loss_templated, loss_grid / loss_cap / loss_grid_per (the
//              capped grids), loss_finite, the argument rules loss_check_head, loss_check_extent and loss_check_terms, and the
//              compile-time dispatch LOSS_SWITCH_CT / _BOOL / _KIND
// Each source keeps its kernels, its finish pass, its B and product rules where they are worded differently, and the way it gets its
// deterministic slots.  metrics.hip, optim.hip, tiles.hip, curves.hip and slices.hip take the zero fill, the grids and the wave sum.
#pragma once
#include <type_traits>

#include "common.h"

namespace {

// what the headers of the criteria name LMN_*_LABELS_U8 / _I64 and LMN_*_SOFTMAX / _SIGMOID: every source static_asserts it
constexpr int LOSS_LABELS_U8 = 0, LOSS_LABELS_I64 = 1, LOSS_SOFTMAX = 0, LOSS_SIGMOID = 1;
constexpr int LOSS_MAXC = 64;          // the largest class count
constexpr int LOSS_TILE_STRIDE = 65;   // row stride of the staged tile of a general-C sums kernel (conflict-free row reads)
// the class counts whose kernels keep a pixel's logits in registers (LOSS_SWITCH_CT)
inline bool loss_templated(int C) { return C == 2 || C == 3 || C == 4 || C == 8; }

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

// E consecutive targets of a plane as 0, 1 or 2 (void: every value but 0 and 1); KIND: LOSS_LABELS_*
template <int KIND, int E>
__device__ __forceinline__ void loss_load_t(const void* __restrict__ plane, int64_t i, int (&t)[E]) {
  if constexpr (KIND == LOSS_LABELS_U8) {
    const uint8_t* p = (const uint8_t*)plane + i;
    if constexpr (E == 4) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t v = (w >> (8 * j)) & 255u;
        t[j] = v <= 1u ? (int)v : 2;
      }
    } else {
      const uint32_t v = p[0];
      t[0] = v <= 1u ? (int)v : 2;
    }
  } else {
    const int64_t* p = (const int64_t*)plane + i;
    if constexpr (E == 4) {
      const longlong2 a = *reinterpret_cast<const longlong2*>(p), b = *reinterpret_cast<const longlong2*>(p + 2);
      const int64_t v[4] = {a.x, a.y, b.x, b.y};
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] = (uint64_t)v[j] <= 1ull ? (int)v[j] : 2;
    } else {
      const int64_t v = p[0];
      t[0] = (uint64_t)v <= 1ull ? (int)v : 2;
    }
  }
}
// E consecutive elements of a plane of logits or values (fp32 or bf16): one 16- or 8-byte load for E = 4
template <int E, typename TT>
__device__ __forceinline__ void loss_load_z(const TT* __restrict__ plane, int64_t i, float (&z)[E]) {
  if constexpr (E == 4) {
    const f32x4 v = ld4(plane + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] = v[j];
  } else {
    z[0] = ld1(plane + i);
  }
}
template <int E>
__device__ __forceinline__ void loss_store(float* __restrict__ plane, int64_t i, const float (&d)[E]) {
  if constexpr (E == 4) st4(plane + i, f32x4{d[0], d[1], d[2], d[3]});
  else plane[i] = d[0];
}

// softmax of the C logits a lane holds in registers; lse = log sum_c exp z_c
template <int C>
__device__ __forceinline__ void loss_softmax(const float (&z)[C], float (&p)[C], float& lse) {
  float mx = -3.0e38f;
#pragma unroll
  for (int c = 0; c < C; ++c) mx = fmaxf(mx, z[c]);
  float den = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) { p[c] = __expf(z[c] - mx); den += p[c]; }
  const float r = 1.f / den;
  lse = mx + __logf(den);
#pragma unroll
  for (int c = 0; c < C; ++c) p[c] *= r;
}
template <int C>
__device__ __forceinline__ void loss_softmax(const float (&z)[C], float (&p)[C]) {
  float lse;
  loss_softmax<C>(z, p, lse);
}

// the rules on the class count, the head, class_mask and the label kind that the entries of the criteria share
inline int loss_check_head(const char* what, int C, bool softmax, uint64_t class_mask, int label_kind) {
  LMN_REQUIRE(C >= 1 && C <= 64, "%s: C=%d not in [1, 64]", what, C);
  LMN_REQUIRE(C >= 2 || !softmax, "%s: C=1 needs a sigmoid head (softmax over one class is constant)", what);
  const uint64_t all = C == 64 ? ~0ull : ((1ull << C) - 1);
  LMN_REQUIRE(class_mask != 0 && !(class_mask & ~all), "%s: class_mask is empty or names a class >= C=%d", what, C);
  LMN_REQUIRE(label_kind == LOSS_LABELS_U8 || label_kind == LOSS_LABELS_I64, "%s: unknown label kind %d", what, label_kind);
  return 0;
}
// the two size rules of logits [B, C, H, W]
inline int loss_check_extent(const char* what, int B, int C, int H, int W) {
  LMN_REQUIRE(H >= 1 && W >= 1, "%s: size %dx%d below 1", what, H, W);
  LMN_REQUIRE((int64_t)B * C * H * W < (1LL << 31), "%s: B * C * H * W = %lld not below 2^31", what, (long long)B * C * H * W);
  return 0;
}
// neither NaN nor an infinity
inline bool loss_finite(float x) { return x - x == 0.f; }

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
__device__ __forceinline__ double loss_wave_sum(double v) {
#pragma unroll
  for (int m = 1; m <= 32; m <<= 1) v += __shfl_xor(v, m, 64);
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
// the share of `cap` blocks that one of `groups` (images, planes) gets, at least 1: the whole grid stays near `cap` blocks
inline int64_t loss_cap(int64_t cap, int64_t groups) { return cap / groups > 0 ? cap / groups : 1; }
inline int loss_grid_per(int64_t work_items, int64_t cap, int64_t groups) { return loss_grid(work_items, loss_cap(cap, groups)); }

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

// Compile-time dispatch: each runs `...` once with a constant of the call.  They nest.
//   LOSS_SWITCH_CT    constexpr int CT = C for C in {2, 3, 4, 8}, 0 for every other class count.  `...` is the body of a generic
//                     lambda, so that `if constexpr (CT > 0)` instantiates the chosen branch alone (no return or break in it)
//   LOSS_SWITCH_BOOL  constexpr bool NAME = v
//   LOSS_SWITCH_KIND  constexpr int KIND = LOSS_LABELS_U8 or LOSS_LABELS_I64
#define LOSS_SWITCH_CT(C, ...)                                                                                   \
  do {                                                                                                           \
    auto _loss_ct = [&](auto _ct) { constexpr int CT = decltype(_ct)::value; __VA_ARGS__; };                     \
    switch (C) {                                                                                                 \
      case 2: _loss_ct(std::integral_constant<int, 2>{}); break;                                                 \
      case 3: _loss_ct(std::integral_constant<int, 3>{}); break;                                                 \
      case 4: _loss_ct(std::integral_constant<int, 4>{}); break;                                                 \
      case 8: _loss_ct(std::integral_constant<int, 8>{}); break;                                                 \
      default: _loss_ct(std::integral_constant<int, 0>{}); break;                                                \
    }                                                                                                            \
  } while (0)
#define LOSS_SWITCH_BOOL(NAME, v, ...)                     \
  do {                                                     \
    if (v) { constexpr bool NAME = true; __VA_ARGS__; }    \
    else { constexpr bool NAME = false; __VA_ARGS__; }     \
  } while (0)
#define LOSS_SWITCH_KIND(kind, ...)                                               \
  do {                                                                            \
    if ((kind) == LOSS_LABELS_I64) { constexpr int KIND = LOSS_LABELS_I64; __VA_ARGS__; } \
    else { constexpr int KIND = LOSS_LABELS_U8; __VA_ARGS__; }                    \
  } while (0)

}  // namespace

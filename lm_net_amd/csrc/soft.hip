// Soft targets (include/soft/lmnet_soft.h): cross entropy + Dice against a distribution per pixel, the distillation term against a
// teacher's logits, and the Mixup / CutMix batch mixer.  Same structure as region.hip: a sums pass that reads logits and target once,
// a one-block finish in fp64 that writes the terms and the backward coefficients, one pointwise dlogits pass.
//   softmax head: sf_softmax_{sums,bwd}_kernel<CT, READER, E>.  CT in {2, 3, 4, 8}: the pixel's C logits and C target values live in
//                 registers, 256 lanes;  CT = 0: any other C, one wave per block, every lane stages its pixel's values in an LDS column
//                 of its own ([C][64], so no barrier).  E = 4 (bf16 teacher only): a lane takes four consecutive pixels, the teacher
//                 comes as one 8-byte load per class (the templates load the student as 16 bytes).  blockIdx.y is the image.
//   sigmoid head: sf_sigmoid_{sums,bwd}_kernel<VEC, BF>: blockIdx.y the class, blockIdx.z the image; four elements per lane when
//                 HW % 4 == 0 and the bases are aligned, one otherwise.
//   sums   fp32 [1 + 3 C]: the ce / kd sum, then I_c, Z_c, Y_c      counts int32 [1]: N
//   slots  fp32 [blocks, ns], ns = 1 + 3 C (teacher readers: 1): deterministic mode, one per block of the sums pass
//   coef   fp32 [1 + 2 C]: the coefficient of the first term, then a_c, c_c of the Dice term
#include <type_traits>

#include "loss_common.h"
#include "../../include/soft/lmnet_soft.h"
static_assert(LMN_SOFT_LABELS_U8 == LOSS_LABELS_U8 && LMN_SOFT_LABELS_I64 == LOSS_LABELS_I64 && LMN_SOFT_SOFTMAX == LOSS_SOFTMAX &&
              LMN_SOFT_SIGMOID == LOSS_SIGMOID, "loss_common.h reads the label kinds and heads of lmnet_soft.h");

namespace {

constexpr int SF_MAXNS = 1 + 3 * LOSS_MAXC;

struct SfArgs {
  const float* logits;
  const void* target;   // q (PROBS) or teacher logits
  const void* ya;       // PAIR: first label map; teacher readers: the optional valid map
  const void* yb;
  const float* lam;
  const float* w_ce;
  int kind, C;
  int64_t hw;
  float T, eps;
};

// where a block of the sums pass adds its partial sums
struct SfOut {
  float* sums;
  int32_t* counts;
  float* slots;   // deterministic mode, else NULL
  int ns;
};

// The ONE log routine: lse of v / T over the C classes of a pixel (max-subtracted), then log softmax(v / T)_c = sf_logp(v_c, T, s).
// log q of the teacher and log p of the student both come from here; the division and the subtractions are compiled without contraction
// so that equal bits in give equal bits out wherever the routine is inlined.
struct SfLse { float mx, lden; };
__device__ __forceinline__ float sf_scaled(float v, float T) {
#pragma clang fp contract(off)
  return v / T;
}
__device__ __forceinline__ float sf_logp(float v, float T, SfLse s) {
#pragma clang fp contract(off)
  const float d = sf_scaled(v, T) - s.mx;
  return d - s.lden;
}

// The C logits and the C target values of the pixel a lane works on.
template <int CT, int READER, int E>
struct SfPix {
  static constexpr bool PAIR = READER == LMN_SOFT_PAIR, BF = READER == LMN_SOFT_TEACHER_BF16;
  static constexpr int NR = CT > 0 ? CT * E : 1, UNR = CT > 0 ? CT : 1;   // UNR: full unroll of a class loop of the templates
  float zr[NR];
  float tr[(CT > 0 && !PAIR) ? NR : 1];
  float* zs;         // CT == 0: the lane's LDS column of logits, stride 64
  float* ts;         // CT == 0: the same of the target (E == 4: uint2 words of four bf16)
  int la, lb, j;
  float lam, oml;
  __device__ __forceinline__ float z(int c) const {
    if constexpr (CT > 0) return zr[c * E + j];
    else return zs[c * 64];
  }
  __device__ __forceinline__ float t(int c) const {
    if constexpr (PAIR) return (c == la ? lam : 0.f) + (c == lb ? oml : 0.f);
    else if constexpr (CT > 0) return tr[c * E + j];
    else if constexpr (E == 4) {
      const uint2 r = reinterpret_cast<const uint2*>(ts)[c * 64];
      const uint32_t w = j < 2 ? r.x : r.y;
      return (j & 1) ? lmn_bf16_hi(w) : lmn_bf16_lo(w);
    } else return ts[c * 64];
  }
  // loads of item `it` of image b (E pixels from it * E); in: the item exists
  __device__ __forceinline__ void load(const SfArgs& a, int C, int b, int64_t it, bool in) {
    const int64_t img = (int64_t)b * C * a.hw, i0 = it * E;
    if constexpr (CT > 0) {
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        if constexpr (E == 4) {
          const f32x4 v = in ? ld4(a.logits + img + c * a.hw + i0) : f32x4{0.f, 0.f, 0.f, 0.f};
          const f32x4 u = in ? ld4((const lmn_bf16*)a.target + img + c * a.hw + i0) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int k = 0; k < 4; ++k) { zr[c * E + k] = v[k]; tr[c * E + k] = u[k]; }
        } else {
          zr[c] = in ? a.logits[img + c * a.hw + i0] : 0.f;
          if constexpr (!PAIR) {
            if constexpr (BF) tr[c] = in ? ld1((const lmn_bf16*)a.target + img + c * a.hw + i0) : 0.f;
            else tr[c] = in ? ((const float*)a.target)[img + c * a.hw + i0] : 0.f;
          }
        }
      }
    } else {
#pragma unroll 4
      for (int c = 0; c < C; ++c) {
        if constexpr (E == 4) {
          reinterpret_cast<uint2*>(ts)[c * 64] = in ? *reinterpret_cast<const uint2*>((const lmn_bf16*)a.target + img + c * a.hw + i0) : uint2{0u, 0u};
        } else {
          zs[c * 64] = in ? a.logits[img + c * a.hw + i0] : 0.f;
          if constexpr (!PAIR) {
            if constexpr (BF) ts[c * 64] = in ? ld1((const lmn_bf16*)a.target + img + c * a.hw + i0) : 0.f;
            else ts[c * 64] = in ? ((const float*)a.target)[img + c * a.hw + i0] : 0.f;
          }
        }
      }
    }
  }
  // pixel jj of the item becomes the current one; -> its validity
  __device__ __forceinline__ bool select(const SfArgs& a, int C, int b, int64_t it, bool in, int jj) {
    j = jj;
    const int64_t pix = (int64_t)b * a.hw + it * E + jj;
    if constexpr (CT == 0 && E == 4) {
      const int64_t at = (int64_t)b * C * a.hw + it * E + jj;
#pragma unroll 4
      for (int c = 0; c < C; ++c) zs[c * 64] = in ? a.logits[at + c * a.hw] : 0.f;
    }
    if (!in) return false;
    if constexpr (PAIR) {
      const int64_t va = loss_label(a.ya, a.kind, pix), vb = loss_label(a.yb, a.kind, pix);
      la = (int)va; lb = (int)vb;
      lam = a.lam[b];
      oml = 1.f - lam;
      return (uint64_t)va < (uint64_t)C && (uint64_t)vb < (uint64_t)C;
    } else if constexpr (READER == LMN_SOFT_PROBS) {
      bool ok = true;
#pragma unroll UNR
      for (int c = 0; c < (CT > 0 ? CT : C); ++c) {
        const float q = t(c);
        ok = ok && q >= 0.f && q < __builtin_inff();
      }
      return ok;
    } else {
      return !a.ya || (uint64_t)loss_label(a.ya, a.kind, pix) < (uint64_t)C;
    }
  }
  template <bool OF_TARGET>
  __device__ __forceinline__ SfLse lse(int C, float T) const {
    float mx = -3.0e38f;
#pragma unroll UNR
    for (int c = 0; c < (CT > 0 ? CT : C); ++c) mx = fmaxf(mx, sf_scaled(OF_TARGET ? t(c) : z(c), T));
    float den = 0.f;
#pragma unroll UNR
    for (int c = 0; c < (CT > 0 ? CT : C); ++c) den += expf(sf_logp(OF_TARGET ? t(c) : z(c), T, SfLse{mx, 0.f}));
    return SfLse{mx, logf(den)};
  }
};

// The per-class sums of a lane.  Templates: 1 + 3 C registers.  General C: every value is summed over the wave at once and lane c
// keeps class c's three sums (a fixed order: deterministic).
template <int CT>
struct SfAcc {
  float a[CT > 0 ? 1 + 3 * CT : 4];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int k = 0; k < (CT > 0 ? 1 + 3 * CT : 4); ++k) a[k] = 0.f;
  }
  __device__ __forceinline__ void first(float v) { a[0] += v; }
  __device__ __forceinline__ void cls(int c, float i, float zz, float yy) {
    if constexpr (CT > 0) { a[1 + 3 * c] += i; a[2 + 3 * c] += zz; a[3 + 3 * c] += yy; }
    else {
      const float si = loss_wave_sum(i), sz = loss_wave_sum(zz), sy = loss_wave_sum(yy);
      if ((int)(threadIdx.x & 63) == c) { a[1] += si; a[2] += sz; a[3] += sy; }
    }
  }
  // red[wave][ns]
  __device__ __forceinline__ void flush(float* red, int C, bool classes) {
    const int lane = threadIdx.x & 63;
    if constexpr (CT > 0) {
#pragma unroll
      for (int k = 0; k < 1 + 3 * CT; ++k) {
        if (k > 0 && !classes) break;
        const float v = loss_wave_sum(a[k]);
        if (lane == 0) red[k] = v;
      }
    } else {
      const float v = loss_wave_sum(a[0]);
      if (lane == 0) red[0] = v;
      if (classes && lane < C) { red[1 + 3 * lane] = a[1]; red[2 + 3 * lane] = a[2]; red[3 + 3 * lane] = a[3]; }
    }
  }
};

template <int CT, int READER, int E>
__global__ __launch_bounds__(CT > 0 ? 256 : 64) void sf_softmax_sums_kernel(SfArgs a, SfOut o) {
  constexpr int NT = CT > 0 ? 256 : 64, NW = NT / 64, UNR = CT > 0 ? CT : 1;
  constexpr bool TEACH = READER >= LMN_SOFT_TEACHER_F32;
  extern __shared__ float sf_lds[];                    // CT == 0: [C][64] logits, then the target's columns
  __shared__ float red[NW][SF_MAXNS];
  __shared__ unsigned red_n[NW];
  const int C = CT > 0 ? CT : a.C, b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  SfPix<CT, READER, E> px;
  px.zs = sf_lds + lane;
  px.ts = E == 4 ? sf_lds + C * 64 + 2 * lane : sf_lds + C * 64 + lane;
  SfAcc<CT> acc;
  acc.zero();
  unsigned n = 0;
  const float eps = a.eps, epc = a.eps / (float)C;
  const int64_t items = a.hw / E;                      // (E == 4: hw % 4 == 0)
  for (int64_t base = (int64_t)blockIdx.x * NT; base < items; base += (int64_t)gridDim.x * NT) {   // (wave-uniform: SfAcc shuffles)
    const int64_t it = base + threadIdx.x;
    const bool in = it < items;
    px.load(a, C, b, it, in);
#pragma unroll
    for (int jj = 0; jj < E; ++jj) {
      const bool valid = px.select(a, C, b, it, in, jj);
      n += valid ? 1u : 0u;
      const SfLse sz = px.template lse<false>(C, a.T);
      if constexpr (TEACH) {
        const SfLse st = px.template lse<true>(C, a.T);
        float kl = 0.f;
#pragma unroll UNR
        for (int c = 0; c < (CT > 0 ? CT : C); ++c) {
          const float lq = sf_logp(px.t(c), a.T, st), lp = sf_logp(px.z(c), a.T, sz), q = expf(lq);
          kl += q > 0.f ? q * (lq - lp) : 0.f;           // 0 * log 0 = 0
        }
        acc.first(valid ? kl : 0.f);
      } else {
        float ce = 0.f;
#pragma unroll UNR
        for (int c = 0; c < (CT > 0 ? CT : C); ++c) {
          const float lp = sf_logp(px.z(c), 1.f, sz), p = expf(lp), q = px.t(c), w = a.w_ce ? a.w_ce[c] : 1.f;
          ce -= w * ((1.f - eps) * q + epc) * lp;
          acc.cls(c, valid ? p * q : 0.f, valid ? p * p : 0.f, valid ? q * q : 0.f);
        }
        acc.first(valid ? ce : 0.f);
      }
    }
  }
  acc.flush(red[wv], C, !TEACH);
  n = loss_wave_sum(n);
  if (lane == 0) red_n[wv] = n;
  __syncthreads();
  for (int k = threadIdx.x; k < o.ns; k += NT) {
    float v = red[0][k];
#pragma unroll
    for (int w = 1; w < NW; ++w) v += red[w][k];
    if (o.slots) o.slots[((int64_t)b * gridDim.x + blockIdx.x) * o.ns + k] = v;
    else atomicAdd(o.sums + k, v);
  }
  if (threadIdx.x == NT - 1) {
    unsigned v = red_n[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) v += red_n[w];
    if (v) atomicAdd(o.counts, (int32_t)v);
  }
}

template <int CT, int READER, int E>
__global__ __launch_bounds__(CT > 0 ? 256 : 64) void sf_softmax_bwd_kernel(SfArgs a, const float* __restrict__ coef,
                                                                           const float* __restrict__ gscale, float* __restrict__ dlogits) {
  constexpr int NT = CT > 0 ? 256 : 64, UNR = CT > 0 ? CT : 1;
  constexpr bool TEACH = READER >= LMN_SOFT_TEACHER_F32;
  extern __shared__ float sf_lds[];
  __shared__ float s_a[LOSS_MAXC], s_c[LOSS_MAXC], s_w[LOSS_MAXC];
  const int C = CT > 0 ? CT : a.C, b = blockIdx.y, lane = threadIdx.x & 63;
  if (!TEACH && (int)threadIdx.x < C) {
    s_a[threadIdx.x] = coef[1 + 2 * threadIdx.x];
    s_c[threadIdx.x] = coef[2 + 2 * threadIdx.x];
    s_w[threadIdx.x] = a.w_ce ? a.w_ce[threadIdx.x] : 1.f;
  }
  __syncthreads();
  SfPix<CT, READER, E> px;
  px.zs = sf_lds + lane;
  px.ts = E == 4 ? sf_lds + C * 64 + 2 * lane : sf_lds + C * 64 + lane;
  const float gs = gscale ? gscale[0] : 1.f, c0 = coef[0];
  const float eps = a.eps, epc = a.eps / (float)C;
  float* dl = dlogits + (int64_t)b * C * a.hw;
  const int64_t items = a.hw / E;
  for (int64_t it = (int64_t)blockIdx.x * NT + threadIdx.x; it < items; it += (int64_t)gridDim.x * NT) {
    px.load(a, C, b, it, true);
    float out[CT > 0 ? CT * E : 1];
#pragma unroll
    for (int jj = 0; jj < E; ++jj) {
      const bool valid = px.select(a, C, b, it, true, jj);
      const int64_t i = it * E + jj;
      if (!valid) {                                      // void: +0 in every class
#pragma unroll UNR
        for (int c = 0; c < (CT > 0 ? CT : C); ++c) {
          if constexpr (CT > 0) out[c * E + jj] = 0.f;
          else dl[c * a.hw + i] = 0.f;
        }
        continue;
      }
      const SfLse sz = px.template lse<false>(C, a.T);
      if constexpr (TEACH) {
        const SfLse st = px.template lse<true>(C, a.T);
#pragma unroll UNR
        for (int c = 0; c < (CT > 0 ? CT : C); ++c) {
          const float q = expf(sf_logp(px.t(c), a.T, st)), p = expf(sf_logp(px.z(c), a.T, sz));
          const float g = gs * (c0 * (p - q));
          if constexpr (CT > 0) out[c * E + jj] = g;
          else dl[c * a.hw + i] = g;
        }
      } else {
        float S = 0.f, dp = 0.f;
#pragma unroll UNR
        for (int c = 0; c < (CT > 0 ? CT : C); ++c) {
          const float p = expf(sf_logp(px.z(c), 1.f, sz)), q = px.t(c);
          S += s_w[c] * ((1.f - eps) * q + epc);
          dp += (s_a[c] * q + s_c[c] * p) * p;
        }
#pragma unroll UNR
        for (int c = 0; c < (CT > 0 ? CT : C); ++c) {
          const float p = expf(sf_logp(px.z(c), 1.f, sz)), q = px.t(c);
          const float g = gs * (c0 * (p * S - s_w[c] * ((1.f - eps) * q + epc)) + p * (s_a[c] * q + s_c[c] * p - dp));
          if constexpr (CT > 0) out[c * E + jj] = g;
          else dl[c * a.hw + i] = g;
        }
      }
    }
    if constexpr (CT > 0) {
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        if constexpr (E == 4) st4(dl + c * a.hw + it * 4, f32x4{out[c * 4], out[c * 4 + 1], out[c * 4 + 2], out[c * 4 + 3]});
        else dl[c * a.hw + it] = out[c];
      }
    }
  }
}

// the Bernoulli divergence of one element and the two probabilities: q = sigmoid(zt / T), p = sigmoid(z / T), every log a softplus of
// the same sig_point
__device__ __forceinline__ float sf_sig_kl(float z, float zt, float T, float& p, float& q) {
  const SigPoint s = sig_point(sf_scaled(z, T)), t = sig_point(sf_scaled(zt, T));
  p = s.p; q = t.p;
  const float a = t.p > 0.f ? t.p * (s.sp_neg - t.sp_neg) : 0.f;        // q (log q - log p)
  const float c = t.omp > 0.f ? t.omp * (s.sp_pos - t.sp_pos) : 0.f;    // (1 - q) (log(1 - q) - log(1 - p))
  return a + c;
}

template <bool VEC, bool BF>
__global__ __launch_bounds__(256) void sf_sigmoid_sums_kernel(SfArgs a, SfOut o) {
  constexpr int E = VEC ? 4 : 1;
  typedef typename std::conditional<BF, lmn_bf16, float>::type TT;
  const int c = blockIdx.y, b = blockIdx.z;
  const int64_t plane = ((int64_t)b * a.C + c) * a.hw;
  const float* lg = a.logits + plane;
  const TT* tg = (const TT*)a.target + plane;
  unsigned n = 0;
  float kl = 0.f;
  const int64_t items = a.hw / E;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < items; q += (int64_t)gridDim.x * 256) {
    float z[E], zt[E];
    loss_load_z<E>(lg, q * E, z);
    loss_load_z<E>(tg, q * E, zt);
#pragma unroll
    for (int j = 0; j < E; ++j) {
      if (a.ya && (uint64_t)loss_label(a.ya, a.kind, plane + q * E + j) > 1ull) continue;   // void: adds to no sum
      float p, qq;
      kl += sf_sig_kl(z[j], zt[j], a.T, p, qq);
      n += 1u;
    }
  }
  __shared__ float red_f[4];
  __shared__ unsigned red_u[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  kl = loss_wave_sum(kl);
  n = loss_wave_sum(n);
  if (lane == 0) { red_f[wv] = kl; red_u[wv] = n; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float v = red_f[0] + red_f[1] + red_f[2] + red_f[3];
    if (o.slots) o.slots[((int64_t)b * a.C + c) * gridDim.x + blockIdx.x] = v;
    else atomicAdd(o.sums, v);
  } else if (threadIdx.x == 1) {
    const unsigned v = red_u[0] + red_u[1] + red_u[2] + red_u[3];
    if (v) atomicAdd(o.counts, (int32_t)v);
  }
}

template <bool VEC, bool BF>
__global__ __launch_bounds__(256) void sf_sigmoid_bwd_kernel(SfArgs a, const float* __restrict__ coef, const float* __restrict__ gscale,
                                                             float* __restrict__ dlogits) {
  constexpr int E = VEC ? 4 : 1;
  typedef typename std::conditional<BF, lmn_bf16, float>::type TT;
  const int c = blockIdx.y, b = blockIdx.z;
  const int64_t plane = ((int64_t)b * a.C + c) * a.hw;
  const float* lg = a.logits + plane;
  const TT* tg = (const TT*)a.target + plane;
  float* dl = dlogits + plane;
  const float gs = gscale ? gscale[0] : 1.f, c0 = coef[0];
  const int64_t items = a.hw / E;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < items; q += (int64_t)gridDim.x * 256) {
    float z[E], zt[E], d[E];
    loss_load_z<E>(lg, q * E, z);
    loss_load_z<E>(tg, q * E, zt);
#pragma unroll
    for (int j = 0; j < E; ++j) {
      d[j] = 0.f;                                        // void: +0
      if (a.ya && (uint64_t)loss_label(a.ya, a.kind, plane + q * E + j) > 1ull) continue;
      float p, qq;
      (void)sf_sig_kl(z[j], zt[j], a.T, p, qq);
      d[j] = gs * (c0 * (p - qq));
    }
    loss_store<E>(dl, q * E, d);
  }
}

struct SfFin {
  int teacher, C, ns, det;
  int64_t nslots;
  float T, smooth, ce_scale, dice_scale;
};

// One block.  Deterministic mode first folds the slots into sums: wave w takes the quantities w, w + 4, ..., its lanes add the slots
// lane, lane + 64, ... in order and the 64 partials meet in a fixed butterfly.  Then the terms and the coefficients in fp64.
__global__ __launch_bounds__(256) void sf_finish_kernel(SfFin f, const float* __restrict__ slots, const float* __restrict__ w_dice,
                                                        float* __restrict__ sums, const int32_t* __restrict__ counts, float* __restrict__ coef,
                                                        float* __restrict__ terms) {
  __shared__ double s_part[LOSS_MAXC];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (f.det) {
    for (int e = wv; e < f.ns; e += 4) {
      double v = 0.0;
      for (int64_t j = lane; j < f.nslots; j += 64) v += (double)slots[j * f.ns + e];
      v = loss_wave_sum(v);
      if (lane == 0) sums[e] = (float)v;
    }
    __syncthreads();
  }
  const double N = (double)counts[0];
  if (f.teacher) {
    if (threadIdx.x == 0) {
      const double kd = N > 0.0 ? (double)f.T * f.T * (double)sums[0] / N : 0.0;
      terms[0] = (float)((double)f.ce_scale * kd);
      terms[1] = (float)kd;
      terms[2] = 0.f;
      coef[0] = N > 0.0 ? (float)((double)f.ce_scale * f.T / N) : 0.f;
    }
    return;
  }
  const int c = threadIdx.x;
  if (c < f.C) {
    const double I = sums[1 + 3 * c], Z = sums[2 + 3 * c], Y = sums[3 + 3 * c], s = f.smooth;
    const double num = 2.0 * I + s, den = Z + Y + s;
    const bool ok = den != 0.0;                          // a denominator that is exactly 0: ratio 1
    const double v = (w_dice ? (double)w_dice[c] : 1.0) / f.C, wv2 = (double)f.dice_scale * v;
    s_part[c] = ok ? v * (1.0 - num / den) : 0.0;
    coef[1 + 2 * c] = ok ? (float)(-wv2 * 2.0 / den) : 0.f;
    coef[2 + 2 * c] = ok ? (float)(wv2 * 2.0 * num / (den * den)) : 0.f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double dice = 0.0;
    for (int k = 0; k < f.C; ++k) dice += s_part[k];
    const double ce = N > 0.0 ? (double)sums[0] / N : 0.0;
    terms[0] = (float)((double)f.ce_scale * ce + (double)f.dice_scale * dice);
    terms[1] = (float)ce;
    terms[2] = (float)dice;
    coef[0] = N > 0.0 ? (float)((double)f.ce_scale / N) : 0.f;
  }
}

inline bool sf_teacher(int reader) { return reader == LMN_SOFT_TEACHER_F32 || reader == LMN_SOFT_TEACHER_BF16; }

// blocks of the sums pass per image (softmax head) or per plane (sigmoid head): a function of reader, head, B, C and HW alone, so that
// lmn_soft_workspace can state the slots exactly
inline int sf_nbx(int reader, int head, int B, int C, int64_t HW) {
  if (head == LMN_SOFT_SOFTMAX) {
    const int64_t items = (reader == LMN_SOFT_TEACHER_BF16 && HW % 4 == 0) ? HW / 4 : HW;
    const int64_t cap = loss_cap(1024, B);
    return loss_templated(C) ? loss_grid(items, cap) : loss_grid(items * 4, cap * 4);   // (general C: blocks of 64 lanes)
  }
  return loss_grid_per(HW % 4 == 0 ? HW / 4 : HW, 2048, (int64_t)B * C);
}
inline int64_t sf_nslots(int reader, int head, int B, int C, int64_t HW) {
  return (int64_t)B * (head == LMN_SOFT_SIGMOID ? C : 1) * sf_nbx(reader, head, B, C, HW);
}
inline int sf_ns(int reader, int C) { return sf_teacher(reader) ? 1 : 1 + 3 * C; }
inline int64_t sf_ws_bytes(int reader, int head, int B, int C, int64_t HW) {
  return lmn_up256((int64_t)4 * sf_nslots(reader, head, B, C, HW) * sf_ns(reader, C));
}

int sf_check(const char* what, int reader, int head, int label_kind, int B, int C, int H, int W) {
  LMN_REQUIRE(reader >= LMN_SOFT_PROBS && reader <= LMN_SOFT_TEACHER_BF16, "%s: unknown reader %d", what, reader);
  LMN_REQUIRE(head == LMN_SOFT_SOFTMAX || head == LMN_SOFT_SIGMOID, "%s: unknown head %d", what, head);
  LMN_REQUIRE(head == LMN_SOFT_SOFTMAX || sf_teacher(reader), "%s: reader %d needs a softmax head", what, reader);
  LMN_REQUIRE(B >= 1 && B <= LMN_SOFT_MAX_BATCH, "%s: B=%d not in [1, %d]", what, B, LMN_SOFT_MAX_BATCH);
  if (int rc = loss_check_head(what, C, head == LMN_SOFT_SOFTMAX, 1ull, label_kind)) return rc;
  return loss_check_extent(what, B, C, H, W);
}

int sf_check_target(const char* what, int reader, const void* target, const void* ya, const void* yb, const float* lam, float T) {
  if (reader == LMN_SOFT_PAIR) LMN_REQUIRE(ya && yb && lam && !target, "%s: the pair reader takes ya, yb and lam and no target", what);
  else LMN_REQUIRE(target && !yb && !lam, "%s: reader %d takes a target and neither yb nor lam", what, reader);
  LMN_REQUIRE(reader != LMN_SOFT_PROBS || !ya, "%s: the probability reader takes no label map", what);
  LMN_REQUIRE(T > 0.f && loss_finite(T), "%s: temperature=%g must be finite and > 0", what, (double)T);
  LMN_REQUIRE(sf_teacher(reader) || T == 1.f, "%s: temperature=%g without a teacher", what, (double)T);
  return 0;
}

// general C: bytes of the LDS columns of one wave
inline size_t sf_lds_bytes(int reader, int C, int E) {
  return (size_t)C * 64 * 4 * (reader == LMN_SOFT_PAIR ? 1 : (E == 4 ? 3 : 2));
}

// run `...` once with the compile-time constants READER and E of the call
#define SF_READER(reader, e4, ...)                                                                                       \
  do {                                                                                                                   \
    if ((reader) == LMN_SOFT_PROBS) { constexpr int READER = LMN_SOFT_PROBS; constexpr int E = 1; __VA_ARGS__; }         \
    else if ((reader) == LMN_SOFT_PAIR) { constexpr int READER = LMN_SOFT_PAIR; constexpr int E = 1; __VA_ARGS__; }      \
    else if ((reader) == LMN_SOFT_TEACHER_F32) { constexpr int READER = LMN_SOFT_TEACHER_F32; constexpr int E = 1; __VA_ARGS__; } \
    else if (e4) { constexpr int READER = LMN_SOFT_TEACHER_BF16; constexpr int E = 4; __VA_ARGS__; }                     \
    else { constexpr int READER = LMN_SOFT_TEACHER_BF16; constexpr int E = 1; __VA_ARGS__; }                             \
  } while (0)

// ---------------------------------------------------------------------------------------------------------------- the batch mixer
struct MixRow { int32_t partner, mode; float lam, oml; int32_t y0, x0, y1, x1; };
static_assert(sizeof(MixRow) == 4 * LMN_MIX_ROW_WORDS, "a row of lmn_mix_batch is LMN_MIX_ROW_WORDS int32 words");

// lam a + oml b with both products and the sum rounded to fp32.  (__fmul_rn / __fadd_rn are plain operators in this toolchain and the
// four-pixel instance contracted them into fused multiply-adds; the pragma takes the permission away, so numpy restates the bits.)
__device__ __forceinline__ float mix_unfused(float lam, float a, float oml, float b) {
#pragma clang fp contract(off)
  const float u = lam * a, v = oml * b;
  return u + v;
}

// blockIdx.z: the sample; blockIdx.y: the channel, or Cin for the label plane; E = 4: four pixels of one image row per lane
template <bool VEC>
__global__ __launch_bounds__(256) void mix_batch_kernel(const float* __restrict__ x, const void* __restrict__ y, int kind,
                                                        const MixRow* __restrict__ rows, int Cin, int H, int W, float* __restrict__ x_out,
                                                        void* __restrict__ ya_out, void* __restrict__ yb_out, float* __restrict__ lam_out) {
  constexpr int E = VEC ? 4 : 1;
  const int b = blockIdx.z, ch = blockIdx.y;
  const MixRow r = rows[b];
  const int64_t hw = (int64_t)H * W;
  if (ch < Cin) {
    const float* xa = x + ((int64_t)b * Cin + ch) * hw;
    const float* xb = x + ((int64_t)r.partner * Cin + ch) * hw;
    float* xo = x_out + ((int64_t)b * Cin + ch) * hw;
    const int64_t items = hw / E;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < items; q += (int64_t)gridDim.x * 256) {
      const int64_t i = q * E;
      float va[E], vo[E];
      loss_load_z<E>(xa, i, va);
      if (r.mode == LMN_MIX_MIXUP) {
        float vb[E];
        loss_load_z<E>(xb, i, vb);
#pragma unroll
        for (int k = 0; k < E; ++k) vo[k] = mix_unfused(r.lam, va[k], r.oml, vb[k]);
      } else {
#pragma unroll
        for (int k = 0; k < E; ++k) vo[k] = va[k];
        if (r.mode == LMN_MIX_CUTMIX) {
          const int yy = (int)(i / W), xx = (int)(i - (int64_t)yy * W);   // (VEC: W % 4 == 0, the four pixels share a row)
          if (yy >= r.y0 && yy < r.y1 && xx + E > r.x0 && xx < r.x1) {
            float vb[E];
            loss_load_z<E>(xb, i, vb);
#pragma unroll
            for (int k = 0; k < E; ++k)
              if (xx + k >= r.x0 && xx + k < r.x1) vo[k] = vb[k];
          }
        }
      }
      loss_store<E>(xo, i, vo);
    }
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) lam_out[b] = r.mode == LMN_MIX_MIXUP ? r.lam : 1.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256) {
    const int yy = (int)(i / W), xx = (int)(i - (int64_t)yy * W);
    const bool box = r.mode == LMN_MIX_CUTMIX && yy >= r.y0 && yy < r.y1 && xx >= r.x0 && xx < r.x1;
    const int64_t own = (int64_t)b * hw + i, other = (int64_t)r.partner * hw + i;
    const int64_t la = loss_label(y, kind, box ? other : own);
    const int64_t lb = r.mode == LMN_MIX_MIXUP ? loss_label(y, kind, other) : la;
    if (kind == LOSS_LABELS_I64) {
      ((int64_t*)ya_out)[own] = la;
      if (yb_out) ((int64_t*)yb_out)[own] = lb;
    } else {
      ((uint8_t*)ya_out)[own] = (uint8_t)la;
      if (yb_out) ((uint8_t*)yb_out)[own] = (uint8_t)lb;
    }
  }
}

inline bool mix_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

}  // namespace

extern "C" {

int64_t lmn_soft_workspace(int reader, int head, int B, int C, int H, int W) {
  if (sf_check("soft_workspace", reader, head, LMN_SOFT_LABELS_U8, B, C, H, W)) return -1;
  return sf_ws_bytes(reader, head, B, C, (int64_t)H * W);
}

int lmn_soft_fwd(const float* logits, int reader, int head, const void* target, const void* ya, const void* yb, int label_kind,
                 const float* lam, float temperature, float eps, float smooth, float ce_scale, float dice_scale, int B, int C, int H,
                 int W, const float* w_ce, const float* w_dice, void* workspace, int64_t ws_bytes, float* sums, int32_t* counts,
                 float* coef, float* terms, lmn_stream_t stream) {
  LMN_REQUIRE(logits && sums && counts && coef && terms, "soft_fwd: null pointer");
  if (int rc = sf_check("soft_fwd", reader, head, label_kind, B, C, H, W)) return rc;
  if (int rc = sf_check_target("soft_fwd", reader, target, ya, yb, lam, temperature)) return rc;
  LMN_REQUIRE(eps >= 0.f && eps <= 1.f, "soft_fwd: label smoothing eps=%g not in [0, 1]", (double)eps);
  LMN_REQUIRE(smooth >= 0.f && loss_finite(smooth), "soft_fwd: smooth=%g must be finite and >= 0", (double)smooth);
  LMN_REQUIRE(loss_finite(ce_scale) && loss_finite(dice_scale), "soft_fwd: scale (%g, %g) is not finite", (double)ce_scale,
              (double)dice_scale);
  LMN_REQUIRE(!sf_teacher(reader) || (!w_ce && !w_dice), "soft_fwd: the teacher readers take no class weight");
  const int64_t HW = (int64_t)H * W;
  const int nbx = sf_nbx(reader, head, B, C, HW), ns = sf_ns(reader, C);
  const int64_t need = sf_ws_bytes(reader, head, B, C, HW);
  LMN_REQUIRE(workspace || !g_lmn_det, "soft_fwd: deterministic mode needs the workspace");
  LMN_REQUIRE(!workspace || ws_bytes >= need, "soft_fwd: workspace of %lld bytes too small, %lld needed", (long long)ws_bytes, (long long)need);
  hipStream_t st = (hipStream_t)stream;
  const SfArgs a{logits, target, ya, yb, lam, w_ce, label_kind, C, HW, temperature, eps};
  const SfOut o{sums, counts, g_lmn_det ? (float*)workspace : nullptr, ns};
  LMN_LAUNCH(loss_zero_kernel, dim3(1), dim3(256), 0, st, (uint32_t*)sums, (int64_t)(1 + 3 * C));
  LMN_LAUNCH(loss_zero_kernel, dim3(1), dim3(64), 0, st, (uint32_t*)counts, (int64_t)1);
  const bool bf = reader == LMN_SOFT_TEACHER_BF16;
  if (head == LMN_SOFT_SOFTMAX) {
    // (sf_nbx sizes the grid from HW alone; with an unaligned base the one-pixel instance runs on the same grid: its loop strides)
    const bool e4 = bf && HW % 4 == 0 && lmn_aligned(logits, 16) && lmn_aligned(target, 8);
    const dim3 grid(nbx, B);
    LOSS_SWITCH_CT(C, SF_READER(reader, e4, {
      const size_t sh = CT > 0 ? 0 : sf_lds_bytes(reader, C, E);
      LMN_LAUNCH((sf_softmax_sums_kernel<CT, READER, E>), grid, dim3(CT > 0 ? 256 : 64), sh, st, a, o);
    }));
  } else {
    const bool vec = HW % 4 == 0 && lmn_aligned(logits, 16) && lmn_aligned(target, bf ? 8 : 16);
    const dim3 grid(nbx, C, B);
    LOSS_SWITCH_BOOL(VEC, vec, LOSS_SWITCH_BOOL(BF, bf, LMN_LAUNCH((sf_sigmoid_sums_kernel<VEC, BF>), grid, dim3(256), 0, st, a, o)));
  }
  const SfFin fin{sf_teacher(reader) ? 1 : 0, C, ns, g_lmn_det ? 1 : 0, sf_nslots(reader, head, B, C, HW), temperature, smooth, ce_scale, dice_scale};
  LMN_LAUNCH(sf_finish_kernel, dim3(1), dim3(256), 0, st, fin, (const float*)o.slots, w_dice, sums, (const int32_t*)counts, coef, terms);
  return lmn_launch_status("soft_fwd");
}

int lmn_soft_bwd(const float* logits, int reader, int head, const void* target, const void* ya, const void* yb, int label_kind,
                 const float* lam, float temperature, float eps, int B, int C, int H, int W, const float* w_ce, const float* coef,
                 const float* gscale, float* dlogits, lmn_stream_t stream) {
  LMN_REQUIRE(logits && coef && dlogits, "soft_bwd: null pointer");
  if (int rc = sf_check("soft_bwd", reader, head, label_kind, B, C, H, W)) return rc;
  if (int rc = sf_check_target("soft_bwd", reader, target, ya, yb, lam, temperature)) return rc;
  LMN_REQUIRE(eps >= 0.f && eps <= 1.f, "soft_bwd: label smoothing eps=%g not in [0, 1]", (double)eps);
  LMN_REQUIRE(!sf_teacher(reader) || !w_ce, "soft_bwd: the teacher readers take no class weight");
  hipStream_t st = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  const SfArgs a{logits, target, ya, yb, lam, w_ce, label_kind, C, HW, temperature, eps};
  const bool bf = reader == LMN_SOFT_TEACHER_BF16;
  if (head == LMN_SOFT_SOFTMAX) {
    const bool e4 = bf && HW % 4 == 0 && lmn_aligned(logits, 16) && lmn_aligned(dlogits, 16) && lmn_aligned(target, 8);
    const int64_t items = e4 ? HW / 4 : HW, cap = loss_cap(4096, B);
    const dim3 grid(loss_templated(C) ? loss_grid(items, cap) : loss_grid(items * 4, cap * 4), B);
    LOSS_SWITCH_CT(C, SF_READER(reader, e4, {
      const size_t sh = CT > 0 ? 0 : sf_lds_bytes(reader, C, E);
      LMN_LAUNCH((sf_softmax_bwd_kernel<CT, READER, E>), grid, dim3(CT > 0 ? 256 : 64), sh, st, a, coef, gscale, dlogits);
    }));
  } else {
    const bool vec = HW % 4 == 0 && lmn_aligned(logits, 16) && lmn_aligned(dlogits, 16) && lmn_aligned(target, bf ? 8 : 16);
    const dim3 grid(loss_grid_per(vec ? HW / 4 : HW, 4096, (int64_t)B * C), C, B);
    LOSS_SWITCH_BOOL(VEC, vec, LOSS_SWITCH_BOOL(BF, bf, LMN_LAUNCH((sf_sigmoid_bwd_kernel<VEC, BF>), grid, dim3(256), 0, st, a, coef, gscale, dlogits)));
  }
  return lmn_launch_status("soft_bwd");
}

int lmn_mix_batch(const float* x, const void* y, int label_kind, const int32_t* rows, int32_t* rows_dev, int B, int Cin, int H, int W,
                  float* x_out, void* ya_out, void* yb_out, float* lam_out, lmn_stream_t stream) {
  LMN_REQUIRE(x && y && rows && rows_dev && x_out && ya_out && lam_out, "mix_batch: null pointer");
  LMN_REQUIRE(label_kind == LMN_SOFT_LABELS_U8 || label_kind == LMN_SOFT_LABELS_I64, "mix_batch: unknown label kind %d", label_kind);
  LMN_REQUIRE(B >= 1 && B <= LMN_SOFT_MAX_BATCH, "mix_batch: B=%d not in [1, %d]", B, LMN_SOFT_MAX_BATCH);
  LMN_REQUIRE(Cin >= 1 && Cin <= 64, "mix_batch: Cin=%d not in [1, 64]", Cin);
  LMN_REQUIRE(H >= 1 && W >= 1, "mix_batch: size %dx%d below 1", H, W);
  LMN_REQUIRE((int64_t)B * Cin * H * W < (1LL << 31), "mix_batch: B * Cin * H * W = %lld not below 2^31", (long long)B * Cin * H * W);
  const int64_t HW = (int64_t)H * W, xbytes = 4 * (int64_t)B * Cin * HW, ybytes = (int64_t)B * HW * (label_kind == LMN_SOFT_LABELS_I64 ? 8 : 1);
  LMN_REQUIRE(!mix_overlap(x, xbytes, x_out, xbytes), "mix_batch: x_out overlaps x (a partner row is read while its own row is written)");
  LMN_REQUIRE(!mix_overlap(y, ybytes, ya_out, ybytes) && !(yb_out && mix_overlap(y, ybytes, yb_out, ybytes)),
              "mix_batch: ya_out or yb_out overlaps y (a partner row is read while its own row is written)");
  const MixRow* r = (const MixRow*)rows;
  for (int b = 0; b < B; ++b) {
    LMN_REQUIRE(r[b].partner >= 0 && r[b].partner < B, "mix_batch: row %d: partner %d not in [0, %d)", b, r[b].partner, B);
    LMN_REQUIRE(r[b].mode >= LMN_MIX_NONE && r[b].mode <= LMN_MIX_CUTMIX, "mix_batch: row %d: unknown mode %d", b, r[b].mode);
    LMN_REQUIRE(r[b].lam >= 0.f && r[b].lam <= 1.f, "mix_batch: row %d: lam=%g not in [0, 1]", b, (double)r[b].lam);
    LMN_REQUIRE(r[b].oml == 1.0f - r[b].lam, "mix_batch: row %d: the fourth word %g is not 1 - lam in fp32", b, (double)r[b].oml);
    LMN_REQUIRE(0 <= r[b].y0 && r[b].y0 <= r[b].y1 && r[b].y1 <= H && 0 <= r[b].x0 && r[b].x0 <= r[b].x1 && r[b].x1 <= W,
                "mix_batch: row %d: box [%d, %d) x [%d, %d) outside %dx%d", b, r[b].y0, r[b].y1, r[b].x0, r[b].x1, H, W);
    LMN_REQUIRE(r[b].mode != LMN_MIX_MIXUP || yb_out, "mix_batch: row %d is a mixup row and yb_out is NULL", b);
  }
  hipStream_t st = (hipStream_t)stream;
  LMN_HIP_OK(hipMemcpyAsync(rows_dev, rows, sizeof(MixRow) * (size_t)B, hipMemcpyHostToDevice, st), "mix_batch");
  const bool vec = W % 4 == 0 && lmn_aligned(x, 16) && lmn_aligned(x_out, 16);
  const dim3 grid(loss_grid_per(vec ? HW / 4 : HW, 4096, (int64_t)B * (Cin + 1)), Cin + 1, B);
  LOSS_SWITCH_BOOL(VEC, vec, LMN_LAUNCH((mix_batch_kernel<VEC>), grid, dim3(256), 0, st, x, y, label_kind, (const MixRow*)rows_dev, Cin, H, W, x_out, ya_out, yb_out, lam_out));
  return lmn_launch_status("mix_batch");
}

}  // extern "C"

// Neighborhood attention for ANY head_dim 1..32 (wide LM_Net variants: filters[i] / 12 heads = 3, 5, 6, 7, 12, 24, ...).  Same
// semantics and buffers as the channel-quad kernels of na.hip (oracle/natten_ref.py; window start clamp(i - K/2, 0, L - K), bias
// index neighbour - query + K - 1), for K odd 3..9.
//
// One thread owns one (pixel, head) -- two adjacent lanes own one when hd is even and above 16, hl = hd / 2 dims each, the dot
// products closed by one lane-pair shuffle: q, dO and the accumulators of the lane's hl dims live in registers (an array of
// HDM >= hl floats whose guards `d < hl` are uniform), moved VW at a time (VW = 4 / 2 / 1 for hl % 4 == 0 / hl % 2 == 0 / odd hl
// -- the widest load the alignment of head * hd allows), so a channel quad never has to straddle two heads.  Lanes walk the heads
// of a pixel first: a wave reads whole NHWC pixels contiguously, and the K x K re-use of k / v between neighbouring queries is
// served by L1 / L2.
//   forward      single pass, online softmax (running max / sum rescaled per neighbour)
//   backward     query pass: lse, dsum = sum_n p_n dp_n (online, first sweep), dq and the rpb gradient (second sweep; per-wave LDS
//                bins, one global add per bin per block -- slot copies in deterministic mode); key pass: every query whose clamped
//                window holds the key, dk and dv gathered -- no atomics on dqkv.
#include "na_gen.h"

#include <stdlib.h>

#include <type_traits>

namespace {

struct NgGeom {
  int B, H, W, C, heads, hd, hl, K;   // hl = hd / LP: the dims of one lane
  float scale;
  uint32_t mH, mW, mHW;   // floor(2^32 / d) for d = heads, W, H*W (lmn_div_row)
};

// VW consecutive channels in / out (fp32 math)
template <int VW, typename TA>
__device__ __forceinline__ void ldv(const TA* p, float* d) {
  if constexpr (VW == 4) {
    const f32x4 v = ld4(p);
    d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
  } else if constexpr (VW == 2) {
    if constexpr (std::is_same<TA, float>::value) {
      const float2 v = *reinterpret_cast<const float2*>(p);
      d[0] = v.x; d[1] = v.y;
    } else {
      const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
      d[0] = lmn_bf16_lo(u); d[1] = lmn_bf16_hi(u);
    }
  } else {
    d[0] = ld1(p);
  }
}
template <int VW, typename TA>
__device__ __forceinline__ void stv(TA* p, const float* d) {
  if constexpr (VW == 4) {
    st4(p, f32x4{d[0], d[1], d[2], d[3]});
  } else if constexpr (VW == 2) {
    if constexpr (std::is_same<TA, float>::value) *reinterpret_cast<float2*>(p) = float2{d[0], d[1]};
    else *reinterpret_cast<uint32_t*>(p) = lmn_pk_bf16(d[0], d[1]);
  } else {
    st1(p, d[0]);
  }
}
// x[0..hd) <- p[0..hd) * s ; the registers past hd stay 0
template <int VW, int HDM, typename TA>
__device__ __forceinline__ void ld_head(const TA* p, int hd, float s, float (&x)[HDM]) {
#pragma unroll
  for (int d = 0; d < HDM; d += VW) {
    if (d < hd) {
      ldv<VW>(p + d, x + d);
#pragma unroll
      for (int e = 0; e < VW; ++e) x[d + e] *= s;
    } else {
#pragma unroll
      for (int e = 0; e < VW; ++e) x[d + e] = 0.f;
    }
  }
}
template <int VW, int HDM, typename TA>
__device__ __forceinline__ void st_head(TA* p, int hd, float s, const float (&x)[HDM]) {
#pragma unroll
  for (int d = 0; d < HDM; d += VW)
    if (d < hd) {
      float t[VW];
#pragma unroll
      for (int e = 0; e < VW; ++e) t[e] = x[d + e] * s;
      stv<VW>(p + d, t);
    }
}
template <int VW, int HDM, typename TA>
__device__ __forceinline__ float dot_head(const TA* p, int hd, const float (&x)[HDM]) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < HDM; d += VW)
    if (d < hd) {
      float t[VW];
      ldv<VW>(p + d, t);
#pragma unroll
      for (int e = 0; e < VW; ++e) s += x[d + e] * t[e];
    }
  return s;
}

__device__ __forceinline__ int ng_wstart(int i, int L, int K) {
  int s = i - (K >> 1);
  s = s < 0 ? 0 : s;
  return s > L - K ? L - K : s;
}

// item idx -> (pixel, head, lane of the head); co = the lane's first channel inside a q / k / v / out row
struct NgItem { int h, b, y, x, sub, co; int64_t pix; };
template <int LP>
__device__ __forceinline__ NgItem ng_decode(const NgGeom& g, uint32_t idx) {
  const uint32_t u = LP == 2 ? idx >> 1 : idx;
  const uint32_t pix = lmn_div_row(u, (uint32_t)g.heads, g.mH);
  const uint32_t b = lmn_div_row(pix, (uint32_t)(g.H * g.W), g.mHW), r = pix - b * (uint32_t)(g.H * g.W);
  const uint32_t y = lmn_div_row(r, (uint32_t)g.W, g.mW);
  const int h = (int)(u - pix * (uint32_t)g.heads), sub = LP == 2 ? (int)(idx & 1) : 0;
  return NgItem{h, (int)b, (int)y, (int)(r - y * (uint32_t)g.W), sub, h * g.hd + sub * g.hl, (int64_t)pix};
}
// a head's dot product from the partial sums of its LP lanes (adjacent lanes: the pair is converged in every loop below)
template <int LP>
__device__ __forceinline__ float pair_sum(float v) {
  if constexpr (LP == 2) v += __shfl_xor(v, 1, 64);
  return v;
}

template <int LP, int VW, int HDM, typename TA>
__global__ __launch_bounds__(256) void na_any_fwd_kernel(const TA* __restrict__ qkv, const float* __restrict__ rpb,
                                                         TA* __restrict__ out, const NgGeom g) {
  const int K = g.K, RB = 2 * K - 1, C3 = 3 * g.C;
  const int total = g.B * g.H * g.W * g.heads * LP;
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
    const NgItem it = ng_decode<LP>(g, (uint32_t)idx);
    const TA* base = qkv + (int64_t)it.b * g.H * g.W * C3 + it.co;
    const float* rp = rpb + it.h * RB * RB;
    const int sy = ng_wstart(it.y, g.H, K), sx = ng_wstart(it.x, g.W, K);
    float q[HDM], o[HDM];
    ld_head<VW>(base + ((int64_t)it.y * g.W + it.x) * C3, g.hl, g.scale, q);
#pragma unroll
    for (int d = 0; d < HDM; ++d) o[d] = 0.f;
    float m = -3.0e38f, l = 0.f;
    for (int ki = 0; ki < K; ++ki)
      for (int kj = 0; kj < K; ++kj) {
        const TA* kp = base + ((int64_t)(sy + ki) * g.W + sx + kj) * C3;
        const float s = pair_sum<LP>(dot_head<VW>(kp + g.C, g.hl, q)) + rp[(sy + ki - it.y + K - 1) * RB + (sx + kj - it.x + K - 1)];
        const float mn = fmaxf(m, s), cr = __expf(m - mn), p = __expf(s - mn);
        l = l * cr + p;
        m = mn;
        float v[HDM];
        ld_head<VW>(kp + 2 * g.C, g.hl, 1.f, v);
#pragma unroll
        for (int d = 0; d < HDM; ++d) o[d] = o[d] * cr + p * v[d];
      }
    st_head<VW>(out + it.pix * g.C + it.co, g.hl, 1.f / l, o);
  }
}

// query pass: dq (q part of dqkv), stat = (lse, dsum) per (pixel, head), rpb gradient
template <int LP, int VW, int HDM, typename TA>
__global__ __launch_bounds__(256) void na_any_bwd_q_kernel(const TA* __restrict__ qkv, const float* __restrict__ rpb,
                                                           const TA* __restrict__ dout, TA* __restrict__ dqkv,
                                                           float* __restrict__ drpb, float* __restrict__ stat, const NgGeom g,
                                                           int det) {
  extern __shared__ float s_bins[];   // [4 waves][heads][RB][RB]: a wave adds in its own table (program order), fixed-order sum below
  const int K = g.K, RB = 2 * K - 1, NB = g.heads * RB * RB, C3 = 3 * g.C;
  for (int i = threadIdx.x; i < 4 * NB; i += 256) s_bins[i] = 0.f;
  __syncthreads();
  float* tab = s_bins + (threadIdx.x >> 6) * NB;
  const int total = g.B * g.H * g.W * g.heads * LP;
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
    const NgItem it = ng_decode<LP>(g, (uint32_t)idx);
    const int64_t ib = (int64_t)it.b * g.H * g.W * C3 + it.co;
    const TA* base = qkv + ib;
    const float* rp = rpb + it.h * RB * RB;
    float* tb = tab + it.h * RB * RB;
    const int sy = ng_wstart(it.y, g.H, K), sx = ng_wstart(it.x, g.W, K);
    float q[HDM], dO[HDM], dq[HDM];
    ld_head<VW>(base + ((int64_t)it.y * g.W + it.x) * C3, g.hl, g.scale, q);
    ld_head<VW>(dout + it.pix * g.C + it.co, g.hl, 1.f, dO);
#pragma unroll
    for (int d = 0; d < HDM; ++d) dq[d] = 0.f;
    // sweep 1: running max, sum of exp, sum of exp * dp
    float m = -3.0e38f, l = 0.f, sdp = 0.f;
    for (int ki = 0; ki < K; ++ki)
      for (int kj = 0; kj < K; ++kj) {
        const TA* kp = base + ((int64_t)(sy + ki) * g.W + sx + kj) * C3;
        const float s = pair_sum<LP>(dot_head<VW>(kp + g.C, g.hl, q)) + rp[(sy + ki - it.y + K - 1) * RB + (sx + kj - it.x + K - 1)];
        const float dp = pair_sum<LP>(dot_head<VW>(kp + 2 * g.C, g.hl, dO));
        const float mn = fmaxf(m, s), cr = __expf(m - mn), p = __expf(s - mn);
        l = l * cr + p;
        sdp = sdp * cr + p * dp;
        m = mn;
      }
    const float lse = m + __logf(l), dsum = sdp / l;
    // sweep 2: ds_n = p_n (dp_n - dsum); dq = sum_n ds_n k_n; rpb bins
    for (int ki = 0; ki < K; ++ki)
      for (int kj = 0; kj < K; ++kj) {
        const TA* kp = base + ((int64_t)(sy + ki) * g.W + sx + kj) * C3;
        const int bo = (sy + ki - it.y + K - 1) * RB + (sx + kj - it.x + K - 1);
        float kk[HDM];
        ld_head<VW>(kp + g.C, g.hl, 1.f, kk);
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < HDM; ++d) s += q[d] * kk[d];
        s = pair_sum<LP>(s) + rp[bo];
        const float ds = __expf(s - lse) * (pair_sum<LP>(dot_head<VW>(kp + 2 * g.C, g.hl, dO)) - dsum);
#pragma unroll
        for (int d = 0; d < HDM; ++d) dq[d] += ds * kk[d];
        if (it.sub == 0) atomicAdd(&tb[bo], ds);
      }
    st_head<VW>(dqkv + ib + ((int64_t)it.y * g.W + it.x) * C3, g.hl, g.scale, dq);
    if (it.sub == 0) {
      stat[it.pix * 2 * g.heads + it.h] = lse;
      stat[it.pix * 2 * g.heads + g.heads + it.h] = dsum;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NB; i += 256) {
    const float v = ((s_bins[i] + s_bins[NB + i]) + s_bins[2 * NB + i]) + s_bins[3 * NB + i];
    if (det || v != 0.f) lmn_red_add(drpb + (det ? (int64_t)blockIdx.x * NB : 0) + i, v, det);
  }
}

// key pass: key j is seen by query i iff 0 <= j - wstart(i) < K on both axes; dk_j = sum_i ds_ij scale q_i, dv_j = sum_i p_ij dO_i
template <int LP, int VW, int HDM, typename TA>
__global__ __launch_bounds__(256) void na_any_bwd_kv_kernel(const TA* __restrict__ qkv, const float* __restrict__ rpb,
                                                            const TA* __restrict__ dout, TA* __restrict__ dqkv,
                                                            const float* __restrict__ stat, const NgGeom g) {
  const int K = g.K, RB = 2 * K - 1, C3 = 3 * g.C;
  const int total = g.B * g.H * g.W * g.heads * LP;
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
    const NgItem it = ng_decode<LP>(g, (uint32_t)idx);
    const int jy = it.y, jx = it.x;
    const int64_t ib = (int64_t)it.b * g.H * g.W * C3 + it.co;
    const TA* base = qkv + ib;
    const float* rp = rpb + it.h * RB * RB;
    const int64_t kpo = ((int64_t)jy * g.W + jx) * C3;
    float kj[HDM], vj[HDM], dk[HDM], dv[HDM];
    ld_head<VW>(base + kpo + g.C, g.hl, 1.f, kj);
    ld_head<VW>(base + kpo + 2 * g.C, g.hl, 1.f, vj);
#pragma unroll
    for (int d = 0; d < HDM; ++d) dk[d] = dv[d] = 0.f;
    for (int iy = jy - K + 1; iy <= jy + K - 1; ++iy) {
      if (iy < 0 || iy >= g.H) continue;
      const int ky = jy - ng_wstart(iy, g.H, K);
      if (ky < 0 || ky >= K) continue;
      for (int ix = jx - K + 1; ix <= jx + K - 1; ++ix) {
        if (ix < 0 || ix >= g.W) continue;
        const int kx = jx - ng_wstart(ix, g.W, K);
        if (kx < 0 || kx >= K) continue;
        const int64_t ipix = ((int64_t)it.b * g.H + iy) * g.W + ix;
        float qi[HDM], dOi[HDM];
        ld_head<VW>(base + ((int64_t)iy * g.W + ix) * C3, g.hl, g.scale, qi);
        ld_head<VW>(dout + ipix * g.C + it.co, g.hl, 1.f, dOi);
        float s = 0.f, dp = 0.f;
#pragma unroll
        for (int d = 0; d < HDM; ++d) {
          s += qi[d] * kj[d];
          dp += dOi[d] * vj[d];
        }
        s = pair_sum<LP>(s) + rp[(jy - iy + K - 1) * RB + (jx - ix + K - 1)];
        dp = pair_sum<LP>(dp);
        const float* sp = stat + ipix * 2 * g.heads;
        const float p = __expf(s - sp[it.h]), ds = p * (dp - sp[g.heads + it.h]);
#pragma unroll
        for (int d = 0; d < HDM; ++d) {
          dk[d] += ds * qi[d];   // (qi carries the scale)
          dv[d] += p * dOi[d];
        }
      }
    }
    st_head<VW>(dqkv + ib + kpo + g.C, g.hl, 1.f, dk);
    st_head<VW>(dqkv + ib + kpo + 2 * g.C, g.hl, 1.f, dv);
  }
}

inline int ng_grid(int64_t total, int cap) {
  int64_t n = (total + 255) / 256;
  if (n > cap) n = cap;
  return (int)(n < 1 ? 1 : n);
}

// lanes per head: two for an even hd above 16 (hd 24: 12 dims a lane, 32: 16 -- a third of the registers, twice the lanes of one
// lane per head); one instantiation per (lanes, vector width, register array size)
inline int ng_lanes(int hd) { return hd > 16 && hd % 2 == 0 ? 2 : 1; }
#define LMN_NG_SELECT(hd, CALL)              \
  do {                                       \
    const int hl_ = (hd) / ng_lanes(hd);     \
    const int vw_ = hl_ % 4 == 0 ? 4 : hl_ % 2 == 0 ? 2 : 1; \
    const int hm_ = hl_ <= 8 ? 8 : hl_ <= 16 ? 16 : 32;      \
    if (ng_lanes(hd) == 2) {                 \
      if (vw_ == 4) CALL(2, 4, 16); else if (vw_ == 2) CALL(2, 2, 16); else CALL(2, 1, 16); \
    } else if (vw_ == 4) {                   \
      if (hm_ == 8) CALL(1, 4, 8); else CALL(1, 4, 16); \
    } else if (vw_ == 2) {                   \
      if (hm_ == 8) CALL(1, 2, 8); else CALL(1, 2, 16); \
    } else {                                 \
      if (hm_ == 8) CALL(1, 1, 8); else if (hm_ == 16) CALL(1, 1, 16); else CALL(1, 1, 32); \
    }                                        \
  } while (0)

int ng_check(int B, int H, int W, int heads, int hd, int K, const char* what) {
  LMN_REQUIRE(K >= 3 && K <= 9 && (K & 1), "%s: window %d (odd, 3..9)", what, K);
  LMN_REQUIRE(B > 0 && H >= K && W >= K, "%s: feature map %dx%d smaller than the %dx%d window", what, H, W, K, K);
  LMN_REQUIRE(hd >= 1 && hd <= LMN_NA_ANY_MAX_HD, "%s: head_dim %d not in 1..%d", what, hd, LMN_NA_ANY_MAX_HD);
  LMN_REQUIRE(heads >= 1 && 4 * heads * (2 * K - 1) * (2 * K - 1) * (int)sizeof(float) <= 64 * 1024,
              "%s: %d heads x %dx%d bias table exceed the LDS bins", what, heads, 2 * K - 1, 2 * K - 1);
  LMN_REQUIRE((int64_t)B * H * W * heads * 2 < (1LL << 31), "%s: %d x %d x %d x %d heads exceeds the 32-bit item index", what, B, H, W,
              heads);
  return 0;
}

}  // namespace

bool lmn_na_force_general() {
  static const int v = getenv("LMN_NA_GENERAL") ? atoi(getenv("LMN_NA_GENERAL")) : 0;
  return v != 0;
}

int lmn_na_any_fwd(const void* qkv, const float* rpb, void* out, int B, int H, int W, int heads, int hd, int K, float scale,
                   int act_dtype, hipStream_t st) {
  if (int rc = ng_check(B, H, W, heads, hd, K, "na_fwd")) return rc;
  const int lp = ng_lanes(hd);
  const NgGeom g{B, H, W, heads * hd, heads, hd, hd / lp, K, scale, lmn_div_magic(heads), lmn_div_magic(W), lmn_div_magic(H * W)};
  const int64_t items = (int64_t)B * H * W * heads * lp;
  const int grid = ng_grid(items, 8192);
  if (g_lmn_prof_on) lmn_prof_cost(2.0 * 2 * K * K * (double)B * H * W * g.C, (act_dtype == LMN_BF16 ? 2.0 : 4.0) * 4 * (double)B * H * W * g.C);
#define LMN_NGF(LP, VW, HM) LMN_LAUNCH((na_any_fwd_kernel<LP, VW, HM, T>), dim3(grid), dim3(256), 0, st, (const T*)qkv, rpb, (T*)out, g)
  LMN_ACT_DISPATCH(act_dtype, LMN_NG_SELECT(hd, LMN_NGF));
#undef LMN_NGF
  return lmn_launch_status("na_fwd");
}

int lmn_na_any_bwd(const void* qkv, const float* rpb, const void* dout, void* dqkv, float* drpb, float* stat, int B, int H, int W,
                   int heads, int hd, int K, float scale, int act_dtype, hipStream_t st) {
  if (int rc = ng_check(B, H, W, heads, hd, K, "na_bwd")) return rc;
  const int lp = ng_lanes(hd);
  const NgGeom g{B, H, W, heads * hd, heads, hd, hd / lp, K, scale, lmn_div_magic(heads), lmn_div_magic(W), lmn_div_magic(H * W)};
  const int64_t items = (int64_t)B * H * W * heads * lp;
  // query pass: persistent blocks (one global add per bias bin per block, as lmn_na_bwd's query pass)
  const int gq = ng_grid(items, 512), gk = ng_grid(items, 8192);
  const int NB = heads * (2 * K - 1) * (2 * K - 1);
  const size_t sh = (size_t)4 * NB * sizeof(float);
  float* dslot = drpb;
  if (g_lmn_det) {   // the bias-table gradient of every block into its own slot, folded in fixed order after the query pass
    lmn_det_begin(st);
    dslot = lmn_det_slots(st, (size_t)gq * NB);
    LMN_REQUIRE(dslot, "na_bwd: deterministic mode: no scratch");
  }
  const double ab = act_dtype == LMN_BF16 ? 2.0 : 4.0;
#define LMN_NGB(LP, VW, HM)                                                                                                     \
  do {                                                                                                                        \
    if (g_lmn_prof_on) lmn_prof_cost(2.0 * 4 * K * K * (double)B * H * W * g.C, ab * 5 * (double)B * H * W * g.C);            \
    LMN_LAUNCH((na_any_bwd_q_kernel<LP, VW, HM, T>), dim3(gq), dim3(256), sh, st, (const T*)qkv, rpb, (const T*)dout, (T*)dqkv, dslot, \
               stat, g, g_lmn_det);                                                                                           \
    if (g_lmn_det) lmn_det_sum(st, dslot, gq, NB, drpb);                                                                      \
    if (g_lmn_prof_on) lmn_prof_cost(2.0 * 4 * K * K * (double)B * H * W * g.C, ab * 2 * (double)B * H * W * g.C);            \
    LMN_LAUNCH((na_any_bwd_kv_kernel<LP, VW, HM, T>), dim3(gk), dim3(256), 0, st, (const T*)qkv, rpb, (const T*)dout, (T*)dqkv,   \
               stat, g);                                                                                                      \
  } while (0)
  LMN_ACT_DISPATCH(act_dtype, LMN_NG_SELECT(hd, LMN_NGB));
#undef LMN_NGB
  return lmn_launch_status("na_bwd");
}

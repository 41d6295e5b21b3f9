// The input side of a 3D case (include/slices/lmnet_slices.h): the integer statistics of an int16 / uint8 volume with a two-level radix
// select for its order statistics, and the gather that writes the fp32 2.5D batches the network reads.
//   workspace (per modality m, all zeroed at the start of lmn_slices_stats):
//     acc   uint64 [M, 8]     n, sum v, sum v^2 (two's complement), max (32767 - v), max (v + 32768): sums and maxima from zero
//     hist  uint32 [M, 1024]  the coarse histogram over (v + 32768) >> 6
//     fine  uint32 [M, 2, 64] the values inside the coarse bin of each rank (one row serves both ranks when they share their bin)
//     ctrl  uint32 [M, 8]     bin_lo, #below it, bin_hi, #below it, r_lo, r_hi, n > 0, 0
//   Every counter has 32 bits: n <= 2^30.  The second pass reads what the one-block step wrote in an earlier launch; no kernel waits
//   on another block.
#include "loss_common.h"
#include "../../include/slices/lmnet_slices.h"

namespace {

constexpr int SL_COARSE = 1024, SL_FINE = 64, SL_CTRL = 8;
constexpr int SL_ROUNDS = 2;   // distinct keys a wave counts by ballot before its lanes fall back to one atomic each

struct SlFg { int v[LMN_SLICES_MAX_MODALITIES]; };

struct SlFin {
  int M, S;
  int mod[LMN_SLICES_MAX_CHANNELS], kind[LMN_SLICES_MAX_CHANNELS];
  double level[LMN_SLICES_MAX_CHANNELS], width[LMN_SLICES_MAX_CHANNELS];
};

inline int64_t sl_ws_bytes(int M) {
  const int64_t b = (int64_t)M * (8 * 8 + 4 * (SL_COARSE + 2 * SL_FINE + SL_CTRL));
  return (b + 255) / 256 * 256;
}

// adds one to h[key] (key < 0: nothing).  A case is often mostly one value (air, zero padding): the lanes of a wave that hold the
// key of the first live lane are counted by one ballot and added by one atomic, SL_ROUNDS times over; what is left goes singly.
// Called by every lane of the loop iteration, live or not.
__device__ __forceinline__ void sl_hist_add(uint32_t* h, int key) {
  const int lane = threadIdx.x & 63;
  unsigned long long rem = __ballot(key >= 0);
#pragma unroll
  for (int r = 0; r < SL_ROUNDS; ++r) {
    if (!rem) break;                                    // (wave-uniform)
    const int leader = __ffsll((long long)rem) - 1;
    const int k = __shfl(key, leader, 64);
    const unsigned long long same = __ballot(key == k);
    if (lane == leader) atomicAdd(&h[k], (uint32_t)__popcll(same));
    if (key == k) key = -1;
    rem &= ~same;
  }
  if (key >= 0) atomicAdd(&h[key], 1u);
}

__device__ __forceinline__ long long sl_wave_sum(long long v) {
#pragma unroll
  for (int m = 1; m <= 32; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ int sl_wave_max(int v) {
#pragma unroll
  for (int m = 1; m <= 32; m <<= 1) v = max(v, __shfl_xor(v, m, 64));
  return v;
}

// PASS 1: the sums, the extrema and the coarse histogram of modality blockIdx.y.  PASS 2: the fine histograms of the chosen bins.
// nvec: the 16-byte chunks of a modality read as such (0 when a modality's base is not 16-byte aligned); the rest is read singly.
template <typename VT, int PASS>
__global__ void __launch_bounds__(256) sl_scan_kernel(const VT* __restrict__ vol, int64_t N, int64_t nvec, SlFg fg,
                                                      unsigned long long* __restrict__ acc, uint32_t* __restrict__ hist,
                                                      uint32_t* __restrict__ fine, const uint32_t* __restrict__ ctrl) {
  constexpr int NB = PASS == 1 ? SL_COARSE : 2 * SL_FINE, EPV = 16 / (int)sizeof(VT);
  __shared__ uint32_t s_h[NB];
  __shared__ long long s_red[4][5];
  const int m = blockIdx.y, fgm = fg.v[m];
  int bin_lo = 0, bin_hi = 0;
  if (PASS == 2) {
    if (!ctrl[m * SL_CTRL + 6]) return;                 // (block-uniform: an empty foreground has nothing to select)
    bin_lo = (int)ctrl[m * SL_CTRL + 0];
    bin_hi = (int)ctrl[m * SL_CTRL + 2];
  }
  for (int i = threadIdx.x; i < NB; i += 256) s_h[i] = 0u;
  __syncthreads();
  const VT* __restrict__ p = vol + (int64_t)m * N;
  long long n = 0, s = 0, q = 0;
  int umn = 0, umx = 0;
  auto one = [&](int v) {
    const bool in = v > fgm;
    int key = -1;
    if (PASS == 1) {
      if (in) {
        n += 1;
        s += v;
        q += (long long)(v * v);
        umn = max(umn, 32767 - v);
        umx = max(umx, v + 32768);
        key = (v + 32768) >> 6;
      }
    } else if (in) {
      const int u = v + 32768, cb = u >> 6;
      if (cb == bin_lo) key = u & 63;
      else if (cb == bin_hi) key = SL_FINE + (u & 63);
    }
    sl_hist_add(s_h, key);
  };
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
  for (int64_t i = tid; i < nvec; i += nth) {
    const uint4 w4 = ((const uint4*)p)[i];
    const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (sizeof(VT) == 2) {
        one((int)(int16_t)(w[j] & 0xffffu));
        one((int)(int16_t)(w[j] >> 16));
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b) one((int)((w[j] >> (8 * b)) & 0xffu));
      }
    }
  }
  for (int64_t i = nvec * EPV + tid; i < N; i += nth) one((int)p[i]);
  __syncthreads();
  if (PASS == 1) {
    n = sl_wave_sum(n);
    s = sl_wave_sum(s);
    q = sl_wave_sum(q);
    umn = sl_wave_max(umn);
    umx = sl_wave_max(umx);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
      s_red[wave][0] = n;
      s_red[wave][1] = s;
      s_red[wave][2] = q;
      s_red[wave][3] = umn;
      s_red[wave][4] = umx;
    }
    __syncthreads();
    if (threadIdx.x < 5) {                              // one 64-bit integer atomic per block and quantity
      const int k = threadIdx.x;
      unsigned long long* a = acc + m * 8 + k;
      if (k < 3) {
        const long long t = s_red[0][k] + s_red[1][k] + s_red[2][k] + s_red[3][k];
        if (t) atomicAdd(a, (unsigned long long)t);
      } else {
        const long long t = max(max(s_red[0][k], s_red[1][k]), max(s_red[2][k], s_red[3][k]));
        if (t) atomicMax(a, (unsigned long long)t);
      }
    }
    for (int i = threadIdx.x; i < NB; i += 256)
      if (s_h[i]) atomicAdd(&hist[m * SL_COARSE + i], s_h[i]);
  } else {
    for (int i = threadIdx.x; i < NB; i += 256)
      if (s_h[i]) atomicAdd(&fine[m * 2 * SL_FINE + i], s_h[i]);
  }
}

// the coarse bin of each rank and the count below it; one wave per modality
__global__ void __launch_bounds__(64) sl_step_kernel(const unsigned long long* __restrict__ acc, const uint32_t* __restrict__ hist,
                                                     uint32_t* __restrict__ ctrl, int q_lo_ppm, int q_hi_ppm) {
  const int m = blockIdx.x, lane = threadIdx.x;
  const long long n = (long long)acc[m * 8];
  if (n == 0) return;                                   // (ctrl stays zero: not live)
  const long long rank[2] = {((long long)q_lo_ppm * (n - 1)) / 1000000, ((long long)q_hi_ppm * (n - 1)) / 1000000};
  constexpr int PER = SL_COARSE / 64;
  const uint32_t* __restrict__ h = hist + m * SL_COARSE + lane * PER;
  uint32_t sum = 0;
  for (int i = 0; i < PER; ++i) sum += h[i];
  uint32_t inc = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)inc, d, 64);
    if (lane >= d) inc += up;
  }
  for (int k = 0; k < 2; ++k) {
    long long before = (long long)inc - sum;
    if (rank[k] >= before && rank[k] < (long long)inc) {
      for (int i = 0; i < PER; ++i) {
        if (rank[k] < before + h[i]) {
          ctrl[m * SL_CTRL + 2 * k] = (uint32_t)(lane * PER + i);
          ctrl[m * SL_CTRL + 2 * k + 1] = (uint32_t)before;
          break;
        }
        before += h[i];
      }
    }
  }
  if (lane == 0) {
    ctrl[m * SL_CTRL + 4] = (uint32_t)rank[0];
    ctrl[m * SL_CTRL + 5] = (uint32_t)rank[1];
    ctrl[m * SL_CTRL + 6] = 1u;
  }
}

// the records and the normalisation table, in fp64 rounded once; one block
__global__ void __launch_bounds__(64) sl_finish_kernel(SlFin f, const unsigned long long* __restrict__ acc, const uint32_t* __restrict__ fine,
                                                       const uint32_t* __restrict__ ctrl, int64_t* __restrict__ stats,
                                                       float* __restrict__ table) {
  __shared__ int s_v[2 * LMN_SLICES_MAX_MODALITIES];
  const int t = threadIdx.x;
  if (t < 2 * f.M) {
    const int m = t >> 1, which = t & 1;
    const uint32_t* __restrict__ c = ctrl + m * SL_CTRL;
    int val = 0;
    if (c[6]) {
      const int bin = (int)c[2 * which];
      const uint32_t within = c[4 + which] - c[2 * which + 1];
      const uint32_t* __restrict__ h = fine + m * 2 * SL_FINE + ((which && c[2] != c[0]) ? SL_FINE : 0);
      uint32_t cum = 0;
      int j = 0;
      for (; j < SL_FINE - 1; ++j) {
        cum += h[j];
        if (within < cum) break;
      }
      val = ((bin << 6) | j) - 32768;
    }
    s_v[t] = val;
  }
  __syncthreads();
  if (t < f.M) {
    const long long n = (long long)acc[t * 8];
    int64_t* __restrict__ r = stats + t * LMN_SLICES_NSTAT;
    r[0] = n;
    r[1] = n ? (long long)acc[t * 8 + 1] : 0;
    r[2] = n ? (long long)acc[t * 8 + 2] : 0;
    r[3] = n ? 32767 - (long long)acc[t * 8 + 3] : 0;
    r[4] = n ? (long long)acc[t * 8 + 4] - 32768 : 0;
    r[5] = s_v[2 * t];
    r[6] = s_v[2 * t + 1];
    r[7] = 0;
  }
  if (t < f.S) {
    const int m = f.mod[t];
    const long long n = (long long)acc[m * 8], s = (long long)acc[m * 8 + 1], q = (long long)acc[m * 8 + 2];
    const double v_lo = (double)s_v[2 * m], v_hi = (double)s_v[2 * m + 1];
    double lo = v_lo, hi = v_hi, a = 0.0, b = 0.0;
    if (f.kind[t] == LMN_SLICES_WINDOW) {
      lo = f.level[t] - 0.5 * f.width[t];
      hi = f.level[t] + 0.5 * f.width[t];
      a = lo;
      b = 1.0 / f.width[t];
    } else if (f.kind[t] == LMN_SLICES_ZSCORE) {
      if (n) {
        // n sum v^2 - (sum v)^2 >= 0 in 128-bit integers: no cancellation, and exactly 0 for a constant volume
        const unsigned __int128 num = (unsigned __int128)((__int128)n * (__int128)q - (__int128)s * (__int128)s);
        const double d = (double)(unsigned long long)(num >> 64) * 18446744073709551616.0 + (double)(unsigned long long)num;
        const double sd = sqrt(d) / (double)n;
        a = (double)s / (double)n;
        b = 1.0 / fmax(sd, 1e-8);
      }
    } else {
      a = v_lo;
      b = v_hi == v_lo ? 0.0 : 1.0 / (v_hi - v_lo);
    }
    table[4 * t + 0] = (float)lo;
    table[4 * t + 1] = (float)hi;
    table[4 * t + 2] = (float)a;
    table[4 * t + 3] = (float)b;
  }
}

// ---------------------------------------------------------------------------------------------------------------- gather
struct SlG {
  int M, D, Hs, Ws, S, K, ctx, stride, edge, border, label_border, h, w, label_kind;
  int mod[LMN_SLICES_MAX_CHANNELS];
  float bval[LMN_SLICES_MAX_MODALITIES];
};

// The pinned coordinate arithmetic: (m0 x + m1 y) + m2 with every product and sum rounded once.  __fmul_rn / __fadd_rn are plain
// operators inside the runtime's header, which the compiler fuses under its default contraction, so they are written out here, where
// the pragma keeps the contract flag off these operations.
__device__ __forceinline__ float sl_coord(float m0, float m1, float m2, float xf, float yf) {
#pragma clang fp contract(off)
  const float px = m0 * xf;
  const float py = m1 * yf;
  const float s = px + py;
  return s + m2;
}
__device__ __forceinline__ float sl_half_up(float s) {
#pragma clang fp contract(off)
  return s + 0.5f;
}

// blockIdx.y is the sample; a lane owns VEC consecutive x of one output row.  vol == NULL: label-only; lab == NULL: image-only.
template <typename VT, int VEC>
__global__ void __launch_bounds__(256) sl_gather_kernel(const VT* __restrict__ vol, const uint8_t* __restrict__ lab,
                                                        const int32_t* __restrict__ z, const float* __restrict__ params,
                                                        const float* __restrict__ table, SlG g, float* __restrict__ x, void* __restrict__ y) {
  const int wv = g.w / VEC;
  const int item = blockIdx.x * 256 + threadIdx.x;
  if (item >= g.h * wv) return;
  const int oy = item / wv, ox = (item - oy * wv) * VEC, b = blockIdx.y;
  const float* __restrict__ pr = params + 8 * b;
  const float m0 = pr[0], m1 = pr[1], m2 = pr[2], m3 = pr[3], m4 = pr[4], m5 = pr[5], gain = pr[6], bias = pr[7];
  const int zc = min(max(z[b], 0), g.D - 1);
  const bool constant = g.border == LMN_SLICES_BORDER_CONSTANT;
  const int64_t plane = (int64_t)g.Hs * g.Ws;
  // coordinates, weights and tap offsets: once per pixel for every channel
  float fx[VEC], fy[VEC];
  int o00[VEC], o01[VEC], o10[VEC], o11[VEC], ol[VEC];
  unsigned inside[VEC];                                 // bits 0..3: the taps 00 01 10 11, bit 4: the label tap
  const float yf = (float)oy;
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const float xf = (float)(ox + j);
    float sx = sl_coord(m0, m1, m2, xf, yf);
    float sy = sl_coord(m3, m4, m5, xf, yf);
    // far outside (or NaN) is as far as just outside: both taps of an axis leave the frame on the same side either way
    sx = fminf(fmaxf(sx, -2.f), (float)g.Ws + 1.f);
    sy = fminf(fmaxf(sy, -2.f), (float)g.Hs + 1.f);
    const float x0f = floorf(sx), y0f = floorf(sy);
    fx[j] = sx - x0f;
    fy[j] = sy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
    const int lx = (int)floorf(sl_half_up(sx)), ly = (int)floorf(sl_half_up(sy));
    const bool ix0 = x0 >= 0 && x0 < g.Ws, ix1 = x1 >= 0 && x1 < g.Ws, iy0 = y0 >= 0 && y0 < g.Hs, iy1 = y1 >= 0 && y1 < g.Hs;
    const bool il = lx >= 0 && lx < g.Ws && ly >= 0 && ly < g.Hs;
    inside[j] = constant ? ((ix0 && iy0) | (ix1 && iy0) << 1 | (ix0 && iy1) << 2 | (ix1 && iy1) << 3 | il << 4) : 31u;
    const int cx0 = min(max(x0, 0), g.Ws - 1), cx1 = min(max(x1, 0), g.Ws - 1), cy0 = min(max(y0, 0), g.Hs - 1), cy1 = min(max(y1, 0), g.Hs - 1);
    o00[j] = cy0 * g.Ws + cx0;
    o01[j] = cy0 * g.Ws + cx1;
    o10[j] = cy1 * g.Ws + cx0;
    o11[j] = cy1 * g.Ws + cx1;
    ol[j] = min(max(ly, 0), g.Hs - 1) * g.Ws + min(max(lx, 0), g.Ws - 1);
  }
  const int64_t opix = (int64_t)oy * g.w + ox, oplane = (int64_t)g.h * g.w;
  if (vol) {
    const int C = g.S * g.K;
    int s0 = 0;
    for (int m = 0; m < g.M; ++m) {
      int s1 = s0;
      while (s1 < g.S && g.mod[s1] == m) ++s1;          // the specs of modality m: [s0, s1)
      if (s1 == s0) continue;
      const float bv = g.bval[m];
      for (int k = 0; k < g.K; ++k) {
        const int zs = zc + (k - g.ctx) * g.stride;
        const bool zero = g.edge == LMN_SLICES_EDGE_ZERO && (zs < 0 || zs >= g.D);
        const VT* __restrict__ src = vol + ((int64_t)m * g.D + min(max(zs, 0), g.D - 1)) * plane;
        float v[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          if (zero) {
            v[j] = 0.f;
            continue;
          }
          const float v00 = (inside[j] & 1u) ? (float)src[o00[j]] : bv, v01 = (inside[j] & 2u) ? (float)src[o01[j]] : bv;
          const float v10 = (inside[j] & 4u) ? (float)src[o10[j]] : bv, v11 = (inside[j] & 8u) ? (float)src[o11[j]] : bv;
          const float top = fmaf(fx[j], v01 - v00, v00), bot = fmaf(fx[j], v11 - v10, v10);
          v[j] = fmaf(fy[j], bot - top, top);
        }
        for (int s = s0; s < s1; ++s) {
          const float lo = table[4 * s], hi = table[4 * s + 1], a = table[4 * s + 2], bb = table[4 * s + 3];
          float o[VEC];
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            const float u = zero ? 0.f : (fminf(fmaxf(v[j], lo), hi) - a) * bb;
            o[j] = fmaf(u, gain, bias);
          }
          float* __restrict__ dst = x + ((int64_t)b * C + s * g.K + k) * oplane + opix;
          if (VEC == 4) *(float4*)dst = make_float4(o[0], o[1], o[2], o[3]);
          else
#pragma unroll
            for (int j = 0; j < VEC; ++j) dst[j] = o[j];
        }
      }
      s0 = s1;
    }
  }
  if (lab) {
    const uint8_t* __restrict__ src = lab + (int64_t)zc * plane;
    int l[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) l[j] = (inside[j] & 16u) ? (int)src[ol[j]] : g.label_border;
    const int64_t at = (int64_t)b * oplane + opix;
    if (g.label_kind == LMN_SLICES_LABELS_I64) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) ((int64_t*)y)[at + j] = l[j];
    } else if (VEC == 4 && ((uintptr_t)y & 3) == 0) {
      *(uint32_t*)((uint8_t*)y + at) = (uint32_t)l[0] | (uint32_t)l[1] << 8 | (uint32_t)l[2] << 16 | (uint32_t)l[3] << 24;
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) ((uint8_t*)y)[at + j] = (uint8_t)l[j];
    }
  }
}

int sl_check_volume(const char* what, int vol_kind, int M, int D, int Hs, int Ws) {
  LMN_REQUIRE(vol_kind == LMN_SLICES_I16 || vol_kind == LMN_SLICES_U8, "%s: unknown volume kind %d", what, vol_kind);
  LMN_REQUIRE(M >= 1 && M <= LMN_SLICES_MAX_MODALITIES, "%s: M=%d not in [1, %d]", what, M, LMN_SLICES_MAX_MODALITIES);
  LMN_REQUIRE(D >= 1 && D <= LMN_SLICES_MAX_DEPTH, "%s: D=%d not in [1, %d]", what, D, LMN_SLICES_MAX_DEPTH);
  LMN_REQUIRE(Hs >= 2 && Hs <= LMN_SLICES_MAX_SIDE && Ws >= 2 && Ws <= LMN_SLICES_MAX_SIDE, "%s: size %dx%d not in [2, %d]", what, Hs, Ws,
              LMN_SLICES_MAX_SIDE);
  return 0;
}

int sl_check_specs(const char* what, int M, int S, const int32_t* spec_mod) {
  LMN_REQUIRE(S >= 1 && S <= LMN_SLICES_MAX_CHANNELS, "%s: S=%d not in [1, %d]", what, S, LMN_SLICES_MAX_CHANNELS);
  for (int s = 0; s < S; ++s) {
    LMN_REQUIRE(spec_mod[s] >= 0 && spec_mod[s] < M, "%s: spec %d names modality %d of %d", what, s, spec_mod[s], M);
    LMN_REQUIRE(s == 0 || spec_mod[s] >= spec_mod[s - 1], "%s: spec %d: modalities must not decrease", what, s);
  }
  return 0;
}

}  // namespace

extern "C" {

int64_t lmn_slices_workspace(int M, int D, int Hs, int Ws) {
  if (sl_check_volume("slices_workspace", LMN_SLICES_I16, M, D, Hs, Ws)) return -1;
  return sl_ws_bytes(M);
}

int lmn_slices_stats(const void* volume, int vol_kind, int M, int D, int Hs, int Ws, const int32_t* foreground, int q_lo_ppm,
                     int q_hi_ppm, int S, const int32_t* spec_mod, const int32_t* spec_kind, const double* spec_level,
                     const double* spec_width, void* workspace, int64_t ws_bytes, int64_t* stats, float* table, lmn_stream_t stream) {
  LMN_REQUIRE(volume && foreground && spec_mod && spec_kind && spec_level && spec_width && workspace && stats && table,
              "slices_stats: null pointer");
  if (int rc = sl_check_volume("slices_stats", vol_kind, M, D, Hs, Ws)) return rc;
  SlFg fg{};
  for (int m = 0; m < M; ++m) {
    LMN_REQUIRE(foreground[m] >= LMN_SLICES_NO_FOREGROUND && foreground[m] <= 32767, "slices_stats: foreground[%d]=%d not in [%d, 32767]", m,
                foreground[m], LMN_SLICES_NO_FOREGROUND);
    fg.v[m] = foreground[m];
  }
  LMN_REQUIRE(q_lo_ppm >= 0 && q_lo_ppm <= q_hi_ppm && q_hi_ppm <= 1000000, "slices_stats: ranks %d, %d ppm not 0 <= lo <= hi <= 1000000",
              q_lo_ppm, q_hi_ppm);
  if (int rc = sl_check_specs("slices_stats", M, S, spec_mod)) return rc;
  SlFin fin{};
  fin.M = M;
  fin.S = S;
  for (int s = 0; s < S; ++s) {
    LMN_REQUIRE(spec_kind[s] >= LMN_SLICES_WINDOW && spec_kind[s] <= LMN_SLICES_PERCENTILE, "slices_stats: spec %d: unknown kind %d", s,
                spec_kind[s]);
    fin.mod[s] = spec_mod[s];
    fin.kind[s] = spec_kind[s];
    if (spec_kind[s] == LMN_SLICES_WINDOW) {
      const double l = spec_level[s], w = spec_width[s];
      LMN_REQUIRE(l >= -1e9 && l <= 1e9 && w > 0.0 && w <= 1e9, "slices_stats: spec %d: window level=%g, width=%g (|level| <= 1e9, 0 < width <= 1e9)",
                  s, l, w);
      fin.level[s] = l;
      fin.width[s] = w;
    }
  }
  const int64_t need = sl_ws_bytes(M);
  LMN_REQUIRE(ws_bytes >= need, "slices_stats: workspace of %lld bytes too small, %lld needed", (long long)ws_bytes, (long long)need);
  LMN_REQUIRE(((uintptr_t)workspace & 7) == 0, "slices_stats: workspace not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* acc = (unsigned long long*)workspace;
  uint32_t* hist = (uint32_t*)(acc + 8 * M);
  uint32_t* fine = hist + (int64_t)M * SL_COARSE;
  uint32_t* ctrl = fine + (int64_t)M * 2 * SL_FINE;
  const int64_t N = (int64_t)D * Hs * Ws, esize = vol_kind == LMN_SLICES_I16 ? 2 : 1;
  const bool vec = ((uintptr_t)volume & 15) == 0 && (N * esize) % 16 == 0;
  const int64_t nvec = vec ? N * esize / 16 : 0;
  const dim3 grid(loss_grid(vec ? nvec : N, 1024), M);
  LMN_LAUNCH(loss_zero_kernel, dim3(loss_grid(need / 4, 64)), dim3(256), 0, st, (uint32_t*)workspace, need / 4);
#define SL_SCAN(PASS)                                                                                                                  \
  do {                                                                                                                                 \
    if (vol_kind == LMN_SLICES_I16)                                                                                                    \
      LMN_LAUNCH((sl_scan_kernel<int16_t, PASS>), grid, dim3(256), 0, st, (const int16_t*)volume, N, nvec, fg, acc, hist, fine, (const uint32_t*)ctrl); \
    else                                                                                                                               \
      LMN_LAUNCH((sl_scan_kernel<uint8_t, PASS>), grid, dim3(256), 0, st, (const uint8_t*)volume, N, nvec, fg, acc, hist, fine, (const uint32_t*)ctrl); \
  } while (0)
  SL_SCAN(1);
  LMN_LAUNCH(sl_step_kernel, dim3(M), dim3(64), 0, st, (const unsigned long long*)acc, (const uint32_t*)hist, ctrl, q_lo_ppm, q_hi_ppm);
  SL_SCAN(2);
#undef SL_SCAN
  LMN_LAUNCH(sl_finish_kernel, dim3(1), dim3(64), 0, st, fin, (const unsigned long long*)acc, (const uint32_t*)fine, (const uint32_t*)ctrl, stats,
             table);
  return lmn_launch_status("slices_stats");
}

int lmn_slices_gather(const void* volume, int vol_kind, const uint8_t* labels, int M, int D, int Hs, int Ws, const int32_t* z,
                      const float* params, int n, const float* table, int S, const int32_t* spec_mod, int context, int stride, int edge,
                      int border, const float* border_value, int label_border, int h, int w, float* x, void* y, int label_kind,
                      lmn_stream_t stream) {
  LMN_REQUIRE(z && params, "slices_gather: null pointer");
  LMN_REQUIRE(volume || labels, "slices_gather: neither a volume nor labels");
  LMN_REQUIRE(!volume == !x && !labels == !y, "slices_gather: a volume needs x and labels need y, and the other way round");
  LMN_REQUIRE(!volume || (table && spec_mod && border_value), "slices_gather: null pointer");
  if (int rc = sl_check_volume("slices_gather", vol_kind, M, D, Hs, Ws)) return rc;
  LMN_REQUIRE(n >= 1 && n <= LMN_SLICES_MAX_BATCH, "slices_gather: n=%d not in [1, %d]", n, LMN_SLICES_MAX_BATCH);
  LMN_REQUIRE(h >= 1 && h <= LMN_SLICES_MAX_OUT && w >= 1 && w <= LMN_SLICES_MAX_OUT, "slices_gather: output size %dx%d not in [1, %d]", h, w,
              LMN_SLICES_MAX_OUT);
  LMN_REQUIRE(context >= 0 && context <= LMN_SLICES_MAX_CONTEXT, "slices_gather: context=%d not in [0, %d]", context, LMN_SLICES_MAX_CONTEXT);
  LMN_REQUIRE(stride >= 1 && stride <= LMN_SLICES_MAX_DEPTH, "slices_gather: stride=%d not in [1, %d]", stride, LMN_SLICES_MAX_DEPTH);
  LMN_REQUIRE(edge == LMN_SLICES_EDGE_REPLICATE || edge == LMN_SLICES_EDGE_ZERO, "slices_gather: unknown edge %d", edge);
  LMN_REQUIRE(border == LMN_SLICES_BORDER_REPLICATE || border == LMN_SLICES_BORDER_CONSTANT, "slices_gather: unknown border %d", border);
  LMN_REQUIRE(label_border >= 0 && label_border <= 255, "slices_gather: label_border=%d not in [0, 255]", label_border);
  LMN_REQUIRE(label_kind == LMN_SLICES_LABELS_U8 || label_kind == LMN_SLICES_LABELS_I64, "slices_gather: unknown label kind %d", label_kind);
  SlG g{};
  const int K = 2 * context + 1;
  if (volume) {
    if (int rc = sl_check_specs("slices_gather", M, S, spec_mod)) return rc;
    LMN_REQUIRE(S * K <= LMN_SLICES_MAX_CHANNELS, "slices_gather: %d specs x %d slices = %d channels, above %d", S, K, S * K,
                LMN_SLICES_MAX_CHANNELS);
    for (int s = 0; s < S; ++s) g.mod[s] = spec_mod[s];
    for (int m = 0; m < M; ++m) {
      LMN_REQUIRE(border_value[m] >= -65536.f && border_value[m] <= 65536.f, "slices_gather: border_value[%d]=%g not in [-65536, 65536]", m,
                  (double)border_value[m]);
      g.bval[m] = border_value[m];
    }
    g.S = S;
  }
  g.M = M; g.D = D; g.Hs = Hs; g.Ws = Ws; g.K = K; g.ctx = context; g.stride = stride; g.edge = edge; g.border = border;
  g.label_border = label_border; g.h = h; g.w = w; g.label_kind = label_kind;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = w % 4 == 0 && ((uintptr_t)x & 15) == 0;
  const dim3 grid((unsigned)(((int64_t)h * (vec ? w / 4 : w) + 255) / 256), n);
#define SL_GATHER(VT)                                                                                                              \
  do {                                                                                                                             \
    if (vec) LMN_LAUNCH((sl_gather_kernel<VT, 4>), grid, dim3(256), 0, st, (const VT*)volume, labels, z, params, table, g, x, y);  \
    else LMN_LAUNCH((sl_gather_kernel<VT, 1>), grid, dim3(256), 0, st, (const VT*)volume, labels, z, params, table, g, x, y);      \
  } while (0)
  if (vol_kind == LMN_SLICES_I16) SL_GATHER(int16_t);
  else SL_GATHER(uint8_t);
#undef SL_GATHER
  return lmn_launch_status("slices_gather");
}

}  // extern "C"

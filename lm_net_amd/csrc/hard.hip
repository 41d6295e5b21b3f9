// Hard pixels (include/hard/lmnet_hard.h): the mean of the K largest per-element cross entropies of a group, K formed on the device,
// the K-th largest value found by an exact radix select over the raw bits of the (non-negative) fp32 values: 11 + 11 + 10 bits.
//   values pass   hp_softmax_values_kernel<CT> (CT in {2, 3, 4, 8}: the pixel's logits in registers; CT = 0: any other C, the logits
//                 are read twice, for the maximum and for the sum, the second time from the cache; 256 lanes, blockIdx.y is the
//                 image) and hp_sigmoid_values_kernel<VEC> (blockIdx.y the class, blockIdx.z the image).  Writes the
//                 value of every element (-1 at a void one), counts Nhard and adds the level-1 histogram of its group (N is the
//                 histogram's total).
//   levels        hp_level_kernel<LEVEL, VEC> over the values alone, blockIdx.y the group: LEVEL 2 and 3 rescan the previous tables
//                 (hp_select) and histogram the next digit of the elements that match the prefix; LEVEL 4 is the sum pass, which
//                 knows tau, writes its block's sum of the values above tau to a slot and (block 0 of a group) the selection record.
//   finish        hp_finish_kernel: one block, the slots of a group in block order in fp64, the terms and the loss.
//   backward      hp_softmax_bwd_kernel<CT> (CT = 0: one wave per block, every lane stages its pixel's logits in an LDS column of its
//                 own, [C][64], so no barrier), hp_sigmoid_bwd_kernel<VEC>: pointwise, classify by the saved value.
// workspace: uint32 hist1 [G][R][2048], hist2 [G][2048], hist3 [G][1024], int32 cnt [G][16] (one zero fill), then fp64 slots [G][nbx].
// Thousands of atomics on ONE word cost tens of microseconds (about 90 per microsecond and word): the first version counted N and
// Nhard per wave on two words and its values pass took 53 us at 8 x 352 x 352.  So N is the total of hist1, Nhard is kept
// in 16 partial counts (one atomic per block, on the count of its index), and hist1, whose few hot bins every block of the values pass
// flushes to, exists in R = hp_replicas(G) copies that hp_select adds.
#include "loss_common.h"
#include "../../include/hard/lmnet_hard.h"
static_assert(LMN_HARD_LABELS_U8 == LOSS_LABELS_U8 && LMN_HARD_LABELS_I64 == LOSS_LABELS_I64 && LMN_HARD_SOFTMAX == LOSS_SOFTMAX &&
              LMN_HARD_SIGMOID == LOSS_SIGMOID, "loss_common.h reads the label kinds and heads of lmnet_hard.h");

namespace {

constexpr int HP_HI = LMN_HARD_BINS_HIGH, HP_LO = LMN_HARD_BINS_LOW;
constexpr int HP_NCNT = 16;                                   // partial counts of Nhard per group
// copies of a group's first histogram: up to 8, fewer where many groups share the zero fill
inline int hp_replicas(int G) { return G <= 8 ? 8 : G <= 16 ? 4 : G <= 32 ? 2 : 1; }
inline int64_t hp_group_words(int G) { return (int64_t)(hp_replicas(G) + 1) * HP_HI + HP_LO + HP_NCNT; }   // zero-filled words of a group
static_assert(HP_HI == 2048 && HP_LO == 1024, "the key is split 11 + 11 + 10 bits");

struct HpArgs {
  const float* logits;
  const void* target;
  const float* weight;
  int kind, C, per_image, use_cut;
  int64_t hw;
  float cut;
};

// the tables of the workspace
struct HpWs {
  uint32_t* hist1;
  uint32_t* hist2;
  uint32_t* hist3;
  int32_t* cnt;
  double* slots;
  int rep;              // copies of hist1 per group (a power of two)
};

// how K is formed
struct HpK {
  float keep;
  int64_t min_kept;
};

// THE value routines.  No contraction: the same element gets the same bits from every instance.  The result is clamped to >= +0
// (a NaN, which finite logits and weights cannot produce, would also become 0), so its bits order as the values do.
__device__ __forceinline__ float hp_clamp(float l) { return l > 0.f ? l : 0.f; }
__device__ __forceinline__ float hp_softmax_value(float w, float mx, float den, float zy) {
#pragma clang fp contract(off)
  const float d = mx - zy;              // >= 0
  const float l = d + logf(den);        // den >= 1
  return hp_clamp(w * l);
}
__device__ __forceinline__ float hp_sigmoid_value(float w, float z, bool t) {
#pragma clang fp contract(off)
  const SigPoint s = sig_point(z);
  return hp_clamp(w * (t ? s.sp_neg : s.sp_pos));
}

// what the values pass of a block adds to its group's tables: the LDS histogram's non-zero bins, and Nhard by one atomic per block
template <int NT>
__device__ __forceinline__ void hp_flush_values(const uint32_t* s_hist, unsigned nh, unsigned block, const HpWs& w, int g) {
  uint32_t* hist1 = w.hist1 + ((int64_t)g * w.rep + (block & (unsigned)(w.rep - 1))) * HP_HI;
  int32_t* cnt = w.cnt + HP_NCNT * g;
  __shared__ unsigned s_nh[NT / 64];
  nh = loss_wave_sum(nh);
  if ((threadIdx.x & 63) == 0) s_nh[threadIdx.x >> 6] = nh;
  __syncthreads();
  for (int k = threadIdx.x; k < HP_HI; k += NT) {
    const uint32_t v = s_hist[k];
    if (v) atomicAdd(hist1 + k, v);
  }
  if (threadIdx.x == 0) {
    unsigned v = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) v += s_nh[i];
    if (v) atomicAdd(cnt + (block & (HP_NCNT - 1)), (int32_t)v);
  }
}

template <int CT>
__global__ __launch_bounds__(256) void hp_softmax_values_kernel(HpArgs a, HpWs w, float* __restrict__ values) {
  constexpr int NT = 256, UNR = CT > 0 ? CT : 4;
  __shared__ uint32_t s_hist[HP_HI];
  const int C = CT > 0 ? CT : a.C, b = blockIdx.y, g = a.per_image ? b : 0;
  for (int k = threadIdx.x; k < HP_HI; k += NT) s_hist[k] = 0u;
  __syncthreads();
  const float* lg = a.logits + (int64_t)b * C * a.hw;
  unsigned nh = 0;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < a.hw; i += (int64_t)gridDim.x * NT) {
    const int64_t pix = (int64_t)b * a.hw + i;
    const int64_t y = loss_label(a.target, a.kind, pix);
    const bool valid = (uint64_t)y < (uint64_t)C;
    float zr[CT > 0 ? CT : 1];
    float mx = -3.0e38f, zy = 0.f;
#pragma unroll UNR
    for (int c = 0; c < (CT > 0 ? CT : C); ++c) {
      const float z = lg[c * a.hw + i];
      if constexpr (CT > 0) zr[c] = z;
      mx = fmaxf(mx, z);
      zy = (int64_t)c == y ? z : zy;
    }
    float den = 0.f;
#pragma unroll UNR
    for (int c = 0; c < (CT > 0 ? CT : C); ++c) {
      float z;
      if constexpr (CT > 0) z = zr[c];
      else z = lg[c * a.hw + i];                       // (the second read: from the cache)
      den += expf(z - mx);
    }
    float v = -1.f;
    if (valid) {
      v = hp_softmax_value(a.weight ? a.weight[y] : 1.f, mx, den, zy);
      atomicAdd(&s_hist[__float_as_uint(v) >> 21], 1u);
      nh += (a.use_cut && v > a.cut) ? 1u : 0u;
    }
    values[pix] = v;
  }
  hp_flush_values<256>(s_hist, nh, blockIdx.x, w, g);
}

template <bool VEC>
__global__ __launch_bounds__(256) void hp_sigmoid_values_kernel(HpArgs a, HpWs w, float* __restrict__ values) {
  constexpr int E = VEC ? 4 : 1;
  __shared__ uint32_t s_hist[HP_HI];
  const int c = blockIdx.y, b = blockIdx.z, g = a.per_image ? b : 0;
  for (int k = threadIdx.x; k < HP_HI; k += 256) s_hist[k] = 0u;
  __syncthreads();
  const int64_t plane = ((int64_t)b * a.C + c) * a.hw;
  const float* lg = a.logits + plane;
  float* vo = values + plane;
  const float wc = a.weight ? a.weight[c] : 1.f;
  unsigned nh = 0;
  const int64_t items = a.hw / E;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < items; q += (int64_t)gridDim.x * 256) {
    float z[E], v[E];
    loss_load_z<E>(lg, q * E, z);
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const uint64_t t = (uint64_t)loss_label(a.target, a.kind, plane + q * E + j);
      v[j] = -1.f;
      if (t <= 1ull) {
        v[j] = hp_sigmoid_value(wc, z[j], t == 1ull);
        atomicAdd(&s_hist[__float_as_uint(v[j]) >> 21], 1u);
        nh += (a.use_cut && v[j] > a.cut) ? 1u : 0u;
      }
    }
    loss_store<E>(vo, q * E, v);
  }
  hp_flush_values<256>(s_hist, nh, blockIdx.x + gridDim.x * blockIdx.y, w, g);
}

// K = min(N, max(1, Kkeep, min_kept, Nhard)); 0 when N = 0
__device__ __forceinline__ uint32_t hp_count(uint32_t N, uint32_t nhard, HpK k) {
  if (N == 0u) return 0u;
  uint64_t K = 1;
  const uint64_t kk = (uint64_t)floor((double)k.keep * (double)N);
  K = kk > K ? kk : K;
  K = (uint64_t)k.min_kept > K ? (uint64_t)k.min_kept : K;
  K = (uint64_t)nhard > K ? (uint64_t)nhard : K;
  return (uint32_t)(K < (uint64_t)N ? K : (uint64_t)N);
}

// A table of 256 * PER bins in the registers of a block: thread t owns the bins [t PER, (t + 1) PER).  All 256 threads call both.
//   scan   a suffix scan over the 256 partial sums in LDS -> the table's total
//   find   the digit d with above(d) < k <= above(d) + hist[d], above(d) = sum_{j > d} hist[j]: s_out = {d, above(d), hist[d]}.  Needs
//          1 <= k <= total: the owning thread walks its bins downwards.
template <int PER>
struct HpTable {
  uint32_t h[PER], tot;
  // copies: the table is the sum of that many tables in a row
  __device__ __forceinline__ uint32_t scan(const uint32_t* __restrict__ hist, uint32_t* s_scan, int copies = 1) {
    const int t = threadIdx.x;
    tot = 0u;
#pragma unroll
    for (int j = 0; j < PER; ++j) h[j] = 0u;
    for (int r = 0; r < copies; ++r) {
#pragma unroll
      for (int j = 0; j < PER; ++j) h[j] += hist[(int64_t)r * 256 * PER + t * PER + j];
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) tot += h[j];
    __syncthreads();                                   // (s_scan and s_out of the previous table have been read)
    s_scan[t] = tot;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const uint32_t v = t + off < 256 ? s_scan[t + off] : 0u;
      __syncthreads();
      s_scan[t] += v;
      __syncthreads();
    }
    return s_scan[0];
  }
  __device__ __forceinline__ void find(uint32_t k, const uint32_t* s_scan, uint32_t* s_out) const {
    const int t = threadIdx.x;
    uint32_t above = s_scan[t] - tot;
    if (above < k && k <= above + tot) {
#pragma unroll
      for (int j = PER - 1; j >= 0; --j) {
        if (k <= above + h[j]) {
          s_out[0] = (uint32_t)(t * PER + j);
          s_out[1] = above;
          s_out[2] = h[j];
          break;
        }
        above += h[j];
      }
    }
    __syncthreads();
  }
};

struct HpSel {
  uint32_t N, K, prefix, rank, n_gt, n_eq;   // prefix: the digits fixed so far; rank: the rank of tau among the elements that match it
};

// the first LEVELS digits of tau for group g, from the tables the earlier passes completed; N is the total of the first table
template <int LEVELS>
__device__ __forceinline__ HpSel hp_select(const HpWs& w, HpK k, int g, uint32_t* s_scan, uint32_t* s_out) {
  HpSel s;
  uint32_t nhard = 0u;
#pragma unroll
  for (int i = 0; i < HP_NCNT; ++i) nhard += (uint32_t)w.cnt[HP_NCNT * g + i];
  HpTable<HP_HI / 256> t1;
  s.N = t1.scan(w.hist1 + (int64_t)g * w.rep * HP_HI, s_scan, w.rep);
  s.K = hp_count(s.N, nhard, k);
  s.prefix = 0u; s.rank = s.K; s.n_gt = 0u; s.n_eq = 0u;
  if (s.K == 0u) return s;                             // (block-uniform)
  t1.find(s.rank, s_scan, s_out);
  s.prefix = s_out[0]; s.n_gt += s_out[1]; s.rank -= s_out[1]; s.n_eq = s_out[2];
  if constexpr (LEVELS >= 2) {
    HpTable<HP_HI / 256> t2;
    t2.scan(w.hist2 + (int64_t)g * HP_HI, s_scan);
    t2.find(s.rank, s_scan, s_out);
    s.prefix = (s.prefix << 11) | s_out[0]; s.n_gt += s_out[1]; s.rank -= s_out[1]; s.n_eq = s_out[2];
  }
  if constexpr (LEVELS >= 3) {
    HpTable<HP_LO / 256> t3;
    t3.scan(w.hist3 + (int64_t)g * HP_LO, s_scan);
    t3.find(s.rank, s_scan, s_out);
    s.prefix = (s.prefix << 10) | s_out[0]; s.n_gt += s_out[1]; s.rank -= s_out[1]; s.n_eq = s_out[2];
  }
  return s;
}

// LEVEL 2, 3: the next histogram of the elements that match the prefix.  LEVEL 4: the sum pass.  M: elements of a group.
template <int LEVEL, bool VEC>
__global__ __launch_bounds__(256) void hp_level_kernel(HpWs w, HpK k, const float* __restrict__ values, int64_t M,
                                                       int32_t* __restrict__ selection) {
  constexpr int E = VEC ? 4 : 1, NB = LEVEL == 2 ? HP_HI : HP_LO;
  __shared__ uint32_t s_hist[LEVEL == 4 ? 1 : NB];
  __shared__ uint32_t s_scan[256], s_out[3];
  __shared__ double s_red[4];
  const int g = blockIdx.y;
  const HpSel s = hp_select<LEVEL - 1>(w, k, g, s_scan, s_out);
  const float* vals = values + (int64_t)g * M;
  const int64_t items = M / E;
  if constexpr (LEVEL == 4) {
    double acc = 0.0;
    if (s.K != 0u) {
      for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < items; q += (int64_t)gridDim.x * 256) {
        float v[E];
        loss_load_z<E>(vals, q * E, v);
#pragma unroll
        for (int j = 0; j < E; ++j)
          if (v[j] >= 0.f && __float_as_uint(v[j]) > s.prefix) acc += (double)v[j];
      }
    }
    acc = loss_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      w.slots[(int64_t)g * gridDim.x + blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
      if (blockIdx.x == 0) {
        int32_t* rec = selection + LMN_HARD_RECORD_WORDS * g;
        rec[0] = (int32_t)s.N; rec[1] = (int32_t)s.K; rec[2] = (int32_t)s.n_gt; rec[3] = (int32_t)s.n_eq; rec[4] = (int32_t)s.prefix;
      }
    }
  } else {
    if (s.K == 0u) return;                             // (block-uniform: nothing to select in an empty group)
    for (int i = threadIdx.x; i < NB; i += 256) s_hist[i] = 0u;
    __syncthreads();
    constexpr int SHIFT = LEVEL == 2 ? 21 : 10;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < items; q += (int64_t)gridDim.x * 256) {
      float v[E];
      loss_load_z<E>(vals, q * E, v);
#pragma unroll
      for (int j = 0; j < E; ++j) {
        const uint32_t bits = __float_as_uint(v[j]);
        if (v[j] >= 0.f && (bits >> SHIFT) == s.prefix) atomicAdd(&s_hist[LEVEL == 2 ? (bits >> 10) & 2047u : bits & 1023u], 1u);
      }
    }
    __syncthreads();
    uint32_t* out = LEVEL == 2 ? w.hist2 + (int64_t)g * HP_HI : w.hist3 + (int64_t)g * HP_LO;
    for (int i = threadIdx.x; i < NB; i += 256) {
      const uint32_t v = s_hist[i];
      if (v) atomicAdd(out + i, v);
    }
  }
}

// One block: wave v takes the groups v, v + 4, ...; its lanes add the group's slots lane, lane + 64, ... in order and the 64 partials
// meet in a fixed butterfly.  Then the terms, and thread 0 adds them in group order.
__global__ __launch_bounds__(256) void hp_finish_kernel(const double* __restrict__ slots, int G, int nbx, float scale,
                                                        const int32_t* __restrict__ selection, float* __restrict__ terms,
                                                        float* __restrict__ loss) {
  __shared__ double s_term[LMN_HARD_MAX_GROUPS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int g = wv; g < G; g += 4) {
    double v = 0.0;
    for (int j = lane; j < nbx; j += 64) v += slots[(int64_t)g * nbx + j];
    v = loss_wave_sum(v);
    if (lane == 0) {
      const int32_t* rec = selection + LMN_HARD_RECORD_WORDS * g;
      const double K = (double)rec[1], rest = (double)(rec[1] - rec[2]), tau = (double)__int_as_float(rec[4]);
      const double t = rec[1] > 0 ? (v + rest * tau) / K : 0.0;
      s_term[g] = t;
      terms[g] = (float)t;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = 0.0;
    for (int g = 0; g < G; ++g) sum += s_term[g];
    loss[0] = (float)((double)scale * sum / (double)G);
  }
}

// the two gradient weights of a group, times gscale * scale / G: {where l > tau, where l == tau, tau}
struct HpCoef { float gt, eq, tau; };
__device__ __forceinline__ HpCoef hp_coef(const int32_t* __restrict__ selection, int g, int G, float scale, const float* __restrict__ gscale) {
  const int32_t* rec = selection + LMN_HARD_RECORD_WORDS * g;
  const double K = (double)rec[1], f = (double)(gscale ? gscale[0] : 1.f) * (double)scale / (double)G;
  HpCoef c;
  c.gt = rec[1] > 0 ? (float)(f / K) : 0.f;
  c.eq = rec[1] > 0 && rec[3] > 0 ? (float)(f * (double)(rec[1] - rec[2]) / ((double)rec[3] * K)) : 0.f;
  c.tau = __int_as_float(rec[4]);
  return c;
}
// the factor of an element with saved value v; sel: it has one (else the gradient is +0, whatever the factor's sign)
__device__ __forceinline__ float hp_factor(const HpCoef& c, float v, bool& sel) {
  sel = v >= c.tau && v >= 0.f;
  return v > c.tau ? c.gt : c.eq;
}

template <int CT>
__global__ __launch_bounds__(CT > 0 ? 256 : 64) void hp_softmax_bwd_kernel(HpArgs a, const float* __restrict__ values,
                                                                           const int32_t* __restrict__ selection, int G, float scale,
                                                                           const float* __restrict__ gscale, float* __restrict__ dlogits) {
  constexpr int NT = CT > 0 ? 256 : 64, UNR = CT > 0 ? CT : 1;
  extern __shared__ float hp_lds[];
  const int C = CT > 0 ? CT : a.C, b = blockIdx.y, g = a.per_image ? b : 0;
  const HpCoef co = hp_coef(selection, g, G, scale, gscale);
  float* zs = hp_lds + (threadIdx.x & 63);
  const float* lg = a.logits + (int64_t)b * C * a.hw;
  float* dl = dlogits + (int64_t)b * C * a.hw;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < a.hw; i += (int64_t)gridDim.x * NT) {
    const int64_t pix = (int64_t)b * a.hw + i;
    bool sel;
    const float f = hp_factor(co, values[pix], sel);
    if (!sel) {                                        // void or not selected: +0 in every class
#pragma unroll UNR
      for (int c = 0; c < (CT > 0 ? CT : C); ++c) dl[c * a.hw + i] = 0.f;
      continue;
    }
    const int64_t y = loss_label(a.target, a.kind, pix);   // (selected: the label lies in [0, C))
    float zr[CT > 0 ? CT : 1];
    float mx = -3.0e38f;
#pragma unroll UNR
    for (int c = 0; c < (CT > 0 ? CT : C); ++c) {
      const float z = lg[c * a.hw + i];
      if constexpr (CT > 0) zr[c] = z;
      else zs[c * 64] = z;
      mx = fmaxf(mx, z);
    }
    float den = 0.f;
#pragma unroll UNR
    for (int c = 0; c < (CT > 0 ? CT : C); ++c) {
      float z;
      if constexpr (CT > 0) z = zr[c];
      else z = zs[c * 64];
      den += expf(z - mx);
    }
    const float fw = f * (a.weight ? a.weight[y] : 1.f), rden = 1.f / den;
#pragma unroll UNR
    for (int c = 0; c < (CT > 0 ? CT : C); ++c) {
      float z;
      if constexpr (CT > 0) z = zr[c];
      else z = zs[c * 64];
      const float p = expf(z - mx) * rden;
      dl[c * a.hw + i] = fw * (p - ((int64_t)c == y ? 1.f : 0.f));
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void hp_sigmoid_bwd_kernel(HpArgs a, const float* __restrict__ values, const int32_t* __restrict__ selection,
                                                             int G, float scale, const float* __restrict__ gscale, float* __restrict__ dlogits) {
  constexpr int E = VEC ? 4 : 1;
  const int c = blockIdx.y, b = blockIdx.z, g = a.per_image ? b : 0;
  const HpCoef co = hp_coef(selection, g, G, scale, gscale);
  const int64_t plane = ((int64_t)b * a.C + c) * a.hw;
  const float* lg = a.logits + plane;
  const float* vs = values + plane;
  float* dl = dlogits + plane;
  const float wc = a.weight ? a.weight[c] : 1.f;
  const int64_t items = a.hw / E;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < items; q += (int64_t)gridDim.x * 256) {
    float z[E], v[E], d[E];
    loss_load_z<E>(lg, q * E, z);
    loss_load_z<E>(vs, q * E, v);
#pragma unroll
    for (int j = 0; j < E; ++j) {
      bool sel;
      const float f = hp_factor(co, v[j], sel);
      d[j] = 0.f;                                      // void or not selected: +0
      if (sel) {
        const bool t = loss_label(a.target, a.kind, plane + q * E + j) == 1;
        const SigPoint s = sig_point(z[j]);
        d[j] = f * wc * (t ? -s.omp : s.p);            // sigmoid(z) - t, without cancellation
      }
    }
    loss_store<E>(dl, q * E, d);
  }
}

inline int hp_groups(int per_image, int B) { return per_image ? B : 1; }
// elements of a group in the values buffer
inline int64_t hp_group_elems(int head, int per_image, int B, int C, int64_t HW) {
  return (per_image ? 1 : (int64_t)B) * (head == LMN_HARD_SIGMOID ? C : 1) * HW;
}
// blocks per group of the level and sum passes: a function of the geometry alone, so that lmn_hard_workspace states the slots exactly
// (with an unaligned base the one-element instance runs on the same grid: its loop strides)
inline int hp_nbx(int G, int64_t M) { return loss_grid_per(M % 4 == 0 ? M / 4 : M, 1024, G); }
inline int64_t hp_tables_bytes(int G) { return lmn_up256((int64_t)4 * G * hp_group_words(G)); }
inline int64_t hp_ws_bytes(int head, int per_image, int B, int C, int64_t HW) {
  const int G = hp_groups(per_image, B);
  return hp_tables_bytes(G) + lmn_up256((int64_t)8 * G * hp_nbx(G, hp_group_elems(head, per_image, B, C, HW)));
}

int hp_check(const char* what, int head, int per_image, int label_kind, int B, int C, int H, int W) {
  LMN_REQUIRE(head == LMN_HARD_SOFTMAX || head == LMN_HARD_SIGMOID, "%s: unknown head %d", what, head);
  LMN_REQUIRE(per_image == 0 || per_image == 1, "%s: per_image=%d is neither 0 nor 1", what, per_image);
  LMN_REQUIRE(B >= 1 && B <= LMN_HARD_MAX_BATCH, "%s: B=%d not in [1, %d]", what, B, LMN_HARD_MAX_BATCH);
  LMN_REQUIRE(!per_image || B <= LMN_HARD_MAX_GROUPS, "%s: per_image: B=%d groups above the limit %d", what, B, LMN_HARD_MAX_GROUPS);
  if (int rc = loss_check_head(what, C, head == LMN_HARD_SOFTMAX, 1ull, label_kind)) return rc;
  return loss_check_extent(what, B, C, H, W);
}

}  // namespace

extern "C" {

int64_t lmn_hard_workspace(int head, int per_image, int B, int C, int H, int W) {
  if (hp_check("hard_workspace", head, per_image, LMN_HARD_LABELS_U8, B, C, H, W)) return -1;
  return hp_ws_bytes(head, per_image, B, C, (int64_t)H * W);
}

int lmn_hard_fwd(const float* logits, const void* target, int label_kind, int head, int per_image, float keep, int64_t min_kept,
                 float cut, float scale, int B, int C, int H, int W, const float* weight, void* workspace, int64_t ws_bytes,
                 float* values, int32_t* selection, float* terms, float* loss, lmn_stream_t stream) {
  LMN_REQUIRE(logits && target && workspace && values && selection && terms && loss, "hard_fwd: null pointer");
  if (int rc = hp_check("hard_fwd", head, per_image, label_kind, B, C, H, W)) return rc;
  LMN_REQUIRE(keep >= 0.f && keep <= 1.f, "hard_fwd: keep=%g not in [0, 1]", (double)keep);
  LMN_REQUIRE(min_kept >= 0, "hard_fwd: min_kept=%lld is negative", (long long)min_kept);
  LMN_REQUIRE(cut < 0.f || loss_finite(cut), "hard_fwd: cut=%g is not finite", (double)cut);
  LMN_REQUIRE(keep > 0.f || min_kept > 0 || cut >= 0.f, "hard_fwd: none of keep, min_kept and cut is given");
  LMN_REQUIRE(loss_finite(scale), "hard_fwd: scale=%g is not finite", (double)scale);
  const int64_t HW = (int64_t)H * W, need = hp_ws_bytes(head, per_image, B, C, HW);
  LMN_REQUIRE(ws_bytes >= need, "hard_fwd: workspace of %lld bytes too small, %lld needed", (long long)ws_bytes, (long long)need);
  LMN_REQUIRE(lmn_aligned(workspace, 8), "hard_fwd: the workspace is not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int G = hp_groups(per_image, B);
  const int64_t M = hp_group_elems(head, per_image, B, C, HW);
  const int nbx = hp_nbx(G, M);
  uint32_t* tab = (uint32_t*)workspace;
  const int R = hp_replicas(G);
  uint32_t* hist2 = tab + (int64_t)G * R * HP_HI;
  const HpWs w{tab, hist2, hist2 + (int64_t)G * HP_HI, (int32_t*)(hist2 + (int64_t)G * (HP_HI + HP_LO)),
               (double*)((char*)workspace + hp_tables_bytes(G)), R};
  const HpArgs a{logits, target, weight, label_kind, C, per_image, cut >= 0.f ? 1 : 0, HW, cut};
  const HpK k{keep, min_kept};
  const int64_t words = (int64_t)G * hp_group_words(G);
  LMN_LAUNCH(loss_zero_kernel, dim3(loss_grid(words, 256)), dim3(256), 0, st, tab, words);
  if (head == LMN_HARD_SOFTMAX) {
    const dim3 grid(loss_grid_per(HW, 1024, B), B);
    LOSS_SWITCH_CT(C, LMN_LAUNCH((hp_softmax_values_kernel<CT>), grid, dim3(256), 0, st, a, w, values));
  } else {
    const bool vec = HW % 4 == 0 && lmn_aligned(logits, 16) && lmn_aligned(values, 16);
    const dim3 grid(loss_grid_per(HW % 4 == 0 ? HW / 4 : HW, 2048, (int64_t)B * C), C, B);
    LOSS_SWITCH_BOOL(VEC, vec, LMN_LAUNCH((hp_sigmoid_values_kernel<VEC>), grid, dim3(256), 0, st, a, w, values));
  }
  const bool vec = M % 4 == 0 && lmn_aligned(values, 16);
  const dim3 grid(nbx, G);
  LOSS_SWITCH_BOOL(VEC, vec, {
    LMN_LAUNCH((hp_level_kernel<2, VEC>), grid, dim3(256), 0, st, w, k, (const float*)values, M, selection);
    LMN_LAUNCH((hp_level_kernel<3, VEC>), grid, dim3(256), 0, st, w, k, (const float*)values, M, selection);
    LMN_LAUNCH((hp_level_kernel<4, VEC>), grid, dim3(256), 0, st, w, k, (const float*)values, M, selection);
  });
  LMN_LAUNCH(hp_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)w.slots, G, nbx, scale, (const int32_t*)selection, terms, loss);
  return lmn_launch_status("hard_fwd");
}

int lmn_hard_bwd(const float* logits, const void* target, int label_kind, int head, int per_image, float scale, int B, int C, int H,
                 int W, const float* weight, const float* values, const int32_t* selection, const float* gscale, float* dlogits,
                 lmn_stream_t stream) {
  LMN_REQUIRE(logits && target && values && selection && dlogits, "hard_bwd: null pointer");
  if (int rc = hp_check("hard_bwd", head, per_image, label_kind, B, C, H, W)) return rc;
  LMN_REQUIRE(loss_finite(scale), "hard_bwd: scale=%g is not finite", (double)scale);
  hipStream_t st = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  const int G = hp_groups(per_image, B);
  const HpArgs a{logits, target, weight, label_kind, C, per_image, 0, HW, 0.f};
  if (head == LMN_HARD_SOFTMAX) {
    const int64_t cap = loss_cap(4096, B);
    const dim3 grid(loss_templated(C) ? loss_grid(HW, cap) : loss_grid(HW * 4, cap * 4), B);
    LOSS_SWITCH_CT(C, LMN_LAUNCH((hp_softmax_bwd_kernel<CT>), grid, dim3(CT > 0 ? 256 : 64), CT > 0 ? 0 : (size_t)C * 64 * 4, st, a, values,
                             selection, G, scale, gscale, dlogits));
  } else {
    const bool vec = HW % 4 == 0 && lmn_aligned(logits, 16) && lmn_aligned(values, 16) && lmn_aligned(dlogits, 16);
    const dim3 grid(loss_grid_per(vec ? HW / 4 : HW, 4096, (int64_t)B * C), C, B);
    LOSS_SWITCH_BOOL(VEC, vec, LMN_LAUNCH((hp_sigmoid_bwd_kernel<VEC>), grid, dim3(256), 0, st, a, values, selection, G, scale, gscale, dlogits));
  }
  return lmn_launch_status("hard_bwd");
}

}  // extern "C"

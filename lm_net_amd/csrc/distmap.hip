// Dense signed squared Euclidean distance maps of label masks, and the boundary and Hausdorff losses on them (include/distmap/
// lmnet_distmap.h; lm_net_amd.loss.distance_maps, BoundaryLoss, HausdorffDTLoss).  The transform is the exact integer EDT of
// surface.hip (surf_col_kernel + surf_row_kernel) made dense: there it is evaluated at the border pixels of the other mask, here at
// every pixel, against the pixels of OPPOSITE membership.
//
//   1. dm_mask_*_kernel   the masks of the scored classes, uint8 [B * nk, H, W]: label == k, or the thresholded softmax / sigmoid.
//   2. dm_col_kernel      per plane, one lane per column and DM_SEG row segments per block: a segment's rows (<= 64) become one bit
//                         mask, so the nearest row of opposite membership above / below any row of the segment is a clz / ffs; the
//                         nearest one outside the segment comes from the other segments through LDS.  Writes g(y, x), the vertical
//                         distance to the nearest pixel of opposite membership in the column (uint16, DM_INF where the column has
//                         none), and adds |M| to the plane's count with one integer atomic per block.
//   3. dm_row_kernel      per (plane, row): g_in^2 (distance to the mask: 0 inside it) and g_out^2 (distance to the complement: 0
//                         outside the mask) of the row in LDS; a pixel takes min_j (x - j)^2 + g^2(y, j) over the array opposite to
//                         its own membership, scanning outwards from x and stopping once d^2 >= the best so far (exact: every later
//                         term is >= d^2).  AT MOST W - 1 STEPS PER PIXEL.  A plane whose count is 0 or H * W is flagged and all 0.
//   4. dl_*_kernel        the losses: per-pixel (softmax head: C in {2, 3, 4, 8} in registers, any other C staged in LDS as loss_ex.hip
//                         does) or per-element (sigmoid head) passes, one family for both terms and both directions.
//      sums (4-byte words): [0] N (uint32, integer atomics)  [1] the sum (float)  [2] scale / N  [3] 0
#include "loss_common.h"
#include "../../include/distmap/lmnet_distmap.h"

#define DM_INF 32768              // column sentinel: DM_INF^2 + 1023^2 < 2^31
#define DM_MAXSIDE LMN_DISTMAP_MAX_SIDE
#define DM_SEG 16                 // row segments per block of dm_col_kernel: ceil(1024 / 16) = 64 rows fit one 64-bit mask
static_assert(LMN_DISTMAP_LABELS_U8 == LOSS_LABELS_U8 && LMN_DISTMAP_LABELS_I64 == LOSS_LABELS_I64 && LMN_DISTMAP_SOFTMAX == LOSS_SOFTMAX &&
              LMN_DISTMAP_SIGMOID == LOSS_SIGMOID, "loss_common.h reads the label kinds and heads of lmnet_distmap.h");

namespace {

__global__ __launch_bounds__(256) void dm_mask_labels_kernel(const void* __restrict__ labels, int kind, int nk, LossCls cls, int64_t hw,
                                                             int64_t total, uint8_t* __restrict__ mask) {
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = idx / hw, i = idx - b * hw;
    const int64_t y = loss_label(labels, kind, idx);      // (a value outside [0, C) equals no class id)
    for (int kk = 0; kk < nk; ++kk) mask[(b * nk + kk) * hw + i] = (uint8_t)(y == (int64_t)cls.id[kk]);
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void dm_mask_logits_kernel(const float* __restrict__ logits, float thr, int C, int nk, LossCls cls,
                                                             int64_t hw, int64_t total, uint8_t* __restrict__ mask) {
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = idx / hw, i = idx - b * hw;
    const float* lg = logits + b * C * hw + i;
    float lse = 0.f;
    if (MODE == LMN_DISTMAP_SOFTMAX) {
      float mx = -3.0e38f;
      for (int c = 0; c < C; ++c) mx = fmaxf(mx, lg[c * hw]);
      float den = 0.f;
      for (int c = 0; c < C; ++c) den += expf(lg[c * hw] - mx);
      lse = mx + logf(den);
    }
    for (int kk = 0; kk < nk; ++kk) {
      const float z = lg[(int64_t)cls.id[kk] * hw];
      const bool on = MODE == LMN_DISTMAP_SOFTMAX ? expf(z - lse) > thr : z > thr;     // (NaN: off)
      mask[(b * nk + kk) * hw + i] = (uint8_t)on;
    }
  }
}

// blockIdx.x: the plane, blockIdx.y: the block of 64 columns.  t[0] / t[1]: the rows of the segment inside / outside the mask.
__global__ __launch_bounds__(64 * DM_SEG) void dm_col_kernel(const uint8_t* __restrict__ mask, int H, int W, uint16_t* __restrict__ g,
                                                             int32_t* __restrict__ count) {
  __shared__ int s_last[2][DM_SEG][64], s_first[2][DM_SEG][64];
  __shared__ int s_cnt[DM_SEG];
  const int lane = threadIdx.x, seg = threadIdx.y;
  const int x = blockIdx.y * 64 + lane, plane = blockIdx.x;
  const int64_t HW = (int64_t)H * W;
  const uint8_t* m = mask + (int64_t)plane * HW;
  uint16_t* gp = g + (int64_t)plane * HW;
  const int L = (H + DM_SEG - 1) / DM_SEG;                // <= 64 rows per segment
  const int y0 = seg * L, n = min(L, H - y0);             // (n <= 0: a segment past the last row)
  const bool live = x < W && n > 0;
  unsigned long long t[2] = {0ull, 0ull};
  if (live) {
    const uint8_t* r = m + (int64_t)y0 * W + x;
    unsigned long long mc = 0;
    for (int i = 0; i < n; ++i) mc |= (unsigned long long)(r[(int64_t)i * W] != 0) << i;
    t[0] = mc;
    t[1] = ~mc & (~0ull >> (64 - n));                     // (1 <= n <= 64)
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    s_last[s][seg][lane] = t[s] ? y0 + 63 - __clzll((long long)t[s]) : -DM_INF;
    s_first[s][seg][lane] = t[s] ? y0 + __ffsll((long long)t[s]) - 1 : 3 * DM_INF;
  }
  int cnt = __popcll(t[0]);
#pragma unroll
  for (int s = 1; s <= 32; s <<= 1) cnt += __shfl_xor(cnt, s, 64);
  if (lane == 0) s_cnt[seg] = cnt;
  __syncthreads();
  if (live) {
    int above[2] = {-DM_INF, -DM_INF}, below[2] = {3 * DM_INF, 3 * DM_INF};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      for (int q = 0; q < seg; ++q) above[s] = max(above[s], s_last[s][q][lane]);
      for (int q = seg + 1; q < DM_SEG; ++q) below[s] = min(below[s], s_first[s][q][lane]);
    }
    for (int i = 0; i < n; ++i) {
      const int y = y0 + i;
      const bool in = (t[0] >> i) & 1;
      const unsigned long long opp = in ? t[1] : t[0];    // the rows of opposite membership (row i is not among them)
      const unsigned long long lo = opp & (~0ull >> (63 - i)), hi = opp >> i;
      const int la = lo ? y0 + 63 - __clzll((long long)lo) : (in ? above[1] : above[0]);
      const int nx = hi ? y + __ffsll((long long)hi) - 1 : (in ? below[1] : below[0]);
      gp[(int64_t)y * W + x] = (uint16_t)min(min(y - la, nx - y), DM_INF);
    }
  }
  if (lane == 0 && seg == 0) {
    cnt = 0;
    for (int s = 0; s < DM_SEG; ++s) cnt += s_cnt[s];
    if (cnt) atomicAdd(count + plane, cnt);
  }
}

// blockIdx.x = plane * H + y; one thread per pixel of the row.
__global__ __launch_bounds__(1024) void dm_row_kernel(const uint8_t* __restrict__ mask, const uint16_t* __restrict__ g,
                                                      const int32_t* __restrict__ count, int H, int W, int32_t* __restrict__ sd2,
                                                      int32_t* __restrict__ flags) {
  __shared__ int s_in[DM_MAXSIDE], s_out[DM_MAXSIDE];
  const int plane = blockIdx.x / H, y = blockIdx.x - plane * H, x = threadIdx.x;
  const int64_t row = (int64_t)plane * H * W + (int64_t)y * W;
  const int cnt = count[plane];
  const int flag = cnt == 0 ? LMN_DISTMAP_FLAG_EMPTY : (cnt == H * W ? LMN_DISTMAP_FLAG_FULL : 0);
  if (y == 0 && x == 0) flags[plane] = flag;
  if (flag) {                                             // (block-uniform) no pixel of opposite membership anywhere: all 0
    if (x < W) sd2[row + x] = 0;
    return;
  }
  bool in = false;
  if (x < W) {
    const int v = g[row + x];
    in = mask[row + x] != 0;
    s_in[x] = in ? 0 : v * v;
    s_out[x] = in ? v * v : 0;
  }
  __syncthreads();
  if (x < W) {
    const int* a = in ? s_out : s_in;
    int best = a[x];
    for (int d = 1; d < W && d * d < best; ++d) {
      const int dd = d * d;
      if (x - d >= 0) best = min(best, dd + a[x - d]);
      if (x + d < W) best = min(best, dd + a[x + d]);
    }
    sd2[row + x] = in ? -best : best;
  }
}

// ------------------------------------------------------------------------------------------------------------------ the losses
struct DlArgs {
  const float* logits;
  const void* target;
  const int32_t* sd2_g;
  const int32_t* sd2_p;
  uint64_t cmask;
  int64_t hw;
  int kind, B, C, nk;
  float half_alpha;
};

// TERM 0: phi of the boundary term; 1: the Hausdorff weight for alpha == 2 (the integer sum converted once); 2: any alpha
template <int TERM>
__device__ __forceinline__ float dl_weight(const DlArgs& a, int64_t off) {
  const int sg = a.sd2_g[off];
  if constexpr (TERM == 0) {
    return sg > 0 ? sqrtf((float)sg) : (sg < 0 ? 1.f - sqrtf((float)-sg) : 0.f);
  } else {
    const int sp = a.sd2_p[off];
    if constexpr (TERM == 1) return (float)(abs(sp) + abs(sg));
    else return powf((float)abs(sp), a.half_alpha) + powf((float)abs(sg), a.half_alpha);
  }
}
// one element: its value f and df / dp, with p the probability, on the 0 / 1 target, w = dl_weight
template <int TERM>
__device__ __forceinline__ void dl_point(float p, bool on, float w, float& f, float& dfdp) {
  if constexpr (TERM == 0) {
    f = p * w;
    dfdp = w;
  } else {
    const float e = p - (on ? 1.f : 0.f);
    f = e * e * w;
    dfdp = 2.f * e * w;
  }
}

// the block's partials into sums / its slot; red: 8 words of LDS nobody reads any more
__device__ __forceinline__ void dl_reduce(float a_sum, unsigned a_n, float* red, uint32_t* __restrict__ sums, float* __restrict__ slot) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  a_sum = loss_wave_sum(a_sum);
  a_n = loss_wave_sum(a_n);
  if (lane == 0) {
    red[wv] = a_sum;
    reinterpret_cast<unsigned*>(red)[4 + wv] = a_n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned* ru = reinterpret_cast<const unsigned*>(red) + 4;
    const unsigned n = ru[0] + ru[1] + ru[2] + ru[3];
    const float v = red[0] + red[1] + red[2] + red[3];
    if (n) atomicAdd(sums, n);                            // the count: an integer atomic, exact in either mode
    if (slot) slot[blockIdx.x] = v;                       // deterministic mode: the block's slot
    else atomicAdd(reinterpret_cast<float*>(sums) + 1, v);
  }
}

// Softmax head, one pixel per thread.  CT > 0: the C = CT logits in registers; CT == 0: staged in LDS ([C][256], one global read each).
template <int CT, int TERM, bool BWD>
__global__ __launch_bounds__(256) void dl_softmax_kernel(DlArgs a, uint32_t* __restrict__ sums, float* __restrict__ slot,
                                                         const float* __restrict__ gscale, float* __restrict__ dlogits) {
  extern __shared__ float dl_sh[];                        // CT == 0: the tile; afterwards the 8 words of dl_reduce
  const int C = CT ? CT : a.C;
  constexpr int UN = CT ? CT : 1;                         // (the staged form: loops over a run-time C)
  float zr[CT ? CT : 1];
  float* zs = dl_sh + threadIdx.x;
  auto Z = [&](int c) -> float {
    if constexpr (CT != 0) return zr[c];
    else return zs[c * 256];
  };
  float k = 0.f;
  if constexpr (BWD) k = (gscale ? gscale[0] : 1.f) * reinterpret_cast<const float*>(sums)[2];
  float a_sum = 0.f;
  unsigned a_n = 0;
  const int64_t hw = a.hw, total = (int64_t)a.B * hw;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = idx / hw, i = idx - b * hw;
    const float* lg = a.logits + b * C * hw + i;
    float mx = -3.0e38f;
#pragma unroll UN
    for (int c = 0; c < C; ++c) {
      const float v = lg[c * hw];
      if constexpr (CT != 0) zr[c] = v;
      else zs[c * 256] = v;
      mx = fmaxf(mx, v);
    }
    const int64_t yl = loss_label(a.target, a.kind, idx);
    if ((uint64_t)yl >= (uint64_t)C) {                    // void: adds to no sum, +0 in every class
      if constexpr (BWD) {
        float* d = dlogits + b * C * hw + i;
#pragma unroll UN
        for (int c = 0; c < C; ++c) d[c * hw] = 0.f;
      }
      continue;
    }
    const int y = (int)yl;
    float den = 0.f;
#pragma unroll UN
    for (int c = 0; c < C; ++c) den += expf(Z(c) - mx);
    const float r = 1.f / den;
    const int64_t base = b * a.nk * hw + i;
    float acc = 0.f, gp = 0.f;                            // the pixel's value and sum_k p_k df/dp_k
    int kk = 0;
#pragma unroll UN
    for (int c = 0; c < C; ++c) {
      if ((a.cmask >> c) & 1) {
        const float p = expf(Z(c) - mx) * r;
        float f, dfdp;
        dl_point<TERM>(p, c == y, dl_weight<TERM>(a, base + kk * hw), f, dfdp);
        acc += f;
        gp += dfdp * p;
        ++kk;
      }
    }
    if constexpr (!BWD) {
      a_sum += acc;
      a_n += (unsigned)a.nk;
    } else {
      float* d = dlogits + b * C * hw + i;
      kk = 0;
#pragma unroll UN
      for (int c = 0; c < C; ++c) {
        const float p = expf(Z(c) - mx) * r;
        float f, dfdp = 0.f;
        if ((a.cmask >> c) & 1) {
          dl_point<TERM>(p, c == y, dl_weight<TERM>(a, base + kk * hw), f, dfdp);
          ++kk;
        }
        d[c * hw] = k * (p * (dfdp - gp));
      }
    }
  }
  if constexpr (!BWD) {
    __syncthreads();                                      // (the tile is dead: its first words take the partials)
    dl_reduce(a_sum, a_n, dl_sh, sums, slot);
  }
}

// Sigmoid head, one element of logits [B, C, H, W] per thread; the planes outside class_mask add nothing and receive +0.
template <int TERM, bool BWD>
__global__ __launch_bounds__(256) void dl_sigmoid_kernel(DlArgs a, uint32_t* __restrict__ sums, float* __restrict__ slot,
                                                         const float* __restrict__ gscale, float* __restrict__ dlogits) {
  __shared__ float red[8];
  float k = 0.f;
  if constexpr (BWD) k = (gscale ? gscale[0] : 1.f) * reinterpret_cast<const float*>(sums)[2];
  float a_sum = 0.f;
  unsigned a_n = 0;
  const int64_t hw = a.hw, total = (int64_t)a.B * a.C * hw;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t plane = idx / hw, i = idx - plane * hw;
    const int64_t b = plane / a.C;
    const int c = (int)(plane - b * a.C);
    float d = 0.f;                                        // unscored plane, void element: +0
    if ((a.cmask >> c) & 1) {
      const int64_t t = loss_label(a.target, a.kind, idx);
      if ((uint64_t)t <= 1ull) {
        const int kk = __popcll(a.cmask & ((1ull << c) - 1ull));
        const SigPoint s = sig_point(a.logits[idx]);
        float f, dfdp;
        dl_point<TERM>(s.p, t == 1, dl_weight<TERM>(a, (b * a.nk + kk) * hw + i), f, dfdp);
        a_sum += f;
        a_n += 1u;
        d = k * (dfdp * (s.p * s.omp));
      }
    }
    if constexpr (BWD) dlogits[idx] = d;
  }
  if constexpr (!BWD) dl_reduce(a_sum, a_n, red, sums, slot);
}

__global__ void dl_finish_kernel(uint32_t* __restrict__ sums, float scale, float* __restrict__ loss) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float* fs = reinterpret_cast<float*>(sums);
  const uint32_t n = sums[0];
  const float coef = n ? scale / (float)n : 0.f;          // no valid element: loss 0, gradient 0
  loss[0] = n ? fs[1] * coef : 0.f;
  fs[2] = coef;
  sums[3] = 0u;
}

bool dm_dims_ok(int B, int nk, int H, int W) {
  return B >= 1 && nk >= 1 && nk <= LOSS_MAXC && H >= 2 && H <= DM_MAXSIDE && W >= 2 && W <= DM_MAXSIDE &&
         (int64_t)B * nk * H * W < (1LL << 31);
}
int64_t dm_mask_bytes(int64_t np, int64_t HW) { return lmn_up256(np * HW); }
int64_t dm_g_bytes(int64_t np, int64_t HW) { return lmn_up256(np * HW * (int64_t)sizeof(uint16_t)); }
int64_t dm_count_bytes(int64_t np) { return lmn_up256(np * (int64_t)sizeof(int32_t)); }

// the argument checks the three device entries share
int dm_check(const char* what, int B, int C, int H, int W, uint64_t class_mask, int kind, bool softmax) {
  LMN_REQUIRE(B >= 1, "%s: B=%d < 1", what, B);
  if (int rc = loss_check_head(what, C, softmax, class_mask, kind)) return rc;
  LMN_REQUIRE(H >= 2 && H <= DM_MAXSIDE && W >= 2 && W <= DM_MAXSIDE, "%s: size %dx%d outside [2, %d]", what, H, W, DM_MAXSIDE);
  LMN_REQUIRE((int64_t)B * __builtin_popcountll(class_mask) * H * W < (1LL << 31), "%s: B * nk * H * W = %lld not below 2^31", what,
              (long long)B * __builtin_popcountll(class_mask) * H * W);
  return 0;
}

int dl_check(const char* what, int target_kind, int head, int term, float alpha, int B, int C, int H, int W, uint64_t class_mask) {
  LMN_REQUIRE(head == LMN_DISTMAP_SOFTMAX || head == LMN_DISTMAP_SIGMOID, "%s: unknown head %d", what, head);
  LMN_REQUIRE(term == LMN_DISTMAP_BOUNDARY || term == LMN_DISTMAP_HAUSDORFF, "%s: unknown term %d", what, term);
  if (int rc = dm_check(what, B, C, H, W, class_mask, target_kind, head == LMN_DISTMAP_SOFTMAX)) return rc;
  LMN_REQUIRE((int64_t)B * C * H * W < (1LL << 31), "%s: B * C * H * W = %lld not below 2^31", what, (long long)B * C * H * W);
  LMN_REQUIRE(term != LMN_DISTMAP_HAUSDORFF || (alpha > 0.f && alpha <= 8.f), "%s: alpha=%g not in (0, 8]", what, (double)alpha);
  return 0;
}

#define DL_TERMS(tid, ...)                                        \
  switch (tid) {                                                  \
    case 0: { constexpr int TERM = 0; __VA_ARGS__; } break;       \
    case 1: { constexpr int TERM = 1; __VA_ARGS__; } break;       \
    default: { constexpr int TERM = 2; __VA_ARGS__; } break;      \
  }

// one pass of either direction over the batch
template <bool BWD>
void dl_launch(hipStream_t st, int head, int tid, const DlArgs& a, uint32_t* sums, float* slot, const float* gscale, float* dlogits,
               int grid) {
  if (head == LMN_DISTMAP_SOFTMAX) {
    const int C = a.C;
    const size_t sh = loss_templated(C) ? 8 * sizeof(float) : (size_t)C * 256 * sizeof(float);    // (<= 64 KiB at C = 64)
    DL_TERMS(tid, LOSS_SWITCH_CT(C, LMN_LAUNCH((dl_softmax_kernel<CT, TERM, BWD>), dim3(grid), dim3(256), sh, st, a, sums, slot, gscale, dlogits)));
  } else {
    DL_TERMS(tid, LMN_LAUNCH((dl_sigmoid_kernel<TERM, BWD>), dim3(grid), dim3(256), 0, st, a, sums, slot, gscale, dlogits));
  }
}

int dl_term_id(int term, float alpha) { return term == LMN_DISTMAP_BOUNDARY ? 0 : (alpha == 2.f ? 1 : 2); }

DlArgs dl_args(const float* logits, const void* target, int target_kind, float alpha, int B, int C, int H, int W, uint64_t class_mask,
               const int32_t* sd2_g, const int32_t* sd2_p) {
  DlArgs a;
  a.logits = logits;
  a.target = target;
  a.sd2_g = sd2_g;
  a.sd2_p = sd2_p;
  a.cmask = class_mask;
  a.hw = (int64_t)H * W;
  a.kind = target_kind;
  a.B = B;
  a.C = C;
  a.nk = __builtin_popcountll(class_mask);
  a.half_alpha = 0.5f * alpha;
  return a;
}

}  // namespace

extern "C" {

int64_t lmn_dist_workspace(int B, int nk, int H, int W) {
  if (!dm_dims_ok(B, nk, H, W)) {
    snprintf(g_lmn_err, sizeof(g_lmn_err), "dist_workspace: B=%d nk=%d %dx%d outside B >= 1, nk in [1, %d], sides in [2, %d], B * nk * H * W < 2^31",
             B, nk, H, W, LOSS_MAXC, DM_MAXSIDE);
    return -1;
  }
  const int64_t HW = (int64_t)H * W, np = (int64_t)B * nk;
  return dm_mask_bytes(np, HW) + dm_g_bytes(np, HW) + dm_count_bytes(np);
}

int lmn_dist_map(const float* logits, const void* labels, int label_kind, float threshold, int mode, int B, int C, int H, int W,
                 uint64_t class_mask, void* workspace, int64_t ws_bytes, int32_t* sd2, int32_t* flags, lmn_stream_t stream) {
  LMN_REQUIRE((logits != nullptr) != (labels != nullptr), "dist_map: exactly one of logits, labels required");
  LMN_REQUIRE(workspace && sd2 && flags, "dist_map: null pointer");
  if (logits) {
    LMN_REQUIRE(mode == LMN_DISTMAP_SOFTMAX || mode == LMN_DISTMAP_SIGMOID, "dist_map: unknown mode %d", mode);
    LMN_REQUIRE(threshold == threshold, "dist_map: threshold is NaN");
  }
  if (int rc = dm_check("dist_map", B, C, H, W, class_mask, labels ? label_kind : LMN_DISTMAP_LABELS_U8,
                        logits && mode == LMN_DISTMAP_SOFTMAX))
    return rc;
  LossCls cls;
  const int nk = loss_classes(class_mask, &cls);
  const int64_t need = lmn_dist_workspace(B, nk, H, W);
  LMN_REQUIRE(need >= 0 && ws_bytes >= need, "dist_map: workspace of %lld bytes too small, %lld needed", (long long)ws_bytes, (long long)need);
  const int64_t HW = (int64_t)H * W, total = (int64_t)B * HW;
  const int np = B * nk;
  uint8_t* mask = (uint8_t*)workspace;
  uint16_t* g = (uint16_t*)(mask + dm_mask_bytes(np, HW));
  int32_t* count = (int32_t*)((uint8_t*)g + dm_g_bytes(np, HW));
  hipStream_t st = (hipStream_t)stream;
  LMN_HIP_OK(hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)np, st), "dist_map");
  const int mgrid = loss_grid(total, 2048);
  if (labels) {
    LMN_LAUNCH(dm_mask_labels_kernel, dim3(mgrid), dim3(256), 0, st, labels, label_kind, nk, cls, HW, total, mask);
  } else if (mode == LMN_DISTMAP_SOFTMAX) {
    LMN_LAUNCH((dm_mask_logits_kernel<LMN_DISTMAP_SOFTMAX>), dim3(mgrid), dim3(256), 0, st, logits, threshold, C, nk, cls, HW, total, mask);
  } else {
    LMN_LAUNCH((dm_mask_logits_kernel<LMN_DISTMAP_SIGMOID>), dim3(mgrid), dim3(256), 0, st, logits, threshold, C, nk, cls, HW, total, mask);
  }
  LMN_LAUNCH(dm_col_kernel, dim3(np, lmn_cdiv(W, 64)), dim3(64, DM_SEG), 0, st, (const uint8_t*)mask, H, W, g, count);
  LMN_LAUNCH(dm_row_kernel, dim3((unsigned)((int64_t)np * H)), dim3(lmn_cdiv(W, 64) * 64), 0, st, (const uint8_t*)mask, (const uint16_t*)g,
             (const int32_t*)count, H, W, sd2, flags);
  return lmn_launch_status("dist_map");
}

int lmn_dist_loss_fwd(const float* logits, const void* target, int target_kind, int head, int term, float alpha, float scale, int B,
                      int C, int H, int W, uint64_t class_mask, const int32_t* sd2_g, const int32_t* sd2_p, void* sums, float* loss,
                      lmn_stream_t stream) {
  LMN_REQUIRE(logits && target && sd2_g && sums && loss, "dist_loss_fwd: null pointer");
  if (int rc = dl_check("dist_loss_fwd", target_kind, head, term, alpha, B, C, H, W, class_mask)) return rc;
  LMN_REQUIRE((term == LMN_DISTMAP_HAUSDORFF) == (sd2_p != nullptr), "dist_loss_fwd: sd2_p goes with the Hausdorff term and only with it");
  LMN_REQUIRE(loss_finite(scale), "dist_loss_fwd: scale=%g is not finite", (double)scale);
  hipStream_t st = (hipStream_t)stream;
  const DlArgs a = dl_args(logits, target, target_kind, alpha, B, C, H, W, class_mask, sd2_g, sd2_p);
  const int grid = loss_grid((head == LMN_DISTMAP_SOFTMAX ? (int64_t)B : (int64_t)B * C) * a.hw, 1024);
  LMN_LAUNCH(loss_zero_kernel, dim3(1), dim3(64), 0, st, (uint32_t*)sums, (int64_t)LMN_DISTMAP_SUMS_WORDS);
  float* slot = nullptr;
  if (g_lmn_det) {
    lmn_det_begin(st);
    slot = lmn_det_slots(st, (size_t)grid);
    LMN_REQUIRE(slot, "dist_loss_fwd: deterministic mode: no scratch");
  }
  dl_launch<false>(st, head, dl_term_id(term, alpha), a, (uint32_t*)sums, slot, nullptr, nullptr, grid);
  if (slot) lmn_det_sum(st, slot, grid, 1, (float*)sums + 1);
  LMN_LAUNCH(dl_finish_kernel, dim3(1), dim3(64), 0, st, (uint32_t*)sums, scale, loss);
  return lmn_launch_status("dist_loss_fwd");
}

int lmn_dist_loss_bwd(const float* logits, const void* target, int target_kind, int head, int term, float alpha, int B, int C, int H,
                      int W, uint64_t class_mask, const int32_t* sd2_g, const int32_t* sd2_p, const void* sums, const float* gscale,
                      float* dlogits, lmn_stream_t stream) {
  LMN_REQUIRE(logits && target && sd2_g && sums && dlogits, "dist_loss_bwd: null pointer");
  if (int rc = dl_check("dist_loss_bwd", target_kind, head, term, alpha, B, C, H, W, class_mask)) return rc;
  LMN_REQUIRE((term == LMN_DISTMAP_HAUSDORFF) == (sd2_p != nullptr), "dist_loss_bwd: sd2_p goes with the Hausdorff term and only with it");
  hipStream_t st = (hipStream_t)stream;
  const DlArgs a = dl_args(logits, target, target_kind, alpha, B, C, H, W, class_mask, sd2_g, sd2_p);
  const int grid = loss_grid((head == LMN_DISTMAP_SOFTMAX ? (int64_t)B : (int64_t)B * C) * a.hw, 4096);
  dl_launch<true>(st, head, dl_term_id(term, alpha), a, (uint32_t*)const_cast<void*>(sums), nullptr, gscale, dlogits, grid);
  return lmn_launch_status("dist_loss_bwd");
}

}  // extern "C"

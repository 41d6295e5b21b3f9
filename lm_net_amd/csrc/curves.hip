// Threshold sweeps (include/curves/lmnet_curves.h): per (image, class) plane, the histogram of the scores of the positive and of the
// negative elements over the bins of an edge table.  As in sigmoid.hip, blockIdx.y is the (b, c) plane and blockIdx.x strides over
// THAT plane only, so a block's counters belong to one plane; a lane takes four consecutive elements (16-byte loads) when
// HW % 4 == 0 and the bases are aligned, one element otherwise.
//   LDS: the edge table (<= 4 KB) and 2 x (n_edges + 1) uint32 counters (<= 8.2 KB).
//   The bin is an upper-bound search of the LDS table: comparisons against the table only (the header's BIN RULE).
//   In a real segmentation map most scores are saturated and fall into the outermost populated bins: 64 lanes adding to one LDS
//   address serialise, so the end bins are counted by wave ballots into registers (as sigmoid_stats_kernel counts) and added once
//   per wave; only the elements in between take an LDS atomic each.  TWO bins at each end go this way -- 0, 1, n_edges - 1 and
//   n_edges -- because a table that starts at threshold 0 and ends at 1 (the binned default: logit edges -inf and +inf,
//   probability edges 0 and 1) leaves bins 0 and n_edges all but empty and sends the saturated scores to bins 1 and n_edges - 1.
//   A block ends with one global integer atomic per non-zero counter, which is why the grid is capped and does not grow with HW.
//   Integer arithmetic throughout: exact and order-independent.
#include "loss_common.h"
#include "pred_common.h"
#include "../../include/curves/lmnet_curves.h"
static_assert(LMN_CURVE_T_U8 == LOSS_LABELS_U8 && LMN_CURVE_T_I64 == LOSS_LABELS_I64, "loss_common.h reads the target kinds of lmnet_curves.h");

namespace {

// E consecutive elements of plane (b, c) as 0 (negative), 1 (positive) or 2 (void).  FORM planes: `t` is the plane itself and the
// value decides (0 / 1 / anything else); FORM labels: `t` is image b's label map, positive where label == c, void outside [0, C).
template <int KIND, int E>
__device__ __forceinline__ void cv_load_raw(const void* __restrict__ t, int64_t i, int64_t (&v)[E]) {
  if constexpr (KIND == LMN_CURVE_T_U8) {
    const uint8_t* p = (const uint8_t*)t + i;
    if constexpr (E == 4) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (int64_t)((w >> (8 * j)) & 255u);
    } else {
      v[0] = (int64_t)p[0];
    }
  } else {
    const int64_t* p = (const int64_t*)t + i;
    if constexpr (E == 4) {
      const longlong2 a = *reinterpret_cast<const longlong2*>(p), b = *reinterpret_cast<const longlong2*>(p + 2);
      v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else {
      v[0] = p[0];
    }
  }
}
template <int KIND, bool LABELS, int E>
__device__ __forceinline__ void cv_load_t(const void* __restrict__ t, int64_t i, int c, int C, int (&out)[E]) {
  int64_t v[E];
  cv_load_raw<KIND, E>(t, i, v);
#pragma unroll
  for (int j = 0; j < E; ++j) {
    if constexpr (LABELS) out[j] = pred_in_range(v[j], C) ? (v[j] == (int64_t)c ? 1 : 0) : 2;
    else out[j] = (uint64_t)v[j] <= 1ull ? (int)v[j] : 2;
  }
}

// L = m + logf(sum_j expf(z_j - m)), m = max_j z_j, per pixel: one lane per pixel, the reads of one class coalesced over the pixels
__global__ __launch_bounds__(256) void curve_lse_kernel(const float* __restrict__ logits, int C, int64_t hw, int64_t pixels,
                                                        float* __restrict__ lse) {
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < pixels; g += (int64_t)gridDim.x * 256) {
    const int64_t b = g / hw, i = g - b * hw;
    const float* lg = logits + b * C * hw + i;
    float m = lg[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, lg[c * hw]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(lg[c * hw] - m);
    lse[g] = m + logf(s);
  }
}

template <int KIND, bool VEC, bool LABELS, bool SOFTMAX>
__global__ __launch_bounds__(256) void curve_hist_kernel(const float* __restrict__ values, const void* __restrict__ target,
                                                         const float* __restrict__ edges, int n_edges, int C, int64_t hw,
                                                         const float* __restrict__ lse, unsigned long long* __restrict__ hist) {
  constexpr int E = VEC ? 4 : 1;
  __shared__ float s_edge[LMN_CURVE_MAX_EDGES];
  __shared__ unsigned s_hist[2 * (LMN_CURVE_MAX_EDGES + 1)];
  const int nb = n_edges + 1;                         // bins of one histogram
  const int plane = blockIdx.y, img = plane / C, c = plane - img * C;
  for (int k = threadIdx.x; k < n_edges; k += 256) s_edge[k] = edges[k];
  for (int k = threadIdx.x; k < 2 * nb; k += 256) s_hist[k] = 0u;
  __syncthreads();
  // the four outer bins 0, 1, n_edges - 1, n_edges (fewer for n_edges < 3) are counted by ballots
  const bool has_b1 = n_edges >= 2, has_bp = n_edges >= 3;
  const float e_0 = s_edge[0], e_1 = s_edge[has_b1 ? 1 : 0], e_pen = s_edge[has_b1 ? n_edges - 2 : 0], e_last = s_edge[n_edges - 1];
  const float* vp = values + (int64_t)plane * hw;
  const float* lp = SOFTMAX ? lse + (int64_t)img * hw : nullptr;
  const int64_t t_elems = LABELS ? (int64_t)img * hw : (int64_t)plane * hw;
  const void* tg = (const uint8_t*)target + t_elems * (KIND == LMN_CURVE_T_I64 ? 8 : 1);
  int cnt[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};       // [negative / positive][bin 0, 1, n_edges - 1, n_edges]: the same value in every lane of a wave
  const int64_t items = hw / E;                       // (VEC: hw % 4 == 0)
  for (int64_t base = (int64_t)blockIdx.x * 256; base < items; base += (int64_t)gridDim.x * 256) {   // whole waves take every trip
    const int64_t q = base + threadIdx.x;
    const bool in = q < items;
    float z[E], l[E];
    int t[E];
#pragma unroll
    for (int j = 0; j < E; ++j) { z[j] = 0.f; l[j] = 0.f; t[j] = 2; }
    if (in) {
      loss_load_z<E>(vp, q * E, z);
      if constexpr (SOFTMAX) loss_load_z<E>(lp, q * E, l);
      cv_load_t<KIND, LABELS, E>(tg, q * E, c, C, t);
    }
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const float s = SOFTMAX ? expf(z[j] - l[j]) : z[j];
      const bool pos = t[j] == 1, neg = t[j] == 0;    // (a lane past the plane's end holds 2: void)
      const bool ge_0 = s >= e_0, ge_1 = s >= e_1, ge_pen = s >= e_pen, ge_last = s >= e_last;   // (NaN: all false, bin 0)
      const bool outer[4] = {!ge_0, has_b1 && ge_0 && !ge_1, has_bp && ge_pen && !ge_last, ge_last};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        cnt[0][k] += __popcll(__ballot(neg && outer[k]));
        cnt[1][k] += __popcll(__ballot(pos && outer[k]));
      }
      if ((pos || neg) && ge_1 && !ge_pen) {          // edges[1] <= s < edges[n_edges - 2]: the bin lies in [2, n_edges - 2]
        int a = 2, b = n_edges - 2;
        while (a < b) {                               // upper bound: the first k with s < edges[k]
          const int mid = (a + b) >> 1;
          if (s >= s_edge[mid]) a = mid + 1;
          else b = mid;
        }
        atomicAdd(&s_hist[(pos ? nb : 0) + a], 1u);
      }
    }
  }
  if ((threadIdx.x & 63) == 0) {                      // once per wave
    const int bin[4] = {0, 1, n_edges - 1, n_edges};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (cnt[0][k]) atomicAdd(&s_hist[bin[k]], (unsigned)cnt[0][k]);
      if (cnt[1][k]) atomicAdd(&s_hist[nb + bin[k]], (unsigned)cnt[1][k]);
    }
  }
  __syncthreads();
  unsigned long long* out = hist + (int64_t)plane * 2 * nb;
  for (int k = threadIdx.x; k < 2 * nb; k += 256) {   // one integer atomic per block and non-zero counter
    const unsigned v = s_hist[k];
    if (v) atomicAdd(out + k, (unsigned long long)v);
  }
}

int cv_check_sizes(const char* what, int score_kind, int B, int64_t HW) {
  LMN_REQUIRE(score_kind == LMN_CURVE_RAW || score_kind == LMN_CURVE_SOFTMAX, "%s: unknown score_kind %d", what, score_kind);
  LMN_REQUIRE(B > 0 && HW > 0 && HW < (1LL << 31) && (int64_t)B * HW < (1LL << 31), "%s: B=%d, HW=%lld (need B >= 1, HW >= 1, B * HW < 2^31)",
              what, B, (long long)HW);
  return 0;
}

}  // namespace

extern "C" {

int64_t lmn_curve_workspace(int score_kind, int B, int64_t HW) {
  if (int rc = cv_check_sizes("curve_workspace", score_kind, B, HW)) return rc;
  return score_kind == LMN_CURVE_SOFTMAX ? 4 * (int64_t)B * HW : 0;
}

int lmn_curve_hist(const float* values, const void* target, int target_kind, int target_form, int score_kind, const float* edges,
                   int n_edges, int B, int C, int64_t HW, void* workspace, int64_t* hist, lmn_stream_t stream) {
  LMN_REQUIRE(values && target && edges && hist, "curve_hist: null pointer");
  LMN_REQUIRE(target_kind == LMN_CURVE_T_U8 || target_kind == LMN_CURVE_T_I64, "curve_hist: unknown target_kind %d", target_kind);
  LMN_REQUIRE(target_form == LMN_CURVE_PLANES || target_form == LMN_CURVE_LABELS, "curve_hist: unknown target_form %d", target_form);
  if (int rc = cv_check_sizes("curve_hist", score_kind, B, HW)) return rc;
  LMN_REQUIRE(n_edges >= 1 && n_edges <= LMN_CURVE_MAX_EDGES, "curve_hist: n_edges=%d not in [1, %d]", n_edges, LMN_CURVE_MAX_EDGES);
  const bool softmax = score_kind == LMN_CURVE_SOFTMAX, labels = target_form == LMN_CURVE_LABELS;
  LMN_REQUIRE(C >= (softmax ? 2 : 1) && C <= LMN_CURVE_MAX_CLASSES, "curve_hist: C=%d not in [%d, %d]", C, softmax ? 2 : 1,
              LMN_CURVE_MAX_CLASSES);
  LMN_REQUIRE((int64_t)B * C <= 65535, "curve_hist: B * C = %lld above 65535", (long long)B * C);
  LMN_REQUIRE(!softmax || workspace, "curve_hist: null pointer (the softmax form needs its workspace)");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = HW % 4 == 0 && lmn_aligned(values, 16) && lmn_aligned(target, target_kind == LMN_CURVE_T_I64 ? 16 : 4) &&
                   (!softmax || lmn_aligned(workspace, 16));
  const int planes = B * C;
  const int64_t items = vec ? HW / 4 : HW;
  const int gx = loss_grid_per(items, 1024, planes);
  const int64_t words = (int64_t)planes * 2 * (n_edges + 1) * 2;
  LMN_LAUNCH(loss_zero_kernel, dim3(loss_grid(words, 64)), dim3(256), 0, st, (uint32_t*)hist, words);
  const float* lse = nullptr;
  if (softmax) {
    const int64_t pixels = (int64_t)B * HW;
    LMN_LAUNCH(curve_lse_kernel, dim3(loss_grid(pixels, 4096)), dim3(256), 0, st, values, C, HW, pixels, (float*)workspace);
    lse = (const float*)workspace;
  }
  unsigned long long* ho = (unsigned long long*)hist;
  LOSS_SWITCH_BOOL(LABELS, labels, LOSS_SWITCH_BOOL(SOFTMAX, softmax, LOSS_SWITCH_KIND(target_kind, LOSS_SWITCH_BOOL(VEC, vec,
    LMN_LAUNCH((curve_hist_kernel<KIND, VEC, LABELS, SOFTMAX>), dim3(gx, planes), dim3(256), 0, st, values, target, edges, n_edges, C, HW, lse, ho)))));
  return lmn_launch_status("curve_hist");
}

}  // extern "C"

// Surface-distance statistics on the device (lm_net_amd.metrics.SurfaceDistanceMeter): what HD, HD95, ASSD and RVD of the
// medpy.metric.binary conventions need, per (sample, class) pair, for the evaluation loop the reference leaves unfinished
// (utils/train_eval_utils.py:7 imports hausdorff_distance, :178-179 set up hausdorff_distance_list / rvd_list, :14-52 ravd /
// RVDEvaluator).  The work is an exact Euclidean distance transform to the border of each mask, evaluated only at the border
// pixels of the other mask.  Every squared distance is an int32 (<= 2 * 1023^2 < 2^21); the only floating-point values are the
// two float64 sums of sqrt, formed in a fixed order.  No float atomics: two runs on one input give bit-identical statistics.
//
//   1. surf_labels_kernel   arg-max of the logits (pred_common.h) or the given label map, and the target, narrowed to uint8
//                           (255 = no class), once for all classes.
//   2. surf_col_kernel      per (map, pair), one lane per column: border test on the four neighbours (outside the image counts
//                           as outside the mask) -> g(y, x) = vertical distance to the nearest border pixel of the column
//                           (uint16, SURF_INF where the column has none).  g == 0 marks the border pixels.
//                           |mask| and the border count go to the statistics with integer atomics.
//   3. surf_row_kernel      per (map, pair, row): g^2 of the OTHER map's row in LDS; every border pixel of this map takes
//                           min_j (x - j)^2 + g^2(y, j), scanning outwards from x and stopping once d^2 >= the best so far
//                           (exact: every later term is >= d^2).  Writes the row's D2 compacted, and their count.
//   4. surf_finish_kernel   per pair: directed maxima, float64 sums of sqrt(D2) (per-thread sums over fixed rows, then a fixed tree) and
//                           the two order statistics of the pooled D2 multiset by a two-level radix select (11 + 10 bits) on
//                           integer histograms in LDS.
#include "pred_common.h"

#define SURF_INF 32768            // column sentinel: SURF_INF^2 + 1023^2 < 2^31
#define SURF_MAXSIDE 1024
#define SURF_SEG 16               // row segments per block of surf_col_kernel: ceil(1024 / 16) = 64 rows fit one 64-bit mask
#define SURF_NSTAT_I 8
#define SURF_NSTAT_F 2

struct SurfCls { uint8_t id[64]; };

static inline int64_t surf_lab_bytes(int64_t B, int64_t HW) { return lmn_up256(2 * B * HW); }
static inline int64_t surf_g_bytes(int64_t np, int64_t HW) { return lmn_up256(2 * np * HW * (int64_t)sizeof(uint16_t)); }
static inline int64_t surf_d2_bytes(int64_t np, int64_t HW) { return lmn_up256(2 * np * HW * (int64_t)sizeof(int32_t)); }
static inline int64_t surf_rc_bytes(int64_t np, int64_t H) { return lmn_up256(2 * np * H * (int64_t)sizeof(int32_t)); }

__global__ __launch_bounds__(256) void surf_labels_kernel(const float* __restrict__ logits, const int64_t* __restrict__ plab,
                                                          const int64_t* __restrict__ target, int C, int64_t hw, int64_t total,
                                                          uint8_t* __restrict__ lab) {
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    int best;
    if (logits) {
      const int64_t b = idx / hw, i = idx - b * hw;
      best = pred_argmax(logits + b * C * hw + i, C, hw);
    } else {
      best = pred_class(plab[idx], C, 255);
    }
    const int64_t t = target[idx];
    lab[idx] = (uint8_t)best;
    lab[total + idx] = (uint8_t)pred_class(t, C, 255);
  }
}

// One lane per column and SURF_SEG row segments per block (threadIdx.y): a segment's rows (<= 64) become bit masks -- the mask
// itself and its left / right neighbour columns -- so the border test is a few 64-bit operations and the nearest border row above /
// below any row of the segment a clz / ffs; the nearest border row outside the segment comes from the other segments through LDS.
// Nothing is carried from row to row: every load of the block is independent.
__global__ __launch_bounds__(64 * SURF_SEG) void surf_col_kernel(const uint8_t* __restrict__ lab, int B, int nk, int H, int W, SurfCls cls,
                                                                 uint16_t* __restrict__ g, unsigned long long* __restrict__ stats_i) {
  __shared__ int s_last[SURF_SEG][64], s_first[SURF_SEG][64];
  __shared__ int s_cnt[SURF_SEG][2];
  const int lane = threadIdx.x, seg = threadIdx.y;
  const int x = blockIdx.x * 64 + lane, pair = blockIdx.y, map = blockIdx.z;
  const int b = pair / nk;
  const uint8_t k = cls.id[pair - b * nk];
  const int64_t HW = (int64_t)H * W, np = (int64_t)B * nk;
  const uint8_t* m = lab + ((int64_t)map * B + b) * HW;
  uint16_t* gp = g + ((int64_t)map * np + pair) * HW;
  const int L = (H + SURF_SEG - 1) / SURF_SEG;            // <= 64 rows per segment
  const int y0 = seg * L, n = min(L, H - y0);             // (n <= 0: a segment past the last row)
  const bool live = x < W && n > 0;
  unsigned long long mc = 0, ml = 0, mr = 0, bd = 0;
  if (live) {
    const uint8_t* r = m + (int64_t)y0 * W + x;
    const bool hl = x > 0, hr = x + 1 < W;
    for (int i = 0; i < n; ++i) {
      const uint8_t* q = r + (int64_t)i * W;
      mc |= (unsigned long long)(q[0] == k) << i;
      ml |= (unsigned long long)(hl && q[-1] == k) << i;
      mr |= (unsigned long long)(hr && q[1] == k) << i;
    }
    const unsigned long long up = (mc << 1) | (unsigned long long)(y0 > 0 && r[-W] == k);
    const unsigned long long dn = (mc >> 1) | ((unsigned long long)(y0 + n < H && r[(int64_t)n * W] == k) << (n - 1));
    bd = mc & ~(up & dn & ml & mr);
  }
  s_last[seg][lane] = bd ? y0 + 63 - __clzll((long long)bd) : -SURF_INF;
  s_first[seg][lane] = bd ? y0 + __ffsll((long long)bd) - 1 : 3 * SURF_INF;
  int cnt = __popcll(mc), nb = __popcll(bd);
#pragma unroll
  for (int s = 1; s <= 32; s <<= 1) {
    cnt += __shfl_xor(cnt, s, 64);
    nb += __shfl_xor(nb, s, 64);
  }
  if (lane == 0) { s_cnt[seg][0] = cnt; s_cnt[seg][1] = nb; }
  __syncthreads();
  if (live) {
    int above = -SURF_INF, below = 3 * SURF_INF;
    for (int s = 0; s < seg; ++s) above = max(above, s_last[s][lane]);
    for (int s = seg + 1; s < SURF_SEG; ++s) below = min(below, s_first[s][lane]);
    for (int i = 0; i < n; ++i) {
      const int y = y0 + i;
      const unsigned long long lo = bd & (~0ull >> (63 - i)), hi = bd >> i;
      const int la = lo ? y0 + 63 - __clzll((long long)lo) : above;
      const int nx = hi ? y + __ffsll((long long)hi) - 1 : below;
      gp[(int64_t)y * W + x] = (uint16_t)min(min(y - la, nx - y), SURF_INF);
    }
  }
  if (lane == 0 && seg == 0) {
    cnt = 0, nb = 0;
    for (int s = 0; s < SURF_SEG; ++s) { cnt += s_cnt[s][0]; nb += s_cnt[s][1]; }
    if (cnt) {
      atomicAdd(stats_i + (int64_t)pair * SURF_NSTAT_I + map, (unsigned long long)cnt);
      atomicAdd(stats_i + (int64_t)pair * SURF_NSTAT_I + 2 + map, (unsigned long long)nb);
    }
  }
}

// The D2 of a row's border pixels are written compacted to the front of the row (in x order) with their count beside them, so the
// finish kernel reads border pixels only.
__global__ __launch_bounds__(1024) void surf_row_kernel(const uint16_t* __restrict__ g, int np, int H, int W,
                                                        const int64_t* __restrict__ stats_i, int32_t* __restrict__ d2,
                                                        int32_t* __restrict__ rowcnt) {
  __shared__ int s_g2[SURF_MAXSIDE];
  __shared__ int s_wn[SURF_MAXSIDE / 64];
  const int y = blockIdx.x, pair = blockIdx.y, map = blockIdx.z, x = threadIdx.x;
  const int64_t HW = (int64_t)H * W;
  const int64_t self = ((int64_t)map * np + pair) * HW + (int64_t)y * W;
  const int64_t other = ((int64_t)(1 - map) * np + pair) * HW + (int64_t)y * W;
  const bool scored = stats_i[(int64_t)pair * SURF_NSTAT_I + 2 + (1 - map)] > 0;   // the other map has a border (block-uniform)
  if (x < W) {
    const int v = g[other + x];
    s_g2[x] = v * v;
  }
  __syncthreads();
  int r = -1;
  if (scored && x < W && g[self + x] == 0) {
    int best = s_g2[x];
    for (int d = 1; d < W && d * d < best; ++d) {
      const int dd = d * d;
      if (x - d >= 0) best = min(best, dd + s_g2[x - d]);
      if (x + d < W) best = min(best, dd + s_g2[x + d]);
    }
    r = best;
  }
  const unsigned long long vote = __ballot(r >= 0);
  const int wave = x >> 6, lane = x & 63, nw = blockDim.x >> 6;
  if (lane == 0) s_wn[wave] = __popcll(vote);
  __syncthreads();
  int off = 0, total = 0;
  for (int w = 0; w < nw; ++w) {
    if (w < wave) off += s_wn[w];
    total += s_wn[w];
  }
  if (r >= 0) d2[self + off + __popcll(vote & ((1ull << lane) - 1))] = r;
  if (x == 0) rowcnt[((int64_t)map * np + pair) * H + y] = total;
}

// bin and rank inside the bin of the element of rank `rank` in a histogram of nb bins (nb a multiple of 64); run by wave 0
__device__ __forceinline__ void surf_select(const int* hist, int nb, int rank, int* out) {
  const int lane = threadIdx.x, per = nb >> 6;
  int sum = 0;
  for (int i = 0; i < per; ++i) sum += hist[lane * per + i];
  int inc = sum;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const int t = __shfl_up(inc, s, 64);
    if (lane >= s) inc += t;
  }
  int before = inc - sum;
  if (rank >= before && rank < inc) {
    for (int i = 0; i < per; ++i) {
      const int h = hist[lane * per + i];
      if (rank < before + h) {
        out[0] = lane * per + i;
        out[1] = rank - before;
        break;
      }
      before += h;
    }
  }
}

__global__ __launch_bounds__(1024) void surf_finish_kernel(const int32_t* __restrict__ d2, const int32_t* __restrict__ rowcnt, int np,
                                                           int H, int W, int64_t* __restrict__ stats_i, double* __restrict__ stats_f) {
  __shared__ int s_hist[2048];
  __shared__ int s_rc[2 * SURF_MAXSIDE];      // border pixels per row: [map][y]
  __shared__ double s_red[1024];
  __shared__ int s_max[2];
  __shared__ int s_sel[4];      // bin, rank in bin of the lower order statistic; the same of the upper
  const int pair = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t HW = (int64_t)H * W;
  int64_t* si = stats_i + (int64_t)pair * SURF_NSTAT_I;
  if (si[0] == 0 || si[1] == 0) {                     // not scored (medpy raises): the counts stay, everything else is 0
    if (tid < 4) si[4 + tid] = 0;
    if (tid < SURF_NSTAT_F) stats_f[(int64_t)pair * SURF_NSTAT_F + tid] = 0.0;
    return;
  }
  const int64_t n = si[2] + si[3];
  const int lo = (int)(95 * (n - 1) / 100), hi = (int)min((int64_t)lo + 1, n - 1);
  for (int i = tid; i < 2048; i += 1024) s_hist[i] = 0;
  for (int i = tid; i < 2 * H; i += 1024) s_rc[i] = rowcnt[((int64_t)(i / H) * np + pair) * H + i % H];
  if (tid < 2) s_max[tid] = 0;
  __syncthreads();
  // pass 1: maxima, sums, histogram of D2 >> 10.  Runs of one bin (noise: nearly every D2 is 0, 1 or 2) are counted in a register.
  int run_bin = 0, run_n = 0;
  for (int map = 0; map < 2; ++map) {
    const int32_t* v = d2 + ((int64_t)map * np + pair) * HW;
    int mx = 0;
    double sum = 0.0;
    for (int y = wave; y < H; y += 16) {
      const int c = s_rc[map * H + y];
      for (int i = lane; i < c; i += 64) {
        const int d = v[(int64_t)y * W + i];
        mx = max(mx, d);
        sum += sqrt((double)d);
        const int bin = min(d >> 10, 2047);
        if (bin != run_bin) {
          if (run_n) atomicAdd(&s_hist[run_bin], run_n);
          run_bin = bin;
          run_n = 0;
        }
        ++run_n;
      }
    }
    if (mx) atomicMax(&s_max[map], mx);
    s_red[tid] = sum;
    __syncthreads();
    for (int s = 512; s >= 1; s >>= 1) {
      if (tid < s) s_red[tid] += s_red[tid + s];
      __syncthreads();
    }
    if (tid == 0) stats_f[(int64_t)pair * SURF_NSTAT_F + map] = s_red[0];
    __syncthreads();
  }
  if (run_n) atomicAdd(&s_hist[run_bin], run_n);
  __syncthreads();
  if (tid < 64) {
    surf_select(s_hist, 2048, lo, s_sel);
    surf_select(s_hist, 2048, hi, s_sel + 2);
  }
  __syncthreads();
  const int bin_lo = s_sel[0], bin_hi = s_sel[2], r_lo = s_sel[1], r_hi = s_sel[3];
  __syncthreads();
  for (int i = tid; i < 2048; i += 1024) s_hist[i] = 0;
  __syncthreads();
  // pass 2: the low 10 bits inside the two selected bins (s_hist[0..1023] lower, [1024..2047] upper)
  int run_v = -1;
  run_n = 0;
  for (int map = 0; map < 2; ++map) {
    const int32_t* v = d2 + ((int64_t)map * np + pair) * HW;
    for (int y = wave; y < H; y += 16) {
      const int c = s_rc[map * H + y];
      for (int i = lane; i < c; i += 64) {
        const int d = v[(int64_t)y * W + i];
        if (d != run_v) {
          if (run_n) {
            if ((run_v >> 10) == bin_lo) atomicAdd(&s_hist[run_v & 1023], run_n);
            if ((run_v >> 10) == bin_hi) atomicAdd(&s_hist[1024 + (run_v & 1023)], run_n);
          }
          run_v = d;
          run_n = 0;
        }
        ++run_n;
      }
    }
  }
  if (run_n) {
    if ((run_v >> 10) == bin_lo) atomicAdd(&s_hist[run_v & 1023], run_n);
    if ((run_v >> 10) == bin_hi) atomicAdd(&s_hist[1024 + (run_v & 1023)], run_n);
  }
  __syncthreads();
  if (tid < 64) {
    surf_select(s_hist, 1024, r_lo, s_sel);
    surf_select(s_hist + 1024, 1024, r_hi, s_sel + 2);
  }
  __syncthreads();
  if (tid == 0) {
    si[4] = s_max[0];
    si[5] = s_max[1];
    si[6] = ((int64_t)bin_lo << 10) | s_sel[0];
    si[7] = ((int64_t)bin_hi << 10) | s_sel[2];
  }
}

static bool surf_dims_ok(int B, int nk, int H, int W) {
  return B >= 1 && nk >= 1 && nk <= 64 && H >= 2 && H <= SURF_MAXSIDE && W >= 2 && W <= SURF_MAXSIDE && (int64_t)B * nk <= 65535;
}

int64_t lmn_surface_workspace(int B, int nk, int H, int W) {
  if (!surf_dims_ok(B, nk, H, W)) {
    snprintf(g_lmn_err, sizeof(g_lmn_err), "surface_workspace: B=%d nk=%d %dx%d outside B >= 1, nk in [1, 64], B * nk <= 65535, sides in [2, %d]",
             B, nk, H, W, SURF_MAXSIDE);
    return -1;
  }
  const int64_t HW = (int64_t)H * W, np = (int64_t)B * nk;
  return surf_lab_bytes(B, HW) + surf_g_bytes(np, HW) + surf_d2_bytes(np, HW) + surf_rc_bytes(np, H);
}

int lmn_surface_dist(const float* pred_logits, const int64_t* pred_labels, const int64_t* target, int B, int C, int H, int W,
                     const int32_t* classes, int nk, void* workspace, int64_t ws_bytes, int64_t* stats_i, double* stats_f,
                     lmn_stream_t stream) {
  LMN_REQUIRE((pred_logits != nullptr) != (pred_labels != nullptr), "surface_dist: exactly one of pred_logits, pred_labels required");
  LMN_REQUIRE(target && classes && workspace && stats_i && stats_f, "surface_dist: null pointer");
  LMN_REQUIRE(C >= 2 && C <= 64, "surface_dist: C=%d not in [2, 64]", C);
  LMN_REQUIRE(H >= 2 && H <= SURF_MAXSIDE && W >= 2 && W <= SURF_MAXSIDE, "surface_dist: size %dx%d outside [2, %d]", H, W, SURF_MAXSIDE);
  LMN_REQUIRE(nk >= 1 && nk <= 64, "surface_dist: nk=%d not in [1, 64]", nk);
  LMN_REQUIRE(B >= 1 && (int64_t)B * nk <= 65535, "surface_dist: B=%d: B * nk outside [1, 65535]", B);
  SurfCls cls;
  memset(&cls, 0, sizeof(cls));
  for (int i = 0; i < nk; ++i) {
    LMN_REQUIRE(classes[i] >= 0 && classes[i] < C, "surface_dist: class id classes[%d] = %d outside [0, %d)", i, (int)classes[i], C);
    cls.id[i] = (uint8_t)classes[i];
  }
  const int64_t need = lmn_surface_workspace(B, nk, H, W);
  LMN_REQUIRE(ws_bytes >= need, "surface_dist: workspace of %lld bytes too small, %lld needed", (long long)ws_bytes, (long long)need);
  const int64_t HW = (int64_t)H * W, total = (int64_t)B * HW;
  const int np = B * nk;
  uint8_t* lab = (uint8_t*)workspace;
  uint16_t* g = (uint16_t*)(lab + surf_lab_bytes(B, HW));
  int32_t* d2 = (int32_t*)((uint8_t*)g + surf_g_bytes(np, HW));
  int32_t* rowcnt = (int32_t*)((uint8_t*)d2 + surf_d2_bytes(np, HW));
  hipStream_t st = (hipStream_t)stream;
  LMN_HIP_OK(hipMemsetAsync(stats_i, 0, sizeof(int64_t) * SURF_NSTAT_I * (size_t)np, st), "surface_dist");
  const int lgrid = lmn_cdiv(total, 256) < 2048 ? lmn_cdiv(total, 256) : 2048;
  LMN_LAUNCH(surf_labels_kernel, dim3(lgrid), dim3(256), 0, st, pred_logits, pred_labels, target, C, HW, total, lab);
  LMN_LAUNCH(surf_col_kernel, dim3(lmn_cdiv(W, 64), np, 2), dim3(64, SURF_SEG), 0, st, (const uint8_t*)lab, B, nk, H, W, cls, g,
             (unsigned long long*)stats_i);
  LMN_LAUNCH(surf_row_kernel, dim3(H, np, 2), dim3(lmn_cdiv(W, 64) * 64), 0, st, (const uint16_t*)g, np, H, W, (const int64_t*)stats_i, d2,
             rowcnt);
  LMN_LAUNCH(surf_finish_kernel, dim3(np), dim3(1024), 0, st, (const int32_t*)d2, (const int32_t*)rowcnt, np, H, W, stats_i, stats_f);
  return lmn_launch_status("surface_dist");
}

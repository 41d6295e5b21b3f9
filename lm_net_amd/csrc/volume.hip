// Per-case 3D surface-distance and overlap statistics on the device (lm_net_amd.metrics.VolumeSurfaceMeter; include/volume/
// lmnet_volume.h): what medpy.metric.binary dc, jc, hd, hd95, assd and ravd of a whole [D, H, W] label volume need, per class, for the
// evaluation loop the reference leaves unfinished (utils/train_eval_utils.py:7, :14-52, :178-179).  surface.hip with one more axis: an
// exact Euclidean distance transform to the border of each mask, separable over z, y, x, evaluated only at the border voxels of the
// other mask.  The border of a mask is its voxels with a 6-neighbour outside it (outside the volume counts as outside); with integer
// pitches every squared distance d2 = (kz dz)^2 + (ky dy)^2 + (kx dx)^2 is an int32 (the entry checks the bound), and the only
// floating-point values are the two float64 sums of sqrt, formed in a fixed order.  No float atomics: two runs are bit-identical.
//
//   0. vol_labels_kernel   arg-max of the logits (pred_common.h) or the given label map, and the target, narrowed to uint8
//                          (255 = no class) into the case buffers at a slice offset, once for all classes.
//   1. vol_z_kernel        per (map, class, y), one lane per (y, x) column: border test on the six neighbours -> g1(z, y, x) = steps
//                          along z to the nearest border voxel of the column (uint16, VOL_NONE where the column has none); g1 == 0
//                          marks the border voxels.  Flags the rows (z, y) that hold a border voxel.  |mask|, the border count and
//                          |P n T| go to the statistics with integer atomics, one per block.
//   2. vol_y_kernel        per (map, class, z), lanes along x, the g1 strip of the slice in LDS: g2(z, y, x) = min_j (ky (y - j))^2 +
//                          (kz g1(z, j, x))^2 (int32, VOL_SAT where the plane x has no border voxel), scanning outwards from y and
//                          stopping once (ky d)^2 >= the best so far, or past the first / last row of the column that has a g1.
//                          Only in rows where the OTHER map has a border voxel: nothing else is ever read.
//   3. vol_x_kernel        per (map, class, row): g2 of the OTHER map's row in LDS; every border voxel of this map takes
//                          min_j (kx (x - j))^2 + g2(z, y, j) with the same exact early exit.  Writes the row's D2 compacted, and
//                          their count.
//   4. vol_finish_kernel   per class: directed maxima, float64 sums of sqrt(D2) (per-thread sums over fixed rows, then a fixed tree) and
//                          the two order statistics of the pooled D2 multiset by a three-level radix select (11 + 10 + 10 bits) on
//                          integer histograms in LDS.  The row counts (up to D * H per map) are read from memory, 64 rows per wave
//                          load.
#include "pred_common.h"
#include "../../include/volume/lmnet_volume.h"

#define VOL_NONE 0xFFFF           // g1 sentinel: the column has no border voxel
#define VOL_SAT 0x7FFFFFFF        // g2 sentinel: never added to
#define VOL_FAR (1 << 20)         // "no border voxel on this side" in z arithmetic
#define VOL_MAXSIDE LMN_VOLUME_MAX_SIDE
#define VOL_SEG 16                // z segments per block of vol_z_kernel: ceil(1024 / 16) = 64 slices fit one 64-bit mask
#define VOL_YT 8                  // rows in flight per block of vol_y_kernel
#define VOL_NSTAT_I LMN_VOLUME_NSTAT_I
#define VOL_NSTAT_F LMN_VOLUME_NSTAT_F

typedef unsigned long long vol_u64;

struct VolCls { uint8_t id[64]; };

static inline int64_t vol_g1_bytes(int64_t nk, int64_t V) { return lmn_up256(2 * nk * V * (int64_t)sizeof(uint16_t)); }
static inline int64_t vol_g2_bytes(int64_t nk, int64_t V) { return lmn_up256(2 * nk * V * (int64_t)sizeof(int32_t)); }
static inline int64_t vol_rc_bytes(int64_t nk, int64_t R) { return lmn_up256(2 * nk * R * (int64_t)sizeof(int32_t)); }
static inline int64_t vol_rf_bytes(int64_t nk, int64_t R) { return lmn_up256(2 * nk * R); }

__global__ __launch_bounds__(256) void vol_labels_kernel(const float* __restrict__ logits, const int64_t* __restrict__ plab,
                                                         const int64_t* __restrict__ target, int C, int64_t hw, int64_t total,
                                                         uint8_t* __restrict__ lab_pred, uint8_t* __restrict__ lab_target) {
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    int best;
    if (logits) {
      const int64_t b = idx / hw, i = idx - b * hw;
      best = pred_argmax(logits + b * C * hw + i, C, hw);
    } else {
      best = pred_class(plab[idx], C, 255);
    }
    lab_pred[idx] = (uint8_t)best;
    lab_target[idx] = (uint8_t)pred_class(target[idx], C, 255);
  }
}

// One lane per (y, x) column and VOL_SEG z segments per block (threadIdx.y): a segment's slices (<= 64) become bit masks -- the mask
// itself and "all four in-plane neighbours inside" -- so the border test is a few 64-bit operations and the nearest border slice
// above / below any slice of the segment a clz / ffs; the nearest one outside the segment comes from the other segments through LDS.
__global__ __launch_bounds__(64 * VOL_SEG) void vol_z_kernel(const uint8_t* __restrict__ lab_pred, const uint8_t* __restrict__ lab_target,
                                                             int nk, int D, int H, int W, VolCls cls, uint16_t* __restrict__ g1,
                                                             uint8_t* __restrict__ rowflag, vol_u64* __restrict__ stats_i) {
  __shared__ int s_last[VOL_SEG][64], s_first[VOL_SEG][64];
  __shared__ int s_cnt[VOL_SEG][3];
  const int lane = threadIdx.x, seg = threadIdx.y;
  const int x = blockIdx.x * 64 + lane, y = blockIdx.y, map = blockIdx.z / nk, j = blockIdx.z - map * nk;
  const uint8_t k = cls.id[j];
  const int64_t HW = (int64_t)H * W, V = (int64_t)D * HW;
  const uint8_t* m = map ? lab_target : lab_pred;
  uint16_t* gp = g1 + ((int64_t)map * nk + j) * V + (int64_t)y * W + x;
  const int L = (D + VOL_SEG - 1) / VOL_SEG;              // <= 64 slices per segment
  const int z0 = seg * L, n = min(L, D - z0);             // (n <= 0: a segment past the last slice)
  const bool live = x < W && n > 0;
  vol_u64 mc = 0, mn = 0, mo = 0, bd = 0;
  if (live) {
    const int64_t off = (int64_t)z0 * HW + (int64_t)y * W + x;
    const uint8_t* r = m + off;
    const bool hl = x > 0, hr = x + 1 < W, hu = y > 0, hd = y + 1 < H;
    for (int i = 0; i < n; ++i) {
      const uint8_t* q = r + (int64_t)i * HW;
      mc |= (vol_u64)(q[0] == k) << i;
      mn |= (vol_u64)((hl && q[-1] == k) && (hr && q[1] == k) && (hu && q[-W] == k) && (hd && q[W] == k)) << i;
    }
    if (map == 0) {                                       // |P n T| is counted once, by the prediction's blocks
      const uint8_t* o = lab_target + off;
      for (int i = 0; i < n; ++i) mo |= (vol_u64)(o[(int64_t)i * HW] == k) << i;
    }
    const vol_u64 up = (mc << 1) | (vol_u64)(z0 > 0 && r[-HW] == k);
    const vol_u64 dn = (mc >> 1) | ((vol_u64)(z0 + n < D && r[(int64_t)n * HW] == k) << (n - 1));
    bd = mc & ~(up & dn & mn);
  }
  s_last[seg][lane] = bd ? z0 + 63 - __clzll((long long)bd) : -VOL_FAR;
  s_first[seg][lane] = bd ? z0 + __ffsll((long long)bd) - 1 : VOL_FAR;
  int cnt = __popcll(mc), nb = __popcll(bd), both = __popcll(mc & mo);
  unsigned any_lo = (unsigned)bd, any_hi = (unsigned)(bd >> 32);
#pragma unroll
  for (int s = 1; s <= 32; s <<= 1) {
    cnt += __shfl_xor(cnt, s, 64);
    nb += __shfl_xor(nb, s, 64);
    both += __shfl_xor(both, s, 64);
    any_lo |= __shfl_xor(any_lo, s, 64);
    any_hi |= __shfl_xor(any_hi, s, 64);
  }
  if (lane == 0) { s_cnt[seg][0] = cnt; s_cnt[seg][1] = nb; s_cnt[seg][2] = both; }
  // the rows (z, y) of this segment in which some lane of the wave has a border voxel (every writer stores the same 1)
  const vol_u64 any = ((vol_u64)any_hi << 32) | any_lo;
  if (lane < n && ((any >> lane) & 1)) rowflag[(((int64_t)map * nk + j) * D + z0 + lane) * H + y] = 1;
  __syncthreads();
  if (live) {
    int above = -VOL_FAR, below = VOL_FAR;
    for (int s = 0; s < seg; ++s) above = max(above, s_last[s][lane]);
    for (int s = seg + 1; s < VOL_SEG; ++s) below = min(below, s_first[s][lane]);
    for (int i = 0; i < n; ++i) {
      const int z = z0 + i;
      const vol_u64 lo = bd & (~0ull >> (63 - i)), hi = bd >> i;
      const int la = lo ? z0 + 63 - __clzll((long long)lo) : above;
      const int nx = hi ? z + __ffsll((long long)hi) - 1 : below;
      gp[(int64_t)z * HW] = (uint16_t)min(min(z - la, nx - z), VOL_NONE);
    }
  }
  if (lane == 0 && seg == 0) {
    cnt = 0, nb = 0, both = 0;
    for (int s = 0; s < VOL_SEG; ++s) { cnt += s_cnt[s][0]; nb += s_cnt[s][1]; both += s_cnt[s][2]; }
    if (cnt) {
      atomicAdd(stats_i + (int64_t)j * VOL_NSTAT_I + map, (vol_u64)cnt);
      atomicAdd(stats_i + (int64_t)j * VOL_NSTAT_I + 2 + map, (vol_u64)nb);
    }
    if (both) atomicAdd(stats_i + (int64_t)j * VOL_NSTAT_I + 8, (vol_u64)both);
  }
}

// g2 of map `map` in slice z: needed in the rows where the other map has a border voxel (vol_x_kernel reads no other row).  The
// strip of 64 columns x H rows of g1 sits in LDS ([y][lane]: a wave's reads of one row are 128 contiguous bytes).
__global__ __launch_bounds__(64 * VOL_YT) void vol_y_kernel(const uint16_t* __restrict__ g1, const uint8_t* __restrict__ rowflag, int nk,
                                                            int D, int H, int W, int kz, int ky, int32_t* __restrict__ g2) {
  extern __shared__ uint16_t s_g1[];                      // [H][64]
  __shared__ int s_any;
  __shared__ int s_lo[64], s_hi[64];
  const int lane = threadIdx.x, ty = threadIdx.y;
  const int x = blockIdx.x * 64 + lane, z = blockIdx.y, map = blockIdx.z / nk, j = blockIdx.z - map * nk;
  const int64_t HW = (int64_t)H * W, V = (int64_t)D * HW;
  const uint8_t* need = rowflag + (((int64_t)(1 - map) * nk + j) * D + z) * H;
  if (lane == 0 && ty == 0) s_any = 0;
  __syncthreads();
  int any = 0;
  for (int y = ty; y < H; y += VOL_YT) any |= need[y];
  if (any && lane == 0) s_any = 1;
  __syncthreads();
  if (!s_any) return;                                     // (block-uniform)
  const int64_t base = ((int64_t)map * nk + j) * V + (int64_t)z * HW;
  if (ty == 0) { s_lo[lane] = H; s_hi[lane] = -1; }
  __syncthreads();
  int lo = H, hi = -1;                                    // first and last row of the lane's column that has a g1
  for (int y = ty; y < H; y += VOL_YT) {
    const uint16_t g = x < W ? g1[base + (int64_t)y * W + x] : (uint16_t)VOL_NONE;
    s_g1[y * 64 + lane] = g;
    if (g != VOL_NONE) { lo = min(lo, y); hi = y; }
  }
  if (hi >= 0) { atomicMin(&s_lo[lane], lo); atomicMax(&s_hi[lane], hi); }
  __syncthreads();
  if (x >= W) return;
  lo = s_lo[lane];
  hi = s_hi[lane];
  for (int y = ty; y < H; y += VOL_YT) {
    if (!need[y]) continue;
    int g = s_g1[y * 64 + lane];
    int best = VOL_SAT;
    if (g != VOL_NONE) best = (kz * g) * (kz * g);
    const int dmax = max(y - lo, hi - y);                 // (no row beyond it has a term; a column without any: no scan, VOL_SAT)
    for (int d = 1; d <= dmax; ++d) {
      const int dd = (ky * d) * (ky * d);
      if (dd >= best) break;                              // exact: every later term is >= (ky d)^2
      if (y - d >= 0 && (g = s_g1[(y - d) * 64 + lane]) != VOL_NONE) best = min(best, dd + (kz * g) * (kz * g));
      if (y + d < H && (g = s_g1[(y + d) * 64 + lane]) != VOL_NONE) best = min(best, dd + (kz * g) * (kz * g));
    }
    g2[base + (int64_t)y * W + x] = best;
  }
}

// The D2 of a row's border voxels are written compacted to the front of the row (in x order) with their count beside them, so the
// finish kernel reads border voxels only.  A row without a border voxel of this map, or a class whose other map has no border at
// all, gets the count 0 and nothing else.
__global__ __launch_bounds__(1024) void vol_x_kernel(const uint16_t* __restrict__ g1, const int32_t* __restrict__ g2,
                                                     const uint8_t* __restrict__ rowflag, int nk, int64_t R, int W, int kx,
                                                     const int64_t* __restrict__ stats_i, int32_t* __restrict__ d2,
                                                     int32_t* __restrict__ rowcnt) {
  __shared__ int s_g2[VOL_MAXSIDE];
  __shared__ int s_wn[VOL_MAXSIDE / 64];
  const int64_t row = blockIdx.x;
  const int j = blockIdx.y, map = blockIdx.z, x = threadIdx.x;
  const int64_t rid = ((int64_t)map * nk + j) * R + row;
  const int64_t self = rid * W, other = (((int64_t)(1 - map) * nk + j) * R + row) * W;
  const bool scored = stats_i[(int64_t)j * VOL_NSTAT_I + 2 + (1 - map)] > 0;   // the other map has a border (block-uniform)
  if (!scored || !rowflag[rid]) {
    if (x == 0) rowcnt[rid] = 0;
    return;
  }
  if (x < W) s_g2[x] = g2[other + x];
  __syncthreads();
  int r = -1;
  if (x < W && g1[self + x] == 0) {
    int best = s_g2[x];
    for (int d = 1; d < W; ++d) {
      const int dd = (kx * d) * (kx * d);
      if (dd >= best) break;
      int v;
      if (x - d >= 0 && (v = s_g2[x - d]) != VOL_SAT) best = min(best, dd + v);
      if (x + d < W && (v = s_g2[x + d]) != VOL_SAT) best = min(best, dd + v);
    }
    r = best;
  }
  const vol_u64 vote = __ballot(r >= 0);
  const int wave = x >> 6, lane = x & 63, nw = blockDim.x >> 6;
  if (lane == 0) s_wn[wave] = __popcll(vote);
  __syncthreads();
  int off = 0, total = 0;
  for (int w = 0; w < nw; ++w) {
    if (w < wave) off += s_wn[w];
    total += s_wn[w];
  }
  if (r >= 0) d2[self + off + __popcll(vote & ((1ull << lane) - 1))] = r;
  if (x == 0) rowcnt[rid] = total;
}

// f(d) for every D2 of one map and class, in a fixed assignment: wave w of 16 takes the rows [64 w, 64 w + 64) of every 1024, reads
// their counts with one load and walks the non-empty ones in order, lanes striding over a row's values.
template <typename F>
__device__ __forceinline__ void vol_each(const int32_t* __restrict__ v, const int32_t* __restrict__ rc, int64_t R, int W, int wave, int lane,
                                         F f) {
  for (int64_t base = (int64_t)wave * 64; base < R; base += 16 * 64) {
    const int64_t row = base + lane;
    const int c = row < R ? rc[row] : 0;
    vol_u64 m = __ballot(c > 0);
    while (m) {                                           // (wave-uniform)
      const int b = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int cb = __shfl(c, b, 64);
      const int32_t* p = v + (base + b) * W;
      for (int i = lane; i < cb; i += 64) f(p[i]);
    }
  }
}

// bin and rank inside the bin of the element of rank `rank` in a histogram of nb bins (nb a multiple of 64); run by wave 0
__device__ __forceinline__ void vol_select(const unsigned* hist, int nb, long long rank, int* bin, long long* within) {
  const int lane = threadIdx.x, per = nb >> 6;
  long long sum = 0;
  for (int i = 0; i < per; ++i) sum += hist[lane * per + i];
  long long inc = sum;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const unsigned lo = __shfl_up((unsigned)inc, s, 64), hi = __shfl_up((unsigned)(inc >> 32), s, 64);
    if (lane >= s) inc += (long long)(((vol_u64)hi << 32) | lo);
  }
  long long before = inc - sum;
  if (rank >= before && rank < inc) {
    for (int i = 0; i < per; ++i) {
      const long long h = hist[lane * per + i];
      if (rank < before + h) {
        *bin = lane * per + i;
        *within = rank - before;
        break;
      }
      before += h;
    }
  }
}

// adds runs of one key to an LDS histogram: noise gives long runs of 0, 1, 2, counted in a register
struct VolRun {
  int key = -1, n = 0;
  __device__ __forceinline__ void flush(unsigned* hist) { if (n) atomicAdd(&hist[key], (unsigned)n); n = 0; }
  __device__ __forceinline__ void add(unsigned* hist, int k) {
    if (k != key) { flush(hist); key = k; }
    ++n;
  }
};

__global__ __launch_bounds__(1024) void vol_finish_kernel(const int32_t* __restrict__ d2, const int32_t* __restrict__ rowcnt, int nk,
                                                          int64_t R, int W, int64_t* __restrict__ stats_i, double* __restrict__ stats_f) {
  __shared__ unsigned s_hist[2048];
  __shared__ double s_red[1024];
  __shared__ int s_max[2];
  __shared__ int s_bin[2];              // of the lower order statistic, of the upper
  __shared__ long long s_rank[2];
  const int j = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int64_t* si = stats_i + (int64_t)j * VOL_NSTAT_I;
  if (si[0] == 0 || si[1] == 0) {                     // not scored (medpy raises): the counts stay, everything else is 0
    if (tid < 4) si[4 + tid] = 0;
    if (tid < VOL_NSTAT_F) stats_f[(int64_t)j * VOL_NSTAT_F + tid] = 0.0;
    return;
  }
  const int64_t n = si[2] + si[3];
  const long long lo = 95 * (n - 1) / 100, hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
  const int32_t* v[2] = {d2 + (int64_t)j * R * W, d2 + ((int64_t)nk + j) * R * W};
  const int32_t* rc[2] = {rowcnt + (int64_t)j * R, rowcnt + ((int64_t)nk + j) * R};
  for (int i = tid; i < 2048; i += 1024) s_hist[i] = 0;
  if (tid < 2) s_max[tid] = 0;
  __syncthreads();
  // level 1: maxima, sums, histogram of the top 11 bits
  VolRun run;
  for (int map = 0; map < 2; ++map) {
    int mx = 0;
    double sum = 0.0;
    vol_each(v[map], rc[map], R, W, wave, lane, [&](int d) {
      mx = max(mx, d);
      sum += sqrt((double)d);
      run.add(s_hist, d >> 20);
    });
    if (mx) atomicMax(&s_max[map], mx);
    s_red[tid] = sum;
    __syncthreads();
    for (int s = 512; s >= 1; s >>= 1) {
      if (tid < s) s_red[tid] += s_red[tid + s];
      __syncthreads();
    }
    if (tid == 0) stats_f[(int64_t)j * VOL_NSTAT_F + map] = s_red[0];
    __syncthreads();
  }
  run.flush(s_hist);
  __syncthreads();
  if (tid < 64) {
    vol_select(s_hist, 2048, lo, &s_bin[0], &s_rank[0]);
    vol_select(s_hist, 2048, hi, &s_bin[1], &s_rank[1]);
  }
  __syncthreads();
  int pre_lo = s_bin[0], pre_hi = s_bin[1];             // the bits of the two order statistics known so far
  long long r_lo = s_rank[0], r_hi = s_rank[1];
  // levels 2 and 3: the next 10 bits inside the two selected prefixes (s_hist[0..1023] lower, [1024..2047] upper)
  for (int shift = 10; shift >= 0; shift -= 10) {
    __syncthreads();
    for (int i = tid; i < 2048; i += 1024) s_hist[i] = 0;
    __syncthreads();
    VolRun a, b;
    for (int map = 0; map < 2; ++map) {
      vol_each(v[map], rc[map], R, W, wave, lane, [&](int d) {
        const int pre = d >> (shift + 10), bits = (d >> shift) & 1023;
        if (pre == pre_lo) a.add(s_hist, bits);
        if (pre == pre_hi) b.add(s_hist + 1024, bits);
      });
    }
    a.flush(s_hist);
    b.flush(s_hist + 1024);
    __syncthreads();
    if (tid < 64) {
      vol_select(s_hist, 1024, r_lo, &s_bin[0], &s_rank[0]);
      vol_select(s_hist + 1024, 1024, r_hi, &s_bin[1], &s_rank[1]);
    }
    __syncthreads();
    pre_lo = (pre_lo << 10) | s_bin[0];
    pre_hi = (pre_hi << 10) | s_bin[1];
    r_lo = s_rank[0];
    r_hi = s_rank[1];
  }
  if (tid == 0) {
    si[4] = s_max[0];
    si[5] = s_max[1];
    si[6] = pre_lo;
    si[7] = pre_hi;
  }
}

static bool vol_dims_ok(int D, int H, int W) {
  return D >= 1 && D <= VOL_MAXSIDE && H >= 2 && H <= VOL_MAXSIDE && W >= 2 && W <= VOL_MAXSIDE;
}

int64_t lmn_volume_workspace(int D, int H, int W, int nk) {
  if (!vol_dims_ok(D, H, W) || nk < 1 || nk > 64) {
    snprintf(g_lmn_err, sizeof(g_lmn_err), "volume_workspace: D=%d %dx%d nk=%d outside D in [1, %d], sides in [2, %d], nk in [1, 64]", D, H,
             W, nk, VOL_MAXSIDE, VOL_MAXSIDE);
    return -1;
  }
  const int64_t R = (int64_t)D * H, V = R * W;
  return vol_g1_bytes(nk, V) + 2 * vol_g2_bytes(nk, V) + vol_rc_bytes(nk, R) + vol_rf_bytes(nk, R);
}

int lmn_volume_labels(const float* pred_logits, const int64_t* pred_labels, const int64_t* target, int n, int C, int H, int W,
                      uint8_t* lab_pred, uint8_t* lab_target, int D_cap, int z0, lmn_stream_t stream) {
  LMN_REQUIRE((pred_logits != nullptr) != (pred_labels != nullptr), "volume_labels: exactly one of pred_logits, pred_labels required");
  LMN_REQUIRE(target && lab_pred && lab_target, "volume_labels: null pointer");
  LMN_REQUIRE(C >= 2 && C <= 64, "volume_labels: C=%d not in [2, 64]", C);
  LMN_REQUIRE(H >= 2 && H <= VOL_MAXSIDE && W >= 2 && W <= VOL_MAXSIDE, "volume_labels: size %dx%d outside [2, %d]", H, W, VOL_MAXSIDE);
  LMN_REQUIRE(D_cap >= 1 && D_cap <= VOL_MAXSIDE, "volume_labels: D_cap=%d not in [1, %d]", D_cap, VOL_MAXSIDE);
  LMN_REQUIRE(n >= 1 && z0 >= 0 && (int64_t)z0 + n <= D_cap, "volume_labels: slices [%d, %d + %d) outside the case buffer of %d slices", z0,
              z0, n, D_cap);
  const int64_t HW = (int64_t)H * W, total = (int64_t)n * HW;
  const int grid = lmn_cdiv(total, 256) < 2048 ? lmn_cdiv(total, 256) : 2048;
  LMN_LAUNCH(vol_labels_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, pred_logits, pred_labels, target, C, HW, total,
             lab_pred + (int64_t)z0 * HW, lab_target + (int64_t)z0 * HW);
  return lmn_launch_status("volume_labels");
}

int lmn_volume_dist(const uint8_t* lab_pred, const uint8_t* lab_target, int D, int H, int W, int C, const int32_t* classes, int nk,
                    int kz, int ky, int kx, void* workspace, int64_t ws_bytes, int64_t* stats_i, double* stats_f, lmn_stream_t stream) {
  LMN_REQUIRE(lab_pred && lab_target && classes && workspace && stats_i && stats_f, "volume_dist: null pointer");
  LMN_REQUIRE(C >= 2 && C <= 64, "volume_dist: C=%d not in [2, 64]", C);
  LMN_REQUIRE(D >= 1 && D <= VOL_MAXSIDE, "volume_dist: D=%d not in [1, %d]", D, VOL_MAXSIDE);
  LMN_REQUIRE(H >= 2 && H <= VOL_MAXSIDE && W >= 2 && W <= VOL_MAXSIDE, "volume_dist: size %dx%d outside [2, %d]", H, W, VOL_MAXSIDE);
  LMN_REQUIRE(nk >= 1 && nk <= 64, "volume_dist: nk=%d not in [1, 64]", nk);
  LMN_REQUIRE(kz >= 1 && ky >= 1 && kx >= 1, "volume_dist: pitches (%d, %d, %d) must be positive integers", kz, ky, kx);
  // every extent below 2^16 first, so that the squares and their sum stay far inside an int64
  const int64_t ez = (int64_t)kz * (D - 1), ey = (int64_t)ky * (H - 1), ex = (int64_t)kx * (W - 1);
  LMN_REQUIRE(ez < 65536 && ey < 65536 && ex < 65536, "volume_dist: extents (%lld, %lld, %lld) = pitch * (side - 1): "
              "(kz (D-1))^2 + (ky (H-1))^2 + (kx (W-1))^2 must be < 2^31", (long long)ez, (long long)ey, (long long)ex);
  const int64_t span = ez * ez + ey * ey + ex * ex;
  LMN_REQUIRE(span < ((int64_t)1 << 31), "volume_dist: (kz (D-1))^2 + (ky (H-1))^2 + (kx (W-1))^2 = %lld must be < 2^31 = 2147483648",
              (long long)span);
  VolCls cls;
  memset(&cls, 0, sizeof(cls));
  for (int i = 0; i < nk; ++i) {
    LMN_REQUIRE(classes[i] >= 0 && classes[i] < C, "volume_dist: class id classes[%d] = %d outside [0, %d)", i, (int)classes[i], C);
    cls.id[i] = (uint8_t)classes[i];
  }
  const int64_t need = lmn_volume_workspace(D, H, W, nk);
  LMN_REQUIRE(ws_bytes >= need, "volume_dist: workspace of %lld bytes too small, %lld needed", (long long)ws_bytes, (long long)need);
  const int64_t R = (int64_t)D * H, V = R * W;
  uint16_t* g1 = (uint16_t*)workspace;
  int32_t* g2 = (int32_t*)((uint8_t*)g1 + vol_g1_bytes(nk, V));
  int32_t* d2 = (int32_t*)((uint8_t*)g2 + vol_g2_bytes(nk, V));
  int32_t* rowcnt = (int32_t*)((uint8_t*)d2 + vol_g2_bytes(nk, V));
  uint8_t* rowflag = (uint8_t*)rowcnt + vol_rc_bytes(nk, R);
  hipStream_t st = (hipStream_t)stream;
  LMN_HIP_OK(hipMemsetAsync(stats_i, 0, sizeof(int64_t) * VOL_NSTAT_I * (size_t)nk, st), "volume_dist");
  LMN_HIP_OK(hipMemsetAsync(rowflag, 0, (size_t)(2 * nk * R), st), "volume_dist");
  const int xt = lmn_cdiv(W, 64);
  LMN_LAUNCH(vol_z_kernel, dim3(xt, H, 2 * nk), dim3(64, VOL_SEG), 0, st, lab_pred, lab_target, nk, D, H, W, cls, g1, rowflag,
             (vol_u64*)stats_i);
  const size_t sh = (size_t)H * 64 * sizeof(uint16_t);    // <= 128 KiB of the CU's 160
  if (sh > 64 * 1024) (void)hipFuncSetAttribute((const void*)vol_y_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
  LMN_LAUNCH(vol_y_kernel, dim3(xt, D, 2 * nk), dim3(64, VOL_YT), sh, st, (const uint16_t*)g1, (const uint8_t*)rowflag, nk, D, H, W, kz, ky,
             g2);
  LMN_LAUNCH(vol_x_kernel, dim3((unsigned)R, nk, 2), dim3(xt * 64), 0, st, (const uint16_t*)g1, (const int32_t*)g2, (const uint8_t*)rowflag,
             nk, R, W, kx, (const int64_t*)stats_i, d2, rowcnt);
  LMN_LAUNCH(vol_finish_kernel, dim3(nk), dim3(1024), 0, st, (const int32_t*)d2, (const int32_t*)rowcnt, nk, R, W, stats_i, stats_f);
  return lmn_launch_status("volume_dist");
}

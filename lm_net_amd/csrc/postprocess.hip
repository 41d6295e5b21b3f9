// Post-processing of predictions on the device (lm_net_amd.post.DevicePostprocess): arg-max, connected-component cleaning (keep the
// largest component of a class, drop components below an area, fill holes), the nearest resize back to the frame and the overlay --
// what the reference's --test / --visualization modes do on the host after .cpu() (train.py:139-145, 182-197,
// utils/train_eval_utils.py:203-221).  Integer arithmetic throughout (the arg-max compare and the two double quotients of the resize
// are the only floating-point operations); every cross-block sum is an int32 atomic add and every selection an integer atomic
// max / min, so the result does not depend on arrival order: two calls on one input give bit-identical outputs.
//
// Connected-component labelling (lmn_cc_label, and twice inside lmn_post_clean), 8- or 4-connected, every label value partitioned:
//   1. cc_tile_kernel     one 256-thread block labels a CC_TH x CC_TW = 32 x 64 tile inside LDS (2 KiB of labels + 8 KiB of
//                         tile-local parents = 10 KiB per block): row runs first, then lock-free unions of vertically / diagonally
//                         adjacent runs, then every pixel writes the tile root of its component as an image pixel index.
//   2. cc_seam_kernel     one thread per pixel next to a tile seam unites the trees across the seam in the global parent array.
//   3. cc_flatten_kernel  every pixel finds its root (in place), adds 1 to areas[root] (pre-reduced per wave) and, for the hole
//                         labelling, marks roots of components that touch the image frame (a bit of the area word).
// A parent is always the smaller index, so a component's root is its smallest row-major pixel index.  No kernel waits for another
// block: every loop is a find / union loop that either lowers a parent or ends.  The tile and the seam pass, the union-find and the
// argument for its safety are in cc_common.h, shared with the 3D cleaning (volpost.hip); the index space here is the image's pixel
// index: pointers offset by the image, base 0, labels clamped by post_labels_kernel beforehand.
//
// Cleaning (lmn_post_clean):
//   4. post_labels_kernel arg-max (pred_common.h) or the given label map -> uint8 L0 (outside [0, C) -> 0)
//   5. post_select_kernel root pixels offer (area << 32 | ~root) to their (sample, class) slot: block-level max in LDS, then one
//                         64-bit atomic max per block and slot; counts components per class.
//   6. post_apply_kernel  L1 = L0 without the components that do not survive keep_largest / min_area.
//   7. (labelling of L1's zero pixels under the dual connectivity) post_fill_kernel: holes take the label left of their root pixel;
//      per-class pixel counts and the number of holes.
// Render (lmn_post_render): post_render_kernel, one launch per 64 samples of a ragged batch: nearest resize to the frame (the
// lmn_preprocess_u8 mask arithmetic with source and destination exchanged), 16 pixels per thread with 16-byte stores, fill or contour
// overlay blended in 8-bit fixed point.  No frame-size intermediate.
#include "cc_common.h"
#include "pred_common.h"

#define POST_MAXSIDE 1024
#define POST_FRAME_BIT (1 << 30)                // areas are < 2^21
#define POST_RCHUNK 64                          // samples per render launch
#define POST_PPB 1024                           // pixels per block of the select and fill passes

namespace {

struct PostRender {
  int32_t hw[POST_RCHUNK][2];
  uint8_t pal[64][4];
};

// The tile and the seam pass of image blockIdx.z / blockIdx.y (cc_common.h; no C: the labels are clamped already).
// only_zero: the hole labelling -- pixels of a non-zero label join nothing (they stay their own roots and are not counted)
__global__ __launch_bounds__(256) void cc_tile_kernel(const uint8_t* __restrict__ lab, int H, int W, int conn8, int only_zero,
                                                      int32_t* __restrict__ parent) {
  const int64_t img = (int64_t)blockIdx.z * H * W;
  cc_tile_body<false>(lab + img, parent + img, 0, H, W, 0, conn8, only_zero);
}

__global__ __launch_bounds__(256) void cc_seam_kernel(const uint8_t* __restrict__ lab, int H, int W, int conn8, int only_zero,
                                                      int32_t* parent) {
  const int64_t img = (int64_t)blockIdx.y * H * W;
  cc_seam_body<false>(lab + img, parent + img, 0, H, W, 0, conn8, only_zero);
}

__global__ __launch_bounds__(256) void cc_flatten_kernel(const uint8_t* __restrict__ lab, int H, int W, int only_zero, int mark_frame,
                                                         int32_t* roots, int32_t* __restrict__ areas) {
  const int HW = H * W, i = blockIdx.x * 256 + threadIdx.x;
  const int64_t img = (int64_t)blockIdx.y * HW;
  int32_t* A = areas + img;
  bool counted = false;
  int r = -1;
  if (i < HW && !(only_zero && lab[img + i] != 0)) {
    counted = true;
    r = cc_root_store(roots + img, i);
    if (mark_frame) {
      const int y = i / W, x = i - y * W;
      if (y == 0 || y == H - 1 || x == 0 || x == W - 1) atomicOr(A + r, POST_FRAME_BIT);
    }
  }
  cc_wave_count(counted, r, A);
}

__global__ __launch_bounds__(256) void post_labels_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ lab8,
                                                          const int64_t* __restrict__ lab64, int C, int64_t hw, int64_t total,
                                                          uint8_t* __restrict__ out) {
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    int best;
    if (logits) {
      const int64_t b = idx / hw, i = idx - b * hw;
      best = pred_argmax(logits + b * C * hw + i, C, hw);
    } else if (lab8) {
      best = pred_class(lab8[idx], C, 0);
    } else {
      best = pred_class(lab64[idx], C, 0);
    }
    out[idx] = (uint8_t)best;
  }
}

// The packed key (cc_common.h) settles "largest area, then smallest root" by itself.  A block reduces its offers per class in LDS
// first, so a map in which every pixel is a root (the 4-connected checkerboard) still issues one global atomic per block and class.
__global__ __launch_bounds__(256) void post_select_kernel(const uint8_t* __restrict__ lab, const int32_t* __restrict__ roots,
                                                          const int32_t* __restrict__ areas, int HW, int C, lmn_post_param_t prm,
                                                          unsigned long long* __restrict__ best, int32_t* __restrict__ stats) {
  __shared__ unsigned long long s_best[64];
  __shared__ int s_n[64], s_pass[64];
  if (threadIdx.x < 64) {
    s_best[threadIdx.x] = 0;
    s_n[threadIdx.x] = 0;
    s_pass[threadIdx.x] = 0;
  }
  __syncthreads();
  const int b = blockIdx.y;
  const int64_t img = (int64_t)b * HW;
  for (int it = 0; it < POST_PPB / 256; ++it) {
    const int i = blockIdx.x * POST_PPB + it * 256 + threadIdx.x;
    if (i < HW && roots[img + i] == i) {
      const int k = lab[img + i], a = areas[img + i];
      atomicAdd(&s_n[k], 1);
      if ((prm.keep_largest_mask >> k) & 1) atomicMax(&s_best[k], cc_key(a, i));
      else if (!((prm.class_mask >> k) & 1) || a >= prm.min_area[k]) atomicAdd(&s_pass[k], 1);
    }
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < C) {
    if (s_n[k]) atomicAdd(stats + ((int64_t)b * C + k) * 4, s_n[k]);
    if (s_pass[k]) atomicAdd(stats + ((int64_t)b * C + k) * 4 + 1, s_pass[k]);
    if (s_best[k]) atomicMax(best + (int64_t)b * 64 + k, s_best[k]);
  }
}

__global__ __launch_bounds__(256) void post_apply_kernel(const uint8_t* __restrict__ lab, const int32_t* __restrict__ roots,
                                                         const int32_t* __restrict__ areas, int HW, int C, lmn_post_param_t prm,
                                                         const unsigned long long* __restrict__ best, uint8_t* __restrict__ out,
                                                         int32_t* __restrict__ stats) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  const int64_t img = (int64_t)b * HW;
  if (blockIdx.x == 0 && threadIdx.x < C && ((prm.keep_largest_mask >> threadIdx.x) & 1)) {   // survivors of a keep_largest class
    const unsigned long long w = best[(int64_t)b * 64 + threadIdx.x];
    stats[((int64_t)b * C + threadIdx.x) * 4 + 1] = (w != 0 && cc_key_size(w) >= prm.min_area[threadIdx.x]) ? 1 : 0;
  }
  if (i >= HW) return;
  int k = lab[img + i];
  if ((prm.class_mask >> k) & 1) {
    const int r = roots[img + i];
    bool keep = areas[img + r] >= prm.min_area[k];
    if ((prm.keep_largest_mask >> k) & 1) keep = keep && cc_key_root(best[(int64_t)b * 64 + k]) == r;
    if (!keep) k = 0;
  }
  out[img + i] = (uint8_t)k;
}

// roots / areas: the labelling of lab's zero pixels under the dual connectivity with frame marks, or NULL (no hole filling)
__global__ __launch_bounds__(256) void post_fill_kernel(const uint8_t* __restrict__ lab, const int32_t* __restrict__ roots,
                                                        const int32_t* __restrict__ areas, int HW, int C, int hole_limit,
                                                        uint8_t* __restrict__ out, int32_t* __restrict__ stats) {
  __shared__ int s_cnt[64];
  __shared__ int s_holes;
  if (threadIdx.x < 64) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x == 0) s_holes = 0;
  __syncthreads();
  const int b = blockIdx.y;
  const int64_t img = (int64_t)b * HW;
  for (int it = 0; it < POST_PPB / 256; ++it) {                 // (a uniform trip count: every lane reaches cc_wave_count's ballots)
    const int i = blockIdx.x * POST_PPB + it * 256 + threadIdx.x;
    int k = -1;
    if (i < HW) {
      k = lab[img + i];
      if (roots && k == 0) {
        const int r = roots[img + i], a = areas[img + r];
        if (!(a & POST_FRAME_BIT) && a <= hole_limit) {
          k = lab[img + r - 1];                // left of the root: inside the image (the hole does not touch the frame), not 0
          if (r == i) atomicAdd(&s_holes, 1);
        }
      }
      out[img + i] = (uint8_t)k;
    }
    cc_wave_count(k >= 0, k, s_cnt);
  }
  __syncthreads();
  if (threadIdx.x < C && s_cnt[threadIdx.x]) atomicAdd(stats + ((int64_t)b * C + threadIdx.x) * 4 + 2, s_cnt[threadIdx.x]);
  if (threadIdx.x == 0 && s_holes) atomicAdd(stats + (int64_t)b * C * 4 + 3, s_holes);
}

// label of frame pixel (y, x) of chunk sample b, -1 outside the sample's valid area
__device__ __forceinline__ int render_label(const uint8_t* __restrict__ lab, int H, int W, const int (*hw)[2], const double* fy,
                                            const double* fx, int b, int y, int x) {
  if (y < 0 || x < 0 || y >= hw[b][0] || x >= hw[b][1]) return -1;
  const int sy = min((int)floor(y * fy[b]), H - 1), sx = min((int)floor(x * fx[b]), W - 1);
  return lab[((int64_t)b * H + sy) * W + sx];
}

// 16 consecutive bytes of the chunk's [nb, Hs, Ws] label plane per thread (they may run over a row or sample end)
__global__ __launch_bounds__(256) void post_render_kernel(const uint8_t* __restrict__ lab, int H, int W, int Hs, int Ws, int nb,
                                                          PostRender rp, const uint8_t* __restrict__ frames, int ch, int a256, int contour,
                                                          uint8_t* __restrict__ lout, uint8_t* __restrict__ ovl) {
  __shared__ int s_hw[POST_RCHUNK][2];
  __shared__ double s_fy[POST_RCHUNK], s_fx[POST_RCHUNK];
  __shared__ uint8_t s_pal[64][4];
  if (threadIdx.x < POST_RCHUNK) {
    const int b = threadIdx.x;
    s_hw[b][0] = rp.hw[b][0];
    s_hw[b][1] = rp.hw[b][1];
    s_fy[b] = b < nb ? (double)H / (double)rp.hw[b][0] : 0.0;
    s_fx[b] = b < nb ? (double)W / (double)rp.hw[b][1] : 0.0;
    *reinterpret_cast<uint32_t*>(s_pal[b]) = *reinterpret_cast<const uint32_t*>(rp.pal[b]);
  }
  __syncthreads();
  const int64_t plane = (int64_t)Hs * Ws, total = plane * nb;
  const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
  if (g >= total) return;
  const int n = (int)min((int64_t)16, total - g);
  int b = (int)(g / plane);
  const int64_t rem = g - (int64_t)b * plane;
  int y = (int)(rem / Ws), x = (int)(rem - (int64_t)y * Ws);
  uint32_t lw[4] = {0, 0, 0, 0}, ow[12], fw[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) ow[q] = fw[q] = 0;
  if (ovl) {                                                   // the 16 pixels' frame bytes: 16-byte loads where all 16 exist
    const uint8_t* f = frames + g * ch;
    const int nw = ch == 3 ? 12 : 4;
    if (n == 16) {
#pragma unroll
      for (int q = 0; q < 12; q += 4) {
        if (q < nw) {
          const uint4 v = *reinterpret_cast<const uint4*>(f + q * 4);
          fw[q] = v.x; fw[q + 1] = v.y; fw[q + 2] = v.z; fw[q + 3] = v.w;
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < 12; ++q) {
        uint32_t v = 0;
        for (int s = 0; s < 4; ++s)
          if (q * 4 + s < n * ch) v |= (uint32_t)f[q * 4 + s] << (8 * s);
        fw[q] = v;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (j < n) {
      const int l = render_label(lab, H, W, s_hw, s_fy, s_fx, b, y, x);
      if (l > 0) lw[j >> 2] |= (uint32_t)l << (8 * (j & 3));
      if (ovl && l >= 0) {
        bool paint = l > 0;
        if (paint && contour)
          paint = render_label(lab, H, W, s_hw, s_fy, s_fx, b, y - 1, x) != l || render_label(lab, H, W, s_hw, s_fy, s_fx, b, y + 1, x) != l ||
                  render_label(lab, H, W, s_hw, s_fy, s_fx, b, y, x - 1) != l || render_label(lab, H, W, s_hw, s_fy, s_fx, b, y, x + 1) != l;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int src = ch == 3 ? 3 * j + c : j;
          int v = (fw[src >> 2] >> (8 * (src & 3))) & 255;
          if (paint) v = ((256 - a256) * v + a256 * (int)s_pal[l][c] + 128) >> 8;
          const int dst = 3 * j + c;
          ow[dst >> 2] |= (uint32_t)v << (8 * (dst & 3));
        }
      }
      if (++x == Ws) {
        x = 0;
        if (++y == Hs) { y = 0; ++b; }
      }
    }
  }
  if (n == 16) {
    if (lout) *reinterpret_cast<uint4*>(lout + g) = uint4{lw[0], lw[1], lw[2], lw[3]};
    if (ovl) {
      uint4* o = reinterpret_cast<uint4*>(ovl + g * 3);
      o[0] = uint4{ow[0], ow[1], ow[2], ow[3]};
      o[1] = uint4{ow[4], ow[5], ow[6], ow[7]};
      o[2] = uint4{ow[8], ow[9], ow[10], ow[11]};
    }
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (j < n) {
        if (lout) lout[g + j] = (uint8_t)(lw[j >> 2] >> (8 * (j & 3)));
        if (ovl) {
#pragma unroll
          for (int c = 0; c < 3; ++c) ovl[(g + j) * 3 + c] = (uint8_t)(ow[(3 * j + c) >> 2] >> (8 * ((3 * j + c) & 3)));
        }
      }
    }
  }
}

bool post_dims_ok(int B, int H, int W) {
  return B >= 1 && B <= 65535 && H >= 2 && H <= POST_MAXSIDE && W >= 2 && W <= POST_MAXSIDE;
}

// the three labelling kernels on a zeroed `areas`
void cc_launch(const uint8_t* lab, int B, int H, int W, int conn8, int only_zero, int mark_frame, int32_t* roots, int32_t* areas,
               hipStream_t st) {
  const int nseam = ((H - 1) / CC_TH) * W + ((W - 1) / CC_TW) * H;
  LMN_LAUNCH(cc_tile_kernel, dim3(lmn_cdiv(W, CC_TW), lmn_cdiv(H, CC_TH), B), dim3(256), 0, st, lab, H, W, conn8, only_zero, roots);
  if (nseam > 0) LMN_LAUNCH(cc_seam_kernel, dim3(lmn_cdiv(nseam, 256), B), dim3(256), 0, st, lab, H, W, conn8, only_zero, roots);
  LMN_LAUNCH(cc_flatten_kernel, dim3(lmn_cdiv(H * W, 256), B), dim3(256), 0, st, lab, H, W, only_zero, mark_frame, roots, areas);
}

}  // namespace

extern "C" {

int lmn_sizeof_post_param(void) { return (int)sizeof(lmn_post_param_t); }

int64_t lmn_post_workspace(int B, int H, int W) {
  if (!post_dims_ok(B, H, W)) {
    snprintf(g_lmn_err, sizeof(g_lmn_err), "post_workspace: B=%d %dx%d outside B in [1, 65535], sides in [2, %d]", B, H, W, POST_MAXSIDE);
    return -1;
  }
  const int64_t N = (int64_t)B * H * W;
  return 2 * lmn_up256(N) + 2 * lmn_up256(4 * N) + lmn_up256((int64_t)B * 64 * 8);
}

int lmn_cc_label(const uint8_t* labels, int B, int H, int W, int connectivity, void* workspace, int64_t ws_bytes, int32_t* roots,
                 int32_t* areas, lmn_stream_t stream) {
  (void)workspace;
  (void)ws_bytes;
  LMN_REQUIRE(labels && roots && areas, "cc_label: null pointer");
  LMN_REQUIRE(post_dims_ok(B, H, W), "cc_label: B=%d %dx%d outside B in [1, 65535], sides in [2, %d]", B, H, W, POST_MAXSIDE);
  LMN_REQUIRE(connectivity == 4 || connectivity == 8, "cc_label: connectivity %d is neither 4 nor 8", connectivity);
  hipStream_t st = (hipStream_t)stream;
  LMN_HIP_OK(hipMemsetAsync(areas, 0, sizeof(int32_t) * (size_t)B * H * W, st), "cc_label");
  cc_launch(labels, B, H, W, connectivity == 8, 0, 0, roots, areas, st);
  return lmn_launch_status("cc_label");
}

int lmn_post_clean(const float* logits, const uint8_t* labels_u8, const int64_t* labels_i64, int B, int C, int H, int W,
                   const lmn_post_param_t* params, void* workspace, int64_t ws_bytes, uint8_t* labels_out, int32_t* stats,
                   lmn_stream_t stream) {
  LMN_REQUIRE((logits != nullptr) + (labels_u8 != nullptr) + (labels_i64 != nullptr) == 1,
              "post_clean: exactly one of logits, labels_u8, labels_i64 required");
  LMN_REQUIRE(params && labels_out, "post_clean: null pointer");
  LMN_REQUIRE(C >= 2 && C <= 64, "post_clean: C=%d not in [2, 64]", C);
  LMN_REQUIRE(post_dims_ok(B, H, W), "post_clean: B=%d %dx%d outside B in [1, 65535], sides in [2, %d]", B, H, W, POST_MAXSIDE);
  const lmn_post_param_t prm = *params;
  const uint64_t all = C == 64 ? ~0ull : ((1ull << C) - 1);
  LMN_REQUIRE(prm.connectivity == 4 || prm.connectivity == 8, "post_clean: connectivity %d is neither 4 nor 8", (int)prm.connectivity);
  LMN_REQUIRE(!(prm.class_mask & 1) && !(prm.class_mask & ~all), "post_clean: class_mask names class 0 or a class >= C=%d", C);
  LMN_REQUIRE(!(prm.keep_largest_mask & ~prm.class_mask), "post_clean: keep_largest_mask names a class outside class_mask");
  LMN_REQUIRE(prm.hole_limit >= 0, "post_clean: hole_limit %d < 0", (int)prm.hole_limit);
  for (int k = 0; k < 64; ++k) LMN_REQUIRE(prm.min_area[k] >= 0, "post_clean: min_area[%d] = %d < 0", k, (int)prm.min_area[k]);
  const int HW = H * W;
  const int64_t N = (int64_t)B * HW;
  hipStream_t st = (hipStream_t)stream;
  const int lgrid = lmn_cdiv(N, 256) < 4096 ? lmn_cdiv(N, 256) : 4096;
  if (!stats) {                                             // labels only: L0 straight into labels_out, one kernel, no scratch
    LMN_REQUIRE(prm.class_mask == 0 && prm.hole_limit == 0, "post_clean: stats may be NULL only when nothing is cleaned or filled");
    LMN_LAUNCH(post_labels_kernel, dim3(lgrid), dim3(256), 0, st, logits, labels_u8, labels_i64, C, (int64_t)HW, N, labels_out);
    return lmn_launch_status("post_clean");
  }
  LMN_REQUIRE(workspace, "post_clean: null pointer");
  const int64_t need = lmn_post_workspace(B, H, W);
  LMN_REQUIRE(ws_bytes >= need, "post_clean: workspace of %lld bytes too small, %lld needed", (long long)ws_bytes, (long long)need);
  uint8_t* lab0 = (uint8_t*)workspace;
  uint8_t* lab1 = lab0 + lmn_up256(N);
  int32_t* roots = (int32_t*)(lab1 + lmn_up256(N));
  int32_t* areas = (int32_t*)((uint8_t*)roots + lmn_up256(4 * N));
  unsigned long long* best = (unsigned long long*)((uint8_t*)areas + lmn_up256(4 * N));
  const dim3 pgrid(lmn_cdiv(HW, 256), B), wgrid(lmn_cdiv(HW, POST_PPB), B);
  LMN_HIP_OK(hipMemsetAsync(stats, 0, sizeof(int32_t) * 4 * (size_t)B * C, st), "post_clean");
  LMN_HIP_OK(hipMemsetAsync(areas, 0, (size_t)(lmn_up256(4 * N) + lmn_up256((int64_t)B * 64 * 8)), st), "post_clean");   // areas and best, adjacent
  LMN_LAUNCH(post_labels_kernel, dim3(lgrid), dim3(256), 0, st, logits, labels_u8, labels_i64, C, (int64_t)HW, N, lab0);
  cc_launch(lab0, B, H, W, prm.connectivity == 8, 0, 0, roots, areas, st);
  LMN_LAUNCH(post_select_kernel, wgrid, dim3(256), 0, st, (const uint8_t*)lab0, (const int32_t*)roots, (const int32_t*)areas, HW, C, prm, best,
             stats);
  LMN_LAUNCH(post_apply_kernel, pgrid, dim3(256), 0, st, (const uint8_t*)lab0, (const int32_t*)roots, (const int32_t*)areas, HW, C, prm,
             (const unsigned long long*)best, lab1, stats);
  const int32_t* hroots = nullptr;
  if (prm.hole_limit > 0) {
    LMN_HIP_OK(hipMemsetAsync(areas, 0, sizeof(int32_t) * (size_t)N, st), "post_clean");
    cc_launch(lab1, B, H, W, prm.connectivity == 4, 1, 1, roots, areas, st);                 // the dual connectivity
    hroots = roots;
  }
  LMN_LAUNCH(post_fill_kernel, wgrid, dim3(256), 0, st, (const uint8_t*)lab1, hroots, (const int32_t*)areas, HW, C, (int)prm.hole_limit,
             labels_out, stats);
  return lmn_launch_status("post_clean");
}

int lmn_post_render(const uint8_t* labels_net, int B, int H, int W, const int32_t* src_hw, int Hs, int Ws, const uint8_t* frames,
                    int channels, const uint8_t* palette, int C, int alpha256, int mode, uint8_t* labels_out, uint8_t* overlay,
                    lmn_stream_t stream) {
  LMN_REQUIRE(labels_net && (labels_out || overlay), "post_render: null pointer");
  LMN_REQUIRE(post_dims_ok(B, H, W), "post_render: B=%d %dx%d outside B in [1, 65535], sides in [2, %d]", B, H, W, POST_MAXSIDE);
  LMN_REQUIRE(Hs >= 1 && Hs < 32768 && Ws >= 1 && Ws < 32768, "post_render: frame %dx%d outside [1, 32767]", Hs, Ws);
  LMN_REQUIRE(C >= 2 && C <= 64, "post_render: C=%d not in [2, 64]", C);
  LMN_REQUIRE(mode == 0 || mode == 1, "post_render: mode %d is neither 0 (fill) nor 1 (contour)", mode);
  LMN_REQUIRE(alpha256 >= 0 && alpha256 <= 256, "post_render: alpha256 = %d outside [0, 256]", alpha256);
  if (overlay) {
    LMN_REQUIRE(frames && palette, "post_render: an overlay needs frames and a palette");
    LMN_REQUIRE(channels == 1 || channels == 3, "post_render: %d frame channels (1 or 3)", channels);
  }
  LMN_REQUIRE(((uintptr_t)labels_out | (uintptr_t)overlay | (uintptr_t)frames) % 16 == 0, "post_render: frames and outputs must be 16-byte aligned");
  for (int b = 0; b < B; ++b) {
    const int hb = src_hw ? src_hw[2 * b] : Hs, wb = src_hw ? src_hw[2 * b + 1] : Ws;
    LMN_REQUIRE(hb >= 1 && hb <= Hs && wb >= 1 && wb <= Ws, "post_render: src_hw[%d] = %dx%d outside the %dx%d frame", b, hb, wb, Hs, Ws);
  }
  PostRender rp;
  memset(&rp, 0, sizeof(rp));
  if (palette)
    for (int k = 0; k < C; ++k)
      for (int c = 0; c < 3; ++c) rp.pal[k][c] = palette[3 * k + c];
  const int64_t plane = (int64_t)Hs * Ws;
  hipStream_t st = (hipStream_t)stream;
  for (int b0 = 0; b0 < B; b0 += POST_RCHUNK) {
    const int nb = B - b0 < POST_RCHUNK ? B - b0 : POST_RCHUNK;
    for (int b = 0; b < nb; ++b) {
      rp.hw[b][0] = src_hw ? src_hw[2 * (b0 + b)] : Hs;
      rp.hw[b][1] = src_hw ? src_hw[2 * (b0 + b) + 1] : Ws;
    }
    const int64_t groups = (plane * nb + 15) / 16;
    LMN_LAUNCH(post_render_kernel, dim3(lmn_cdiv(groups, 256)), dim3(256), 0, st, labels_net + (int64_t)b0 * H * W, H, W, Hs, Ws, nb, rp,
               overlay ? frames + (int64_t)b0 * plane * channels : (const uint8_t*)nullptr, channels, alpha256, mode,
               labels_out ? labels_out + (int64_t)b0 * plane : (uint8_t*)nullptr, overlay ? overlay + (int64_t)b0 * plane * 3 : (uint8_t*)nullptr);
  }
  return lmn_launch_status("post_render");
}

}  // extern "C"

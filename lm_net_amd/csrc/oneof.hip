// The OneOf block of the training transform on the device (dataset/data_loading.py:215-225; include/lmnet_oneof.h): one of
// ToGray, GridDistortion, ElasticTransform, CLAHE, HueSaturationValue, ChannelShuffle, GridDropout, RGBShift, GaussianBlur per
// sample, drawn on the host (lm_net_amd.data.DeviceAugment(one_of=...)), between ColorJitter and Normalize.
//
// lmn_augment_oneof_u8 runs the kernels of augment_common.h (geometry; ColorJitter with uint8 output into scratch2), then the
// members that look at neighbours write scratch2 -> scratch, each as one launch over the whole batch whose blocks leave at once
// unless their sample drew that member:
//   gaussian_blur   oneof_blur_kernel: 32 x 32 tile + halo of 3 in LDS, row pass into LDS, column pass; integer, exact
//   clahe           clahe_lut_kernel (one block per tile: histogram in LDS, clip, redistribute, cumulative sum, LUT) and
//                   clahe_apply_kernel (bilinear blend of four LUTs; channels 3: on L of a table-driven integer 8-bit LAB)
//   elastic         elastic_blur_kernel twice (rows, then columns) on the sample's two noise fields
//   grid_distortion / elastic   oneof_remap_kernel: cv2.remap arithmetic (1/32 pixel, 32768-scale weights, BORDER_REFLECT_101),
//                   labels by nearest pixel from labels_tmp
// and oneof_final_kernel applies the pointwise members (to_gray, rgb_shift, channel_shuffle, hsv, grid_dropout) on the fly and
// normalises every sample to fp32 NCHW, reading scratch (neighbourhood members) or scratch2 (the rest).
// Every expression is evaluated as written (no FMA contraction): tests/oneof_ref.py reproduces it bit for bit.
#include "augment_common.h"
#include "../../include/lmnet_oneof.h"

#pragma clang fp contract(off)

// BORDER_REFLECT_101 as a periodic fold: legal for any distance from the frame
__device__ __forceinline__ int reflect101(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;
  if (n == 1) return 0;
  const int p = 2 * n - 2;
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

__device__ __forceinline__ bool oneof_spatial(int op) {
  return op == LMN_ONEOF_GRID_DISTORTION || op == LMN_ONEOF_ELASTIC || op == LMN_ONEOF_CLAHE || op == LMN_ONEOF_GAUSSIAN_BLUR;
}

// ---------------------------------------------------------------- 8-bit LAB, integer and table-driven (T: lab_tables)
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
__device__ __forceinline__ int clamp_u8(int v) { return min(max(v, 0), 255); }

__device__ __forceinline__ void lab_fwd(const int32_t* __restrict__ T, int r, int g, int b, int& L, int& A, int& Bv) {
  const int R = T[LMN_LAB_GAMMA + r], G = T[LMN_LAB_GAMMA + g], Bl = T[LMN_LAB_GAMMA + b];
  const int32_t* C = T + LMN_LAB_FWD;
  const int fX = T[LMN_LAB_CBRT + descale(R * C[0] + G * C[1] + Bl * C[2], 12)];
  const int fY = T[LMN_LAB_CBRT + descale(R * C[3] + G * C[4] + Bl * C[5], 12)];
  const int fZ = T[LMN_LAB_CBRT + descale(R * C[6] + G * C[7] + Bl * C[8], 12)];
  L = clamp_u8(descale(296 * fY - 1336935, 15));                 // (116 fY - 16) * 2.55
  A = clamp_u8(descale(500 * (fX - fY) + 128 * 32768, 15));
  Bv = clamp_u8(descale(200 * (fY - fZ) + 128 * 32768, 15));
}

__device__ __forceinline__ int64_t lab_finv(int64_t f) {          // f^-1 of CIE LAB, 2^15 scale in and out
  if (f > 6780) return (f * f * f) >> 30;
  const int64_t t = (f - 4520) * 4208;                           // (f - 16/116) / 7.787
  return (t > 0 ? t : 0) >> 15;
}

__device__ __forceinline__ void lab_inv(const int32_t* __restrict__ T, int L, int A, int Bv, int& r, int& g, int& b) {
  const int fy = T[LMN_LAB_FY + L], fx = fy + T[LMN_LAB_DA + A], fz = fy - T[LMN_LAB_DB + Bv];
  const int64_t X = lab_finv(fx), Y = lab_finv(fy), Z = lab_finv(fz);
  const int32_t* C = T + LMN_LAB_INV;
  int o[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int64_t lin = ((int64_t)C[3 * c] * X + (int64_t)C[3 * c + 1] * Y + (int64_t)C[3 * c + 2] * Z + 4096) >> 13;   // 2^14 scale
    o[c] = T[LMN_LAB_INVGAMMA + (int)(lin < 0 ? 0 : (lin > 16384 ? 16384 : lin))];
  }
  r = o[0]; g = o[1]; b = o[2];
}

// ---------------------------------------------------------------- gaussian_blur
__constant__ int c_blur_w[3][7] = {{0, 0, 1, 2, 1, 0, 0}, {0, 1, 4, 6, 4, 1, 0}, {2, 7, 14, 18, 14, 7, 2}};  // cv2 small kernels, sigma 0

#define BLUR_T 32
#define BLUR_R 3
#define BLUR_S (BLUR_T + 2 * BLUR_R)

// grid (tiles, B): out = (sum wy wx v + half) >> shift with the dyadic weights above (shift 4, 8, 12 for k 3, 5, 7)
template <int CH>
__global__ __launch_bounds__(256) void oneof_blur_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                         const lmn_oneof_param_t* __restrict__ oneof, int H, int W) {
  const int b = blockIdx.y;
  if (oneof[b].op != LMN_ONEOF_GAUSSIAN_BLUR) return;
  __shared__ uint8_t raw[BLUR_S][BLUR_S * CH];
  __shared__ uint16_t hs[BLUR_S][BLUR_T * CH];
  const int r = oneof[b].k >> 1, shift = 4 * r;
  const int* w = c_blur_w[r - 1];
  const int tiles_x = (W + BLUR_T - 1) / BLUR_T;
  const int x0 = (blockIdx.x % tiles_x) * BLUR_T, y0 = (blockIdx.x / tiles_x) * BLUR_T;
  const uint8_t* s = src + (int64_t)b * H * W * CH;
  for (int i = threadIdx.x; i < BLUR_S * BLUR_S; i += 256) {
    const int ry = i / BLUR_S, rx = i % BLUR_S;
    const int ys = reflect101(y0 + ry - BLUR_R, H), xs = reflect101(x0 + rx - BLUR_R, W);
#pragma unroll
    for (int c = 0; c < CH; ++c) raw[ry][rx * CH + c] = s[((int64_t)ys * W + xs) * CH + c];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < BLUR_S * BLUR_T * CH; i += 256) {
    const int ry = i / (BLUR_T * CH), j = i % (BLUR_T * CH);
    int acc = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) acc += w[k] * raw[ry][j + k * CH];
    hs[ry][j] = (uint16_t)acc;                                   // <= 64 * 255
  }
  __syncthreads();
  uint8_t* d = dst + (int64_t)b * H * W * CH;
  for (int i = threadIdx.x; i < BLUR_T * BLUR_T * CH; i += 256) {
    const int oy = i / (BLUR_T * CH), j = i % (BLUR_T * CH);
    const int y = y0 + oy, x = x0 + j / CH;
    if (y >= H || x >= W) continue;
    int acc = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) acc += w[k] * hs[oy + k][j];
    d[((int64_t)y * W + x) * CH + j % CH] = (uint8_t)((acc + (1 << (shift - 1))) >> shift);
  }
}

// ---------------------------------------------------------------- clahe
template <int CH>
__device__ __forceinline__ int clahe_level(const uint8_t* __restrict__ px, const int32_t* __restrict__ T) {
  if (CH == 1) return px[0];
  int L, A, Bv;
  lab_fwd(T, px[0], px[1], px[CH - 1], L, A, Bv);
  return L;
}

// grid (64, B): the LUT of tile blockIdx.x of the 8 x 8 grid over the frame padded (reflect-101, bottom / right) to multiples of 8
template <int CH>
__global__ __launch_bounds__(256) void clahe_lut_kernel(const uint8_t* __restrict__ src, const lmn_oneof_param_t* __restrict__ oneof,
                                                        const int32_t* __restrict__ T, uint8_t* __restrict__ luts, int H, int W) {
  const int b = blockIdx.y, t = threadIdx.x;
  if (oneof[b].op != LMN_ONEOF_CLAHE) return;
  __shared__ int hist[256];
  __shared__ int excess;
  const int th = ((H + 7) >> 3), tw = ((W + 7) >> 3), area = th * tw;
  const int ty = blockIdx.x >> 3, tx = blockIdx.x & 7;
  hist[t] = 0;
  if (t == 0) excess = 0;
  __syncthreads();
  const uint8_t* s = src + (int64_t)b * H * W * CH;
  for (int i = t; i < area; i += 256) {
    const int y = reflect101(ty * th + i / tw, H), x = reflect101(tx * tw + i % tw, W);
    atomicAdd(&hist[clahe_level<CH>(s + ((int64_t)y * W + x) * CH, T)], 1);
  }
  __syncthreads();
  const int clip = max((int)(oneof[b].v[0] * (double)area / 256.0), 1);
  int h = hist[t];
  if (h > clip) {
    atomicAdd(&excess, h - clip);
    h = clip;
  }
  __syncthreads();
  const int batch = excess / 256, resid = excess - batch * 256;
  h += batch;
  if (resid) {
    const int step = max(256 / resid, 1);
    if (t % step == 0 && t / step < resid) ++h;
  }
  hist[t] = h;
  __syncthreads();
  int cum = 0;
  for (int i = 0; i <= t; ++i) cum += hist[i];
  const float scale = 255.f / (float)area;
  luts[((int64_t)b * 64 + blockIdx.x) * 256 + t] = (uint8_t)sat_u8f((float)cum * scale);
}

template <int CH>
__global__ __launch_bounds__(256) void clahe_apply_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                          const lmn_oneof_param_t* __restrict__ oneof, const int32_t* __restrict__ T,
                                                          const uint8_t* __restrict__ luts, int H, int W) {
  const int b = blockIdx.y;
  if (oneof[b].op != LMN_ONEOF_CLAHE) return;
  const int HW = H * W;
  const float inv_th = 1.f / (float)((H + 7) >> 3), inv_tw = 1.f / (float)((W + 7) >> 3);
  const uint8_t* lut = luts + (int64_t)b * 64 * 256;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
    const int x = i % W, y = i / W;
    const float tyf = (float)y * inv_th - 0.5f, txf = (float)x * inv_tw - 0.5f;
    int ty1 = (int)floorf(tyf), tx1 = (int)floorf(txf);
    const float ya = tyf - (float)ty1, xa = txf - (float)tx1, ya1 = 1.f - ya, xa1 = 1.f - xa;
    const int ty2 = min(ty1 + 1, 7), tx2 = min(tx1 + 1, 7);
    ty1 = max(ty1, 0);
    tx1 = max(tx1, 0);
    const uint8_t* s = src + ((int64_t)b * HW + i) * CH;
    uint8_t* d = dst + ((int64_t)b * HW + i) * CH;
    int L = s[0], A = 0, Bv = 0;
    if (CH == 3) lab_fwd(T, s[0], s[1], s[CH - 1], L, A, Bv);
    const float l11 = (float)lut[(ty1 * 8 + tx1) * 256 + L], l12 = (float)lut[(ty1 * 8 + tx2) * 256 + L];
    const float l21 = (float)lut[(ty2 * 8 + tx1) * 256 + L], l22 = (float)lut[(ty2 * 8 + tx2) * 256 + L];
    const int v = sat_u8f((l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya);
    if (CH == 3) {
      int r, g, bl;
      lab_inv(T, v, A, Bv, r, g, bl);
      d[0] = (uint8_t)r; d[1] = (uint8_t)g; d[CH - 1] = (uint8_t)bl;
    } else {
      d[0] = (uint8_t)v;
    }
  }
}

// ---------------------------------------------------------------- elastic: separable Gaussian of the two noise fields
// fields of slot s: ws + s * 4 H W floats: [2][H][W] row-blurred, then [2][H][W] finished (blurred both ways, times alpha).
// pass 0: noise (tables) -> row-blurred; pass 1: row-blurred -> finished.  fp32, every output sums its taps in order -r .. +r.
// A thread forms EL_T consecutive outputs along the blurred axis from one sliding read of 2 r + EL_T source values (tap k of
// output j is source j + k: the loop over m = j + k visits every output's taps in ascending k).
#define EL_T 4
__global__ __launch_bounds__(256) void elastic_blur_kernel(const lmn_oneof_param_t* __restrict__ oneof, const float* __restrict__ tables,
                                                           float* __restrict__ ws, int H, int W, int pass) {
  const int b = blockIdx.y;
  const lmn_oneof_param_t& q = oneof[b];
  if (q.op != LMN_ONEOF_ELASTIC) return;
  const int HW = H * W, r = q.radius;
  const float* wgt = tables + q.tab_off;
  float* base = ws + (int64_t)q.slot * 4 * HW;
  const float* src = pass == 0 ? wgt + (2 * r + 1) : base;
  float* dst = pass == 0 ? base : base + 2 * (int64_t)HW;
  const float alpha = (float)q.v[0];
  const int n = pass == 0 ? W : H;                       // length of the blurred axis
  const int groups = (n + EL_T - 1) / EL_T, other = pass == 0 ? H : W;
  const int items = groups * other;                      // per field
  for (int i = blockIdx.x * 256 + threadIdx.x; i < 2 * items; i += gridDim.x * 256) {
    const int f = i / items, j0 = i - f * items;
    // pass 0: the group index runs fastest (a row at a time); pass 1: x runs fastest (coalesced rows)
    const int o = pass == 0 ? j0 / groups : j0 % W;      // position on the other axis (y in pass 0, x in pass 1)
    const int a0 = (pass == 0 ? j0 % groups : j0 / W) * EL_T;
    const float* p = src + (int64_t)f * HW + (pass == 0 ? (int64_t)o * W : o);
    const int stride = pass == 0 ? 1 : W;
    float acc[EL_T];
#pragma unroll
    for (int j = 0; j < EL_T; ++j) acc[j] = 0.f;
    for (int m = -r; m <= r + EL_T - 1; ++m) {
      const float v = p[(int64_t)reflect101(a0 + m, n) * stride];
#pragma unroll
      for (int j = 0; j < EL_T; ++j) {
        const int k = m - j;
        if (k >= -r && k <= r) acc[j] = acc[j] + wgt[k + r] * v;
      }
    }
    float* d = dst + (int64_t)f * HW + (pass == 0 ? (int64_t)o * W : o);
#pragma unroll
    for (int j = 0; j < EL_T; ++j)
      if (a0 + j < n) d[(int64_t)(a0 + j) * stride] = pass == 0 ? acc[j] : acc[j] * alpha;
  }
}

// ---------------------------------------------------------------- grid_distortion / elastic: cv2.remap with float maps
template <int CH>
__global__ __launch_bounds__(256) void oneof_remap_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                          const int64_t* __restrict__ lab_src, int64_t* __restrict__ lab_dst,
                                                          const lmn_oneof_param_t* __restrict__ oneof, const float* __restrict__ tables,
                                                          const float* __restrict__ ws, int H, int W) {
  const int b = blockIdx.y;
  const lmn_oneof_param_t& q = oneof[b];
  const bool grid = q.op == LMN_ONEOF_GRID_DISTORTION;
  if (!grid && q.op != LMN_ONEOF_ELASTIC) return;
  const int HW = H * W;
  const float* xx = tables + q.tab_off;                                   // grid: xx[W], yy[H]
  const float* dxy = ws + ((int64_t)q.slot * 4 + 2) * HW;                 // elastic: dx[H][W], dy[H][W]
  for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
    const int x = i % W, y = i / W;
    float mx, my;
    if (grid) {
      mx = xx[x];
      my = xx[W + y];
    } else {
      mx = (float)x + dxy[i];
      my = (float)y + dxy[HW + i];
    }
    if (src) {
      const int ix = (int)rintf(mx * 32.f), iy = (int)rintf(my * 32.f);   // 1/32 pixel
      const int sx = ix >> 5, sy = iy >> 5, fx = ix & 31, fy = iy & 31;
      const int w00 = (32 - fy) * (32 - fx) * 32, w01 = (32 - fy) * fx * 32, w10 = fy * (32 - fx) * 32, w11 = fy * fx * 32;
      const int xa = reflect101(sx, W), xb = reflect101(sx + 1, W), ya = reflect101(sy, H), yb = reflect101(sy + 1, H);
      const uint8_t* s = src + (int64_t)b * HW * CH;
      uint8_t* d = dst + ((int64_t)b * HW + i) * CH;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int v00 = s[((int64_t)ya * W + xa) * CH + c], v01 = s[((int64_t)ya * W + xb) * CH + c];
        const int v10 = s[((int64_t)yb * W + xa) * CH + c], v11 = s[((int64_t)yb * W + xb) * CH + c];
        d[c] = (uint8_t)clamp_u8((v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11 + 16384) >> 15);
      }
    }
    if (lab_src) {
      const int lx = reflect101((int)rintf(mx), W), ly = reflect101((int)rintf(my), H);
      lab_dst[(int64_t)b * HW + i] = lab_src[(int64_t)b * HW + (int64_t)ly * W + lx];
    }
  }
}

// labels of the samples the remap kernel does not touch: labels_tmp -> labels
__global__ __launch_bounds__(256) void oneof_label_copy_kernel(const int64_t* __restrict__ lab_src, int64_t* __restrict__ lab_dst,
                                                               const lmn_oneof_param_t* __restrict__ oneof, int HW) {
  const int b = blockIdx.y, op = oneof[b].op;
  if (op == LMN_ONEOF_GRID_DISTORTION || op == LMN_ONEOF_ELASTIC) return;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) lab_dst[(int64_t)b * HW + i] = lab_src[(int64_t)b * HW + i];
}

// ---------------------------------------------------------------- pointwise members + Normalize
template <int CH>
__global__ __launch_bounds__(256) void oneof_final_kernel(const uint8_t* __restrict__ scratch, const uint8_t* __restrict__ scratch2,
                                                          const lmn_oneof_param_t* __restrict__ oneof, float* __restrict__ out,
                                                          const AugGeom g) {
  const int b = blockIdx.y;
  const lmn_oneof_param_t& q = oneof[b];
  const int op = q.op, HW = g.H * g.W;
  const uint8_t* src = (oneof_spatial(op) ? scratch : scratch2) + (int64_t)b * HW * CH;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
    int u[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) u[c] = src[(int64_t)i * CH + c];
    if (op == LMN_ONEOF_GRID_DROPOUT) {
      if ((i % g.W) % q.unit < q.hole && (i / g.W) % q.unit < q.hole) {
#pragma unroll
        for (int c = 0; c < CH; ++c) u[c] = 0;
      }
    } else if (CH == 3) {
      if (op == LMN_ONEOF_TO_GRAY) {
        const int gr = rgb2gray(u[0], u[1], u[CH - 1]);
#pragma unroll
        for (int c = 0; c < CH; ++c) u[c] = gr;
      } else if (op == LMN_ONEOF_RGB_SHIFT) {                              // LUT clip(v + shift, 0, 255).astype(uint8)
#pragma unroll
        for (int c = 0; c < CH; ++c) u[c] = (int)fmin(fmax((double)u[c] + q.v[c], 0.0), 255.0);
      } else if (op == LMN_ONEOF_CHANNEL_SHUFFLE) {
        const int t0 = u[0], t1 = u[1], t2 = u[CH - 1];
#pragma unroll
        for (int c = 0; c < CH; ++c) u[c] = q.perm[c] == 0 ? t0 : (q.perm[c] == 1 ? t1 : t2);
      } else if (op == LMN_ONEOF_HSV) {
        int h, s, v;
        aug_rgb2hsv(u[0], u[1], u[CH - 1], h, s, v);
        double t = fmod((double)h + q.v[0], 180.0);                        // np.mod(h + shift, 180).astype(uint8)
        if (t < 0.0) t += 180.0;
        s = (int)fmin(fmax((double)s + q.v[1], 0.0), 255.0);
        v = (int)fmin(fmax((double)v + q.v[2], 0.0), 255.0);
        aug_hsv2rgb((int)t, s, v, u[0], u[1], u[CH - 1]);
      }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) out[((int64_t)b * CH + c) * HW + i] = aug_normalize(u[c], g.m255[c], g.inv[c]);
  }
}

// ---------------------------------------------------------------- entries
int lmn_sizeof_oneof_param(void) { return (int)sizeof(lmn_oneof_param_t); }

static inline int64_t oneof_lut_bytes(int B) { return (int64_t)B * 64 * 256; }

int64_t lmn_oneof_workspace(int B, int H, int W, int channels, int n_elastic) {
  if (B <= 0 || H <= 0 || W <= 0 || n_elastic < 0 || n_elastic > B || (channels != 1 && channels != 3)) return -1;
  return oneof_lut_bytes(B) + (int64_t)n_elastic * 4 * H * W * (int64_t)sizeof(float);
}

#define ONEOF_LAUNCH_CH(kern, grid, ...)                                              \
  do {                                                                                \
    if (channels == 1) LMN_LAUNCH((kern<1>), grid, dim3(256), 0, st, __VA_ARGS__);    \
    else LMN_LAUNCH((kern<3>), grid, dim3(256), 0, st, __VA_ARGS__);                  \
  } while (0)

int lmn_augment_oneof_u8(const uint8_t* images, const uint8_t* masks, const lmn_aug_param_t* params, const int32_t* src_hw,
                         lmn_aug_param_t* params_dev, int B, int Hs, int Ws, int H, int W, int channels, int mask_mode,
                         const double* mean, const double* std, uint8_t* scratch, uint64_t* gray_sum, float* out, int64_t* labels,
                         const lmn_oneof_param_t* oneof, lmn_oneof_param_t* oneof_dev, const float* tables, int64_t n_tables,
                         float* tables_dev, const int32_t* lab_tables, uint8_t* scratch2, int64_t* labels_tmp, void* workspace,
                         int64_t workspace_bytes, lmn_stream_t stream) {
  const char* who = "augment_oneof_u8";
  AugGeom g;
  int rc = aug_check_args(who, images, masks, params, src_hw, params_dev, B, Hs, Ws, H, W, channels, mask_mode, mean, std, scratch,
                          gray_sum, out, labels, g);
  if (rc) return rc;
  LMN_REQUIRE(oneof && oneof_dev, "%s: oneof and oneof_dev required", who);
  LMN_REQUIRE(!images || scratch2, "%s: images need scratch2", who);
  LMN_REQUIRE(n_tables >= 0 && (n_tables == 0 || (tables && tables_dev)), "%s: %lld table floats need tables and tables_dev", who,
              (long long)n_tables);
  const int64_t HW = (int64_t)H * W;
  int n_el = 0, n_geo = 0, n_blur = 0, n_clahe = 0;
  for (int b = 0; b < B; ++b) n_el += oneof[b].op == LMN_ONEOF_ELASTIC;
  uint64_t slots_seen[1024] = {0};  // B <= 65535
  for (int b = 0; b < B; ++b) {
    const lmn_oneof_param_t& q = oneof[b];
    LMN_REQUIRE(q.op >= 0 && q.op < LMN_ONEOF_NOPS, "%s: unknown op id %d of sample %d", who, q.op, b);
    const bool colour = q.op == LMN_ONEOF_TO_GRAY || q.op == LMN_ONEOF_HSV || q.op == LMN_ONEOF_CHANNEL_SHUFFLE || q.op == LMN_ONEOF_RGB_SHIFT;
    LMN_REQUIRE(!colour || channels == 3, "%s: op %d of sample %d is a colour member, channels=%d", who, q.op, b, channels);
    switch (q.op) {
      case LMN_ONEOF_GAUSSIAN_BLUR:
        LMN_REQUIRE(q.k == 3 || q.k == 5 || q.k == 7, "%s: gaussian_blur k=%d of sample %d not in {3, 5, 7}", who, q.k, b);
        ++n_blur;
        break;
      case LMN_ONEOF_CHANNEL_SHUFFLE: {
        int seen = 0;
        for (int c = 0; c < 3; ++c) seen |= (q.perm[c] >= 0 && q.perm[c] < 3) ? 1 << q.perm[c] : 8;
        LMN_REQUIRE(seen == 7, "%s: channel_shuffle of sample %d is not a permutation of 0..2", who, b);
        break;
      }
      case LMN_ONEOF_RGB_SHIFT:
      case LMN_ONEOF_HSV:
        LMN_REQUIRE(fabs(q.v[0]) <= 255.0 && fabs(q.v[1]) <= 255.0 && fabs(q.v[2]) <= 255.0, "%s: shifts of sample %d outside +-255", who, b);
        break;
      case LMN_ONEOF_GRID_DROPOUT:
        LMN_REQUIRE(q.unit >= 2 && q.hole >= 1 && q.hole < q.unit, "%s: grid_dropout unit %d / hole %d of sample %d", who, q.unit, q.hole, b);
        break;
      case LMN_ONEOF_CLAHE:
        LMN_REQUIRE(q.v[0] >= 1.0 && q.v[0] <= 1e6, "%s: clahe clip %g of sample %d outside [1, 1e6]", who, q.v[0], b);
        LMN_REQUIRE(!images || channels == 1 || lab_tables, "%s: clahe on 3 channels needs lab_tables", who);
        ++n_clahe;
        break;
      case LMN_ONEOF_GRID_DISTORTION:
        LMN_REQUIRE(q.tab_off >= 0 && q.tab_off + H + W <= n_tables, "%s: grid_distortion maps of sample %d outside the tables", who, b);
        ++n_geo;
        break;
      case LMN_ONEOF_ELASTIC:
        LMN_REQUIRE(q.v[1] > 0.0, "%s: elastic sigma %g of sample %d must be positive", who, q.v[1], b);
        LMN_REQUIRE(fabs(q.v[0]) <= 1e6, "%s: elastic alpha %g of sample %d above 1e6", who, q.v[0], b);
        LMN_REQUIRE(HW < (1 << 29), "%s: elastic on more than 2^29 pixels", who);
        LMN_REQUIRE(q.radius >= 0 && q.radius <= LMN_ONEOF_MAX_RADIUS, "%s: elastic radius %d of sample %d", who, q.radius, b);
        LMN_REQUIRE(q.tab_off >= 0 && q.tab_off + 2 * q.radius + 1 + 2 * HW <= n_tables, "%s: elastic tables of sample %d outside the tables", who, b);
        LMN_REQUIRE(q.slot >= 0 && q.slot < n_el && !(slots_seen[q.slot >> 6] >> (q.slot & 63) & 1), "%s: elastic slot %d of sample %d", who, q.slot, b);
        slots_seen[q.slot >> 6] |= 1ull << (q.slot & 63);
        ++n_geo;
        break;
      default: break;
    }
  }
  LMN_REQUIRE(!masks || !n_geo || labels_tmp, "%s: grid_distortion / elastic with masks need labels_tmp", who);
  const int64_t need = lmn_oneof_workspace(B, H, W, channels, n_el);
  LMN_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes, (long long)need);
  LMN_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", who);

  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(oneof_dev, oneof, sizeof(lmn_oneof_param_t) * (size_t)B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && n_tables) e = hipMemcpyAsync(tables_dev, tables, sizeof(float) * (size_t)n_tables, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) {
    snprintf(g_lmn_err, sizeof(g_lmn_err), "%s: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  const bool relabel = masks && n_geo;
  rc = aug_launch_geom("augment_oneof_u8 (geometry)", images, masks, params, params_dev, B, channels, scratch, gray_sum,
                       relabel ? labels_tmp : labels, g, st);
  if (rc) return rc;
  const dim3 grid = aug_grid(H * W, B);
  uint8_t* luts = (uint8_t*)workspace;
  float* fields = (float*)((uint8_t*)workspace + oneof_lut_bytes(B));
  if (images) {
    unsigned long long* gs = (unsigned long long*)gray_sum;
    if (channels == 1)
      LMN_LAUNCH((augment_color_kernel<1, true>), grid, dim3(256), 0, st, scratch, params_dev, gs, (float*)nullptr, scratch2, g);
    else
      LMN_LAUNCH((augment_color_kernel<3, true>), grid, dim3(256), 0, st, scratch, params_dev, gs, (float*)nullptr, scratch2, g);
    if (n_blur) {
      const dim3 tg(lmn_cdiv(W, BLUR_T) * lmn_cdiv(H, BLUR_T), B);
      ONEOF_LAUNCH_CH(oneof_blur_kernel, tg, scratch2, scratch, oneof_dev, H, W);
    }
    if (n_clahe) {
      ONEOF_LAUNCH_CH(clahe_lut_kernel, dim3(64, B), scratch2, oneof_dev, lab_tables, luts, H, W);
      ONEOF_LAUNCH_CH(clahe_apply_kernel, grid, scratch2, scratch, oneof_dev, lab_tables, luts, H, W);
    }
  }
  if (n_el) {
    LMN_LAUNCH(elastic_blur_kernel, aug_grid(2 * H * lmn_cdiv(W, EL_T), B), dim3(256), 0, st, oneof_dev, tables_dev, fields, H, W, 0);
    LMN_LAUNCH(elastic_blur_kernel, aug_grid(2 * lmn_cdiv(H, EL_T) * W, B), dim3(256), 0, st, oneof_dev, tables_dev, fields, H, W, 1);
  }
  if (n_geo) {
    const uint8_t* rs = images ? scratch2 : nullptr;
    const int64_t* ls = masks ? labels_tmp : nullptr;
    ONEOF_LAUNCH_CH(oneof_remap_kernel, grid, rs, scratch, ls, labels, oneof_dev, tables_dev, fields, H, W);
    if (relabel) LMN_LAUNCH(oneof_label_copy_kernel, grid, dim3(256), 0, st, labels_tmp, labels, oneof_dev, H * W);
  }
  if (images) ONEOF_LAUNCH_CH(oneof_final_kernel, grid, scratch, scratch2, oneof_dev, out, g);
  return lmn_launch_status("augment_oneof_u8");
}

// Device code and host checks shared by lmn_augment_u8 (augment.hip) and lmn_augment_oneof_u8 (oneof.hip).
//
// Training augmentations on the device: the per-sample part of the reference's training transform
// (dataset/data_loading.py:207-216, 227-228) for a batch of raw uint8 frames already in HBM:
//   RandomResizedCrop -> ShiftScaleRotate(BORDER_CONSTANT) -> HorizontalFlip -> VerticalFlip -> ColorJitter -> Normalize.
// The parameters of every sample are drawn on the host (lm_net_amd.data.DeviceAugment) and arrive as lmn_aug_param_t.
//
// Kernel 1 (augment_geom_kernel) resamples TWICE, as the reference does, without materialising the crop-resized frame: for
// output pixel (x, y) it undoes the flips, maps the pixel through the inverse SSR matrix with cv2.warpAffine's fixed-point
// arithmetic (OpenCV <= 4.10, WarpAffineInvoker: AB_BITS 10, INTER_BITS 5, cvRound of M*x*1024) and blends the four
// neighbours with the INTER_REMAP_COEF_SCALE (32768) weights of remapBilinear; each neighbour is the value of
// cv2.resize(INTER_LINEAR) of the crop window at that pixel, computed from the raw frame with the arithmetic of
// lmn_preprocess_u8 (rows.hip prep_axis).  Masks take INTER_NEAREST both times.  Border value 0 for both.
// Kernel 2 (augment_color_kernel) applies ColorJitter in the sample's op order with albumentations 1.3/1.4
// adjust_{brightness,contrast,saturation,hue}_torchvision uint8 semantics and normalises to fp32 NCHW.
// Contrast needs the mean gray level of the image as contrast sees it: kernel 1 sums it per sample (integer atomics).
//
// Every float / double expression here is evaluated as written: no FMA contraction, so the numpy restatement
// (tests/augment_ref.py) reproduces it bit for bit.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

struct AugGeom {
  int Hs, Ws, H, W, mask_mode;
  double m255[3], inv[3];
};

// rows.hip prep_axis with the scale n_src / n_dst passed in (same value, computed once per block)
__device__ __forceinline__ void aug_axis(int d, int n_src, double scale, bool clamp_frac, int& s0, int& s1, int& a0, int& a1) {
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (clamp_frac) {  // columns: cv2 zeroes the fraction at the borders; rows are clamped instead
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n_src - 1) { s = n_src - 1; f = 0.f; }
  }
  a0 = (int)rintf((1.f - f) * 2048.f);
  a1 = (int)rintf(f * 2048.f);
  s0 = min(max(s, 0), n_src - 1);
  s1 = min(max(s + 1, 0), n_src - 1);
}

struct Axis {
  int s0, s1, a0, a1;
};

// value of channel c of cv2.resize(crop, (W, H), INTER_LINEAR) at the pixel whose axes are ax (column) / ay (row)
template <int CH>
__device__ __forceinline__ int rc_value(const uint8_t* __restrict__ src, int64_t row_stride, const Axis& ax, const Axis& ay, int c) {
  const uint8_t* r0 = src + ay.s0 * row_stride;
  const uint8_t* r1 = src + ay.s1 * row_stride;
  const int h0 = r0[ax.s0 * CH + c] * ax.a0 + r0[ax.s1 * CH + c] * ax.a1;  // horizontal pass, scale 2^11
  const int h1 = r1[ax.s0 * CH + c] * ax.a0 + r1[ax.s1 * CH + c] * ax.a1;
  const int v = (((ay.a0 * (h0 >> 4)) >> 16) + ((ay.a1 * (h1 >> 4)) >> 16) + 2) >> 2;  // cv2 VResizeLinear<uchar>
  return min(max(v, 0), 255);
}

__device__ __forceinline__ int sat_short(int v) { return min(max(v, -32768), 32767); }

// cv2.warpAffine: source coordinate of destination pixel (x, y) in units of 2^-shift, from the inverse matrix row (a, b, c):
// cvRound((b*y + c) * 1024) + round_delta + cvRound(a*x*1024), then >> shift
__device__ __forceinline__ int warp_coord(double a, double b, double c, int x, int y, int round_delta, int shift) {
  const int X0 = (int)rint((b * (double)y + c) * 1024.0) + round_delta;
  const int dx = (int)rint(a * (double)x * 1024.0);
  return (X0 + dx) >> shift;
}

__device__ __forceinline__ int rgb2gray(int r, int g, int b) { return (r * 4899 + g * 9617 + b * 1868 + 8192) >> 14; }  // cv2 RGB2GRAY

__device__ __forceinline__ int sat_u8f(float v) { return min(max((int)rintf(v), 0), 255); }  // saturate_cast<uchar>(float)

// cv2 RGB2HSV on uint8 (hue range 180): hsv_shift 12, sdiv = cvRound((255 << 12) / v), hdiv = cvRound((180 << 12) / (6 diff))
__device__ __forceinline__ void aug_rgb2hsv(int r, int g, int b, int& h, int& s, int& v) {
  v = max(max(r, g), b);
  const int vmin = min(min(r, g), b);
  const int diff = v - vmin;
  const int sdiv = v ? (int)rint(1044480.0 / (double)v) : 0;                  // (255 << 12) / v
  const int hdiv = diff ? (int)rint(737280.0 / (6.0 * (double)diff)) : 0;     // (180 << 12) / (6 diff)
  s = (diff * sdiv + 2048) >> 12;
  h = (v == r) ? (g - b) : (v == g) ? (b - r + 2 * diff) : (r - g + 4 * diff);
  h = (h * hdiv + 2048) >> 12;
  h += h < 0 ? 180 : 0;
}

// cv2 HSV2RGB_b: float, hscale 6/180, saturate_cast<uchar>(x * 255)
__device__ __forceinline__ void aug_hsv2rgb(int hn, int s, int v, int& r, int& g, int& b) {
  const float sv = (float)s * (1.0f / 255.0f), vv = (float)v * (1.0f / 255.0f);
  float hh = (float)hn * (6.0f / 180.0f);
  if (hh >= 6.f) hh -= 6.f;
  int sector = (int)floorf(hh);
  hh -= (float)sector;
  if ((unsigned)sector >= 6u) { sector = 0; hh = 0.f; }
  const float t0 = vv, t1 = vv * (1.f - sv), t2 = vv * (1.f - sv * hh), t3 = vv * (1.f - sv * (1.f - hh));
  float bo, go, ro;
  switch (sector) {  // sector_data {b, g, r}: {1,3,0} {1,0,2} {3,0,1} {0,2,1} {0,1,3} {2,1,0}
    case 0: bo = t1; go = t3; ro = t0; break;
    case 1: bo = t1; go = t0; ro = t2; break;
    case 2: bo = t3; go = t0; ro = t1; break;
    case 3: bo = t0; go = t2; ro = t1; break;
    case 4: bo = t0; go = t1; ro = t3; break;
    default: bo = t2; go = t1; ro = t0; break;
  }
  r = sat_u8f(ro * 255.f);
  g = sat_u8f(go * 255.f);
  b = sat_u8f(bo * 255.f);
}

// one ColorJitter op on a pixel (albumentations adjust_*_torchvision on uint8; a factor of 1, or hue 0, is the identity)
template <int CH>
__device__ __forceinline__ void cj_op(int op, int (&u)[CH], const double* cj, double mean_gray) {
  const double f = cj[op];
  if (op == 0) {                        // brightness: LUT clip(v * f, 0, 255).astype(uint8)
    if (f == 1.0) return;
#pragma unroll
    for (int c = 0; c < CH; ++c) u[c] = (int)fmin(fmax((double)u[c] * f, 0.0), 255.0);
  } else if (op == 1) {                 // contrast: LUT clip(v * f + mean * (1 - f), 0, 255).astype(uint8); f = 0 fills int(mean + .5)
    if (f == 1.0) return;
    if (f == 0.0) {
      const int m = (int)(mean_gray + 0.5);
#pragma unroll
      for (int c = 0; c < CH; ++c) u[c] = m;
      return;
    }
    const double k = mean_gray * (1.0 - f);
#pragma unroll
    for (int c = 0; c < CH; ++c) u[c] = (int)fmin(fmax((double)u[c] * f + k, 0.0), 255.0);
  } else if (CH == 3) {
    if (op == 2) {                      // saturation: cv2.addWeighted(img, f, gray3, 1 - f, 0) in float, cvRound
      if (f == 1.0) return;
      const float g = (float)rgb2gray(u[0], u[1], u[CH - 1]);
      const float alpha = (float)f, beta = (float)(1.0 - f);
#pragma unroll
      for (int c = 0; c < CH; ++c) u[c] = sat_u8f(((float)u[c] * alpha + g * beta) + 0.f);
    } else {                            // hue: cv2 RGB2HSV (uint8, range 180), h -> lut[h], HSV2RGB
      if (f == 0.0) return;
      int h, sat, v;
      aug_rgb2hsv(u[0], u[1], u[CH - 1], h, sat, v);
      double t = fmod((double)h + 180.0 * f, 180.0);                              // np.mod(h + 180 f, 180).astype(uint8)
      if (t < 0.0) t += 180.0;
      aug_hsv2rgb((int)t, sat, v, u[0], u[1], u[CH - 1]);
    }
  }
}

template <int CH>
__device__ __forceinline__ int gray_of(const int (&u)[CH]) {
  if (CH == 3) return rgb2gray(u[0], u[1], u[CH - 1]);
  return u[0];
}

// Kernel 1: geometry.  Grid (blocks, B): blockIdx.y is the sample, the x blocks stride over its H*W output pixels.
template <int CH>
__global__ __launch_bounds__(256) void augment_geom_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask,
                                                           const lmn_aug_param_t* __restrict__ params, uint8_t* __restrict__ scratch,
                                                           unsigned long long* __restrict__ gray_sum, int64_t* __restrict__ labels,
                                                           const AugGeom g) {
  const int b = blockIdx.y;
  const lmn_aug_param_t& p = params[b];
  const int ch = p.h, cw = p.w, fl = p.flips, ssr = p.apply_ssr;
  const double scy = (double)ch / (double)g.H, scx = (double)cw / (double)g.W;  // prep_axis / resize_nearest scales
  const double a0 = p.iM[0], a1 = p.iM[1], a2 = p.iM[2], b0 = p.iM[3], b1 = p.iM[4], b2 = p.iM[5];
  const int64_t row_stride = (int64_t)g.Ws * CH;
  const uint8_t* isrc = img ? img + (((int64_t)b * g.Hs + p.y0) * g.Ws + p.x0) * CH : nullptr;
  const uint8_t* msrc = mask ? mask + ((int64_t)b * g.Hs + p.y0) * g.Ws + p.x0 : nullptr;
  const bool want_gray = img && p.apply_cj && p.cj[1] != 1.0;
  const int HW = g.H * g.W;
  unsigned long long gsum = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
    const int x = i % g.W, y = i / g.W;
    const int rx = (fl & 1) ? g.W - 1 - x : x, ry = (fl & 2) ? g.H - 1 - y : y;  // pixel of the warped frame
    if (img) {
      int v[CH];
      if (ssr) {
        const int X = warp_coord(a0, a1, a2, rx, ry, 16, 5), Y = warp_coord(b0, b1, b2, rx, ry, 16, 5);  // 1/32 pixel
        const int sx = sat_short(X >> 5), sy = sat_short(Y >> 5), fx = X & 31, fy = Y & 31;
        // remap weights (32 - fy | fy) x (32 - fx | fx) x 32.  cv2's table saturates the (0, 0) entry to 32767 and its fix-up
        // adds the missing 1 to the weight of the fourth neighbour: (32767 v00 + v11 + 2^14) >> 15 == v00 for bytes, as here.
        const int w00 = (32 - fy) * (32 - fx) * 32, w01 = (32 - fy) * fx * 32, w10 = fy * (32 - fx) * 32, w11 = fy * fx * 32;
        const bool inx0 = (unsigned)sx < (unsigned)g.W, inx1 = (unsigned)(sx + 1) < (unsigned)g.W;
        const bool iny0 = (unsigned)sy < (unsigned)g.H, iny1 = (unsigned)(sy + 1) < (unsigned)g.H;
        Axis ax0, ax1, ay0, ay1;
        aug_axis(inx0 ? sx : 0, cw, scx, true, ax0.s0, ax0.s1, ax0.a0, ax0.a1);
        aug_axis(inx1 ? sx + 1 : 0, cw, scx, true, ax1.s0, ax1.s1, ax1.a0, ax1.a1);
        aug_axis(iny0 ? sy : 0, ch, scy, false, ay0.s0, ay0.s1, ay0.a0, ay0.a1);
        aug_axis(iny1 ? sy + 1 : 0, ch, scy, false, ay1.s0, ay1.s1, ay1.a0, ay1.a1);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const int v00 = (iny0 && inx0) ? rc_value<CH>(isrc, row_stride, ax0, ay0, c) : 0;
          const int v01 = (iny0 && inx1) ? rc_value<CH>(isrc, row_stride, ax1, ay0, c) : 0;
          const int v10 = (iny1 && inx0) ? rc_value<CH>(isrc, row_stride, ax0, ay1, c) : 0;
          const int v11 = (iny1 && inx1) ? rc_value<CH>(isrc, row_stride, ax1, ay1, c) : 0;
          v[c] = min(max((v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11 + 16384) >> 15, 0), 255);
        }
      } else {
        Axis ax, ay;
        aug_axis(rx, cw, scx, true, ax.s0, ax.s1, ax.a0, ax.a1);
        aug_axis(ry, ch, scy, false, ay.s0, ay.s1, ay.a0, ay.a1);
#pragma unroll
        for (int c = 0; c < CH; ++c) v[c] = rc_value<CH>(isrc, row_stride, ax, ay, c);
      }
      uint8_t* d = scratch + ((int64_t)b * HW + i) * CH;
#pragma unroll
      for (int c = 0; c < CH; ++c) d[c] = (uint8_t)v[c];
      if (want_gray) {  // the image as contrast sees it: the ops ahead of contrast in this sample's order (all pointwise)
        for (int k = 0; k < 4 && p.order[k] != 1; ++k) cj_op<CH>(p.order[k], v, p.cj, 0.0);
        gsum += (unsigned long long)gray_of<CH>(v);
      }
    }
    if (mask) {
      int mx = rx, my = ry;
      bool in = true;
      if (ssr) {  // INTER_NEAREST: round_delta = AB_SCALE / 2, >> AB_BITS
        mx = sat_short(warp_coord(a0, a1, a2, rx, ry, 512, 10));
        my = sat_short(warp_coord(b0, b1, b2, rx, ry, 512, 10));
        in = (unsigned)mx < (unsigned)g.W && (unsigned)my < (unsigned)g.H;
      }
      int v = 0;
      if (in) {
        const int sx = min((int)floor(mx * scx), cw - 1), sy = min((int)floor(my * scy), ch - 1);
        v = msrc[(int64_t)sy * g.Ws + sx];
      }
      labels[(int64_t)b * HW + i] = g.mask_mode ? v : (v > 127 ? 1 : 0);
    }
  }
  if (want_gray) {  // block-uniform branch
    __shared__ unsigned long long red[4];
    for (int o = 32; o > 0; o >>= 1) gsum += __shfl_down(gsum, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = gsum;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(gray_sum + b, red[0] + red[1] + red[2] + red[3]);
  }
}

// Normalize: (float)((double)u - 255 mean), then * 1 / (255 std) in double (numpy: float32 array -= float64 mean, *= float64)
__device__ __forceinline__ float aug_normalize(int u, double m255, double inv) {
  const float t = (float)((double)u - m255);
  return (float)((double)t * inv);
}

// Kernel 2: ColorJitter + Normalize, scratch [B,H,W,CH] uint8 -> out [B,CH,H,W] fp32 (each channel plane written coalesced).
// U8OUT (the OneOf entry): the jittered bytes go to out_u8 [B,H,W,CH] instead, and Normalize runs after the OneOf stage.
template <int CH, bool U8OUT>
__global__ __launch_bounds__(256) void augment_color_kernel(const uint8_t* __restrict__ scratch, const lmn_aug_param_t* __restrict__ params,
                                                            const unsigned long long* __restrict__ gray_sum, float* __restrict__ out,
                                                            uint8_t* __restrict__ out_u8, const AugGeom g) {
  const int b = blockIdx.y;
  const lmn_aug_param_t& p = params[b];
  const int HW = g.H * g.W;
  const bool cj = p.apply_cj;
  const double mean_gray = (cj && p.cj[1] != 1.0) ? (double)gray_sum[b] / (double)HW : 0.0;  // numpy mean of a uint8 image: exact
  for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
    const uint8_t* s = scratch + ((int64_t)b * HW + i) * CH;
    int u[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) u[c] = s[c];
    if (cj)
      for (int k = 0; k < 4; ++k) cj_op<CH>(p.order[k], u, p.cj, mean_gray);
    if (U8OUT) {
      uint8_t* d = out_u8 + ((int64_t)b * HW + i) * CH;
#pragma unroll
      for (int c = 0; c < CH; ++c) d[c] = (uint8_t)u[c];
    } else {
#pragma unroll
      for (int c = 0; c < CH; ++c) out[((int64_t)b * CH + c) * HW + i] = aug_normalize(u[c], g.m255[c], g.inv[c]);
    }
  }
}

// Argument checks shared by the two entries (host arithmetic only, before any HIP call); fills g.  `who` names the entry.
static inline int aug_check_args(const char* who, const uint8_t* images, const uint8_t* masks, const lmn_aug_param_t* params,
                                 const int32_t* src_hw, const lmn_aug_param_t* params_dev, int B, int Hs, int Ws, int H, int W,
                                 int channels, int mask_mode, const double* mean, const double* std, const uint8_t* scratch,
                                 const uint64_t* gray_sum, const float* out, const int64_t* labels, AugGeom& g) {
  LMN_REQUIRE(channels == 1 || channels == 3, "%s: channels=%d not in {1, 3}", who, channels);
  LMN_REQUIRE(mask_mode == 0 || mask_mode == 1, "%s: mask_mode=%d not in {0, 1}", who, mask_mode);
  LMN_REQUIRE(params && params_dev, "%s: params and params_dev required", who);
  LMN_REQUIRE((images && out) || (masks && labels), "%s: nothing to do", who);
  LMN_REQUIRE(!images || (out && mean && std && scratch && gray_sum), "%s: images need out, mean, std, scratch and gray_sum", who);
  LMN_REQUIRE(!masks || labels, "%s: masks need labels", who);
  LMN_REQUIRE(B > 0 && Hs > 0 && Ws > 0, "%s: empty source batch", who);
  LMN_REQUIRE(H > 0 && W > 0, "%s: output size %dx%d", who, H, W);
  LMN_REQUIRE(B <= 65535, "%s: B=%d above 65535", who, B);
  LMN_REQUIRE(Hs < 32768 && Ws < 32768 && H < 32768 && W < 32768 && (int64_t)H * W < (1 << 30), "%s: side above 32767", who);
  for (int b = 0; b < B; ++b) {
    const lmn_aug_param_t& p = params[b];
    const int hb = src_hw ? src_hw[2 * b] : Hs, wb = src_hw ? src_hw[2 * b + 1] : Ws;
    LMN_REQUIRE(hb >= 1 && hb <= Hs && wb >= 1 && wb <= Ws, "%s: src_hw[%d] = %dx%d outside the %dx%d frame", who, b, hb, wb, Hs, Ws);
    LMN_REQUIRE(p.h > 0 && p.w > 0 && p.y0 >= 0 && p.x0 >= 0 && p.y0 <= hb - p.h && p.x0 <= wb - p.w,
                "%s: crop window %d (y0 %d, x0 %d, %dx%d) empty or outside the %dx%d source", who, b, p.y0, p.x0, p.h, p.w, hb, wb);
    LMN_REQUIRE(p.flips >= 0 && p.flips <= 3, "%s: flips[%d] = %d not in 0..3", who, b, p.flips);
    if (p.apply_ssr) {  // fixed-point coordinates of every pixel (cvRound(M * x * 1024) and their sums) stay inside int32
      const bool ok = fabs(p.iM[0]) <= 16.0 && fabs(p.iM[1]) <= 16.0 && fabs(p.iM[3]) <= 16.0 && fabs(p.iM[4]) <= 16.0 &&
                      fabs(p.iM[2]) <= 262144.0 && fabs(p.iM[5]) <= 262144.0;
      LMN_REQUIRE(ok, "%s: inverse SSR matrix %d out of range (|linear| <= 16, |shift| <= 2^18)", who, b);
    }
    if (p.apply_cj) {
      int seen = 0;
      for (int k = 0; k < 4; ++k) seen |= (p.order[k] >= 0 && p.order[k] < 4) ? 1 << p.order[k] : 16;
      LMN_REQUIRE(seen == 15, "%s: ColorJitter order %d is not a permutation of 0..3", who, b);
      const bool ok = p.cj[0] >= 0.0 && p.cj[0] <= 1e6 && p.cj[1] >= 0.0 && p.cj[1] <= 1e6 && p.cj[2] >= 0.0 && p.cj[2] <= 1e6 &&
                      p.cj[3] >= -0.5 && p.cj[3] <= 0.5;
      LMN_REQUIRE(ok, "%s: ColorJitter factors of sample %d out of range", who, b);
    }
  }
  g = AugGeom{Hs, Ws, H, W, mask_mode, {0, 0, 0}, {1, 1, 1}};
  if (images) {
    for (int c = 0; c < channels; ++c) {
      LMN_REQUIRE(std[c] > 0.0, "%s: std[%d] must be positive", who, c);
      g.m255[c] = mean[c] * 255.0;
      g.inv[c] = 1.0 / (std[c] * 255.0);
    }
  }
  return 0;
}

static inline dim3 aug_grid(int HW, int B) { return dim3(lmn_cdiv(HW, 256) < 1024 ? lmn_cdiv(HW, 256) : 1024, B); }

// parameter copy + gray-sum reset on the stream, then the geometry kernel (labels_dst: where the label map goes)
static inline int aug_launch_geom(const char* who, const uint8_t* images, const uint8_t* masks, const lmn_aug_param_t* params,
                                  lmn_aug_param_t* params_dev, int B, int channels, uint8_t* scratch, uint64_t* gray_sum,
                                  int64_t* labels_dst, const AugGeom& g, hipStream_t st) {
  hipError_t e = hipMemcpyAsync(params_dev, params, sizeof(lmn_aug_param_t) * (size_t)B, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && images) e = hipMemsetAsync(gray_sum, 0, sizeof(uint64_t) * (size_t)B, st);
  if (e != hipSuccess) {
    snprintf(g_lmn_err, sizeof(g_lmn_err), "%s: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  const dim3 grid = aug_grid(g.H * g.W, B);
  unsigned long long* gs = (unsigned long long*)gray_sum;
  if (channels == 1)
    LMN_LAUNCH((augment_geom_kernel<1>), grid, dim3(256), 0, st, images, masks, params_dev, scratch, gs, masks ? labels_dst : nullptr, g);
  else
    LMN_LAUNCH((augment_geom_kernel<3>), grid, dim3(256), 0, st, images, masks, params_dev, scratch, gs, masks ? labels_dst : nullptr, g);
  return lmn_launch_status(who);
}

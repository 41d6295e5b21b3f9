"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the training augmentations of row N4 (lmn_augment_u8 /
lm_net_amd.data.DeviceAugment); never imported by the product path.

Follows `dataset/data_loading.py:207-214` (RandomResizedCrop -> ShiftScaleRotate(BORDER_CONSTANT) -> HorizontalFlip ->
VerticalFlip -> ColorJitter) and `:227-228` (Normalize, ToTensorV2), for parameters drawn elsewhere (the dicts of
`lm_net_amd.data.pack_params`).  The arithmetic lives in two third-party packages that are NOT part of the reference and not
installed here: OpenCV (version unpinned by the reference) and albumentations (unpinned).  Restated from their published
algorithms:

  * RandomResizedCrop: cv2.resize of the crop window, `oracle.preprocess_ref.resize_linear_u8` (INTER_LINEAR, image) and
    `resize_nearest` (INTER_NEAREST, mask).
  * cv2.warpAffine (imgproc/src/imgwarp.cpp, WarpAffineInvoker + remapBilinear / remapNearest, the fixed-point path of
    OpenCV 4.10 and earlier), BORDER_CONSTANT 0: the forward matrix is inverted in double (D = 1/(M0 M4 - M1 M3), ...);
    AB_BITS 10, INTER_BITS 5; X = cvRound((M1 y + M2) * 1024) + round_delta + cvRound(M0 x * 1024) (round_delta 16 for
    INTER_LINEAR, 512 for INTER_NEAREST); INTER_LINEAR splits X >> 5 into the integer source pixel (X >> 10, saturated to
    short) and a 1/32 fraction, whose INTER_REMAP_COEF_SCALE (32768) weight table is the float product of the 1-D weights
    (1 - t, t), saturated to short, with cv2's fix-up that makes the four weights sum to 32768; the pixel is
    (sum v w + 2^14) >> 15 with out-of-frame neighbours at 0.  INTER_NEAREST takes X >> 10 (0 outside the frame).
    A.ShiftScaleRotate's matrix is `lm_net_amd.data.ssr_matrix` (getRotationMatrix2D about (W/2, H/2) plus the shift).
  * cv2.cvtColor uint8 (imgproc/src/color_rgb / color_hsv): RGB2GRAY (R 4899 + G 9617 + B 1868 + 2^13) >> 14; RGB2HSV_b with
    hsv_shift 12, sdiv_table[v] = cvRound((255 << 12) / v), hdiv_table180[d] = cvRound((180 << 12) / (6 d)), hue range 180;
    HSV2RGB_b in float32 (hscale 6/180, s and v times 1/255, sector table) and saturate_cast<uchar>(x * 255).  Channel 0 is R:
    the reference hands cv2.imread's BGR frames to ColorJitter, which treats them as RGB.
  * albumentations 1.3/1.4 ColorJitter with the uint8 `adjust_*_torchvision` functions (augmentations/functional.py):
    brightness LUT clip(v f, 0, 255).astype(uint8); contrast LUT clip(v f + mean (1 - f), 0, 255).astype(uint8) with mean =
    the float64 mean of the gray image (f = 0: fill int(mean + 0.5)); saturation cv2.addWeighted(img, f, gray, 1 - f, 0)
    (float32, cvRound); hue RGB2HSV, h -> np.mod(h + 180 f, 180).astype(uint8), HSV2RGB; saturation and hue are no-ops on one
    channel; a factor of 1 (hue 0) returns the image untouched.  The four ops run in the sampled order.
  * A.Normalize: `oracle.preprocess_ref.normalize`.

PARITY UNPINNED against OpenCV and albumentations themselves: the reference holds no fixtures for its data pipeline and
neither package can be imported here.  OpenCV 4.11 and later compute warpAffine coordinates in float and may differ from
this restatement in the last bit; builds whose addWeighted / cvtColor go through FMA or IPP kernels may differ in rounding.
Pinned by hand-checkable cases in tests/test_augment_cpu.py.
"""
import numpy as np

from oracle import preprocess_ref as P

AB_BITS, INTER_BITS = 10, 5
INTER_TAB_SIZE = 1 << INTER_BITS
COEF_SCALE = 32768


# ---------------------------------------------------------------- warpAffine
def invert_affine(M):
    M = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(-1)]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    A12, A21 = M[1] * -D, M[3] * -D
    return [A11, A12, -A11 * M[2] - A12 * M[5], A21, A22, -A21 * M[2] - A22 * M[5]]


def remap_table():
    """[32, 32, 4] int weights (w00, w01, w10, w11) of cv2's bilinear remap for fraction (fy, fx)."""
    t = np.arange(INTER_TAB_SIZE, dtype=np.float32) / np.float32(INTER_TAB_SIZE)
    tab1 = np.stack([np.float32(1) - t, t], axis=1)                              # [32, 2]
    v = tab1[:, None, :, None] * tab1[None, :, None, :]                          # [fy, fx, k1, k2] float32
    itab = np.clip(np.rint(v * np.float32(COEF_SCALE)), -32768, 32767).astype(np.int64).reshape(32, 32, 4)
    diff = itab.sum(axis=2) - COEF_SCALE
    # cv2's fix-up scans the weights from [ksize/2][ksize/2] = [1][1] on; for this table only entry (0, 0) (1.0 saturated to
    # 32767) is short, and the missing unit lands on its w11
    itab[..., 3] -= np.where(diff != 0, diff, 0)
    return itab


def _round(v):
    return np.rint(v).astype(np.int64)


def warp_affine(img, M, inter_linear):
    """img uint8 [H,W] or [H,W,C] -> cv2.warpAffine(img, M, (W, H), flags, BORDER_CONSTANT, 0), output size = input size."""
    H, W = img.shape[:2]
    a = invert_affine(M)
    x = np.arange(W, dtype=np.float64)
    y = np.arange(H, dtype=np.float64)
    rd = (1 << AB_BITS) // INTER_TAB_SIZE // 2 if inter_linear else (1 << AB_BITS) // 2     # round_delta
    X = (_round((a[1] * y + a[2]) * 1024.0)[:, None] + rd) + _round(a[0] * x * 1024.0)[None, :]
    Y = (_round((a[4] * y + a[5]) * 1024.0)[:, None] + rd) + _round(a[3] * x * 1024.0)[None, :]
    src = img.reshape(H, W, -1).astype(np.int64)
    if not inter_linear:
        sx, sy = np.clip(X >> AB_BITS, -32768, 32767), np.clip(Y >> AB_BITS, -32768, 32767)
        inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
        out = np.where(inside[..., None], src[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)], 0)
        return out.astype(img.dtype).reshape(img.shape)
    X, Y = X >> (AB_BITS - INTER_BITS), Y >> (AB_BITS - INTER_BITS)
    sx, sy = np.clip(X >> INTER_BITS, -32768, 32767), np.clip(Y >> INTER_BITS, -32768, 32767)
    w = remap_table()[Y & (INTER_TAB_SIZE - 1), X & (INTER_TAB_SIZE - 1)]      # [H, W, 4]

    def tap(dy, dx):
        yy, xx = sy + dy, sx + dx
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return np.where(inside[..., None], src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0)

    acc = (tap(0, 0) * w[..., 0:1] + tap(0, 1) * w[..., 1:2] + tap(1, 0) * w[..., 2:3] + tap(1, 1) * w[..., 3:4])
    out = np.clip((acc + (1 << 14)) >> 15, 0, 255)
    return out.astype(np.uint8).reshape(img.shape)


# ---------------------------------------------------------------- colour conversions (uint8)
def rgb2gray(img):
    i = img.astype(np.int64)
    return ((i[..., 0] * 4899 + i[..., 1] * 9617 + i[..., 2] * 1868 + (1 << 13)) >> 14).astype(np.uint8)


def rgb2hsv(img):
    i = img.astype(np.int64)
    r, g, b = i[..., 0], i[..., 1], i[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    k = np.arange(256, dtype=np.float64)
    with np.errstate(divide="ignore"):
        sdiv = np.where(k > 0, np.rint((255 << 12) / k), 0).astype(np.int64)
        hdiv = np.where(k > 0, np.rint((180 << 12) / (6.0 * k)), 0).astype(np.int64)
    s = (diff * sdiv[v] + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv[diff] + (1 << 11)) >> 12
    h = np.where(h < 0, h + 180, h)
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


def hsv2rgb(hsv):
    f32 = np.float32
    h = hsv[..., 0].astype(f32) * (f32(6) / f32(180))
    s = hsv[..., 1].astype(f32) * (f32(1) / f32(255))
    v = hsv[..., 2].astype(f32) * (f32(1) / f32(255))
    h = np.where(h >= f32(6), h - f32(6), h)
    sector = np.floor(h).astype(np.int64)
    h = h - sector.astype(f32)
    bad = (sector < 0) | (sector >= 6)
    sector, h = np.where(bad, 0, sector), np.where(bad, f32(0), h)
    one = f32(1)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], axis=-1)
    sd = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])[sector]   # (b, g, r) per pixel
    bgr = np.take_along_axis(tab, sd, axis=-1)
    rgb = bgr[..., ::-1] * f32(255)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------- ColorJitter (albumentations uint8 functions)
def _gray_mean(img):
    g = img[..., 0] if img.shape[-1] == 1 else rgb2gray(img)
    return g.mean(), int(g.astype(np.int64).sum())


def adjust_brightness(img, f):
    if f == 1:
        return img
    lut = np.clip(np.arange(0, 256) * f, 0, 255).astype(np.uint8)
    return lut[img]


def adjust_contrast(img, f):
    if f == 1:
        return img
    mean, _ = _gray_mean(img)
    if f == 0:
        return np.full_like(img, int(mean + 0.5))
    lut = np.arange(0, 256) * f
    lut = lut + mean * (1 - f)
    return np.clip(lut, 0, 255).astype(np.uint8)[img]


def adjust_saturation(img, f):
    if f == 1 or img.shape[-1] == 1:
        return img
    gray = rgb2gray(img)[..., None]
    if f == 0:
        return np.repeat(gray, 3, axis=-1)
    alpha, beta = np.float32(f), np.float32(1 - f)
    t = (img.astype(np.float32) * alpha + gray.astype(np.float32) * beta) + np.float32(0)
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def adjust_hue(img, f):
    if f == 0 or img.shape[-1] == 1:
        return img
    hsv = rgb2hsv(img)
    lut = np.mod(np.arange(0, 256, dtype=np.int16) + 180 * f, 180).astype(np.uint8)
    hsv[..., 0] = lut[hsv[..., 0]]
    return hsv2rgb(hsv)


OPS = (adjust_brightness, adjust_contrast, adjust_saturation, adjust_hue)


def color_jitter(img, factors, order):
    """img uint8 [H,W,C] -> (jittered image, gray sum of the image contrast saw, or None when contrast did not run)."""
    gsum = None
    for k in order:
        if k == 1 and factors[1] != 1:
            gsum = _gray_mean(img)[1]
        img = OPS[k](img, factors[k])
    return img, gsum


# ---------------------------------------------------------------- the whole per-sample transform
def augment_one(img, mask, p, size, mean, std, mask_mode=0):
    """img uint8 [Hs,Ws,C] (or None), mask uint8 [Hs,Ws] (or None), p: a `pack_params` dict -> (fp32 [C,H,W], int64 [H,W],
    gray sum of the contrast op or None)."""
    H, W = size
    y0, x0, h, w = p["crop"]
    M, fl, cj = p.get("M"), int(p.get("flips", 0)), p.get("cj")
    x = y = gsum = None
    if img is not None:
        im = P.resize_linear_u8(img[y0:y0 + h, x0:x0 + w], H, W)
        if M is not None:
            im = warp_affine(im, M, True)
        if fl & 1:
            im = im[:, ::-1]
        if fl & 2:
            im = im[::-1]
        im = np.ascontiguousarray(im)
        if cj is not None:
            im, gsum = color_jitter(im, cj, p.get("order", (0, 1, 2, 3)))
        x = P.normalize(im, mean, std).transpose(2, 0, 1)
    if mask is not None:
        mk = (mask > 127).astype(np.uint8) if mask_mode == 0 else mask
        mk = P.resize_nearest(mk[y0:y0 + h, x0:x0 + w], H, W)
        if M is not None:
            mk = warp_affine(mk, M, False)
        if fl & 1:
            mk = mk[:, ::-1]
        if fl & 2:
            mk = mk[::-1]
        y = mk.astype(np.int64)
    return x, y, gsum


def augment(images, masks, params, size, mean, std, mask_mode=0, src_hw=None):
    """Batch form: images uint8 [B,Hs,Ws,C] (padded when src_hw [B,2] is given), masks [B,Hs,Ws] -> stacked outputs and the
    per-sample gray sums (0 where contrast did not run, as the device buffer)."""
    xs, ys, gs = [], [], []
    for b, p in enumerate(params):
        hs, ws = (images if images is not None else masks).shape[1:3] if src_hw is None else src_hw[b]
        im = None if images is None else images[b, :hs, :ws].reshape(hs, ws, -1)
        mk = None if masks is None else masks[b, :hs, :ws]
        x, y, g = augment_one(im, mk, p, size, mean, std, mask_mode)
        xs.append(x)
        ys.append(y)
        gs.append(0 if g is None else g)
    return (None if images is None else np.stack(xs), None if masks is None else np.stack(ys), np.array(gs, dtype=np.int64))

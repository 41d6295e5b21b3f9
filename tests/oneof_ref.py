"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the OneOf block of the training transform (lmn_augment_oneof_u8 /
lm_net_amd.data.DeviceAugment(one_of=...)); never imported by the product path.

Follows `dataset/data_loading.py:215-225`: one of ToGray, GridDistortion, ElasticTransform, CLAHE, HueSaturationValue,
ChannelShuffle, GridDropout, RGBShift, GaussianBlur on the colour-jittered uint8 frame (and, for the two geometric members, on
the labels), for values drawn elsewhere (the `"oneof"` dicts of `lm_net_amd.data.pack_oneof`).  Restated from the published
algorithms of OpenCV and albumentations, neither of which is installed here -- PARITY with the libraries themselves is UNPINNED,
as for tests/augment_ref.py; the hand-checkable cases and the scipy cross-checks of tests/test_oneof_cpu.py pin this file:

  * to_gray: cv2 RGB2GRAY (augment_ref.rgb2gray) copied to the three channels.
  * rgb_shift: albumentations' uint8 LUT clip(v + shift, 0, 255).astype(uint8) per channel, in double.
  * channel_shuffle: out[c] = in[perm[c]].
  * hsv: cv2 RGB2HSV / HSV2RGB on uint8 (augment_ref), hue LUT np.mod(h + shift, 180).astype(uint8), saturation and value LUTs
    clip(v + shift, 0, 255).astype(uint8).
  * grid_dropout (defaults): unit = max(2, min(H, W) // 10) on both axes, hole = min(max(int(unit ratio), 1), unit - 1), no
    offset; pixels with x % unit < hole and y % unit < hole become 0; the mask stays (mask_fill_value=None).
  * gaussian_blur: cv2.GaussianBlur with sigma 0 and ksize 3, 5, 7 takes the fixed kernels [1,2,1]/4, [1,4,6,4,1]/16,
    [2,7,14,18,14,7,2]/64; all dyadic, so out = (sum wy wx v + half) >> shift is exact; BORDER_REFLECT_101.
  * clahe: cv2.createCLAHE(clip, (8, 8)): frame padded bottom / right by reflect-101 to multiples of 8; per tile a 256-bin
    histogram clipped at max(int(clip area / 256), 1), the excess spread as excess // 256 to every bin and the residual to every
    max(256 // residual, 1)-th bin; lut = saturate(rint(cumsum * (255.f / area))); per pixel the float32 bilinear blend of the
    four neighbouring tiles' LUT values at tile coordinate y * (1.f / tile_h) - 0.5 (clamped at the grid's edge), rint.  On 3
    channels: on L of an 8-bit LAB in table-driven integer arithmetic (lm_net_amd.data.lab_tables, the tables the kernels use; the
    forward path is cv2's RGB2Lab_b: gamma table, 2^12 fixed-point matrix, cube-root table of 2^15 scale).
  * cv2.remap with float maps, INTER_LINEAR (coordinates rounded to 1/32 pixel, the 32768-scale weight table of
    augment_ref.remap_table, whose (0, 0) entry blends bytes exactly like the plain products) and INTER_NEAREST (rint of the
    map) for labels, BORDER_REFLECT_101 -- used by grid_distortion (maps from lm_net_amd.data.grid_distortion_map:
    albumentations' piecewise linspace, cells sampled without their end point so that factors of 1 are the identity) and
    elastic (albumentations >= 1.4: two U[-1, 1) noise fields blurred by a separable Gaussian of radius int(4 sigma + 0.5) with
    reflect-101 as a periodic fold, rows then columns, fp32 accumulation in tap order, times alpha; map = (x + dx, y + dy)).
"""
import numpy as np

import augment_ref as A
from lm_net_amd import data as D
from lm_net_amd import hip
from oracle import preprocess_ref as P

f32 = np.float32
BLUR = {3: ([1, 2, 1], 4), 5: ([1, 4, 6, 4, 1], 8), 7: ([2, 7, 14, 18, 14, 7, 2], 12)}     # 1-D weights, shift of the 2-D sum


def reflect101(i, n):
    """BORDER_REFLECT_101 as a periodic fold (any distance from the frame)."""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


# ---------------------------------------------------------------- 8-bit LAB (integer, the tables of lm_net_amd.data.lab_tables)
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def rgb2lab(img):
    """uint8 [...,3] (channel 0 = R) -> int64 L8, a8, b8."""
    T = D.lab_tables().astype(np.int64)
    i = img.astype(np.int64)
    R, G, B = (T[hip.LAB_GAMMA + i[..., c]] for c in range(3))
    C = T[hip.LAB_FWD:hip.LAB_FWD + 9]
    fX, fY, fZ = (T[hip.LAB_CBRT + _descale(R * C[3 * k] + G * C[3 * k + 1] + B * C[3 * k + 2], 12)] for k in range(3))
    L = np.clip(_descale(296 * fY - 1336935, 15), 0, 255)
    a = np.clip(_descale(500 * (fX - fY) + 128 * 32768, 15), 0, 255)
    b = np.clip(_descale(200 * (fY - fZ) + 128 * 32768, 15), 0, 255)
    return L, a, b


def _finv(f):
    lin = np.maximum((f - 4520) * 4208, 0) >> 15
    return np.where(f > 6780, (f * f * f) >> 30, lin)


def lab2rgb(L, a, b):
    T = D.lab_tables().astype(np.int64)
    fy = T[hip.LAB_FY + L]
    X, Y, Z = _finv(fy + T[hip.LAB_DA + a]), _finv(fy), _finv(fy - T[hip.LAB_DB + b])
    C = T[hip.LAB_INV:hip.LAB_INV + 9]
    out = []
    for c in range(3):
        lin = (C[3 * c] * X + C[3 * c + 1] * Y + C[3 * c + 2] * Z + 4096) >> 13
        out.append(T[hip.LAB_INVGAMMA + np.clip(lin, 0, 16384)])
    return np.stack(out, axis=-1).astype(np.uint8)


# ---------------------------------------------------------------- members
def to_gray(img):
    return np.repeat(A.rgb2gray(img)[..., None], 3, axis=-1)


def rgb_shift(img, shift):
    out = np.empty_like(img)
    for c in range(3):
        out[..., c] = np.clip(np.arange(256, dtype=np.float64) + float(shift[c]), 0, 255).astype(np.uint8)[img[..., c]]
    return out


def channel_shuffle(img, perm):
    return np.ascontiguousarray(img[..., list(perm)])


def hsv_shift(img, shift):
    hsv = A.rgb2hsv(img)
    k = np.arange(256, dtype=np.float64)
    hsv[..., 0] = np.mod(k + float(shift[0]), 180).astype(np.uint8)[hsv[..., 0]]
    hsv[..., 1] = np.clip(k + float(shift[1]), 0, 255).astype(np.uint8)[hsv[..., 1]]
    hsv[..., 2] = np.clip(k + float(shift[2]), 0, 255).astype(np.uint8)[hsv[..., 2]]
    return A.hsv2rgb(hsv)


def grid_dropout_holes(H, W, ratio=0.5):
    """bool [H,W]: the pixels grid_dropout zeroes."""
    unit = max(2, min(H, W) // 10)
    hole = min(max(int(unit * ratio), 1), unit - 1)
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    return (x % unit < hole) & (y % unit < hole)


def grid_dropout(img, ratio=0.5):
    out = img.copy()
    out[grid_dropout_holes(img.shape[0], img.shape[1], ratio)] = 0
    return out


def gaussian_blur(img, k):
    w, shift = BLUR[k]
    r = k // 2
    H, W = img.shape[:2]
    src = img.astype(np.int64)
    ys, xs = np.arange(H), np.arange(W)
    rows = sum(w[j] * src[:, reflect101(xs + j - r, W)] for j in range(k))
    acc = sum(w[j] * rows[reflect101(ys + j - r, H)] for j in range(k))
    return ((acc + (1 << (shift - 1))) >> shift).astype(np.uint8)


def clahe_plane(v, clip):
    """v int [H,W] in 0..255 -> CLAHE with an 8 x 8 grid."""
    H, W = v.shape
    th, tw = (H + 7) // 8, (W + 7) // 8
    area = th * tw
    pad = v[reflect101(np.arange(8 * th), H)][:, reflect101(np.arange(8 * tw), W)]
    clip_int = max(int(float(clip) * area / 256), 1)
    luts = np.zeros((8, 8, 256), dtype=np.int64)
    scale = f32(255) / f32(area)
    for ty in range(8):
        for tx in range(8):
            h = np.bincount(pad[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].reshape(-1), minlength=256).astype(np.int64)
            excess = int(np.maximum(h - clip_int, 0).sum())
            h = np.minimum(h, clip_int)
            batch, resid = excess // 256, excess % 256
            h += batch
            if resid:
                step = max(256 // resid, 1)
                idx = np.arange(0, 256, step)[:resid]
                h[idx] += 1
            luts[ty, tx] = np.clip(np.rint(np.cumsum(h).astype(f32) * scale), 0, 255).astype(np.int64)
    tyf = np.arange(H, dtype=f32) * (f32(1) / f32(th)) - f32(0.5)
    txf = np.arange(W, dtype=f32) * (f32(1) / f32(tw)) - f32(0.5)
    ty1, tx1 = np.floor(tyf).astype(np.int64), np.floor(txf).astype(np.int64)
    ya, xa = (tyf - ty1.astype(f32))[:, None], (txf - tx1.astype(f32))[None, :]
    ya1, xa1 = f32(1) - ya, f32(1) - xa
    ty2, tx2 = np.minimum(ty1 + 1, 7)[:, None], np.minimum(tx1 + 1, 7)[None, :]
    ty1, tx1 = np.maximum(ty1, 0)[:, None], np.maximum(tx1, 0)[None, :]
    l11, l12 = luts[ty1, tx1, v].astype(f32), luts[ty1, tx2, v].astype(f32)
    l21, l22 = luts[ty2, tx1, v].astype(f32), luts[ty2, tx2, v].astype(f32)
    res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya
    return np.clip(np.rint(res), 0, 255).astype(np.int64)


def clahe(img, clip):
    if img.shape[-1] == 1:
        return clahe_plane(img[..., 0].astype(np.int64), clip).astype(np.uint8)[..., None]
    L, a, b = rgb2lab(img)
    return lab2rgb(clahe_plane(L, clip), a, b)


def remap(img, labels, mx, my):
    """cv2.remap of img uint8 [H,W,C] (INTER_LINEAR) and labels int [H,W] (INTER_NEAREST) with float32 maps [H,W],
    BORDER_REFLECT_101.  Either may be None."""
    H, W = mx.shape
    out = lab = None
    if img is not None:
        ix, iy = np.rint(mx * f32(32)).astype(np.int64), np.rint(my * f32(32)).astype(np.int64)
        sx, sy, fx, fy = ix >> 5, iy >> 5, ix & 31, iy & 31
        w = A.remap_table()[fy, fx]
        src = img.astype(np.int64)
        xa, xb, ya, yb = reflect101(sx, W), reflect101(sx + 1, W), reflect101(sy, H), reflect101(sy + 1, H)
        acc = src[ya, xa] * w[..., 0:1] + src[ya, xb] * w[..., 1:2] + src[yb, xa] * w[..., 2:3] + src[yb, xb] * w[..., 3:4]
        out = np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)
    if labels is not None:
        lab = labels[reflect101(np.rint(my).astype(np.int64), H), reflect101(np.rint(mx).astype(np.int64), W)]
    return out, lab


def grid_distortion_maps(H, W, d):
    xx = D.grid_distortion_map(W, int(d["num_steps"]), d["xsteps"])
    yy = D.grid_distortion_map(H, int(d["num_steps"]), d["ysteps"])
    return np.broadcast_to(xx[None, :], (H, W)), np.broadcast_to(yy[:, None], (H, W))


def blur_field(field, sigma):
    """float32 [H,W] -> separable Gaussian (rows, then columns), reflect-101 fold, fp32 accumulation in tap order -r..r."""
    w = D.gaussian_weights(sigma)
    r = (w.size - 1) // 2
    H, W = field.shape
    xs, ys = np.arange(W), np.arange(H)
    acc = np.zeros((H, W), dtype=f32)
    for k in range(-r, r + 1):
        acc = acc + w[k + r] * field[:, reflect101(xs + k, W)]
    out = np.zeros((H, W), dtype=f32)
    for k in range(-r, r + 1):
        out = out + w[k + r] * acc[reflect101(ys + k, H)]
    return out


def elastic_maps(H, W, d):
    noise = D.elastic_noise(d["seed"], H, W)
    alpha = f32(float(d["alpha"]))
    dx, dy = blur_field(noise[0], d["sigma"]) * alpha, blur_field(noise[1], d["sigma"]) * alpha
    x, y = np.arange(W, dtype=f32)[None, :], np.arange(H, dtype=f32)[:, None]
    return x + dx, y + dy


def oneof_apply(img, labels, d):
    """img uint8 [H,W,C] or None, labels int64 [H,W] or None, d: None or a `"oneof"` dict -> (img, labels) after the member."""
    if d is None:
        return img, labels
    op = d["op"]
    if op in ("grid_distortion", "elastic"):
        H, W = (img if img is not None else labels).shape[:2]
        mx, my = grid_distortion_maps(H, W, d) if op == "grid_distortion" else elastic_maps(H, W, d)
        return remap(img, labels, np.ascontiguousarray(mx, dtype=f32), np.ascontiguousarray(my, dtype=f32))
    if img is None:
        return img, labels
    if op == "to_gray":
        img = to_gray(img)
    elif op == "rgb_shift":
        img = rgb_shift(img, d["shift"])
    elif op == "channel_shuffle":
        img = channel_shuffle(img, d["perm"])
    elif op == "hsv":
        img = hsv_shift(img, d["shift"])
    elif op == "grid_dropout":
        img = grid_dropout(img, d.get("ratio", 0.5))
    elif op == "gaussian_blur":
        img = gaussian_blur(img, d["k"])
    elif op == "clahe":
        img = clahe(img, d["clip"])
    else:
        raise ValueError(op)
    return img, labels


# ---------------------------------------------------------------- composed with augment_ref (the whole per-sample transform)
def augment_one(img, mask, p, size, mean, std, mask_mode=0):
    """augment_ref.augment_one with the OneOf member of p["oneof"] between ColorJitter and Normalize."""
    H, W = size
    y0, x0, h, w = p["crop"]
    M, fl, cj = p.get("M"), int(p.get("flips", 0)), p.get("cj")
    im = y = gsum = None
    if img is not None:
        im = P.resize_linear_u8(img[y0:y0 + h, x0:x0 + w], H, W)
        if M is not None:
            im = A.warp_affine(im, M, True)
        im = im[:, ::-1] if fl & 1 else im
        im = np.ascontiguousarray(im[::-1] if fl & 2 else im)
        if cj is not None:
            im, gsum = A.color_jitter(im, cj, p.get("order", (0, 1, 2, 3)))
    if mask is not None:
        mk = (mask > 127).astype(np.uint8) if mask_mode == 0 else mask
        mk = P.resize_nearest(mk[y0:y0 + h, x0:x0 + w], H, W)
        if M is not None:
            mk = A.warp_affine(mk, M, False)
        mk = mk[:, ::-1] if fl & 1 else mk
        y = np.ascontiguousarray(mk[::-1] if fl & 2 else mk).astype(np.int64)
    im, y = oneof_apply(im, y, p.get("oneof"))
    x = None if im is None else P.normalize(np.ascontiguousarray(im), mean, std).transpose(2, 0, 1)
    return x, y, gsum


def augment(images, masks, params, size, mean, std, mask_mode=0, src_hw=None):
    """Batch form of augment_one (the conventions of augment_ref.augment)."""
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

"""Device-side input pipeline.

The reference prepares every sample on the CPU with albumentations (`dataset/data_loading.py:203-229`):
`cv2.imread` (uint8 HWC, channel order as read), mask `cv2.threshold(127, 1)`, then `A.Resize(256, 256)`,
`A.Normalize()` and `ToTensorV2()` for validation; the training transform adds flips and colour / geometric
augmentations in front of the same Normalize.  `DevicePreprocess` runs the resize + (optional) flips + normalise +
layout change for a whole batch of raw uint8 frames already in HBM as ONE kernel (`lmn_preprocess_u8`), so decoded
frames can go to the GPU as bytes (3 B/pixel over PCIe instead of 12) and an 8-GPU loop is not fed by a CPU
albumentations pool.  `DeviceAugment` runs the per-sample part of the training transform (`:207-214`, `:227-228`):
RandomResizedCrop -> ShiftScaleRotate -> HorizontalFlip -> VerticalFlip -> ColorJitter -> Normalize, as two kernels
(`lmn_augment_u8`) on parameters drawn on the host.  `DeviceAugment(one_of="reference")` adds the `A.OneOf([...9 ops], p=0.4)`
block (`:215-225`) between ColorJitter and Normalize (`lmn_augment_oneof_u8`, include/lmnet_oneof.h): ToGray, GridDistortion,
ElasticTransform, CLAHE, HueSaturationValue, ChannelShuffle, GridDropout, RGBShift and GaussianBlur, all on the device.
"""
import ctypes
import math

import numpy as np
import torch

from . import hip


class DevicePreprocess:
    """`x, y = DevicePreprocess((256, 256))(images_u8, masks_u8, flips=None)`.

    images_u8: uint8 [B,Hs,Ws,3] on the GPU (channels=1: [B,Hs,Ws] or [B,Hs,Ws,1]); masks_u8: uint8 [B,Hs,Ws] or None; flips: uint8
    [B] or None (bit 0 horizontal, bit 1 vertical -- `A.HorizontalFlip` / `A.VerticalFlip`, drawn by the caller).
    Returns fp32 [B,channels,H,W] (what `LM_Net.forward` takes) and int64 [B,H,W] labels: in {0,1} for mask_mode="binary" (the
    reference's `cv2.threshold(127, 1)`), the mask's class ids for mask_mode="labels" (nearest resize, no threshold).
    mean / std: `channels` values each (the defaults are the 3-channel `A.Normalize()` ones; give a grayscale pair for channels=1)."""

    MASK_MODES = {"binary": 0, "labels": 1}

    def __init__(self, size=(256, 256), mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), channels=3, mask_mode="binary"):
        if channels not in (1, 3):
            raise ValueError("DevicePreprocess: channels = %r, must be 1 or 3" % (channels,))
        if mask_mode not in self.MASK_MODES:
            raise ValueError("DevicePreprocess: mask_mode = %r, must be 'binary' or 'labels'" % (mask_mode,))
        if len(mean) != channels or len(std) != channels:
            raise ValueError("DevicePreprocess: mean and std need %d values each for channels=%d" % (channels, channels))
        self.size = (int(size[0]), int(size[1]))
        self.mean, self.std = tuple(mean), tuple(std)     # A.Normalize() defaults, max_pixel_value = 255
        self.channels, self.mask_mode = int(channels), mask_mode

    def __call__(self, images, masks=None, flips=None):
        ref = images if images is not None else masks
        if ref is None:
            raise ValueError("DevicePreprocess: images or masks required")
        if not ref.is_cuda:
            raise RuntimeError("DevicePreprocess runs on the HIP device only (got %s); there is no CPU path" % ref.device)
        B, (H, W) = ref.shape[0], self.size
        if images is not None:
            ok = (images.dim() == 4 and images.shape[3] == self.channels) or (self.channels == 1 and images.dim() == 3)
            if not ok:
                raise ValueError("DevicePreprocess(channels=%d): images of shape %s" % (self.channels, tuple(images.shape)))
        x = torch.empty(B, self.channels, H, W, device=ref.device, dtype=torch.float32) if images is not None else None
        y = torch.empty(B, H, W, device=ref.device, dtype=torch.int64) if masks is not None else None
        if self.channels == 3 and self.mask_mode == "binary":
            hip.preprocess_u8(images, masks, flips, x, y, self.mean, self.std)
        else:
            hip.preprocess_u8_ex(images, masks, flips, x, y, self.mean, self.std, self.channels, self.MASK_MODES[self.mask_mode])
        return x, y


def ssr_matrix(H, W, angle, scale, dx, dy):
    """The forward 2x3 matrix of A.ShiftScaleRotate on an H x W frame: cv2.getRotationMatrix2D((W/2, H/2), angle, scale) plus the
    shift (dx*W, dy*H).  The centre (W/2, H/2) is the albumentations 1.3 convention (later releases moved it by half a pixel)."""
    a = math.radians(angle)
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    cx, cy = W / 2.0, H / 2.0
    return [alpha, beta, (1.0 - alpha) * cx - beta * cy + dx * W, -beta, alpha, beta * cx + (1.0 - alpha) * cy + dy * H]


def invert_affine(M):
    """cv2.invertAffineTransform arithmetic (the inversion cv2.warpAffine applies to a forward matrix), in double."""
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22, A12, A21 = M[4] * D, M[0] * D, -M[1] * D, -M[3] * D
    return [A11, A12, -A11 * M[2] - A12 * M[5], A21, A22, -A21 * M[2] - A22 * M[5]]


def pack_params(samples):
    """List of per-sample dicts -> ctypes array of hip.AugParam (lmn_aug_param_t).  Keys: crop (y0, x0, h, w); M (forward SSR
    matrix, 6 values) or None = no warp; flips (bit 0 horizontal, bit 1 vertical); cj (brightness, contrast, saturation, hue)
    or None = no ColorJitter; order (a permutation of 0..3, default 0, 1, 2, 3)."""
    arr = (hip.AugParam * len(samples))()
    for p, s in zip(arr, samples):
        y0, x0, h, w = (int(v) for v in s["crop"])
        if h <= 0 or w <= 0 or y0 < 0 or x0 < 0:
            raise ValueError("DeviceAugment: crop window %r is empty or starts outside the frame" % (tuple(s["crop"]),))
        p.y0, p.x0, p.h, p.w = y0, x0, h, w
        fl = int(s.get("flips", 0))
        if fl not in (0, 1, 2, 3):
            raise ValueError("DeviceAugment: flips = %r, must be 0..3" % (fl,))
        p.flips = fl
        M = s.get("M")
        if M is not None:
            M = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(-1)]
            if len(M) != 6 or not all(math.isfinite(v) for v in M):
                raise ValueError("DeviceAugment: M must be 6 finite values (a 2x3 matrix)")
            p.apply_ssr, p.M[:], p.iM[:] = 1, M, invert_affine(M)
        cj = s.get("cj")
        if cj is not None:
            cj = [float(v) for v in cj]
            order = [int(v) for v in s.get("order", (0, 1, 2, 3))]
            if sorted(order) != [0, 1, 2, 3]:
                raise ValueError("DeviceAugment: ColorJitter order %r is not a permutation of 0..3" % (order,))
            if len(cj) != 4 or not all(math.isfinite(v) for v in cj) or min(cj[:3]) < 0 or abs(cj[3]) > 0.5:
                raise ValueError("DeviceAugment: ColorJitter factors %r (brightness, contrast, saturation >= 0; |hue| <= 0.5)" % (cj,))
            p.apply_cj, p.cj[:], p.order[:] = 1, cj, order
    return arr


# ---------------------------------------------------------------- the OneOf block (dataset/data_loading.py:215-225)
# member -> its settings and their albumentations defaults
ONEOF_MEMBERS = {
    "to_gray": {}, "grid_distortion": {"num_steps": 5, "distort_limit": 0.3}, "elastic": {"alpha": 1.0, "sigma": 50.0},
    "clahe": {"clip_limit": (1.0, 4.0), "tile_grid": (8, 8)}, "hsv": {"hue": 20.0, "sat": 30.0, "val": 20.0}, "channel_shuffle": {},
    "grid_dropout": {"ratio": 0.5}, "rgb_shift": {"r": 20.0, "g": 20.0, "b": 20.0}, "gaussian_blur": {"blur_limit": (3, 7)},
}
ONEOF_REFERENCE = ("to_gray", "grid_distortion", "elastic", "clahe", "hsv", "channel_shuffle", "grid_dropout", "rgb_shift",
                   "gaussian_blur")                      # data_loading.py:216-224, in that order
ONEOF_COLOUR = ("to_gray", "hsv", "channel_shuffle", "rgb_shift")      # need channels == 3


def _oneof_check(name, cfg):
    """Range checks of one member's settings; raises ValueError."""
    def bad(what):
        raise ValueError("DeviceAugment: one_of member %r: %s" % (name, what))
    if name == "grid_distortion" and not (1 <= int(cfg["num_steps"]) <= 64 and cfg["num_steps"] == int(cfg["num_steps"])
                                          and 0 <= cfg["distort_limit"] < 1):
        bad("num_steps in 1..64 and 0 <= distort_limit < 1")
    if name == "elastic" and not (cfg["sigma"] > 0 and int(4.0 * cfg["sigma"] + 0.5) <= hip.ONEOF_MAX_RADIUS and abs(cfg["alpha"]) <= 1e6):
        bad("sigma in (0, %d] and |alpha| <= 1e6" % (hip.ONEOF_MAX_RADIUS // 4))
    if name == "clahe" and not (len(cfg["clip_limit"]) == 2 and 1 <= cfg["clip_limit"][0] <= cfg["clip_limit"][1] <= 1e6
                                and tuple(cfg["tile_grid"]) == (8, 8)):
        bad("1 <= clip_limit[0] <= clip_limit[1] and tile_grid (8, 8)")
    if name == "hsv" and not all(0 <= cfg[k] <= 255 for k in ("hue", "sat", "val")):
        bad("hue, sat, val limits in 0..255")
    if name == "rgb_shift" and not all(0 <= cfg[k] <= 255 for k in ("r", "g", "b")):
        bad("r, g, b limits in 0..255")
    if name == "grid_dropout" and not 0 < cfg["ratio"] <= 1:
        bad("0 < ratio <= 1")
    if name == "gaussian_blur":
        lo, hi = cfg["blur_limit"]
        if not (lo in (3, 5, 7) and hi in (3, 5, 7) and lo <= hi):
            bad("blur_limit: odd sizes 3..7, increasing")


def parse_one_of(one_of, channels):
    """`one_of` of DeviceAugment -> [(member, settings)]; raises ValueError (unknown member or setting, empty list, a colour member
    on one channel, a setting out of range)."""
    if isinstance(one_of, str):
        if one_of != "reference":
            raise ValueError("DeviceAugment: one_of = %r, must be None, 'reference' or a list of members" % (one_of,))
        one_of = list(ONEOF_REFERENCE)
    members = []
    for m in one_of:
        name, over = (m, {}) if isinstance(m, str) else (m[0], dict(m[1]))
        if name not in ONEOF_MEMBERS:
            raise ValueError("DeviceAugment: unknown one_of member %r (known: %s)" % (name, ", ".join(ONEOF_MEMBERS)))
        unknown = [k for k in over if k not in ONEOF_MEMBERS[name]]
        if unknown:
            raise ValueError("DeviceAugment: one_of member %r has no setting %s" % (name, unknown))
        cfg = dict(ONEOF_MEMBERS[name], **over)
        _oneof_check(name, cfg)
        members.append((name, cfg))
    if not members:
        raise ValueError("DeviceAugment: one_of is empty")
    colour = [n for n, _ in members if n in ONEOF_COLOUR]
    if channels != 3 and colour:
        raise ValueError("DeviceAugment: one_of members %s need channels == 3" % ", ".join(colour))
    return members


_LAB = []


def lab_tables():
    """The int32 tables of the 8-bit LAB conversion CLAHE uses on 3-channel frames (offsets hip.LAB_*), built once in double and
    shared by the kernels and their numpy restatement, so that both index CLAHE's LUT with the same L8.  sRGB primaries, D65
    white; forward: gamma table (scale 2040) -> XYZ / white in 2^12 fixed point -> f() table (scale 2^15) -> L8 = (116 fY - 16) *
    2.55, a8 = 500 (fX - fY) + 128, b8 = 200 (fY - fZ) + 128; inverse: fy, fx - fy, fy - fz tables -> f^-1 in integers -> RGB in
    2^12 fixed point -> inverse-gamma table of 2^14 + 1 entries."""
    if _LAB:
        return _LAB[0]
    T = np.zeros(hip.LAB_TABLE_INTS, dtype=np.int64)
    v = np.arange(256) / 255.0
    T[hip.LAB_GAMMA:hip.LAB_GAMMA + 256] = np.rint(2040.0 * np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4))
    t = np.arange(3072) / 2040.0
    T[hip.LAB_CBRT:hip.LAB_CBRT + 3072] = np.rint(32768.0 * np.where(t < 0.008856, t * 7.787 + 16.0 / 116.0, np.cbrt(t)))
    k = np.arange(256)
    T[hip.LAB_FY:hip.LAB_FY + 256] = np.rint(32768.0 * ((k * 100.0 / 255.0 + 16.0) / 116.0))
    T[hip.LAB_DA:hip.LAB_DA + 256] = np.rint(32768.0 * (k - 128.0) / 500.0)
    T[hip.LAB_DB:hip.LAB_DB + 256] = np.rint(32768.0 * (k - 128.0) / 200.0)
    M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    white = M.sum(axis=1)                                       # D65: (0.950456, 1, 1.088754)
    fwd = np.rint(4096.0 * M / white[:, None]).astype(np.int64)
    fwd[:, 1] += 4096 - fwd.sum(axis=1)                         # white maps to exactly 1.0 on every row
    T[hip.LAB_FWD:hip.LAB_FWD + 9] = fwd.reshape(-1)
    T[hip.LAB_INV:hip.LAB_INV + 9] = np.rint(4096.0 * np.linalg.inv(M) * white[None, :]).reshape(-1)
    u = np.arange(16385) / 16384.0
    T[hip.LAB_INVGAMMA:] = np.rint(255.0 * np.where(u <= 0.0031308, u * 12.92, 1.055 * u ** (1.0 / 2.4) - 0.055))
    _LAB.append(T.astype(np.int32))
    return _LAB[0]


def grid_distortion_map(n, num_steps, steps):
    """albumentations' grid_distortion map of one axis of n pixels: piecewise `np.linspace` over `num_steps` cells of n //
    num_steps pixels (and the rest), cell k stretched by steps[k]; float32 [n].  The cells are sampled WITHOUT their end point, so
    that factors of 1 give the identity map (albumentations includes the end point, which stretches a cell of c pixels by
    c / (c - 1) even at distort_limit 0)."""
    step = n // num_steps
    xx = np.zeros(n, dtype=np.float32)
    prev = 0.0
    for idx in range(num_steps + 1):
        start = idx * step
        end = start + step
        if end > n:
            end, cur = n, float(n)
        else:
            cur = prev + step * float(steps[idx])
        xx[start:end] = np.linspace(prev, cur, end - start, endpoint=False)
        prev = cur
    return xx


def gaussian_weights(sigma):
    """Taps -r..r of scipy.ndimage.gaussian_filter(sigma, truncate=4): r = int(4 sigma + 0.5), exp(-x^2 / 2 sigma^2) normalised in
    double, then float32."""
    r = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * x * x)
    return (w / w.sum()).astype(np.float32)


def elastic_noise(seed, H, W):
    """The two noise fields (dx, dy) of an elastic sample: U[-1, 1) float32 [2,H,W] from the sample's seed."""
    return np.random.default_rng(int(seed)).random((2, H, W), dtype=np.float32) * np.float32(2) - np.float32(1)


def pack_oneof(samples, size):
    """List of per-sample dicts (the `"oneof"` entry of each: None, or {"op": member, ...drawn values}) -> (ctypes array of
    hip.OneOfParam, float32 host tables or None, number of elastic samples).  Keys per member: rgb_shift "shift" (r, g, b); hsv
    "shift" (hue, sat, val); channel_shuffle "perm"; gaussian_blur "k"; clahe "clip"; grid_dropout "ratio"; grid_distortion
    "num_steps", "xsteps", "ysteps" (num_steps + 1 factors each); elastic "seed", "alpha", "sigma".  The tables hold, per
    grid_distortion sample, its maps xx[W], yy[H], and per elastic sample the Gaussian taps and the two noise fields."""
    H, W = int(size[0]), int(size[1])
    arr = (hip.OneOfParam * len(samples))()
    tabs, off, n_el = [], 0, 0

    def push(a):
        nonlocal off
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        tabs.append(a)
        off += a.size

    for q, s in zip(arr, samples):
        d = s.get("oneof")
        if d is None:
            continue
        name = d.get("op")
        if name not in ONEOF_MEMBERS:
            raise ValueError("DeviceAugment: unknown one_of member %r" % (name,))
        q.op = hip.ONEOF_OPS[name]
        if name in ("rgb_shift", "hsv"):
            sh = [float(v) for v in d["shift"]]
            if len(sh) != 3 or not all(abs(v) <= 255 for v in sh):
                raise ValueError("DeviceAugment: %s shift %r: three values within +-255" % (name, sh))
            q.v[:] = sh
        elif name == "channel_shuffle":
            perm = [int(v) for v in d["perm"]]
            if sorted(perm) != [0, 1, 2]:
                raise ValueError("DeviceAugment: channel_shuffle perm %r is not a permutation of 0..2" % (perm,))
            q.perm[:] = perm
        elif name == "gaussian_blur":
            if d["k"] not in (3, 5, 7):
                raise ValueError("DeviceAugment: gaussian_blur k = %r, must be 3, 5 or 7" % (d["k"],))
            q.k = int(d["k"])
        elif name == "clahe":
            if not 1 <= float(d["clip"]) <= 1e6:
                raise ValueError("DeviceAugment: clahe clip = %r, must be in [1, 1e6]" % (d["clip"],))
            q.v[0] = float(d["clip"])
        elif name == "grid_dropout":
            ratio = float(d.get("ratio", 0.5))
            unit = max(2, min(H, W) // 10)
            q.unit, q.hole = unit, min(max(int(unit * ratio), 1), unit - 1)
        elif name == "grid_distortion":
            n = int(d["num_steps"])
            if len(d["xsteps"]) != n + 1 or len(d["ysteps"]) != n + 1 or n < 1:
                raise ValueError("DeviceAugment: grid_distortion needs num_steps + 1 factors per axis")
            q.tab_off = off
            push(grid_distortion_map(W, n, d["xsteps"]))
            push(grid_distortion_map(H, n, d["ysteps"]))
        elif name == "elastic":
            sigma, alpha = float(d["sigma"]), float(d["alpha"])
            if not (sigma > 0 and int(4.0 * sigma + 0.5) <= hip.ONEOF_MAX_RADIUS and abs(alpha) <= 1e6):
                raise ValueError("DeviceAugment: elastic sigma = %r / alpha = %r" % (sigma, alpha))
            w = gaussian_weights(sigma)
            q.radius, q.slot, q.tab_off = (w.size - 1) // 2, n_el, off
            q.v[0], q.v[1] = alpha, sigma
            push(w)
            push(elastic_noise(d["seed"], H, W))
            n_el += 1
    return arr, (np.concatenate(tabs) if tabs else None), n_el


class DeviceAugment:
    """`x, y = DeviceAugment((256, 256))(images_u8, masks_u8, params=None, src_hw=None)`: the reference's training augmentations on
    the device (`dataset/data_loading.py:207-225`, then Normalize); the OneOf block with `one_of="reference"`.

    images_u8: uint8 [B,Hs,Ws,channels] on the GPU (channels=1: also [B,Hs,Ws]); masks_u8: uint8 [B,Hs,Ws] or None.  Returns fp32
    [B,channels,H,W] and int64 [B,H,W] labels (mask_mode as in `DevicePreprocess`), what `LM_Net.forward` and `SegLoss` take.
    src_hw (host int32 [B,2], optional): the valid size of each sample inside a padded [B,Hmax,Wmax,C] batch, so that frames of
    different sizes go through one launch; every crop window lies inside it.

    `sample(B, src_hw)` draws the parameters (params=None draws a new batch; `last_params` keeps the ones used):
      - RandomResizedCrop(size, scale, ratio): 10 tries of area U[scale] x frame area, log-uniform aspect ratio, then the
        centre-crop fallback;
      - ShiftScaleRotate(shift_limit, scale_limit, rotate_limit, BORDER_CONSTANT) with probability p_ssr: angle U[-rotate_limit,
        rotate_limit], scale U[1 - scale_limit, 1 + scale_limit], shifts U[-shift_limit, shift_limit] of W / H, matrix
        `ssr_matrix` (centre (W/2, H/2): the albumentations 1.3 convention; later releases moved it by half a pixel);
      - HorizontalFlip(p_hflip), VerticalFlip(p_vflip);
      - ColorJitter(*cj) with probability p_cj: factors U[max(0, 1 - x), 1 + x], hue U[-h, h], the op order shuffled.
      - one_of (None = no OneOf block: same draws, same two kernels as before; "reference" = the nine members of
        `data_loading.py:216-224` with equal weight; or a list of member names / (name, {settings}) pairs from ONEOF_MEMBERS) with
        probability p_oneof, after ColorJitter and before Normalize.  One member is drawn per sample; its values follow the sample's
        other draws: to_gray; grid_distortion (num_steps + 1 factors 1 + U[-distort_limit, distort_limit] per axis, reflect-101
        border, labels remapped by nearest pixel); elastic (a seed for the two noise fields, blurred with sigma, times alpha; at the
        defaults alpha = 1, sigma = 50 the displacement stays below 1/64 pixel and the 1/32-pixel remap returns its input); clahe
        (clip U[clip_limit], 8 x 8 tiles; on L of an integer 8-bit LAB for 3 channels); hsv (shifts U[-limit, limit]);
        channel_shuffle (a permutation); grid_dropout (unit = max(2, min(H, W) // 10), mask untouched); rgb_shift (shifts U[-limit,
        limit]); gaussian_blur (k from the odd sizes of blur_limit, cv2's fixed kernels).  to_gray, hsv, channel_shuffle and
        rgb_shift need channels == 3.  `last_oneof` keeps (OneOfParam array, host tables) of the last call.
    generator: None, an int seed, a numpy Generator or a torch.Generator: a seed gives the same parameters every time.  The
    stream is not albumentations' own (matching its RNG is not a goal)."""

    MASK_MODES = {"binary": 0, "labels": 1}

    def __init__(self, size=(256, 256), mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), channels=3, mask_mode="binary",
                 scale=(0.8, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), shift_limit=0.1, scale_limit=0.1, rotate_limit=30, p_ssr=0.5,
                 p_hflip=0.5, p_vflip=0.5, cj=(0.2, 0.2, 0.2, 0.2), p_cj=0.4, generator=None, one_of=None, p_oneof=0.4):
        if channels not in (1, 3):
            raise ValueError("DeviceAugment: channels = %r, must be 1 or 3" % (channels,))
        if mask_mode not in self.MASK_MODES:
            raise ValueError("DeviceAugment: mask_mode = %r, must be 'binary' or 'labels'" % (mask_mode,))
        if len(mean) != channels or len(std) != channels or min(std) <= 0:
            raise ValueError("DeviceAugment: mean and std need %d values each (std > 0) for channels=%d" % (channels, channels))
        if len(size) != 2 or min(size) <= 0 or max(size) >= 32768:
            raise ValueError("DeviceAugment: size %r" % (tuple(size),))
        if not (0 < scale[0] <= scale[1]) or not (0 < ratio[0] <= ratio[1]):
            raise ValueError("DeviceAugment: scale %r / ratio %r must be positive, increasing pairs" % (tuple(scale), tuple(ratio)))
        for name, v in (("p_ssr", p_ssr), ("p_hflip", p_hflip), ("p_vflip", p_vflip), ("p_cj", p_cj)):
            if not 0.0 <= v <= 1.0:
                raise ValueError("DeviceAugment: %s = %r outside [0, 1]" % (name, v))
        if not (0 <= shift_limit and 0 <= scale_limit < 1 and 0 <= rotate_limit):
            raise ValueError("DeviceAugment: shift_limit, scale_limit (< 1) and rotate_limit must be non-negative")
        if len(cj) != 4 or min(cj) < 0 or cj[3] > 0.5:
            raise ValueError("DeviceAugment: cj = %r: four non-negative limits, hue <= 0.5" % (tuple(cj),))
        self.size = (int(size[0]), int(size[1]))
        self.mean, self.std = tuple(mean), tuple(std)
        self.channels, self.mask_mode = int(channels), mask_mode
        self.scale, self.ratio = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        self.shift_limit, self.scale_limit, self.rotate_limit = float(shift_limit), float(scale_limit), float(rotate_limit)
        self.p_ssr, self.p_hflip, self.p_vflip, self.p_cj = float(p_ssr), float(p_hflip), float(p_vflip), float(p_cj)
        self.cj = tuple(float(v) for v in cj)
        if not 0.0 <= p_oneof <= 1.0:
            raise ValueError("DeviceAugment: p_oneof = %r outside [0, 1]" % (p_oneof,))
        self.one_of = None if one_of is None else parse_one_of(one_of, int(channels))
        self.p_oneof = float(p_oneof)
        if self.one_of is not None and any(n == "grid_distortion" and min(self.size) < c["num_steps"] for n, c in self.one_of):
            raise ValueError("DeviceAugment: grid_distortion num_steps above the output size %r" % (self.size,))
        if generator is None or isinstance(generator, (int, np.integer)):
            self._rng = np.random.default_rng(generator)
        elif isinstance(generator, np.random.Generator):
            self._rng = generator
        elif isinstance(generator, torch.Generator):
            self._rng = None
        else:
            raise ValueError("DeviceAugment: generator must be None, an int seed, a numpy Generator or a torch.Generator")
        self._torch_gen = generator if self._rng is None else None
        self.last_params = None        # the parameters of the last call (kept alive until its H2D copy has run)
        self.last_gray_sum = None      # int64 [B] device tensor: the contrast op's gray sums of the last call (0 where it did not run)
        self.last_oneof = None         # (OneOfParam array, host tables or None) of the last call with one_of set
        self._lab_dev = {}             # device -> the LAB tables, uploaded with the first call that needs them

    def _generator(self):
        if self._rng is not None:
            return self._rng
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=self._torch_gen))   # one numpy stream per batch, seeded from torch's
        return np.random.default_rng(seed)

    @staticmethod
    def _src_hw(B, src_hw):
        hw = np.asarray(src_hw.cpu() if isinstance(src_hw, torch.Tensor) else src_hw, dtype=np.int64)
        if hw.shape == (2,):
            hw = np.broadcast_to(hw, (B, 2))
        if hw.shape != (B, 2) or hw.min() < 1:
            raise ValueError("DeviceAugment: src_hw must be (h, w) or [B, 2] positive sizes, got shape %s" % (hw.shape,))
        return hw

    def _crop(self, rng, hs, ws):
        area = hs * ws
        lr = (math.log(self.ratio[0]), math.log(self.ratio[1]))
        for _ in range(10):
            target = rng.uniform(*self.scale) * area
            aspect = math.exp(rng.uniform(*lr))
            w = int(round(math.sqrt(target * aspect)))
            h = int(round(math.sqrt(target / aspect)))
            if 0 < w <= ws and 0 < h <= hs:
                return int(rng.integers(0, hs - h + 1)), int(rng.integers(0, ws - w + 1)), h, w
        in_ratio = ws / hs                      # RandomResizedCrop's centre-crop fallback
        if in_ratio < min(self.ratio):
            w, h = ws, int(round(ws / min(self.ratio)))
        elif in_ratio > max(self.ratio):
            h, w = hs, int(round(hs * max(self.ratio)))
        else:
            h, w = hs, ws
        return (hs - h) // 2, (ws - w) // 2, h, w

    def sample_dicts(self, B, src_hw):
        """B per-sample parameter dicts (the `pack_params` form) for frames of valid size src_hw ((h, w) or [B, 2])."""
        hw = self._src_hw(B, src_hw)
        rng = self._generator()
        H, W = self.size
        out = []
        for b in range(B):
            crop = self._crop(rng, int(hw[b, 0]), int(hw[b, 1]))
            ssr = rng.random() < self.p_ssr
            angle = rng.uniform(-self.rotate_limit, self.rotate_limit)
            scale = rng.uniform(1.0 - self.scale_limit, 1.0 + self.scale_limit)
            dx = rng.uniform(-self.shift_limit, self.shift_limit)
            dy = rng.uniform(-self.shift_limit, self.shift_limit)
            flips = int(rng.random() < self.p_hflip) | (int(rng.random() < self.p_vflip) << 1)
            cj = rng.random() < self.p_cj
            fac = [rng.uniform(max(0.0, 1.0 - v), 1.0 + v) for v in self.cj[:3]] + [rng.uniform(-self.cj[3], self.cj[3])]
            order = [int(v) for v in rng.permutation(4)]
            out.append({"crop": crop, "M": ssr_matrix(H, W, angle, scale, dx, dy) if ssr else None, "flips": flips,
                        "cj": fac if cj else None, "order": order,
                        "angle": angle, "scale": scale, "dx": dx, "dy": dy})
            if self.one_of is not None:
                out[-1]["oneof"] = self._draw_oneof(rng)
        return out

    def _draw_oneof(self, rng):
        """One sample's draw of the OneOf block: None (probability 1 - p_oneof) or {"op": member, ...its values}."""
        fire = rng.random() < self.p_oneof
        name, cfg = self.one_of[int(rng.integers(len(self.one_of)))]
        if not fire:
            return None
        d = {"op": name}
        if name == "rgb_shift":
            d["shift"] = [rng.uniform(-cfg[k], cfg[k]) for k in ("r", "g", "b")]
        elif name == "hsv":
            d["shift"] = [rng.uniform(-cfg[k], cfg[k]) for k in ("hue", "sat", "val")]
        elif name == "channel_shuffle":
            d["perm"] = [int(v) for v in rng.permutation(3)]
        elif name == "gaussian_blur":
            lo, hi = cfg["blur_limit"]
            d["k"] = int(lo) + 2 * int(rng.integers((int(hi) - int(lo)) // 2 + 1))
        elif name == "clahe":
            d["clip"] = rng.uniform(*cfg["clip_limit"])
        elif name == "grid_dropout":
            d["ratio"] = cfg["ratio"]
        elif name == "grid_distortion":
            n, lim = int(cfg["num_steps"]), cfg["distort_limit"]
            d["num_steps"] = n
            d["xsteps"] = [1.0 + rng.uniform(-lim, lim) for _ in range(n + 1)]
            d["ysteps"] = [1.0 + rng.uniform(-lim, lim) for _ in range(n + 1)]
        elif name == "elastic":
            d["seed"], d["alpha"], d["sigma"] = int(rng.integers(0, 2 ** 32)), cfg["alpha"], cfg["sigma"]
        return d

    def sample(self, B, src_hw):
        """A batch of parameters: ctypes array of B `hip.AugParam` (lmn_aug_param_t)."""
        return pack_params(self.sample_dicts(B, src_hw))

    @staticmethod
    def validate(params, src_hw):
        """Every crop window inside its sample's valid size (src_hw [B, 2]); raises ValueError."""
        if len(params) != len(src_hw):
            raise ValueError("DeviceAugment: %d parameter sets for a batch of %d" % (len(params), len(src_hw)))
        for b, p in enumerate(params):
            hs, ws = int(src_hw[b][0]), int(src_hw[b][1])
            if p.h <= 0 or p.w <= 0 or p.y0 < 0 or p.x0 < 0 or p.y0 + p.h > hs or p.x0 + p.w > ws:
                raise ValueError("DeviceAugment: crop window %d (y0 %d, x0 %d, %dx%d) outside its %dx%d source"
                                 % (b, p.y0, p.x0, p.h, p.w, hs, ws))

    def __call__(self, images, masks=None, params=None, src_hw=None, oneof=None):
        """params: None (draw), a list of sample dicts, or a packed AugParam array.  With one_of set, the OneOf draws come from the
        dicts' "oneof" entries; with a packed array give `oneof` = what `pack_oneof` returned (default: no member fires)."""
        ref = images if images is not None else masks
        if ref is None:
            raise ValueError("DeviceAugment: images or masks required")
        B, Hs, Ws = ref.shape[0], ref.shape[1], ref.shape[2]
        if images is not None:
            ok = (images.dim() == 4 and images.shape[3] == self.channels) or (self.channels == 1 and images.dim() == 3)
            if not ok or images.dtype != torch.uint8:
                raise ValueError("DeviceAugment(channels=%d): uint8 images of shape %s" % (self.channels, tuple(images.shape)))
        if masks is not None and (tuple(masks.shape) != (B, Hs, Ws) or masks.dtype != torch.uint8):
            raise ValueError("DeviceAugment: masks must be uint8 [B,Hs,Ws] = %s, got %s" % ((B, Hs, Ws), tuple(masks.shape)))
        hw = self._src_hw(B, src_hw if src_hw is not None else (Hs, Ws))
        if hw[:, 0].max() > Hs or hw[:, 1].max() > Ws:
            raise ValueError("DeviceAugment: src_hw exceeds the %dx%d frame" % (Hs, Ws))
        if self.one_of is None and oneof is not None:
            raise ValueError("DeviceAugment: oneof parameters given, but one_of is not set")
        if self.one_of is not None and not isinstance(params, ctypes.Array):
            dicts = self.sample_dicts(B, hw) if params is None else params
            params, oneof = pack_params(dicts), pack_oneof(dicts, self.size)
        elif params is None:
            params = self.sample(B, hw)
        elif not isinstance(params, ctypes.Array):
            params = pack_params(params)
        self.validate(params, hw)
        if self.one_of is not None:
            if oneof is None:
                oneof = pack_oneof([{}] * B, self.size)
            if len(oneof[0]) != B:
                raise ValueError("DeviceAugment: %d OneOf parameter sets for a batch of %d" % (len(oneof[0]), B))
            if self.channels != 3 and any(q.op in [hip.ONEOF_OPS[n] for n in ONEOF_COLOUR] for q in oneof[0]):
                raise ValueError("DeviceAugment: one_of members %s need channels == 3" % ", ".join(ONEOF_COLOUR))
        if not ref.is_cuda:
            raise RuntimeError("DeviceAugment runs on the HIP device only (got %s); there is no CPU path" % ref.device)
        self.last_params = params
        dev, (H, W), C = ref.device, self.size, self.channels
        x = torch.empty(B, C, H, W, device=dev, dtype=torch.float32) if images is not None else None
        y = torch.empty(B, H, W, device=dev, dtype=torch.int64) if masks is not None else None
        scratch = torch.empty(B, H, W, C, device=dev, dtype=torch.uint8) if images is not None else None
        gray = torch.empty(B, device=dev, dtype=torch.int64) if images is not None else None
        pdev = torch.empty(B * ctypes.sizeof(hip.AugParam), device=dev, dtype=torch.uint8)
        if self.one_of is not None:
            self._call_oneof(images, masks, params, hw if src_hw is not None else None, oneof, pdev, scratch, gray, x, y)
            self.last_gray_sum = gray
            return x, y
        hip.augment_u8(images.contiguous() if images is not None else None, masks.contiguous() if masks is not None else None, params,
                       hw.astype(np.int32) if src_hw is not None else None, pdev, scratch, gray, x, y, self.mean, self.std, C,
                       self.MASK_MODES[self.mask_mode])
        self.last_gray_sum = gray
        return x, y

    def _call_oneof(self, images, masks, params, hw, oneof, pdev, scratch, gray, x, y):
        """The call through lmn_augment_oneof_u8: the buffers of the plain call plus the second scratch, the label copy (when a
        geometric member fired), the device copies of the OneOf parameters and tables, and the workspace."""
        arr, tables, n_el = oneof
        self.last_oneof = (arr, tables)
        ref = images if images is not None else masks
        dev, (H, W), C, B = ref.device, self.size, self.channels, ref.shape[0]
        ops = [q.op for q in arr]
        geo = any(o in (hip.ONEOF_OPS["grid_distortion"], hip.ONEOF_OPS["elastic"]) for o in ops)
        lab = None
        if images is not None and C == 3 and hip.ONEOF_OPS["clahe"] in ops:
            lab = self._lab_dev.get(dev)
            if lab is None:
                lab = self._lab_dev[dev] = torch.empty(hip.LAB_TABLE_INTS, device=dev, dtype=torch.int32)
                lab.copy_(torch.from_numpy(lab_tables()))
        scratch2 = torch.empty(B, H, W, C, device=dev, dtype=torch.uint8) if images is not None else None
        ytmp = torch.empty(B, H, W, device=dev, dtype=torch.int64) if masks is not None and geo else None
        odev = torch.empty(B * ctypes.sizeof(hip.OneOfParam), device=dev, dtype=torch.uint8)
        tdev = torch.empty(tables.size, device=dev, dtype=torch.float32) if tables is not None else None
        ws = torch.empty(hip.oneof_workspace(B, H, W, C, n_el), device=dev, dtype=torch.uint8)
        hip.augment_oneof_u8(images.contiguous() if images is not None else None, masks.contiguous() if masks is not None else None,
                             params, hw.astype(np.int32) if hw is not None else None, pdev, scratch, gray, x, y, self.mean, self.std,
                             C, self.MASK_MODES[self.mask_mode], arr, odev, tables, tdev, lab, scratch2, ytmp, ws)


# ---------------------------------------------------------------- the input side of a 3D case (include/slices/lmnet_slices.h)
_SLICES_KINDS = {"window": hip.SLICES_WINDOW, "zscore": hip.SLICES_ZSCORE, "percentile": hip.SLICES_PERCENTILE}
_SLICES_EDGES = {"replicate": hip.SLICES_EDGE_REPLICATE, "zero": hip.SLICES_EDGE_ZERO}
_SLICES_BORDERS = {"replicate": hip.SLICES_BORDER_REPLICATE, "constant": hip.SLICES_BORDER_CONSTANT}


def _norm_spec(spec):
    """one norm spec -> (kind, level, width); raises ValueError"""
    if isinstance(spec, str):
        spec = (spec,)
    if not isinstance(spec, tuple) or not spec or spec[0] not in _SLICES_KINDS:
        raise ValueError("VolumeSlicer: norm spec %r is none of 'zscore', ('percentile',), ('window', level, width)" % (spec,))
    if spec[0] == "window":
        if len(spec) != 3 or not all(math.isfinite(float(v)) for v in spec[1:]) or abs(float(spec[1])) > 1e9 or not 0 < float(spec[2]) <= 1e9:
            raise ValueError("VolumeSlicer: norm spec %r: ('window', level, width) with |level| <= 1e9 and 0 < width <= 1e9" % (spec,))
        return hip.SLICES_WINDOW, float(spec[1]), float(spec[2])
    if len(spec) != 1:
        raise ValueError("VolumeSlicer: norm spec %r takes no values" % (spec,))
    return _SLICES_KINDS[spec[0]], 0.0, 1.0


def _per_modality(what, v, M):
    v = list(v) if isinstance(v, (list, tuple)) else [v] * M
    if len(v) != M:
        raise ValueError("VolumeSlicer: %s needs one value or %d, one per modality" % (what, M))
    return v


def resize_map(dst_hw, src_hw):
    """The inverse map of a plain resize as a 3x3 matrix in double: output pixel index -> source pixel index, s = (x + 0.5) * src /
    dst - 0.5 per axis (align_corners=False)."""
    (h, w), (Hs, Ws) = dst_hw, src_hw
    ax, ay = Ws / float(w), Hs / float(h)
    return np.array([[ax, 0.0, 0.5 * ax - 0.5], [0.0, ay, 0.5 * ay - 0.5], [0.0, 0.0, 1.0]], dtype=np.float64)


def slice_param_row(dst_hw, src_hw, M=None, flips=0, gain=1.0, bias=0.0):
    """The fp32 row of 8 of one sample of lmn_slices_gather: the inverse map from output pixel index to source pixel index composed in
    double -- undo the flips, then `invert_affine(M)` (M: a forward 2x3 matrix on the output grid, the convention of `ssr_matrix`;
    None: no warp), then the plain resize -- followed by gain and bias."""
    h, w = dst_hw
    T = np.eye(3)
    if flips & 1:
        T = np.array([[-1.0, 0.0, w - 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) @ T
    if flips & 2:
        T = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, h - 1.0], [0.0, 0.0, 1.0]]) @ T
    if M is not None:
        iM = invert_affine([float(v) for v in np.asarray(M, dtype=np.float64).reshape(-1)])
        T = np.array([iM[:3], iM[3:], [0.0, 0.0, 1.0]]) @ T
    T = resize_map(dst_hw, src_hw) @ T
    return np.array([T[0, 0], T[0, 1], T[0, 2], T[1, 0], T[1, 1], T[1, 2], gain, bias], dtype=np.float64).astype(np.float32)


class VolumeSlicer:
    """The first stage of a CT / MR case: an int16 (or uint8) volume already in HBM -> the fp32 2.5D batches `LM_Net.forward` and
    `TiledPredictor` read, with windowing, z-scoring, percentile clipping, slice stacking and resizing on the device
    (`lmn_slices_stats`, `lmn_slices_gather`; include/slices/lmnet_slices.h).  2 bytes per voxel cross PCIe, once.

      open_case(volume, labels=None)   volume int16 / uint8 [D, Hs, Ws] or [M, D, Hs, Ws], labels uint8 [D, Hs, Ws]; launches the
                                       statistics and returns without synchronising.  `stats` (device int64 [M, 8]: n, sum v,
                                       sum v^2, min, max, v_lo, v_hi, 0 of the foreground) and `table` (device fp32 [S, 4]: lo, hi,
                                       a, b per norm spec) belong to the open case.
      slices(z0, z1)                   (x fp32 [n, C, h, w], y [n, h, w] or None) of the consecutive slices z0 .. z1 - 1: validation.
      batch(z, params=None)            the same for any list (or device int32 tensor) of slice indices, repeats allowed, under the
                                       per-sample parameters `sample(n, rng)` draws: training.
      restore(labels_net)              uint8 [n, h, w] -> [n, Hs, Ws] by the same gather in label-only mode, for
                                       `VolumePostprocess.push` / `VolumeSurfaceMeter.push` at native resolution.

    norm: "zscore", ("window", level, width), ("percentile",), or a list with one entry per modality, each a spec or a list of specs.
    o = (min(max(v, lo), hi) - a) * b with (lo, hi, a, b) = window: (level - width / 2, level + width / 2, lo, 1 / width); zscore:
    (v_lo, v_hi, mean, 1 / max(std, 1e-8)), mean and population std of the unclipped foreground; percentile: (v_lo, v_hi, v_lo,
    1 / (v_hi - v_lo)).  v_lo / v_hi are the `clip` = (q_lo, q_hi) percent order statistics of the foreground (rank q (n - 1) rounded
    down; None: min and max); foreground: None = every voxel, or v > foreground (one value or one per modality).
    C = sum over modalities of (its specs) x (2 context + 1), in the order modality, spec, dz = -context .. context; channel dz of
    slice z reads slice z + dz * stride, clamped to the volume under edge="replicate", a plane of 0 (before gain and bias) under
    edge="zero".  The image is resized bilinearly (align_corners=False), the label by the nearest pixel under the half-pixel rule
    (torch's nearest-exact), both under one matrix; border="replicate" clamps taps to the frame, "constant" gives border_value (raw
    units, one or one per modality) and label_border outside it.

    sample(n, rng) draws per sample a ShiftScaleRotate matrix (`ssr_matrix` on the output grid, probability p_ssr), the two flips and
    an intensity gain 1 + U[-gain_limit, gain_limit] and bias U[-bias_limit, bias_limit]; rng: None, an int seed or a numpy
    Generator.  Nothing synchronises.  The returned tensors are the slicer's own, kept per geometry: a later call of the same
    geometry overwrites them, and after the first call of a geometry nothing is allocated on the device.  Outputs and staging are per
    geometry, not per stream: use from two streams at once needs one VolumeSlicer object per stream."""

    _SLOTS = 8

    def __init__(self, size=(352, 352), norm="zscore", modalities=1, context=1, stride=1, edge="replicate", foreground=None, clip=None,
                 border="replicate", border_value=0, label_border=0, label_dtype=torch.uint8, shift_limit=0.1, scale_limit=0.1,
                 rotate_limit=30, p_ssr=0.5, p_hflip=0.5, p_vflip=0.5, gain_limit=0.1, bias_limit=0.1):
        M = int(modalities)
        if not 1 <= M <= hip.SLICES_MAX_MODALITIES:
            raise ValueError("VolumeSlicer: modalities = %r outside the limit [1, %d]" % (modalities, hip.SLICES_MAX_MODALITIES))
        if len(size) != 2 or not all(1 <= int(v) <= hip.SLICES_MAX_OUT for v in size):
            raise ValueError("VolumeSlicer: size %r outside the limit [1, %d]" % (tuple(size), hip.SLICES_MAX_OUT))
        if not 0 <= int(context) <= hip.SLICES_MAX_CONTEXT or not 1 <= int(stride) <= hip.SLICES_MAX_DEPTH:
            raise ValueError("VolumeSlicer: context = %r outside [0, %d] or stride = %r outside [1, %d]"
                             % (context, hip.SLICES_MAX_CONTEXT, stride, hip.SLICES_MAX_DEPTH))
        if edge not in _SLICES_EDGES or border not in _SLICES_BORDERS:
            raise ValueError("VolumeSlicer: edge = %r must be 'replicate' or 'zero', border = %r 'replicate' or 'constant'" % (edge, border))
        if label_dtype not in (torch.uint8, torch.int64):
            raise ValueError("VolumeSlicer: label_dtype %r is neither torch.uint8 nor torch.int64" % (label_dtype,))
        if not 0 <= int(label_border) <= 255:
            raise ValueError("VolumeSlicer: label_border = %r outside [0, 255]" % (label_border,))
        per_mod = norm if isinstance(norm, list) else [norm] * M
        if len(per_mod) != M:
            raise ValueError("VolumeSlicer: norm lists %d modalities, modalities = %d" % (len(per_mod), M))
        self.specs = []                                       # (modality, kind, level, width), modality-major
        for m, entry in enumerate(per_mod):
            for spec in (entry if isinstance(entry, list) else [entry]):
                self.specs.append((m,) + _norm_spec(spec))
        self.context, self.stride = int(context), int(stride)
        self.channels = len(self.specs) * (2 * self.context + 1)
        if not 1 <= self.channels <= hip.SLICES_MAX_CHANNELS:
            raise ValueError("VolumeSlicer: %d norm specs x %d slices = %d channels, outside the limit [1, %d]"
                             % (len(self.specs), 2 * self.context + 1, self.channels, hip.SLICES_MAX_CHANNELS))
        fg = _per_modality("foreground", foreground, M)
        self.foreground = [hip.SLICES_NO_FOREGROUND if v is None else int(v) for v in fg]
        if not all(hip.SLICES_NO_FOREGROUND <= v <= 32767 for v in self.foreground):
            raise ValueError("VolumeSlicer: foreground %r outside int16" % (foreground,))
        if clip is None:
            self.q_ppm = (0, 1000000)
        else:
            if len(clip) != 2 or not 0.0 <= float(clip[0]) <= float(clip[1]) <= 100.0:
                raise ValueError("VolumeSlicer: clip = %r: two percentages, 0 <= q_lo <= q_hi <= 100" % (clip,))
            self.q_ppm = (int(round(float(clip[0]) * 1e4)), int(round(float(clip[1]) * 1e4)))
        self.border_value = [float(v) for v in _per_modality("border_value", border_value, M)]
        if not all(abs(v) <= 65536.0 for v in self.border_value):
            raise ValueError("VolumeSlicer: border_value %r outside [-65536, 65536]" % (border_value,))
        for name, v in (("p_ssr", p_ssr), ("p_hflip", p_hflip), ("p_vflip", p_vflip)):
            if not 0.0 <= v <= 1.0:
                raise ValueError("VolumeSlicer: %s = %r outside [0, 1]" % (name, v))
        if not (0 <= shift_limit and 0 <= scale_limit < 1 and 0 <= rotate_limit and 0 <= gain_limit < 1 and 0 <= bias_limit):
            raise ValueError("VolumeSlicer: shift_limit, scale_limit (< 1), rotate_limit, gain_limit (< 1) and bias_limit must be non-negative")
        self.size, self.modalities = (int(size[0]), int(size[1])), M
        self.edge, self.border, self.label_border, self.label_dtype = edge, border, int(label_border), label_dtype
        self.shift_limit, self.scale_limit, self.rotate_limit = float(shift_limit), float(scale_limit), float(rotate_limit)
        self.p_ssr, self.p_hflip, self.p_vflip = float(p_ssr), float(p_hflip), float(p_vflip)
        self.gain_limit, self.bias_limit = float(gain_limit), float(bias_limit)
        self.volume = self.labels = self.stats = self.table = None
        self._scratch = {}             # geometry -> device tensors, made once (a plain dict, as the criteria keep theirs)
        self._stage = {}               # rows -> (pinned staging slots, their events, next slot)

    # ------------------------------------------------------------------ parameters
    def sample(self, n, rng=None):
        """n per-sample dicts: "M" (forward 2x3 matrix on the output grid, `ssr_matrix`, or None), "flips" (bit 0 horizontal, bit 1
        vertical), "gain", "bias"."""
        rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        h, w = self.size
        out = []
        for _ in range(int(n)):
            ssr = rng.random() < self.p_ssr
            angle = rng.uniform(-self.rotate_limit, self.rotate_limit)
            scale = rng.uniform(1.0 - self.scale_limit, 1.0 + self.scale_limit)
            dx = rng.uniform(-self.shift_limit, self.shift_limit)
            dy = rng.uniform(-self.shift_limit, self.shift_limit)
            flips = int(rng.random() < self.p_hflip) | (int(rng.random() < self.p_vflip) << 1)
            out.append({"M": ssr_matrix(h, w, angle, scale, dx, dy) if ssr else None, "flips": flips,
                        "gain": 1.0 + rng.uniform(-self.gain_limit, self.gain_limit), "bias": rng.uniform(-self.bias_limit, self.bias_limit)})
        return out

    def rows(self, n, params=None, dst_hw=None, src_hw=None):
        """float32 [n, 8]: the parameter rows of n samples (params None: the plain resize, gain 1, bias 0)."""
        dst_hw = self.size if dst_hw is None else dst_hw
        src_hw = self._src_hw() if src_hw is None else src_hw
        if params is None:
            return np.tile(slice_param_row(dst_hw, src_hw), (n, 1))
        if len(params) != n:
            raise ValueError("VolumeSlicer: %d parameter sets for %d slices" % (len(params), n))
        rows = np.empty((n, 8), dtype=np.float32)
        for i, p in enumerate(params):
            fl = int(p.get("flips", 0))
            M = p.get("M")
            vals = [float(p.get("gain", 1.0)), float(p.get("bias", 0.0))] + ([] if M is None else [float(v) for v in np.asarray(M).reshape(-1)])
            if fl not in (0, 1, 2, 3) or not all(math.isfinite(v) for v in vals) or (M is not None and len(vals) != 8):
                raise ValueError("VolumeSlicer: sample %d: flips 0..3, a finite gain and bias, M six finite values or None" % i)
            rows[i] = slice_param_row(dst_hw, src_hw, M, fl, vals[0], vals[1])
        return rows

    # ------------------------------------------------------------------ the case
    def _src_hw(self):
        if self.volume is None:
            raise ValueError("VolumeSlicer: no case is open")
        return int(self.volume.shape[2]), int(self.volume.shape[3])

    def _cached(self, key, make):
        if key not in self._scratch:
            self._scratch[key] = make()
        return self._scratch[key]

    def open_case(self, volume, labels=None):
        M = self.modalities
        if volume.dim() == 3:
            volume = volume.unsqueeze(0)
        if volume.dim() != 4 or volume.dtype not in (torch.int16, torch.uint8):
            raise ValueError("VolumeSlicer.open_case: an int16 or uint8 volume [D, Hs, Ws] or [M, D, Hs, Ws] required, got %s %s"
                             % (volume.dtype, tuple(volume.shape)))
        Mv, D, Hs, Ws = (int(d) for d in volume.shape)
        if Mv != M:
            raise ValueError("VolumeSlicer.open_case: %d modalities in the volume, modalities = %d (limit [1, %d])" % (Mv, M, hip.SLICES_MAX_MODALITIES))
        if not 1 <= D <= hip.SLICES_MAX_DEPTH:
            raise ValueError("VolumeSlicer.open_case: D = %d outside the limit [1, %d]" % (D, hip.SLICES_MAX_DEPTH))
        if not (2 <= Hs <= hip.SLICES_MAX_SIDE and 2 <= Ws <= hip.SLICES_MAX_SIDE):
            raise ValueError("VolumeSlicer.open_case: slices of %d x %d outside the limit [2, %d]" % (Hs, Ws, hip.SLICES_MAX_SIDE))
        if labels is not None and (labels.dtype != torch.uint8 or tuple(labels.shape) != (D, Hs, Ws)):
            raise ValueError("VolumeSlicer.open_case: labels must be uint8 [D, Hs, Ws] = %s, got %s %s" % ((D, Hs, Ws), labels.dtype, tuple(labels.shape)))
        if not volume.is_cuda or (labels is not None and not labels.is_cuda):
            raise RuntimeError("VolumeSlicer runs on the HIP device only (got %s); there is no CPU path" % volume.device)
        dev, S = volume.device, len(self.specs)
        ws, stats, table = self._cached(("case", dev, M), lambda: (
            torch.empty(hip.slices_workspace(M, D, Hs, Ws), device=dev, dtype=torch.uint8),
            torch.empty(M, hip.SLICES_NSTAT, device=dev, dtype=torch.int64), torch.empty(S, 4, device=dev, dtype=torch.float32)))
        self.volume = volume.contiguous()
        self.labels = None if labels is None else labels.contiguous()
        hip.slices_stats(self.volume, self.foreground, self.q_ppm[0], self.q_ppm[1], self.specs, ws, stats, table)
        self.stats, self.table = stats, table

    def _upload(self, dev, z, rows):
        """(z device int32 [n], params device fp32 [n, 8]): 9 n words through a pinned staging slot and one non-blocking copy.  z None:
        the caller has its indices on the device already."""
        n = rows.shape[0]
        key = (dev, n)
        if key not in self._stage:
            self._stage[key] = [[torch.zeros(9 * n, dtype=torch.float32).pin_memory() for _ in range(self._SLOTS)], [None] * self._SLOTS, 0]
        slots, events, s = self._stage[key]
        self._stage[key][2] = (s + 1) % self._SLOTS
        if events[s] is not None and not events[s].query():
            events[s].synchronize()                             # (the copy that read this slot _SLOTS calls ago: finished long since)
        host = slots[s]
        host[:8 * n] = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32).reshape(-1))
        if z is not None:
            host[8 * n:].view(torch.int32)[:] = torch.from_numpy(np.ascontiguousarray(z, dtype=np.int32))
        dbuf = self._cached(("rows", dev, n), lambda: torch.empty(9 * n, device=dev, dtype=torch.float32))
        dbuf.copy_(host, non_blocking=True)
        if events[s] is None:
            events[s] = torch.cuda.Event()
        events[s].record()
        return dbuf[8 * n:].view(torch.int32), dbuf[:8 * n].view(n, 8)

    def _gather(self, z, rows):
        if self.volume is None:
            raise ValueError("VolumeSlicer: no case is open")
        dev, (h, w), n = self.volume.device, self.size, rows.shape[0]
        if not 1 <= n <= hip.SLICES_MAX_BATCH:
            raise ValueError("VolumeSlicer: %d slices outside the limit [1, %d]" % (n, hip.SLICES_MAX_BATCH))
        has_y = self.labels is not None
        x, y = self._cached(("out", dev, n, h, w, has_y), lambda: (
            torch.empty(n, self.channels, h, w, device=dev, dtype=torch.float32),
            torch.empty(n, h, w, device=dev, dtype=self.label_dtype) if has_y else None))
        zdev, pdev = self._upload(dev, None if isinstance(z, torch.Tensor) else z, rows)
        if isinstance(z, torch.Tensor):
            zdev = z
        hip.slices_gather(self.volume, self.labels, zdev, pdev, self.table, [s[0] for s in self.specs], self.context, self.stride,
                          _SLICES_EDGES[self.edge], _SLICES_BORDERS[self.border], self.border_value, self.label_border, x, y)
        return x, y

    def slices(self, z0, z1):
        D = 0 if self.volume is None else int(self.volume.shape[1])
        if self.volume is not None and not 0 <= int(z0) < int(z1) <= D:
            raise ValueError("VolumeSlicer.slices: [%r, %r) is not a range of slices inside [0, %d)" % (z0, z1, D))
        z = np.arange(int(z0), int(z1), dtype=np.int32)
        return self._gather(z, self.rows(z.size))

    def batch(self, z, params=None):
        if self.volume is None:
            raise ValueError("VolumeSlicer: no case is open")
        D = int(self.volume.shape[1])
        if isinstance(z, torch.Tensor):
            if z.dtype != torch.int32 or z.dim() != 1 or not z.is_cuda or not z.is_contiguous():
                raise ValueError("VolumeSlicer.batch: z as a tensor must be a contiguous device int32 [n] (indices outside the volume are clamped)")
            n = int(z.numel())
        else:
            z = np.asarray(z, dtype=np.int64).reshape(-1)
            if z.size and (z.min() < 0 or z.max() >= D):
                raise ValueError("VolumeSlicer.batch: slice indices outside [0, %d)" % D)
            z, n = z.astype(np.int32), int(z.size)
        return self._gather(z, self.rows(n, params))

    def restore(self, labels_net):
        if self.volume is None:
            raise ValueError("VolumeSlicer: no case is open")
        if labels_net.dim() != 3 or labels_net.dtype != torch.uint8 or not labels_net.is_cuda:
            raise ValueError("VolumeSlicer.restore: uint8 device labels [n, h, w] required, got %s %s" % (labels_net.dtype, tuple(labels_net.shape)))
        n, h, w = (int(d) for d in labels_net.shape)
        if not 1 <= n <= hip.SLICES_MAX_DEPTH or not (2 <= h <= hip.SLICES_MAX_SIDE and 2 <= w <= hip.SLICES_MAX_SIDE):
            raise ValueError("VolumeSlicer.restore: labels %s outside the limits n in [1, %d], h, w in [2, %d]"
                             % (tuple(labels_net.shape), hip.SLICES_MAX_DEPTH, hip.SLICES_MAX_SIDE))
        dev, (Hs, Ws) = labels_net.device, self._src_hw()
        y = self._cached(("restore", dev, n, h, w, Hs, Ws), lambda: torch.empty(n, Hs, Ws, device=dev, dtype=torch.uint8))
        zdev, pdev = self._upload(dev, np.arange(n, dtype=np.int32), self.rows(n, None, (Hs, Ws), (h, w)))
        hip.slices_gather(None, labels_net.contiguous(), zdev, pdev, None, None, 0, 1, hip.SLICES_EDGE_REPLICATE,
                          hip.SLICES_BORDER_REPLICATE, None, 0, None, y)
        return y


class DeviceMix:
    """Mixup (Zhang et al. 2018) and CutMix (Yun et al. 2019) of a batch that is already on the device -- the output of
    ``DeviceAugment`` / ``DevicePreprocess`` -- in one pass (``lmn_mix_batch``, include/soft/lmnet_soft.h).

    ``mix(x, y, rows=None) -> (x_mixed, MixedTarget(ya, yb, lam))`` for fp32 ``x`` ``[B, Cin, H, W]`` and a uint8 / int64 label map ``y``
    ``[B, H, W]``, out of place.  A Mixup sample is ``lam * x[b] + (1 - lam) * x[partner]`` -- evaluated unfused in fp32, so numpy
    restates it bit for bit -- with ``ya = y[b]``, ``yb = y[partner]``: the two-hot target ``SoftSegLoss`` takes.  A CutMix sample takes
    pixels AND labels inside its box from the partner, so ``ya == yb``, ``lam == 1``, void labels travel with their pixels, and with
    ``mixup_alpha == 0`` the result is a hard label map every criterion of the package takes (``target.labels``).

    ``sample(B, H, W)`` draws the rows on the host -- ``(partner, mode, lam, boxes)`` -- by the rule timm documents for its ``Mixup``
    (timm is not a dependency: parity with its code is not pinned): a sample is mixed with probability ``prob``; CutMix is chosen with
    ``switch_prob`` when both alphas are positive, else whichever alpha is positive; ``lam ~ Beta(alpha, alpha)``; the CutMix box has
    side ratio ``sqrt(1 - lam)`` and a uniform centre, is clipped to the image, and ``lam`` becomes the kept area fraction;
    ``partner = B - 1 - b`` (``"flip"``) or a permutation (``"perm"``); ``per_sample=False`` makes one draw for the batch.
    generator: None, an int seed, a numpy Generator or a torch.Generator, as in ``DeviceAugment``.  Device tensors only; nothing
    synchronises; the row buffer of a geometry is kept and the outputs come from torch's caching allocator."""

    MODES = {"none": hip.MIX_NONE, "mixup": hip.MIX_MIXUP, "cutmix": hip.MIX_CUTMIX}

    def __init__(self, mixup_alpha=0.0, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, per_sample=True, partner="flip", generator=None):
        if not (0.0 <= mixup_alpha < float("inf") and 0.0 <= cutmix_alpha < float("inf")):
            raise ValueError("DeviceMix: mixup_alpha = %r, cutmix_alpha = %r must be finite and >= 0" % (mixup_alpha, cutmix_alpha))
        if not 0.0 <= prob <= 1.0 or not 0.0 <= switch_prob <= 1.0:
            raise ValueError("DeviceMix: prob = %r, switch_prob = %r outside [0, 1]" % (prob, switch_prob))
        if partner not in ("flip", "perm"):
            raise ValueError("DeviceMix: partner = %r, expected 'flip' or 'perm'" % (partner,))
        self.mixup_alpha, self.cutmix_alpha, self.prob, self.switch_prob = float(mixup_alpha), float(cutmix_alpha), float(prob), float(switch_prob)
        self.per_sample, self.partner = bool(per_sample), partner
        if generator is None or isinstance(generator, (int, np.integer)):
            self._rng = np.random.default_rng(generator)
        elif isinstance(generator, np.random.Generator):
            self._rng = generator
        elif isinstance(generator, torch.Generator):
            self._rng = None
        else:
            raise ValueError("DeviceMix: generator must be None, an int seed, a numpy Generator or a torch.Generator")
        self._torch_gen = generator if self._rng is None else None
        self.last_rows = None          # the host table of the last call (kept alive until its H2D copy has run)
        self._scratch = {}

    def _generator(self):
        if self._rng is not None:
            return self._rng
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=self._torch_gen))   # one numpy stream per batch, seeded from torch's
        return np.random.default_rng(seed)

    def _draw(self, rng, H, W):
        """(mode, lam, box) of one draw"""
        if not rng.random() < self.prob or (self.mixup_alpha <= 0.0 and self.cutmix_alpha <= 0.0):
            return hip.MIX_NONE, np.float32(1.0), (0, 0, 0, 0)
        cut = self.cutmix_alpha > 0.0 and (self.mixup_alpha <= 0.0 or rng.random() < self.switch_prob)
        alpha = self.cutmix_alpha if cut else self.mixup_alpha
        lam = np.float32(min(max(rng.beta(alpha, alpha), 0.0), 1.0))
        if not cut:
            return hip.MIX_MIXUP, lam, (0, 0, 0, 0)
        ratio = math.sqrt(1.0 - float(lam))
        ch, cw = int(H * ratio), int(W * ratio)
        cy, cx = int(rng.integers(H)), int(rng.integers(W))
        y0, y1 = min(max(cy - ch // 2, 0), H), min(max(cy + ch // 2, 0), H)
        x0, x1 = min(max(cx - cw // 2, 0), W), min(max(cx + cw // 2, 0), W)
        return hip.MIX_CUTMIX, np.float32(1.0 - (y1 - y0) * (x1 - x0) / float(H * W)), (y0, x0, y1, x1)

    def sample(self, B, H, W):
        """The host table of one batch, int32 ``[B, 8]`` (``hip.mix_rows``): partner, mode, lam, 1 - lam, y0, x0, y1, x1."""
        rng = self._generator()
        partner = np.arange(B - 1, -1, -1) if self.partner == "flip" else rng.permutation(B)
        draws = [self._draw(rng, H, W) for _ in range(B)] if self.per_sample else [self._draw(rng, H, W)] * B
        return hip.mix_rows(partner, [d[0] for d in draws], [d[1] for d in draws], [d[2] for d in draws])

    def mix(self, x, y, rows=None):
        from .loss import MixedTarget
        if not torch.is_tensor(x) or x.dim() != 4 or x.dtype != torch.float32:
            raise ValueError("DeviceMix: x must be an fp32 tensor [B, Cin, H, W], got %s %s" % (getattr(x, "dtype", None), tuple(getattr(x, "shape", ()))))
        B, Cin, H, W = x.shape
        if not torch.is_tensor(y) or tuple(y.shape) != (B, H, W) or y.dtype not in (torch.uint8, torch.int64):
            raise ValueError("DeviceMix: y must be a uint8 or int64 label map %s, got %s %s" % ((B, H, W), getattr(y, "dtype", None), tuple(getattr(y, "shape", ()))))
        if B > hip.SOFT_MAX_BATCH or not 1 <= Cin <= 64 or min(B, H, W) < 1 or B * Cin * H * W >= 1 << 31:
            raise ValueError("DeviceMix: B = %d, Cin = %d, B * Cin * H * W = %d outside the limits B <= %d, Cin <= 64, B * Cin * H * W in [1, 2^31)"
                             % (B, Cin, B * Cin * H * W, hip.SOFT_MAX_BATCH))
        if not x.is_cuda or not y.is_cuda:
            raise RuntimeError("lm_net_amd.DeviceMix: device tensors required (the HIP path has no CPU fallback)")
        rows = self.sample(B, H, W) if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        if tuple(rows.shape) != (B, hip.MIX_ROW_WORDS):
            raise ValueError("DeviceMix: rows %s, expected %s" % (tuple(rows.shape), (B, hip.MIX_ROW_WORDS)))
        key = (x.device, B)
        if key not in self._scratch:
            self._scratch[key] = torch.empty((B, hip.MIX_ROW_WORDS), device=x.device, dtype=torch.int32)
        soft = self.mixup_alpha > 0.0 or bool((rows[:, 1] == hip.MIX_MIXUP).any())
        x, y = x.contiguous(), y.contiguous()
        x_out, ya, lam = torch.empty_like(x), torch.empty_like(y), torch.empty(B, device=x.device)
        yb = torch.empty_like(y) if soft else None
        self.last_rows = rows
        hip.mix_batch(x, y, rows, self._scratch[key], x_out, ya, yb, lam)
        target = MixedTarget(ya, ya if yb is None else yb, lam)
        target.hard = not soft
        return x_out, target

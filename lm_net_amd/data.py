"""Device-side input pipeline.

The reference prepares every sample on the CPU with albumentations (`dataset/data_loading.py:203-229`):
`cv2.imread` (uint8 HWC, channel order as read), mask `cv2.threshold(127, 1)`, then `A.Resize(256, 256)`,
`A.Normalize()` and `ToTensorV2()` for validation; the training transform adds flips and colour / geometric
augmentations in front of the same Normalize.  `DevicePreprocess` runs the resize + (optional) flips + normalise +
layout change for a whole batch of raw uint8 frames already in HBM as ONE kernel (`lmn_preprocess_u8`), so decoded
frames can go to the GPU as bytes (3 B/pixel over PCIe instead of 12) and an 8-GPU loop is not fed by a CPU
albumentations pool.  `DeviceAugment` runs the per-sample part of the training transform (`:207-214`, `:227-228`):
RandomResizedCrop -> ShiftScaleRotate -> HorizontalFlip -> VerticalFlip -> ColorJitter -> Normalize, as two kernels
(`lmn_augment_u8`) on parameters drawn on the host.  Only the `A.OneOf([...9 ops], p=0.4)` block (`:215-225`) stays on the
CPU side (out of scope).
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


class DeviceAugment:
    """`x, y = DeviceAugment((256, 256))(images_u8, masks_u8, params=None, src_hw=None)`: the reference's training augmentations on
    the device (`dataset/data_loading.py:207-214`, then Normalize), OneOf block excluded.

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
    generator: None, an int seed, a numpy Generator or a torch.Generator: a seed gives the same parameters every time.  The
    stream is not albumentations' own (matching its RNG is not a goal)."""

    MASK_MODES = {"binary": 0, "labels": 1}

    def __init__(self, size=(256, 256), mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), channels=3, mask_mode="binary",
                 scale=(0.8, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), shift_limit=0.1, scale_limit=0.1, rotate_limit=30, p_ssr=0.5,
                 p_hflip=0.5, p_vflip=0.5, cj=(0.2, 0.2, 0.2, 0.2), p_cj=0.4, generator=None):
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
        return out

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

    def __call__(self, images, masks=None, params=None, src_hw=None):
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
        if params is None:
            params = self.sample(B, hw)
        elif not isinstance(params, ctypes.Array):
            params = pack_params(params)
        self.validate(params, hw)
        if not ref.is_cuda:
            raise RuntimeError("DeviceAugment runs on the HIP device only (got %s); there is no CPU path" % ref.device)
        self.last_params = params
        dev, (H, W), C = ref.device, self.size, self.channels
        x = torch.empty(B, C, H, W, device=dev, dtype=torch.float32) if images is not None else None
        y = torch.empty(B, H, W, device=dev, dtype=torch.int64) if masks is not None else None
        scratch = torch.empty(B, H, W, C, device=dev, dtype=torch.uint8) if images is not None else None
        gray = torch.empty(B, device=dev, dtype=torch.int64) if images is not None else None
        pdev = torch.empty(B * ctypes.sizeof(hip.AugParam), device=dev, dtype=torch.uint8)
        hip.augment_u8(images.contiguous() if images is not None else None, masks.contiguous() if masks is not None else None, params,
                       hw.astype(np.int32) if src_hw is not None else None, pdev, scratch, gray, x, y, self.mean, self.std, C,
                       self.MASK_MODES[self.mask_mode])
        self.last_gray_sum = gray
        return x, y

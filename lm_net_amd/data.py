"""Device-side input pipeline.

The reference prepares every sample on the CPU with albumentations (`dataset/data_loading.py:203-229`):
`cv2.imread` (uint8 HWC, channel order as read), mask `cv2.threshold(127, 1)`, then `A.Resize(256, 256)`,
`A.Normalize()` and `ToTensorV2()` for validation; the training transform adds flips and colour / geometric
augmentations in front of the same Normalize.  `DevicePreprocess` runs the resize + (optional) flips + normalise +
layout change for a whole batch of raw uint8 frames already in HBM as ONE kernel (`lmn_preprocess_u8`), so decoded
frames can go to the GPU as bytes (3 B/pixel over PCIe instead of 12) and an 8-GPU loop is not fed by a CPU
albumentations pool.  The colour / elastic augmentations of the training transform stay on the CPU side (out of scope).
"""
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

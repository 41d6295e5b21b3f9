"""Post-processing of predictions on the device (the users of the deploy path).

The reference's ``--test`` and ``--visualization`` modes take the arg-max, move it to the CPU and go on in numpy / cv2
(``train.py:139-145, 182-197``, ``utils/train_eval_utils.py:203-221``).  ``DevicePostprocess`` keeps the whole output side on the
GPU: arg-max -> connected-component cleaning (keep the largest component, drop small ones, fill holes) -> nearest resize back to the
frame the input came from -> overlay.  Every quantity is an integer; two calls on one input give bit-identical outputs.

Semantics, per sample, with L0 the uint8 label map after arg-max (first maximum wins) / clamping (values outside [0, C) -> 0):

1. Components: pixels joined by a path of ``connectivity``-neighbour steps (4 or 8) through pixels of equal label; every label, 0
   included, is partitioned.  A component's root is the smallest row-major index ``y * W + x`` of its pixels.
2. Cleaning, for each class k in ``classes``: with ``keep_largest`` only the class-k component of largest area survives (equal
   areas: the smallest root); a component of area < ``min_area`` does not survive.  Pixels of the others become 0 -> L1.
3. Hole filling on L1: a component of label 0 under the DUAL connectivity (4 for 8, 8 for 4) with no pixel on the image frame and an
   area within the limit is a hole; its pixels take the label of the pixel left of its root pixel -> L2 = ``labels_net``.
4. ``stats[b, k]`` = (components of class k in L0, components of class k that survive, pixels of class k in L2, holes filled for
   k = 0 and 0 otherwise).
5. ``labels[b, y, x] = L2[b, min(floor(y * (H / hs)), H - 1), min(floor(x * (W / ws)), W - 1)]`` for y < hs, x < ws, in double:
   the INTER_NEAREST arithmetic of ``lmn_preprocess_u8`` with source and destination exchanged; 0 outside the valid area.
6. Overlay: ``a = round(alpha * 256)``; a painted pixel of class k becomes ``((256 - a) * pixel + a * palette[k] + 128) >> 8`` per
   channel.  Class 0 is never painted.  ``"fill"`` paints every pixel of a class, ``"contour"`` only pixels of the frame-resolution
   label map with a 4-neighbour of another label (outside the valid area counts as another label).

Default palette (in the frame's channel order, as the reference applies its colours to the array it has): classes 1, 2, 3 =
(0, 0, 255), (0, 255, 0), (255, 0, 0), the reference's three; every other class k the PASCAL-VOC colour-map rule: bit j of the
red / green / blue byte, counted from the top, is bit 3j / 3j + 1 / 3j + 2 of k.

``VolumePostprocess`` is the same cleaning for a whole CT case, a label volume [D, H, W]: 3D components under connectivity 6, 18 or
26, the n largest of a class, a minimal volume, cavities (include/volpost/lmnet_volpost.h); its docstring has the semantics.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from . import hip

PostOutput = namedtuple("PostOutput", ["labels_net", "labels", "overlay", "stats"])

_INT32_MAX = 2 ** 31 - 1


def alpha256(alpha):
    """round(alpha * 256), halves up, for alpha in [0, 1]."""
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("DevicePostprocess: alpha = %r outside [0, 1]" % alpha)
    return int(math.floor(alpha * 256.0 + 0.5))


def default_palette(n_classes):
    """uint8 [n_classes, 3]: the module docstring's rule."""
    pal = np.zeros((n_classes, 3), np.uint8)
    for k in range(n_classes):
        v, rgb = k, [0, 0, 0]
        for j in range(8):
            for c in range(3):
                rgb[c] |= ((v >> c) & 1) << (7 - j)
            v >>= 3
        pal[k] = rgb
    for k, colour in ((1, (0, 0, 255)), (2, (0, 255, 0)), (3, (255, 0, 0))):
        if k < n_classes:
            pal[k] = colour
    return pal


def _clean_args(cls, size, n_classes, classes, min_size, fill_holes):
    """The constructor checks DevicePostprocess and VolumePostprocess share -> (classes, {class: minimal size}, hole_limit).
    cls: the class name of the messages; size: its word for what a component measures, "area" or "volume"."""
    if not 2 <= n_classes <= 64:
        raise ValueError("%s: n_classes = %d outside [2, 64]" % (cls, n_classes))
    classes = list(range(1, n_classes)) if classes is None else [int(k) for k in classes]
    if len(set(classes)) != len(classes) or any(not 1 <= k < n_classes for k in classes):
        raise ValueError("%s: classes %r must be distinct ids in [1, %d) (background is never removed)" % (cls, classes, n_classes))
    if isinstance(min_size, (int, np.integer)):
        sizes = {k: int(min_size) for k in classes}
    else:
        if len(min_size) != len(classes):
            raise ValueError("%s: min_%s needs one entry per class in classes (%d)" % (cls, size, len(classes)))
        sizes = {k: int(a) for k, a in zip(classes, min_size)}
    if any(a < 0 or a > _INT32_MAX for a in sizes.values()):
        raise ValueError("%s: min_%s must be in [0, 2^31)" % (cls, size))
    if isinstance(fill_holes, (bool, np.bool_)):
        hole_limit = _INT32_MAX if fill_holes else 0
    else:
        hole_limit = int(fill_holes)
        if not 0 <= hole_limit <= _INT32_MAX:
            raise ValueError("%s: fill_holes = %r: a bool or a maximal hole %s in [0, 2^31)" % (cls, fill_holes, size))
    return classes, sizes, hole_limit


def _check_pred(cls, what, batch, n_classes, pred):
    """A prediction as both cleaners take it: fp32 logits [batch, C, H, W] or a uint8 / int64 label map [batch, H, W] on the device
    -> (contiguous pred, batch size, H, W).  cls, what: the class and method name of the messages; batch: its letter for the batch."""
    if not isinstance(pred, torch.Tensor) or not pred.is_cuda:
        raise RuntimeError("lm_net_amd.%s%s: device tensors required (the HIP path has no CPU path)" % (cls, what))
    if pred.dim() == 4 and pred.is_floating_point():
        if pred.shape[1] != n_classes:
            raise ValueError("%s: logits with %d channels, n_classes = %d" % (cls, pred.shape[1], n_classes))
        pred = pred.contiguous().float()
    elif pred.dim() == 3 and pred.dtype in (torch.uint8, torch.int64):
        pred = pred.contiguous()
    else:
        raise ValueError("%s: pred must be logits [%s, C, H, W] or a uint8 / int64 label map [%s, H, W]" % (cls, batch, batch))
    return pred, int(pred.shape[0]), int(pred.shape[-2]), int(pred.shape[-1])


class DevicePostprocess:
    """post(pred, src_hw=None, frames=None) -> PostOutput(labels_net, labels, overlay, stats); see the module docstring.

    pred: fp32 logits [B, C, H, W] or an integer label map [B, H, W] (uint8 or int64), 2 <= H, W <= 1024, on the device.
    src_hw: host [B, 2] or (h, w): each sample's valid size inside the padded [B, Hs, Ws, ...] frame buffer (the DeviceAugment
    convention); without frames, Hs, Ws = the largest h and w.  frames: uint8 [B, Hs, Ws, 3] or [B, Hs, Ws(, 1)] (replicated), Hs, Ws
    < 32768 (a view that is not contiguous or not 16-byte aligned is copied first).  labels is None without src_hw and frames, overlay
    is None without frames.

    No host synchronisation; every launch goes to the caller's current stream.  The cleaning parameters, src_hw and the palette are
    read on the host at the call and travel as kernel arguments (no host-to-device copy), so a call may be captured into a
    torch.cuda.graph; the capture then holds the parameters and src_hw of the captured call.  Not recorded by plans."""

    def __init__(self, n_classes, connectivity=8, classes=None, keep_largest=False, min_area=0, fill_holes=False, palette=None,
                 alpha=1.0, overlay="fill"):
        classes, areas, hole_limit = _clean_args("DevicePostprocess", "area", n_classes, classes, min_area, fill_holes)
        if connectivity not in (4, 8):
            raise ValueError("DevicePostprocess: connectivity %r is neither 4 nor 8" % (connectivity,))
        if isinstance(keep_largest, (bool, np.bool_)):
            largest = list(classes) if keep_largest else []
        else:
            largest = [int(k) for k in keep_largest]
            if any(k not in classes for k in largest):
                raise ValueError("DevicePostprocess: keep_largest %r names a class outside classes %r" % (largest, classes))
        if overlay not in ("fill", "contour"):
            raise ValueError("DevicePostprocess: overlay %r is neither 'fill' nor 'contour'" % (overlay,))
        pal = default_palette(n_classes) if palette is None else np.asarray(palette)
        if pal.shape != (n_classes, 3) or (palette is not None and (pal.min() < 0 or pal.max() > 255)):
            raise ValueError("DevicePostprocess: palette of shape %s, [%d, 3] values in [0, 255] required" % (pal.shape, n_classes))
        self.n, self.connectivity, self.classes, self.keep_largest = n_classes, connectivity, classes, largest
        self.min_area, self.hole_limit = areas, hole_limit
        self.palette = np.ascontiguousarray(pal, dtype=np.uint8)
        self.alpha256, self.mode = alpha256(alpha), 0 if overlay == "fill" else 1
        self.params = hip.PostParam()
        self.params.connectivity, self.params.hole_limit = connectivity, hole_limit
        self.params.class_mask = sum(1 << k for k in classes)
        self.params.keep_largest_mask = sum(1 << k for k in largest)
        for k, a in areas.items():
            self.params.min_area[k] = a

    def _pred(self, pred, what):
        pred, B, H, W = _check_pred("DevicePostprocess", what, "B", self.n, pred)
        if B < 1 or not (2 <= H <= 1024 and 2 <= W <= 1024):
            raise ValueError("DevicePostprocess: B=%d, %dx%d outside B >= 1, sides in [2, 1024]" % (B, H, W))
        return pred, B, H, W

    @torch.no_grad()
    def components(self, pred):
        """(roots, areas), int32 [B, H, W] each: the labelling of L0 under ``connectivity``.  roots = the root of the pixel's
        component, areas = the component's pixel count at its root pixel and 0 elsewhere."""
        pred, B, H, W = self._pred(pred, ".components")
        dev = pred.device
        prm = hip.PostParam()                                   # L0 alone: arg-max / clamping, one kernel, nothing cleaned
        prm.connectivity = self.connectivity
        lab = torch.empty(B, H, W, device=dev, dtype=torch.uint8)
        hip.post_clean(pred, self.n, prm, None, lab, None)
        roots = torch.empty(B, H, W, device=dev, dtype=torch.int32)
        areas = torch.empty(B, H, W, device=dev, dtype=torch.int32)
        hip.cc_label(lab, self.connectivity, roots, areas)
        return roots, areas

    @torch.no_grad()
    def __call__(self, pred, src_hw=None, frames=None):
        pred, B, H, W = self._pred(pred, "")
        dev = pred.device
        hw = None
        if src_hw is not None:
            hw = np.asarray(src_hw.cpu() if isinstance(src_hw, torch.Tensor) else src_hw, dtype=np.int64)
            if hw.shape == (2,):
                hw = np.broadcast_to(hw, (B, 2))
            if hw.shape != (B, 2) or hw.min() < 1 or hw.max() >= 32768:
                raise ValueError("DevicePostprocess: src_hw must be (h, w) or [B=%d, 2] with 1 <= h, w < 32768" % B)
            hw = np.ascontiguousarray(hw, dtype=np.int32)
        if frames is not None:
            if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
                raise RuntimeError("lm_net_amd.DevicePostprocess: device tensors required (the HIP path has no CPU path)")
            if (frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or frames.shape[0] != B
                    or (frames.dim() == 4 and frames.shape[3] not in (1, 3))):
                raise ValueError("DevicePostprocess: frames must be uint8 [B=%d, Hs, Ws, 3] or [B, Hs, Ws(, 1)]" % B)
            frames = frames.contiguous()
            if frames.data_ptr() % 16:                          # (a view with a storage offset: the render kernel loads 16 bytes)
                frames = frames.clone()
            Hs, Ws = int(frames.shape[1]), int(frames.shape[2])
            if not (1 <= Hs < 32768 and 1 <= Ws < 32768):
                raise ValueError("DevicePostprocess: frame size %dx%d outside [1, 32767]" % (Hs, Ws))
            if hw is not None and (hw[:, 0].max() > Hs or hw[:, 1].max() > Ws):
                raise ValueError("DevicePostprocess: src_hw exceeds the %dx%d frames" % (Hs, Ws))
        elif hw is not None:
            Hs, Ws = int(hw[:, 0].max()), int(hw[:, 1].max())
        labels_net = torch.empty(B, H, W, device=dev, dtype=torch.uint8)
        stats = torch.empty(B, self.n, 4, device=dev, dtype=torch.int32)
        ws = torch.empty(hip.post_workspace(B, H, W), device=dev, dtype=torch.uint8)
        hip.post_clean(pred, self.n, self.params, ws, labels_net, stats)
        labels = overlay = None
        if frames is not None or hw is not None:
            labels = torch.empty(B, Hs, Ws, device=dev, dtype=torch.uint8)
            if frames is not None:
                overlay = torch.empty(B, Hs, Ws, 3, device=dev, dtype=torch.uint8)
            hip.post_render(labels_net, hw, Hs, Ws, frames, self.palette, self.n, self.alpha256, self.mode, labels, overlay)
        return PostOutput(labels_net, labels, overlay, stats)


VolumeOutput = namedtuple("VolumeOutput", ["labels", "stats"])


class VolumePostprocess:
    """3D connected-component cleaning of ONE case, a label volume [D, H, W]: post(volume) -> VolumeOutput(labels, stats).

    DevicePostprocess cleans every slice as its own 2D sample, which is wrong for a case: "keep the largest component" per slice
    deletes the parts of an organ that are a second island in some slice (they are joined to it through the neighbouring slices), a
    false-positive blob survives in every slice where it is the only component, and a cavity is a 3D notion.  Semantics, with L0 the
    uint8 volume after arg-max (first maximum wins) / clamping (values outside [0, C) -> 0), exactly DevicePostprocess step 1:

    1. Components: voxels joined by a path of ``connectivity``-neighbour steps (6, 18 or 26: scipy.ndimage.generate_binary_structure(3,
       1 | 2 | 3)) through voxels of equal label; every label, 0 included, is partitioned.  A component's root is the smallest linear
       index ``(z * H + y) * W + x`` of its voxels.
    2. Cleaning, for each class k in ``classes``: the ``keep_largest[k]`` largest components survive (all of them when that is 0; equal
       sizes: the smaller root first); among those, the ones with at least ``min_volume[k]`` voxels survive.  Voxels of the others
       become 0 -> L1.
    3. Hole filling on L1: a component of label 0 under the DUAL connectivity (6 for 18 and 26, 26 for 6) with no voxel on any of the
       six faces of the volume and a volume within the limit is a hole; its voxels take the label of the voxel at x - 1 of its root
       voxel -> L2 = ``labels``.  (scipy.ndimage.binary_fill_holes(L1 > 0, generate_binary_structure(3, 1 or 3)) plus a labelling
       rule.)  Every voxel of a one-slice volume lies on a face, so a one-slice volume has no holes.
    4. ``stats[k]`` = (components of class k in L0, components of class k that survive, voxels of class k in L2, holes filled for
       k = 0 and 0 otherwise), int32 [C, 4] on the device.

    ``keep_largest``: False; True (1 for every class in ``classes``); an int n in [1, 4] (the n largest of every class in ``classes``:
    2 for kidneys and lungs); or a dict {class: n}.  ``min_volume``: an int or one int per class in ``classes``.  ``fill_holes``: a
    bool or a maximal hole volume.

    push(pred) appends n consecutive slices of the current case -- fp32 logits [n, C, H, W] or a uint8 / int64 label map [n, H, W], the
    input contract of DevicePostprocess -- narrowed to uint8 into a case buffer that grows as VolumeSurfaceMeter's does; close_case()
    cleans what was pushed; post(volume) is both.  Limits, checked when a case is closed: 1 <= D <= 1024, 2 <= H, W <= 1024, and a
    scratch of about 9.2 bytes per voxel within ``workspace_mb`` (one labelling cannot be chunked).  No call synchronises with the host
    and every launch goes to the caller's current stream; ``labels[z0:z1]`` goes into VolumeSurfaceMeter.push as it is.  Every quantity
    is an integer: two calls on one input give bit-identical outputs.  Not recorded by plans."""

    def __init__(self, n_classes, connectivity=26, classes=None, keep_largest=False, min_volume=0, fill_holes=False, workspace_mb=2048):
        classes, volumes, hole_limit = _clean_args("VolumePostprocess", "volume", n_classes, classes, min_volume, fill_holes)
        if connectivity not in (6, 18, 26):
            raise ValueError("VolumePostprocess: connectivity %r is none of 6, 18, 26" % (connectivity,))
        if isinstance(keep_largest, (bool, np.bool_)):
            keep = {k: 1 for k in classes} if keep_largest else {}
        elif isinstance(keep_largest, (int, np.integer)):
            keep = {k: int(keep_largest) for k in classes}
        elif isinstance(keep_largest, dict):
            keep = {int(k): int(n) for k, n in keep_largest.items()}
            if any(k not in classes for k in keep):
                raise ValueError("VolumePostprocess: keep_largest %r names a class outside classes %r" % (keep_largest, classes))
        else:
            raise ValueError("VolumePostprocess: keep_largest = %r: a bool, an int in [1, %d] or a dict {class: n}"
                             % (keep_largest, hip.VOLPOST_MAX_KEEP))
        if any(not 1 <= n <= hip.VOLPOST_MAX_KEEP for n in keep.values()):
            raise ValueError("VolumePostprocess: keep_largest = %r: component counts must be in [1, %d]" % (keep_largest, hip.VOLPOST_MAX_KEEP))
        if not workspace_mb > 0:
            raise ValueError("VolumePostprocess: workspace_mb must be positive")
        self.n, self.connectivity, self.classes = n_classes, connectivity, classes
        self.keep_largest, self.min_volume, self.hole_limit = keep, volumes, hole_limit
        self.workspace_bytes = int(workspace_mb * (1 << 20))
        self.class_mask = sum(1 << k for k in classes)
        self._keep = [keep.get(k, 0) for k in range(n_classes)]            # the host arrays of lmn_volpost_clean, indexed by class
        self._minv = [volumes.get(k, 0) for k in range(n_classes)]
        self._l0 = hip.PostParam()                                         # nothing cleaned: lmn_post_clean writes L0 alone, one kernel
        self._l0.connectivity = 8                                          # (checked by the entry, used by nothing on this route)
        self._case, self._depth = None, 0                                  # uint8 [capacity, H, W]; slices pushed

    def scratch_bytes(self, D, H, W):
        """Bytes of scratch one case of D x H x W voxels needs; ValueError when that exceeds workspace_mb."""
        need = hip.volpost_workspace(D, H, W)
        if need > self.workspace_bytes:
            raise ValueError("VolumePostprocess: a %dx%dx%d case needs %d bytes of scratch, workspace_mb allows %d (one labelling cannot "
                             "be chunked)" % (D, H, W, need, self.workspace_bytes))
        return need

    @torch.no_grad()
    def push(self, pred):
        """Append n consecutive slices of the current case: fp32 logits [n, C, H, W] or a uint8 / int64 label map [n, H, W]."""
        pred, n, H, W = _check_pred("VolumePostprocess", ".push", "n", self.n, pred)
        side = hip.VOLPOST_MAX_SIDE
        if n < 1:
            raise ValueError("VolumePostprocess.push: no slices")
        if self._case is not None and tuple(self._case.shape[1:]) != (H, W):
            raise ValueError("VolumePostprocess.push: slices of %dx%d into an open case of %dx%d" % ((H, W) + tuple(self._case.shape[1:])))
        if not (2 <= H <= side and 2 <= W <= side) or self._depth + n > side:
            raise ValueError("VolumePostprocess.push: a case of %d slices of %dx%d is outside 1 <= D <= %d, 2 <= H, W <= %d"
                             % (self._depth + n, H, W, side, side))
        cap = 0 if self._case is None else self._case.shape[0]
        if self._depth + n > cap:                                # grow the case buffer (device copy, no sync)
            cap = min(max(self._depth + n, 2 * cap), side)
            grown = torch.empty(cap, H, W, device=pred.device, dtype=torch.uint8)
            if self._case is not None:
                grown[:self._depth].copy_(self._case[:self._depth])
            self._case = grown
        hip.post_clean(pred, self.n, self._l0, None, self._case[self._depth:self._depth + n], None)
        self._depth += n

    def _take_case(self, what):
        if self._case is None or self._depth == 0:
            raise ValueError("VolumePostprocess.%s: no slices were pushed" % what)
        lab, self._case, self._depth = self._case[:self._depth], None, 0
        return lab

    @torch.no_grad()
    def close_case(self):
        """Clean the slices pushed since the last case: VolumeOutput(labels uint8 [D, H, W], stats int32 [C, 4])."""
        lab = self._take_case("close_case")
        D, H, W = (int(d) for d in lab.shape)
        dev = lab.device
        ws = torch.empty(self.scratch_bytes(D, H, W), device=dev, dtype=torch.uint8)
        labels = torch.empty(D, H, W, device=dev, dtype=torch.uint8)
        stats = torch.empty(self.n, hip.VOLPOST_NSTAT, device=dev, dtype=torch.int32)
        hip.volpost_clean(lab, self.n, self.connectivity, self.class_mask, self._keep, self._minv, self.hole_limit, ws, labels, stats)
        return VolumeOutput(labels, stats)

    def _whole(self, volume, what):
        if self._depth:
            raise ValueError("VolumePostprocess%s: a case with %d pushed slices is open; close_case() first" % (what, self._depth))
        self.push(volume)

    def __call__(self, volume):
        """Clean one whole case: push + close_case."""
        self._whole(volume, "")
        return self.close_case()

    @torch.no_grad()
    def components(self, volume):
        """(roots, sizes), int32 [D, H, W] each: the labelling of L0 under ``connectivity``.  roots = the root of the voxel's component,
        sizes = the component's voxel count at its root voxel and 0 elsewhere."""
        self._whole(volume, ".components")
        lab = self._take_case("components")
        roots = torch.empty(lab.shape, device=lab.device, dtype=torch.int32)
        sizes = torch.empty(lab.shape, device=lab.device, dtype=torch.int32)
        hip.cc3d_label(lab, self.connectivity, roots, sizes)
        return roots, sizes

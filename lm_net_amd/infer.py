"""Inference on frames of any size: overlapping tiles, mirrored copies and a windowed blend, all on the device.

    pred = TiledPredictor(model, tile=(352, 352), overlap=0.5, flips=("h", "v", "hv"))
    res = pred(images)            # normalised fp32 [B, channel, H, W] on the device, any 1 <= H, W <= 8192
    res.map, res.labels           # fp32 [B, C, H, W]; uint8 [B, H, W]

The model takes frames whose sides are multiples of 16 (LM_Net.forward).  TiledPredictor cuts a frame of any size into tiles of
one such size (lmn_tile_gather: the frame padded up to one tile where it is smaller, the last tile of an axis pulled back to the edge,
every tile followed by its mirrored copies), runs the model on `tile_batch` of them at a time and merges the tile outputs back into
one full-size map under a smooth window (lmn_tile_blend: one launch, a fixed order of every pixel's sum, the arg-max in the same
launch).  Geometry and semantics: include/tiles/lmnet_tiles.h.  There is no eager fallback: a CPU tensor raises.

`.map` and `.labels` go straight into lm_net_amd.metrics.ConfusionMeter / SurfaceDistanceMeter and lm_net_amd.post.DevicePostprocess
(up to their own limit of 1024 pixels a side)."""
import collections

import numpy as np
import torch

from . import hip

TiledPrediction = collections.namedtuple("TiledPrediction", ["map", "labels"])


def window_table(t, kind="gaussian", sigma_scale=0.125):
    """The 1-D window of a tile side of t pixels: float64 on the host, rounded ONCE to fp32 (the values the kernel multiplies).
    "constant": ones; "gaussian": exp(-0.5 ((i - (t - 1) / 2) / (sigma_scale t))^2)."""
    if kind == "constant":
        return np.ones(int(t), dtype=np.float32)
    if kind != "gaussian":
        raise ValueError("TiledPredictor: window=%r, expected 'gaussian' or 'constant'" % (kind,))
    i = np.arange(int(t), dtype=np.float64)
    return np.exp(-0.5 * ((i - (t - 1) / 2.0) / (float(sigma_scale) * t)) ** 2).astype(np.float32)


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


class TiledPredictor:
    """model: an lm_net_amd.LM_Net in eval mode (a tiled pass must not move BatchNorm statistics).
    tile: (h, w), multiples of 16 in [32, 1024].  stride: (h, w) in pixels, 1 <= s <= tile; None: tile - round(tile * overlap) with
    0 <= overlap <= 0.75.  window: "gaussian" (sigma = sigma_scale * tile) or "constant".  flips: a subset of ("h", "v", "hv"); the
    identity always comes first.  average: "logits", "softmax" (probabilities are averaged) or "sigmoid".  pad: "reflect" (an axis
    shorter than the tile must then have length >= 2) or "zero" (0 is the mean after normalisation).  tile_batch: tiles per model call;
    the last, short batch is filled up by repeating its final entry, so the model sees ONE input shape (one plan, or one graph
    replay under model.enable_graphs()).  workspace_mb: the tile outputs of as many images as fit are blended in one launch; a single
    image that does not fit raises ValueError.

    A call runs under torch.no_grad(), does not synchronise with the host and, apart from the model's own output and the cached
    tables and workspace of a geometry, allocates nothing after the first call of that geometry: `.map` and `.labels` are that
    geometry's buffers, overwritten by its next call (clone what must outlive it)."""

    def __init__(self, model, tile=(352, 352), overlap=0.5, stride=None, window="gaussian", sigma_scale=0.125, flips=(), average="logits",
                 pad="reflect", tile_batch=8, workspace_mb=1024):
        if getattr(model, "training", False):
            raise RuntimeError("TiledPredictor: the model is in training mode; call model.eval() (a tiled pass must not move "
                               "BatchNorm statistics)")
        self.model = model
        self.tile = _pair(tile)
        if any(t % 16 or not hip.TILE_MIN <= t <= hip.TILE_MAX for t in self.tile):
            raise ValueError("TiledPredictor: tile %dx%d: sides must be multiples of 16 in [%d, %d]"
                             % (self.tile + (hip.TILE_MIN, hip.TILE_MAX)))
        if stride is None:
            if not 0.0 <= float(overlap) <= 0.75:
                raise ValueError("TiledPredictor: overlap=%r outside [0, 0.75]" % (overlap,))
            self.stride = tuple(t - int(round(t * float(overlap))) for t in self.tile)
        else:
            self.stride = _pair(stride)
        if any(not 1 <= s <= t for s, t in zip(self.stride, self.tile)):
            raise ValueError("TiledPredictor: stride %dx%d outside [1, tile]" % self.stride)
        if not float(sigma_scale) > 0.0:
            raise ValueError("TiledPredictor: sigma_scale=%r is not positive" % (sigma_scale,))
        self._windows = tuple(window_table(t, window, sigma_scale) for t in self.tile)
        self.window, self.sigma_scale = window, float(sigma_scale)
        self.flips = tuple(flips)
        self.average, self.pad = average, pad
        hip.tile_param(1, 1, self.tile[0], self.tile[1], self.tile, self.stride, pad, self.flips, average)      # checks the names
        if int(tile_batch) < 1 or not float(workspace_mb) > 0:
            raise ValueError("TiledPredictor: tile_batch=%r, workspace_mb=%r" % (tile_batch, workspace_mb))
        self.tile_batch, self.workspace_mb = int(tile_batch), float(workspace_mb)
        self._cache = {}

    def _geometry(self, images):
        """Everything a geometry (input shape, device) needs, built once: the two parameter structs per group size, the window tables
        on the device, the tile batch, the workspace of tile outputs, the map and the labels."""
        key = (tuple(images.shape), images.device)
        g = self._cache.get(key)
        if g is not None:
            return g
        B, ch, H, W = images.shape
        if not (1 <= H <= hip.TILE_MAX_LEN and 1 <= W <= hip.TILE_MAX_LEN):
            raise ValueError("TiledPredictor: frame %dx%d: sides must be in [1, %d]" % (H, W, hip.TILE_MAX_LEN))
        if self.pad == "reflect" and any(L < 2 and L < t for L, t in ((H, self.tile[0]), (W, self.tile[1]))):
            raise ValueError("TiledPredictor: frame %dx%d: pad='reflect' needs length >= 2 on an axis shorter than the tile" % (H, W))
        C = int(getattr(self.model, "n_classes"))
        if not 1 <= C <= hip.TILE_MAX_CLASSES:
            raise ValueError("TiledPredictor: %d classes; the blend takes 1..%d" % (C, hip.TILE_MAX_CLASSES))
        th, tw = self.tile
        one = hip.tile_param(1, C, H, W, self.tile, self.stride, self.pad, self.flips, self.average)
        E = hip.tile_entries(one)
        per_image, limit = E * C * th * tw * 4, int(self.workspace_mb * (1 << 20))
        if per_image > limit:
            raise ValueError("TiledPredictor: the tile outputs of one %dx%d frame take %d bytes (%d entries of %d x %dx%d fp32), "
                             "workspace_mb=%g allows %d" % (H, W, per_image, E, C, th, tw, self.workspace_mb, limit))
        group = min(B, limit // per_image)
        dev = images.device
        g = dict(E=E, C=C, group=group,
                 wy=torch.from_numpy(self._windows[0]).to(dev), wx=torch.from_numpy(self._windows[1]).to(dev),
                 batch=torch.empty((self.tile_batch, ch, th, tw), device=dev, dtype=torch.float32),
                 z=torch.empty((group * E, C, th, tw), device=dev, dtype=torch.float32),
                 map=torch.empty((B, C, H, W), device=dev, dtype=torch.float32),
                 labels=(torch.empty((B, H, W), device=dev, dtype=torch.uint8) if C >= 2 and self.average != "sigmoid" else None),
                 params={})
        for n in {group, B % group or group}:                      # (the last group of a batch may be smaller)
            g["params"][n] = (hip.tile_param(n, ch, H, W, self.tile, self.stride, self.pad, self.flips, self.average),
                              hip.tile_param(n, C, H, W, self.tile, self.stride, self.pad, self.flips, self.average))
        self._cache[key] = g
        return g

    @torch.no_grad()
    def __call__(self, images):
        if self.model.training:
            raise RuntimeError("TiledPredictor: the model is in training mode; call model.eval()")
        if not images.is_cuda:
            raise RuntimeError("TiledPredictor: device tensor required (the HIP path has no CPU fallback)")
        if images.dim() != 4 or images.dtype != torch.float32:
            raise ValueError("TiledPredictor: expected normalised fp32 [B, channel, H, W], got %s %s" % (images.dtype, tuple(images.shape)))
        images = images.contiguous()
        g = self._geometry(images)
        B, E, tb = images.shape[0], g["E"], self.tile_batch
        for b0 in range(0, B, g["group"]):
            n = min(g["group"], B - b0)
            p_src, p_out = g["params"][n]
            src, z = images[b0:b0 + n], g["z"][:n * E]
            for e0 in range(0, n * E, tb):
                k = min(tb, n * E - e0)
                hip.tile_gather(src, p_src, e0, k, g["batch"][:k])
                if k < tb:                                          # fill entries: copies of the last one, their outputs ignored
                    g["batch"][k:].copy_(g["batch"][k - 1:k].expand(tb - k, -1, -1, -1))
                out = self.model(g["batch"])
                if out.shape[1:] != z.shape[1:]:
                    raise RuntimeError("TiledPredictor: the model returned %s for tiles of %s" % (tuple(out.shape), tuple(g["batch"].shape)))
                z[e0:e0 + k].copy_(out[:k])
            hip.tile_blend(z, p_out, g["wy"], g["wx"], g["map"][b0:b0 + n], None if g["labels"] is None else g["labels"][b0:b0 + n])
        return TiledPrediction(g["map"], g["labels"])

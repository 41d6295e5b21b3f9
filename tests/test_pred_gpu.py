"""GPU: one prediction, every consumer.  ConfusionMeter, ImageStatsMeter, SurfaceDistanceMeter and DevicePostprocess all begin by
turning logits or a label map into one class id per pixel (csrc/pred_common.h, lm_net_amd.metrics._prediction); here they all read
the same tie-heavy logits and must agree, exactly, with numpy's first-maximum arg-max.

B = 3 at 37 x 45 (the shape of test_image_stats_gpu.py: 256-pixel tiles straddle the image boundaries).  C = 2, 3, 4: the three
confusion kernels templated on C; 5, 9, 64: the LDS form; C <= 8 / C > 8: the ballot and the atomic form of the per-image statistics.
Logits take the four values {-1, 0, 0.25, 1}, so a tied maximum is common (25 % of pixels at C = 2, more above), and one image row
has every class equal.  About 20 % of the labels are void (255, -100, one stray 77)."""
import functools

import numpy as np
import pytest
import torch

import void_ref as V

pytestmark = pytest.mark.gpu

B, H, W = 3, 37, 45
CLASSES = (2, 3, 4, 5, 9, 64)
VALUES = np.array([-1.0, 0.0, 0.25, 1.0], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _case(C):
    """(logits fp32 [B,C,H,W], labels int64 [B,H,W], reference prediction int64 [B,H,W]), numpy, read-only."""
    u = V.uniform("pred_gpu/%d/lg" % C, B * C * H * W)
    lg = VALUES[np.minimum((u * 4).astype(np.int64), 3)].reshape(B, C, H, W)
    lg[1, :, 11, :] = 0.25                                           # a row in which every class is equal
    y = V.labels(B, H, W, C, "pred_gpu/%d/y" % C)
    y = V.with_void(y, "pred_gpu/%d/v255" % C, 255, 0.1)
    y = V.with_void(y, "pred_gpu/%d/v100" % C, -100, 0.1).numpy()
    y[2, 5, 5] = 77
    pred = V.argmax_first(lg).astype(np.int64)
    # the input itself, before anything runs on the device
    top = lg.max(1, keepdims=True)
    tied = ((lg == top).sum(1) >= 2).mean()
    void = ((y < 0) | (y >= C)).mean()
    print("C = %d: %.1f %% of pixels with a tied maximum, %.1f %% void labels" % (C, 100 * tied, 100 * void))
    assert tied >= 0.20 and 0.15 <= void <= 0.25
    assert (pred[1, 11] == 0).all() and np.array_equal(pred, torch.from_numpy(lg).argmax(1).numpy())
    for a in (lg, y, pred):
        a.setflags(write=False)
    return lg, y, pred


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                      # (a copy: the cached case is read-only)


def _stray(C, dtype):
    """(map with a few stray pixels, the same map with -1 there): the reference prediction in `dtype` with pixels set to values
    outside [0, C) -- C and 255, and -1 and 300 where the dtype holds them."""
    _, _, pred = _case(C)
    m, want = pred.copy(), pred.copy()
    vals = [C, 255] if dtype == np.uint8 else [-1, C, 255, 300]
    for j, v in enumerate(vals):
        for b in range(B):
            m[b, 3 + 7 * j, 2 + 5 * b:40:9] = v
            want[b, 3 + 7 * j, 2 + 5 * b:40:9] = -1
    assert (want < 0).sum() == len(vals) * sum(len(range(2 + 5 * b, 40, 9)) for b in range(B))
    return m.astype(dtype), want


def _routes(C, int32):
    """name -> (device prediction, host prediction with -1 for "no class")"""
    lg, _, pred = _case(C)
    out = {"logits": (_dev(lg), pred), "uint8": (_dev(pred.astype(np.uint8)), pred), "int64": (_dev(pred), pred)}
    for name, dt in (("uint8 stray", np.uint8), ("int64 stray", np.int64)) + ((("int32 stray", np.int32),) if int32 else ()):
        m, want = _stray(C, dt)
        out[name] = (_dev(m), want)
    return out


def _confusion(pred, y, C):
    keep = (y >= 0) & (y < C) & (pred >= 0)
    return np.bincount(C * y[keep] + pred[keep], minlength=C * C).reshape(C, C)


@pytest.mark.parametrize("C", CLASSES)
def test_confusion_meter(C):
    from lm_net_amd.metrics import ConfusionMeter
    _, y, pred = _case(C)
    got = {}
    for name, (p, host) in _routes(C, int32=True).items():
        m = ConfusionMeter(C)
        m.update(p, _dev(y))
        got[name] = m.total.cpu().numpy()
        assert got[name].dtype == np.float64 and np.array_equal(got[name], _confusion(host, y, C)), name
    assert np.array_equal(got["uint8"], got["logits"]) and np.array_equal(got["int64"], got["logits"])
    assert got["logits"].sum() == ((y >= 0) & (y < C)).sum()
    with pytest.raises(ValueError, match="channels"):               # (once passed on: (C + 1)^2 floats into C x C counts)
        ConfusionMeter(C).update(torch.zeros(1, C + 1, 4, 4, device="cuda"), torch.zeros(1, 4, 4, device="cuda", dtype=torch.int64))


@pytest.mark.parametrize("C", CLASSES)
def test_image_stats_meter(C):
    from lm_net_amd import ImageStatsMeter
    _, y, pred = _case(C)
    got = {}
    for name, (p, host) in _routes(C, int32=True).items():
        m = ImageStatsMeter(C, ignore_index=255)
        m.update(p, _dev(y))
        got[name] = m.raw().cpu().numpy()
        assert got[name].dtype == np.int64 and np.array_equal(got[name], V.image_stats(host, y, C)), name
    assert np.array_equal(got["uint8"], got["logits"]) and np.array_equal(got["int64"], got["logits"])


@pytest.mark.parametrize("C", CLASSES)
def test_surface_distance_meter_counts(C):
    from lm_net_amd.metrics import SurfaceDistanceMeter
    _, y, pred = _case(C)
    got = {}
    for name, (p, host) in _routes(C, int32=True).items():
        m = SurfaceDistanceMeter(C)
        m.update(p, _dev(y))
        si, sf = (a.cpu().numpy() for a in m.raw())
        got[name] = (si, sf)
        n_pred = np.stack([(host == k).sum((1, 2)) for k in m.classes], 1)
        n_target = np.stack([(y == k).sum((1, 2)) for k in m.classes], 1)
        assert np.array_equal(si[..., 0], n_pred) and np.array_equal(si[..., 1], n_target), name
    for name in ("uint8", "int64"):                                  # the same masks: every statistic, the float64 sums bit for bit
        assert np.array_equal(got[name][0], got["logits"][0]) and got[name][1].tobytes() == got["logits"][1].tobytes(), name


@pytest.mark.parametrize("C", CLASSES)
def test_postprocess_labels(C):
    from lm_net_amd.post import DevicePostprocess
    post = DevicePostprocess(C)                                      # nothing cleaned: labels_net is the prediction
    for name, (p, host) in _routes(C, int32=False).items():
        net = post(p).labels_net.cpu().numpy()
        assert net.dtype == np.uint8 and np.array_equal(net, np.maximum(host, 0)), name      # "no class" -> class 0

"""GPU: lm_net_amd.metrics.CurveMeter fed by LM_Net(3, 1), a multi-label LM_Net(3, 3) (filters [12] * 5, seeded weights, eval mode) and
by the probability map of lm_net_amd.infer.TiledPredictor(average="sigmoid"), each against the brute-force restatement
tests/curves_ref.py on the logits or maps copied to the host.  All exact: the kernel sees the fp32 values as they are, and none of
these uses a softmax head, so none needs a margin."""
import gc

import numpy as np
import pytest
import torch

import curves_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.fixture(scope="module")
def model():
    """model(C): LM_Net(3, C) with seeded weights in eval mode, built once per class count and released when this module is done"""
    from lm_net_amd import LM_Net
    from tools.detweights import fill_module
    nets = {}

    def get(C):
        if C not in nets:
            net = LM_Net(3, C, filters=[12] * 5)
            fill_module(net, 5)
            nets[C] = net.to(DEV).eval()
        return nets[C]

    yield get
    nets.clear()
    gc.collect()


def frame(B, H, W):
    from tools.detweights import det_input
    return det_input((B, 3, H, W), "curves/%dx%d" % (H, W))


def assert_meter_equals_restatement(m, values, t, scores, n_images):
    """the raw histograms cell for cell, then the curves and areas the host derives from them"""
    v = values.detach().float().cpu().numpy()
    assert np.array_equal(m.raw().cpu().numpy(), R.hist(v, t, m.thresholds.size, scores))
    cnt = R.counts(v, t, m.thresholds.size, scores)
    assert cnt[0].shape[0] == n_images
    for a, b in zip(m.counts(per_image=True), cnt):
        assert np.array_equal(a, b)
    pooled = tuple(a.sum(0) for a in cnt)
    close = lambda a, b: np.allclose(a, b, rtol=0, atol=1e-12, equal_nan=True)
    assert close(m.auroc(), R.auroc(*pooled)) and close(m.average_precision(), R.average_precision(*pooled))
    fpr, tpr, _ = m.roc()
    assert close(fpr, R.roc(*pooled)[0]) and close(tpr, R.roc(*pooled)[1])
    return pooled


@pytest.mark.parametrize("C", [1, 3], ids=["binary", "multilabel"])
def test_sigmoid_heads(C, model):
    """LM_Net(3, 1) with a [B, H, W] target and a multi-label LM_Net(3, 3) with [B, 3, H, W] planes, on a 2x3x32x48 input"""
    from lm_net_amd import CurveMeter
    net = model(C)
    with torch.no_grad():
        z = net(frame(2, 32, 48).to(DEV))
    assert tuple(z.shape) == (2, C, 32, 48)
    t = R.plane_targets((2, C, 32, 48), "model/t%d" % C, 0.1, np.uint8)
    m = CurveMeter(C, "sigmoid", 101)
    m.update(z, torch.from_numpy(t[:, 0] if C == 1 else t).to(DEV))
    tp, fp, fn, tn = assert_meter_equals_restatement(m, z, t, "sigmoid", 2)
    thr, best = m.best_threshold("f1")
    with np.errstate(divide="ignore", invalid="ignore"):
        f1 = np.where(2 * tp + fp + fn > 0, 2 * tp / (2 * tp + fp + fn), 1.0)
    assert np.array_equal(best, f1.max(1)) and np.array_equal(thr, m.thresholds[f1.argmax(1)])


def test_tiled_probability_map(model):
    """TiledPredictor(average="sigmoid").map of a 40x50 frame (one padded 64x64 tile and its mirror) fed to
    CurveMeter(scores="probability")"""
    from lm_net_amd import CurveMeter
    from lm_net_amd.infer import TiledPredictor
    pred = TiledPredictor(model(3), tile=64, flips=("h",), average="sigmoid")
    res = pred(frame(2, 40, 50).to(DEV))
    assert tuple(res.map.shape) == (2, 3, 40, 50) and float(res.map.min()) >= 0.0 and float(res.map.max()) <= 1.0
    t = R.plane_targets((2, 3, 40, 50), "model/tiled", 0.1)
    m = CurveMeter(3, "probability", 101)
    m.update(res.map, torch.from_numpy(t).to(DEV))
    assert_meter_equals_restatement(m, res.map, t, "probability", 2)

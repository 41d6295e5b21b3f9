"""GPU: per-image tp / fp / fn / tn (lmn_image_stats, include/lmnet_loss.h) and lm_net_amd.ImageStatsMeter: every count exact against
the numpy restatement of tests/void_ref.py and the reference golden (tests/golden/void_loss_stats.npz).  B = 3 at 37 x 45: 1665
pixels per image, so that 256-pixel tiles of the flat batch would straddle both image boundaries."""
import numpy as np
import pytest
import torch

import void_ref as V
from helpers import load_golden

pytestmark = pytest.mark.gpu


def _stats(pred, y, C, ignore_index=255):
    from lm_net_amd import hip
    out = torch.full((y.shape[0], C, 4), -7, device="cuda", dtype=torch.int64)      # (the entry overwrites)
    hip.image_stats(pred, y, C, ignore_index, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _valid_counts(y, C):
    return np.repeat(((y >= 0) & (y < C)).sum((1, 2)).numpy()[:, None], C, 1)


@pytest.mark.parametrize("C", V.STATS_C)
def test_counts_exact_vs_restatement_and_golden(C):
    g = load_golden("void_loss_stats.npz")
    lg, y = V.stats_case(C)
    pred = V.argmax_first(lg.numpy())
    want = V.image_stats(pred, y.numpy(), C)
    assert np.array_equal(want, g["stats/%d" % C])
    a = _stats(lg.cuda(), y.cuda(), C)                                                # logits
    b = _stats(torch.from_numpy(pred).to(torch.uint8).cuda(), y.cuda(), C)            # uint8 label map
    assert np.array_equal(a, want) and np.array_equal(b, want)
    assert np.array_equal(a.sum(-1), _valid_counts(y, C))
    assert np.array_equal(_stats(lg.cuda(), y.cuda(), C), a)                          # a second call: identical


@pytest.mark.parametrize("C", V.STATS_C)
def test_edge_cases_exact(C):
    B, H, W = 3, 37, 45
    key = "stats_gpu/%d" % C
    lg = V.det_input((B, C, H, W), key + "/lg")
    y0 = V.labels(B, H, W, C, key + "/y")
    # forced arg-max ties: the first maximum wins
    lg[:, C - 1] = torch.where(torch.from_numpy(V.uniform(key + "/tie", B * H * W) < 0.3).reshape(B, H, W), lg[:, :C - 1].max(1).values,
                               lg[:, C - 1])
    lg[0, :, 3] = 0.25                                                                # a row where every class ties: class 0
    pred = V.argmax_first(lg.numpy())
    assert (pred[0, 3] == 0).all() and np.array_equal(pred, lg.argmax(1).numpy())
    cases = {"no_void": (y0.clone(), None), "void": (V.with_void(y0, key + "/v"), 255)}
    yv = V.with_void(y0, key + "/v")
    yv[1] = 255
    cases["image_void"] = (yv, 255)
    yw = V.with_void(y0, key + "/v")
    yw[2] = torch.where(yw[2] == 255, yw[2], (torch.from_numpy(pred[2]) + 1) % C)     # one image without a correct pixel
    cases["none_correct"] = (yw, 255)
    ys = V.with_void(y0, key + "/v", -100)
    ys[0, 5, 5] = 77                                                                  # a stray label is void too
    cases["stray"] = (ys, -100)
    for name, (y, ii) in cases.items():
        want = V.image_stats(pred, y.numpy(), C)
        got = _stats(lg.cuda(), y.cuda(), C, ii)
        assert np.array_equal(got, want), name
        assert np.array_equal(got.sum(-1), _valid_counts(y, C)), name
        if name == "image_void":
            assert not got[1].any()
        if name == "none_correct":
            assert not got[2, :, 0].any() and got[2].any()
    # uint8 label-map prediction where 255 (and any value >= C) means "no class"
    p8 = torch.from_numpy(pred).to(torch.uint8)
    p8[torch.from_numpy(V.uniform(key + "/nc", B * H * W) < 0.1).reshape(B, H, W)] = 255
    if C < 64:
        p8[0, 0, :5] = C
    y, ii = cases["void"]
    want = V.image_stats(np.where(p8.numpy() >= C, -1, p8.numpy()), y.numpy(), C)
    got = _stats(p8.cuda(), y.cuda(), C, ii)
    assert np.array_equal(got, want) and np.array_equal(got.sum(-1), _valid_counts(y, C))
    assert np.array_equal(_stats(p8.cuda(), y.cuda(), C, ii), got)


@pytest.mark.parametrize("C", V.STATS_C)
def test_meter_scores_vs_golden(C):
    """ImageStatsMeter.score against the reference's metric functions: 1e-12 on the goldens made from float64 statistics; the "s32"
    goldens (the reference's own float32 arithmetic on int64 statistics: every metric / reduction pair) at 1e-6."""
    from lm_net_amd import ImageStatsMeter
    g = load_golden("void_loss_stats.npz")
    lg, y = V.stats_case(C)
    m = ImageStatsMeter(C, ignore_index=255)
    m.update(lg[:2].cuda(), y[:2].cuda())                                             # logits, then an int64 label map
    m.update(lg[2:].argmax(1).cuda(), y[2:].cuda())
    tp, fp, fn, tn = m.stats()
    assert np.array_equal(torch.stack([tp, fp, fn, tn], -1).numpy(), g["stats/%d" % C])
    cw = V.stats_class_weights(C)

    def close(a, b, tol):
        return (np.isnan(a) and np.isnan(b)) or a == b or abs(a - b) <= tol * abs(b)
    for i, name in enumerate(V.METRICS):
        pname, kw = V.PRODUCT_NAMES.get(name, (name, {}))
        for j, r in enumerate(V.REDUCTIONS):
            got = m.score(pname, r, class_weights=cw if "weighted" in r else None, **kw)
            assert close(got, float(g["s64/%d" % C][i, j]), 1e-12), (name, r, got)
            assert close(got, float(g["s32/%d" % C][i, j]), 1e-6), (name, r, got)
    per = m.per_image("iou")
    assert per.shape == (3, C) and close(float(per.mean()), m.score("iou", "macro-imagewise"), 1e-12)

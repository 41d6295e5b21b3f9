"""GPU: lmn_augment_u8 through lm_net_amd.data.DeviceAugment against the numpy restatement (tests/augment_ref.py): labels,
normalised floats and the contrast gray sums bit-exact, for sampled parameters and forced corner cases, ragged batches, and
augmented batches feeding a training step."""
import numpy as np
import pytest
import torch

import augment_ref as A

pytestmark = pytest.mark.gpu

MEAN3, STD3 = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MEAN1, STD1 = (0.5,), (0.25,)


def _frames(rng, B, hs, ws, C, mask_mode):
    img = rng.integers(0, 256, (B, hs, ws, C), dtype=np.uint8)
    img[:, : hs // 3] //= 3                                 # some structure, so contrast / hue see non-uniform frames
    mask = rng.integers(0, 256 if mask_mode == "binary" else 64, (B, hs, ws), dtype=np.uint8)
    return img, mask


def _corner_cases(B, hs, ws, H, W):
    """Forced corner cases (cycled over the batch): a large rotation + shift with most pixels on the border, the full frame,
    a 1-pixel-wide crop, every ColorJitter op alone and all four in a fixed order."""
    from lm_net_amd.data import ssr_matrix
    full = (0, 0, hs, ws)
    cases = [
        {"crop": full, "M": ssr_matrix(H, W, 75.0, 0.9, 0.45, -0.4), "flips": 3},
        {"crop": full},
        {"crop": (hs // 4, ws // 2, max(1, hs // 2), 1), "M": ssr_matrix(H, W, -20.0, 1.1, 0.05, 0.1), "flips": 1},
        {"crop": (1, 0, hs - 1, ws), "cj": [1.2, 1.0, 1.0, 0.0]},
        {"crop": full, "cj": [1.0, 0.8, 1.0, 0.0], "flips": 2},
        {"crop": full, "cj": [1.0, 1.0, 0.0, 0.0]},
        {"crop": full, "cj": [1.0, 1.0, 1.0, -0.2]},
        {"crop": (0, 1, hs, ws - 1), "M": ssr_matrix(H, W, 30.0, 1.0, 0.0, 0.0), "cj": [0.85, 1.15, 1.1, 0.13], "order": [3, 2, 1, 0]},
        {"crop": full, "cj": [1.0, 0.0, 1.0, 0.0]},
        {"crop": full, "cj": [0.0, 1.1, 1.0, 0.0], "order": [1, 0, 2, 3]},
        {"crop": full, "cj": [1.1, 0.9, 1.2, 0.5], "order": [0, 2, 3, 1]},
    ]
    return [cases[b % len(cases)] for b in range(B)]


def _check(aug, img, mask, params, size, mean, std, mm, src_hw=None):
    x, y = aug(torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda(), params=params, src_hw=src_hw)
    torch.cuda.synchronize()
    xr, yr, gr = A.augment(img, mask, params, size, mean, std, mm, src_hw=src_hw)
    B, C = img.shape[0], img.shape[3]
    assert x.shape == (B, C) + tuple(size) and y.shape == (B,) + tuple(size) and y.dtype == torch.int64
    yg, xg = y.cpu().numpy(), x.cpu().numpy()
    for b in range(B):   # per sample first, so that a failure names the case
        assert np.array_equal(yg[b], yr[b]), (b, params[b], int((yg[b] != yr[b]).sum()))
        assert np.array_equal(xg[b], xr[b]), (b, params[b], int((xg[b] != xr[b]).sum()))
    assert np.array_equal(aug.last_gray_sum.cpu().numpy(), gr)
    return x, y


@pytest.mark.parametrize("B,hs,ws,h,w", [(3, 37, 53, 32, 48), (2, 512, 620, 256, 256), (8, 530, 622, 352, 352),
                                         (2, 100, 80, 352, 352)])
@pytest.mark.parametrize("C,mask_mode", [(3, "binary"), (1, "labels"), (3, "labels"), (1, "binary")])
def test_augment_matches_restatement(B, hs, ws, h, w, C, mask_mode):
    from lm_net_amd.data import DeviceAugment
    rng = np.random.default_rng(B * 1000 + hs + 7 * C)
    img, mask = _frames(rng, B, hs, ws, C, mask_mode)
    mean, std = (MEAN3, STD3) if C == 3 else (MEAN1, STD1)
    mm = DeviceAugment.MASK_MODES[mask_mode]
    aug = DeviceAugment((h, w), mean, std, channels=C, mask_mode=mask_mode, generator=hs + C, p_ssr=0.7, p_cj=0.7)
    sampled = aug.sample_dicts(B, (hs, ws))
    _check(aug, img, mask, sampled, (h, w), mean, std, mm)
    _check(aug, img, mask, _corner_cases(B, hs, ws, h, w), (h, w), mean, std, mm)
    if B < 11:   # every corner case at least once
        cases = _corner_cases(11, hs, ws, h, w)
        big_img, big_mask = _frames(rng, 11, hs, ws, C, mask_mode)
        _check(aug, big_img, big_mask, cases, (h, w), mean, std, mm)


def test_params_none_samples_and_repeats_bit_identical():
    from lm_net_amd.data import DeviceAugment
    rng = np.random.default_rng(1)
    img, mask = _frames(rng, 4, 120, 150, 3, "binary")
    aug = DeviceAugment((96, 96), generator=3, p_ssr=1.0, p_cj=1.0)
    ti, tm = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()
    x1, y1 = aug(ti, tm)
    p = aug.last_params
    g1 = aug.last_gray_sum.clone()
    x2, y2 = aug(ti, tm, params=p)
    assert torch.equal(x1, x2) and torch.equal(y1, y2) and torch.equal(g1, aug.last_gray_sum)
    xr, yr, gr = A.augment(img, mask, _dicts_of(p), (96, 96), MEAN3, STD3)
    assert np.array_equal(x1.cpu().numpy(), xr) and np.array_equal(y1.cpu().numpy(), yr) and np.array_equal(g1.cpu().numpy(), gr)
    # images only / masks only
    xo, none = aug(ti, None, params=p)
    assert none is None and torch.equal(xo, x1)
    none, yo = aug(None, tm, params=p)
    assert none is None and torch.equal(yo, y1)


def _dicts_of(params):
    out = []
    for p in params:
        d = {"crop": (p.y0, p.x0, p.h, p.w), "flips": p.flips}
        if p.apply_ssr:
            d["M"] = list(p.M)
        if p.apply_cj:
            d["cj"], d["order"] = list(p.cj), list(p.order)
        out.append(d)
    return out


@pytest.mark.parametrize("C", [3, 1])
def test_ragged_batch_in_padded_buffer(C):
    from lm_net_amd.data import DeviceAugment
    rng = np.random.default_rng(5 + C)
    sizes = [(530, 622), (300, 411), (97, 640), (512, 100)]
    Hm, Wm = max(s[0] for s in sizes), max(s[1] for s in sizes)
    img = np.full((4, Hm, Wm, C), 255, dtype=np.uint8)      # padding that must never be read
    mask = np.full((4, Hm, Wm), 200, dtype=np.uint8)
    for b, (hs, ws) in enumerate(sizes):
        img[b, :hs, :ws] = rng.integers(0, 256, (hs, ws, C), dtype=np.uint8)
        mask[b, :hs, :ws] = rng.integers(0, 256, (hs, ws), dtype=np.uint8)
    mean, std = (MEAN3, STD3) if C == 3 else (MEAN1, STD1)
    aug = DeviceAugment((352, 352), mean, std, channels=C, generator=21, p_ssr=0.8, p_cj=0.8)
    src_hw = np.array(sizes, dtype=np.int32)
    params = aug.sample_dicts(4, src_hw)
    x, y = _check(aug, img, mask, params, (352, 352), mean, std, 0, src_hw=src_hw)
    for b, (hs, ws) in enumerate(sizes):   # and each sample against the restatement of its unpadded frame alone
        xr, yr, _ = A.augment_one(np.ascontiguousarray(img[b, :hs, :ws]), np.ascontiguousarray(mask[b, :hs, :ws]), params[b],
                                  (352, 352), mean, std, 0)
        assert np.array_equal(x[b].cpu().numpy(), xr) and np.array_equal(y[b].cpu().numpy(), yr)
    x2, _ = aug(torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda(), src_hw=src_hw)   # sampled inside src_hw
    assert torch.isfinite(x2).all()


def test_augmented_batches_feed_training_steps():
    from lm_net_amd import LM_Net
    from lm_net_amd.data import DeviceAugment
    from lm_net_amd.loss import SegLoss
    from lm_net_amd.metrics import ConfusionMeter
    from lm_net_amd.optim import FusedAdamW
    rng = np.random.default_rng(9)
    for C, K, mode, mean, std in ((3, 2, "binary", MEAN3, STD3), (1, 9, "labels", MEAN1, STD1)):
        img = torch.from_numpy(rng.integers(0, 256, (2, 150, 170, C), dtype=np.uint8)).cuda()
        mask = torch.from_numpy(rng.integers(0, 256 if mode == "binary" else K, (2, 150, 170), dtype=np.uint8)).cuda()
        x, y = DeviceAugment((64, 96), mean, std, channels=C, mask_mode=mode, generator=C)(img, mask)
        torch.manual_seed(0)
        m = LM_Net(C, K).cuda().train()
        opt = FusedAdamW(m, lr=1e-3)
        loss = (SegLoss().cuda() if K == 2 else SegLoss(None, None))(m(x), y)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and all(torch.isfinite(p).all() for p in m.parameters())
        meter = ConfusionMeter(K)
        with torch.no_grad():
            meter.update(m(x), y)
        r = meter.compute()
        assert np.array(r["confusion"]).sum() == 2 * 64 * 96

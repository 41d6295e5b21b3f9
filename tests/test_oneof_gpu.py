"""GPU: lmn_augment_oneof_u8 through lm_net_amd.data.DeviceAugment(one_of=...) against the numpy restatement (tests/oneof_ref.py
composed with tests/augment_ref.py): normalised floats, labels and the contrast gray sums bit-exact, every member alone and mixed
batches, the plain path unchanged, ragged batches, and an augmented batch feeding a training step."""
import numpy as np
import pytest
import torch

import oneof_ref as R

pytestmark = pytest.mark.gpu

MEAN3, STD3 = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MEAN1, STD1 = (0.5,), (0.25,)
ONES = [1.0] * 6


def _frames(rng, B, hs, ws, C, mask_mode):
    img = rng.integers(0, 256, (B, hs, ws, C), dtype=np.uint8)
    img[:, : hs // 3] //= 3                                 # some structure: histograms, hue and contrast see non-uniform frames
    img[:, :, : ws // 4, 0] = 255 - img[:, :, : ws // 4, 0] // 5
    mask = rng.integers(0, 256 if mask_mode == "binary" else 64, (B, hs, ws), dtype=np.uint8)
    return img, mask


def _member_draws(rng, name):
    """Forced draws of one member: (description, dict) pairs covering its branches."""
    u = rng.uniform
    if name == "to_gray":
        return [{"op": name}]
    if name == "rgb_shift":
        return [{"op": name, "shift": [u(-20, 20), u(-20, 20), u(-20, 20)]}, {"op": name, "shift": [-255.0, 255.0, 0.0]}]
    if name == "channel_shuffle":
        return [{"op": name, "perm": p} for p in ([2, 0, 1], [1, 0, 2], [0, 1, 2])]
    if name == "hsv":
        return [{"op": name, "shift": [u(-20, 20), u(-30, 30), u(-20, 20)]}, {"op": name, "shift": [-179.5, 200.0, -100.0]}]
    if name == "grid_dropout":
        return [{"op": name, "ratio": 0.5}, {"op": name, "ratio": 0.9}]
    if name == "gaussian_blur":
        return [{"op": name, "k": k} for k in (3, 5, 7)]
    if name == "clahe":
        return [{"op": name, "clip": 1.0}, {"op": name, "clip": u(1, 4)}, {"op": name, "clip": 40.0}]
    if name == "grid_distortion":
        return [{"op": name, "num_steps": 5, "xsteps": list(1 + u(-0.3, 0.3, 6)), "ysteps": list(1 + u(-0.3, 0.3, 6))},
                {"op": name, "num_steps": 3, "xsteps": list(1 + u(-0.9, 0.9, 4)), "ysteps": ONES[:4]}]
    if name == "elastic":   # radius 12, and radius 16 > half of 32 rows (the periodic fold)
        return [{"op": name, "seed": 11, "alpha": 30.0, "sigma": 3.0}, {"op": name, "seed": 12, "alpha": 40.0, "sigma": 4.0}]
    raise KeyError(name)


def _check(aug, img, mask, params, size, mean, std, mm, src_hw=None):
    ti = None if img is None else torch.from_numpy(img).cuda()
    tm = None if mask is None else torch.from_numpy(mask).cuda()
    x, y = aug(ti, tm, params=params, src_hw=src_hw)
    torch.cuda.synchronize()
    xr, yr, gr = R.augment(img, mask, params, size, mean, std, mm, src_hw=src_hw)
    for b in range(len(params)):   # per sample first, so that a failure names the case
        if mask is not None:
            yg = y[b].cpu().numpy()
            assert np.array_equal(yg, yr[b]), (b, params[b].get("oneof"), int((yg != yr[b]).sum()))
        if img is not None:
            xg = x[b].cpu().numpy()
            assert np.array_equal(xg, xr[b]), (b, params[b].get("oneof"), int((xg != xr[b]).sum()), float(np.abs(xg - xr[b]).max()))
    if img is not None:
        assert np.array_equal(aug.last_gray_sum.cpu().numpy(), gr)
    return x, y


ALL = ("to_gray", "grid_distortion", "elastic", "clahe", "hsv", "channel_shuffle", "grid_dropout", "rgb_shift", "gaussian_blur")
GRAY_OK = ("grid_distortion", "elastic", "clahe", "grid_dropout", "gaussian_blur")


@pytest.mark.parametrize("size", [(32, 48), (36, 52)])
@pytest.mark.parametrize("C,mask_mode", [(3, "binary"), (1, "labels"), (3, "labels"), (1, "binary")])
@pytest.mark.parametrize("name", ALL)
def test_member_alone_matches_restatement(name, C, mask_mode, size):
    from lm_net_amd.data import DeviceAugment, ssr_matrix
    if C == 1 and name not in GRAY_OK:
        with pytest.raises(ValueError):
            DeviceAugment(size, MEAN1, STD1, channels=1, one_of=[name])
        return
    B, hs, ws = 3, 37, 53
    rng = np.random.default_rng(100 * ALL.index(name) + 10 * C + size[0])
    img, mask = _frames(rng, B, hs, ws, C, mask_mode)
    mean, std = (MEAN3, STD3) if C == 3 else (MEAN1, STD1)
    aug = DeviceAugment(size, mean, std, channels=C, mask_mode=mask_mode, one_of=[name])
    base = [{"crop": (0, 0, hs, ws)}, {"crop": (1, 2, hs - 3, ws - 4), "M": ssr_matrix(size[0], size[1], 20.0, 1.05, 0.05, -0.1), "flips": 1},
            {"crop": (0, 0, hs, ws), "cj": [1.1, 0.9, 1.2, 0.1], "order": [2, 0, 3, 1], "flips": 2}]
    draws = _member_draws(rng, name)
    for shift in range(len(draws)):    # every draw meets every base sample at most once per call: the whole batch on this member
        params = [dict(base[b], oneof=draws[(b + shift) % len(draws)]) for b in range(B)]
        _check(aug, img, mask, params, size, mean, std, DeviceAugment.MASK_MODES[mask_mode])


def test_mixed_reference_batch_matches_restatement():
    from lm_net_amd.data import DeviceAugment
    B, hs, ws, size = 11, 120, 150, (64, 96)
    rng = np.random.default_rng(21)
    img, mask = _frames(rng, B, hs, ws, 3, "binary")
    # the reference's elastic defaults are the identity (tests/test_oneof_cpu.py); sample them with a field that moves pixels
    members = [m if m != "elastic" else ("elastic", {"alpha": 40.0, "sigma": 4.0}) for m in ALL]
    for one_of, seed in (("reference", 3), (members, 4)):
        aug = DeviceAugment(size, generator=seed, p_ssr=0.7, p_cj=0.7, one_of=one_of, p_oneof=1.0)
        params = aug.sample_dicts(B, (hs, ws))
        assert all(p["oneof"] is not None for p in params) and len({p["oneof"]["op"] for p in params}) >= 5
        _check(aug, img, mask, params, size, MEAN3, STD3, 0)


def test_multi_block_352():
    """352 x 352: 121 blur tiles per sample, CLAHE tiles of 44 x 44 pixels (8 strides of the histogram loop); every member once."""
    from lm_net_amd.data import DeviceAugment
    hs, ws, size = 100, 80, (352, 352)
    rng = np.random.default_rng(33)
    aug = DeviceAugment(size, generator=8, one_of="reference", p_oneof=1.0)
    for pair in (("gaussian_blur", "clahe"), ("grid_distortion", "hsv")):
        img, mask = _frames(rng, 2, hs, ws, 3, "binary")
        params = aug.sample_dicts(2, (hs, ws))
        draws = []
        for name in pair:
            d = _member_draws(rng, name)
            draws.append(d[-1] if name != "clahe" else d[1])
        params = [dict(p, oneof=d) for p, d in zip(params, draws)]
        _check(aug, img, mask, params, size, MEAN3, STD3, 0)
    sampled = aug.sample_dicts(2, (hs, ws))                 # and two members as the sampler draws them
    _check(aug, img, mask, sampled, size, MEAN3, STD3, 0)


def test_p_oneof_zero_equals_the_plain_entry():
    from lm_net_amd.data import DeviceAugment
    rng = np.random.default_rng(1)
    img, mask = _frames(rng, 4, 120, 150, 3, "binary")
    ti, tm = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()
    plain = DeviceAugment((96, 96), generator=3, p_ssr=1.0, p_cj=1.0)
    x0, y0 = plain(ti, tm)
    g0 = plain.last_gray_sum.clone()
    aug = DeviceAugment((96, 96), generator=3, p_ssr=1.0, p_cj=1.0, one_of="reference", p_oneof=0.0)
    x1, y1 = aug(ti, tm, params=plain.last_params)                                   # packed parameters: no member fires
    assert all(q.op == 0 for q in aug.last_oneof[0])
    assert torch.equal(x0.view(torch.int32), x1.view(torch.int32)) and torch.equal(y0, y1) and torch.equal(g0, aug.last_gray_sum)
    x2, y2 = aug(ti, tm)                                                             # sampled with p_oneof = 0
    assert all(q.op == 0 for q in aug.last_oneof[0]) and bool(torch.isfinite(x2).all())


def test_repeat_ragged_and_partial_calls():
    from lm_net_amd.data import DeviceAugment
    rng = np.random.default_rng(5)
    sizes = [(120, 150), (61, 150), (120, 47), (90, 100), (33, 41)]
    B = len(sizes)
    img = np.full((B, 120, 150, 3), 255, dtype=np.uint8)    # padding that must never be read
    mask = np.full((B, 120, 150), 200, dtype=np.uint8)
    for b, (hs, ws) in enumerate(sizes):
        fi, fm = _frames(rng, 1, hs, ws, 3, "binary")
        img[b, :hs, :ws], mask[b, :hs, :ws] = fi[0], fm[0]
    src_hw = np.array(sizes, dtype=np.int32)
    members = [m if m != "elastic" else ("elastic", {"alpha": 30.0, "sigma": 3.0}) for m in ALL]
    aug = DeviceAugment((64, 96), generator=17, p_ssr=0.8, p_cj=0.8, one_of=members, p_oneof=1.0)
    params = aug.sample_dicts(B, src_hw)
    for b, name in enumerate(("elastic", "grid_distortion", "clahe", "gaussian_blur")):       # the members with buffers of their own
        params[b]["oneof"] = _member_draws(rng, name)[0]
    x, y = _check(aug, img, mask, params, (64, 96), MEAN3, STD3, 0, src_hw=src_hw)
    ti, tm = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()
    x2, y2 = aug(ti, tm, params=params, src_hw=src_hw)      # the same parameters again
    assert torch.equal(x.view(torch.int32), x2.view(torch.int32)) and torch.equal(y, y2)
    xo, none = aug(ti, None, params=params, src_hw=src_hw)  # images only / masks only
    assert none is None and torch.equal(xo.view(torch.int32), x.view(torch.int32))
    none, yo = aug(None, tm, params=params, src_hw=src_hw)
    assert none is None and torch.equal(yo, y)


def test_oneof_batch_feeds_a_training_step():
    from lm_net_amd import LM_Net
    from lm_net_amd.data import DeviceAugment
    from lm_net_amd.loss import SegLoss
    from lm_net_amd.optim import FusedAdamW
    rng = np.random.default_rng(9)
    img = torch.from_numpy(rng.integers(0, 256, (4, 150, 170, 3), dtype=np.uint8)).cuda()
    mask = torch.from_numpy(rng.integers(0, 256, (4, 150, 170), dtype=np.uint8)).cuda()
    x, y = DeviceAugment((64, 96), generator=3, one_of="reference", p_oneof=1.0)(img, mask)
    torch.manual_seed(0)
    m = LM_Net(3, 2).cuda().train()
    opt = FusedAdamW(m, lr=1e-3)
    loss = SegLoss().cuda()(m(x), y)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and all(torch.isfinite(p).all() for p in m.parameters())

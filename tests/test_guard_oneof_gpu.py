"""GPU: lmn_augment_oneof_u8 inside guard bands (tests/guard.py): the guard manifest's test of the entry, which it reaches through
DeviceAugment (the launch log below names the wrapper).  One mixed batch containing every member, every buffer of the call carved
from a GuardPool at its exact size -- frames, masks, both parameter tables, the uploaded host tables, the LAB tables, both scratches,
the label copy, the gray sums, the workspace at exactly lmn_oneof_workspace bytes, out and labels -- with canaries flush against
each."""
import numpy as np
import pytest
import torch

from guard import GuardPool, LaunchLog

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


class _PoolTorch:
    """Stands in for the `torch` global of lm_net_amd.data: `torch.empty` on the device carves from the pool at the exact size."""

    def __init__(self, pool):
        self._pool = pool

    def __getattr__(self, name):
        real = getattr(torch, name)
        if name != "empty":
            return real
        pool = self._pool

        def empty(*a, **k):
            t = real(*a, **k)
            return pool.take("empty#%d %s %s" % (len(pool.entries), tuple(t.shape), t.dtype), t.shape, t.dtype) if t.is_cuda else t
        return empty


@pytest.mark.parametrize("channels", [3, 1])
def test_augment_oneof_u8_every_member(channels, monkeypatch):
    from lm_net_amd import data, hip
    members = [m for m in data.ONEOF_REFERENCE if channels == 3 or m not in data.ONEOF_COLOUR]
    B, Hs, Ws, H, W = len(members) + 1, 41, 59, 36, 52
    g = torch.Generator().manual_seed(7)
    img = torch.randint(0, 256, (B, Hs, Ws, channels), generator=g).to(torch.uint8).to(DEV)
    msk = torch.randint(0, 5, (B, Hs, Ws), generator=g).to(torch.uint8).to(DEV)
    hw = np.array([[Hs - (b % 3) * 4, Ws - (b % 4) * 5] for b in range(B)], dtype=np.int64)
    mean, std = (0.4, 0.5, 0.6)[:channels], (0.2, 0.25, 0.3)[:channels]
    draws = {"to_gray": {}, "rgb_shift": {"shift": [3.5, -20.0, 11.0]}, "channel_shuffle": {"perm": [1, 2, 0]},
             "hsv": {"shift": [-7.0, 12.5, 19.0]}, "grid_dropout": {"ratio": 0.5}, "gaussian_blur": {"k": 7}, "clahe": {"clip": 2.5},
             "grid_distortion": {"num_steps": 5, "xsteps": [1.2, 0.8, 1.3, 0.7, 1.1, 1.0], "ysteps": [0.75, 1.25, 1.0, 1.3, 0.9, 1.0]},
             "elastic": {"seed": 5, "alpha": 40.0, "sigma": 4.0}}

    def run(img_t, msk_t):
        aug = data.DeviceAugment((H, W), mean=mean, std=std, channels=channels, mask_mode="labels", generator=11, p_ssr=0.7, p_cj=0.7,
                                 one_of=members)
        params = aug.sample_dicts(B, hw)
        for p, m in zip(params, members + [None]):              # every member once, and one sample without
            p["oneof"] = None if m is None else dict(draws[m], op=m)
        return aug, aug(img_t, msk_t, params=params, src_hw=hw)

    _, (x0, y0) = run(img.clone(), msk.clone())
    torch.cuda.synchronize()
    pool = GuardPool(DEV, 8 << 20)
    img_t, msk_t = pool.take("images", None, None, init=img), pool.take("masks", None, None, init=msk)
    monkeypatch.setattr(data, "torch", _PoolTorch(pool))
    with LaunchLog() as log:
        aug, (x1, y1) = run(img_t, msk_t)
    pool.assert_clean("augment_oneof_u8")
    pool.assert_inputs_unchanged()
    assert log.names == ["augment_oneof_u8"]
    sizes = [e[2] for e in pool.entries]
    n_px = B * H * W
    want = [hip.oneof_workspace(B, H, W, channels, 1), n_px * channels, n_px * 8, B * 72, B * 176, 4 * aug.last_oneof[1].size]
    assert all(w in sizes for w in want), (want, sizes)
    assert sizes.count(n_px * channels) == 2 and sizes.count(n_px * 8) == 2          # both scratches; labels and their copy
    assert (channels == 3) == (4 * hip.LAB_TABLE_INTS in sizes)
    assert len(pool.entries) == (13 if channels == 3 else 12)
    assert torch.equal(x0.view(torch.int32), x1.view(torch.int32)) and torch.equal(y0, y1) and bool(torch.isfinite(x1).all())

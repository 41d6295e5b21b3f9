"""GPU: lmn_mix_batch behind lm_net_amd.data.DeviceMix against the numpy fp32 restatement soft_ref.mix: x_out, ya, yb and lam_out
bit-equal.  The Mixup expression is evaluated unfused on the device (fadd(fmul(lam, a), fmul(1 - lam, b)) with the host's fp32
1 - lam), so contraction cannot change a bit and equality, not a tolerance, is the bar.  Shapes: one sample whose partner is itself,
W % 4 == 0 (16-byte loads) and odd W (scalar), several blocks per plane; both label types; rows mixing all three modes in one batch;
boxes touching every edge, empty and full; yb = NULL with no mixup row."""
import numpy as np
import pytest
import torch

import soft_ref as R
from kernel_forms import launched

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SHAPES = [(1, 1, 2, 2), (4, 3, 16, 20), (3, 3, 9, 11), (5, 16, 32, 36), (2, 1, 33, 31)]


def _boxes(B, H, W):
    """boxes touching every edge, an empty one and the full image, in turn"""
    all_ = [(0, 0, H // 2 + 1, W // 2 + 1), (H // 2, W // 2, H, W), (0, W // 3, H, W - W // 3), (H // 3, 0, H - H // 3, W), (H // 2, W // 2, H // 2, W // 2),
            (0, 0, H, W), (1 % H, 1 % W, H, W)]
    return [all_[b % len(all_)] for b in range(B)]


def _case(shape, dtype, seed, modes):
    from lm_net_amd import hip
    B, Cin, H, W = shape
    rng = np.random.default_rng(seed)
    x = (3.0 * rng.standard_normal(shape)).astype(np.float32)
    y = rng.integers(0, 9, (B, H, W)).astype(dtype)
    y[rng.random(y.shape) < 0.2] = R.VOID
    lam = rng.random(B).astype(np.float32)
    lam[0] = (np.float32(0.0), np.float32(1.0), np.float32(1.0 / 3.0))[seed % 3]
    rows = hip.mix_rows(rng.permutation(B), [modes[b % len(modes)] for b in range(B)], lam, _boxes(B, H, W))
    return x, y, rows


def _equal(got, want, what):
    for name, g, w in zip(("x_out", "ya", "yb", "lam"), got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name, np.abs(g.astype(np.float64) - w).max())


@pytest.mark.parametrize("dtype", [np.uint8, np.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mix_equals_the_restatement_bit_for_bit(shape, dtype):
    from lm_net_amd import DeviceMix
    B, Cin, H, W = shape
    mixer = DeviceMix(mixup_alpha=0.4, cutmix_alpha=1.0, generator=1)
    for seed, modes in enumerate([(R.MIXUP, R.CUTMIX, R.NONE), (R.CUTMIX, R.MIXUP), (R.MIXUP,), (R.CUTMIX,), (R.NONE,)]):
        x, y, rows = _case(shape, dtype, seed, modes)
        (xo, t), names = launched(lambda: mixer.mix(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), rows=rows))
        assert not t.hard and any(n.startswith("mix_batch_kernel<%s>" % ("true" if W % 4 == 0 else "false")) for n in names), sorted(names)
        _equal((xo, t.ya, t.yb, t.lam), R.mix(x, y, rows), (shape, modes))
    # drawn rows
    x, y, _ = _case(shape, dtype, 9, (R.NONE,))
    rows = mixer.sample(B, H, W)
    xo, t = mixer.mix(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), rows=rows)
    _equal((xo, t.ya, t.yb, t.lam), R.mix(x, y, rows), (shape, "drawn"))


@pytest.mark.parametrize("shape", SHAPES[1:3], ids=lambda s: "x".join(map(str, s)))
def test_cutmix_only_gives_a_hard_label_map(shape):
    """mixup_alpha = 0: no row is a mixup row, the entry gets yb = NULL, ya == yb, lam == 1 and target.labels is the label map, void
    labels included."""
    from lm_net_amd import DeviceMix
    B, Cin, H, W = shape
    mixer = DeviceMix(mixup_alpha=0.0, cutmix_alpha=1.0, generator=2)
    x, y, rows = _case(shape, np.int64, 4, (R.CUTMIX, R.NONE))
    xo, t = mixer.mix(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), rows=rows)
    want = R.mix(x, y, rows)
    assert t.hard and t.yb is t.ya and t.labels is t.ya
    _equal((xo, t.ya, t.yb, t.lam), want, shape)
    assert (want[1] == R.VOID).any() and bool((t.lam == 1).all())
    soft = DeviceMix(mixup_alpha=0.4, generator=2).mix(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))[1]
    with pytest.raises(ValueError, match="can draw Mixup"):
        soft.labels

"""GPU: the two entries of include/volume/lmnet_volume.h that write device memory, lmn_volume_labels and lmn_volume_dist, inside guard
bands (tests/guard.py): the guard manifest's tests of these entries.  Every buffer -- the logits or labels, the target, the two uint8
case buffers, the workspace at exactly lmn_volume_workspace bytes and the statistics -- is carved from a GuardPool at its exact
size, canaries flush against each.  The shapes are two of tests/test_volume_kernels_gpu.py: (3, 5, 70), where x crosses a 64-lane
boundary and no row ends on a 4-byte boundary of the uint16 / uint8 arrays, and (17, 66, 130)."""
import numpy as np
import pytest
import torch

import volume_ref as R
from guard import LaunchLog, pools

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SHAPES = [(3, 5, 70), (17, 66, 130)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", ["logits", "labels"])
def test_volume_labels_entry(form, shape):
    """The last n slices of a case buffer of D slices: the entry writes slices [z0, D) of both buffers and not a byte before them."""
    from lm_net_amd import hip
    D, H, W = shape
    C, n = 5, 2
    z0 = D - n
    rng = np.random.default_rng(D + H)
    target = rng.integers(-1, C + 1, (n, H, W))                      # -1 and C belong to no class
    if form == "logits":
        pred = rng.integers(0, 3, (n, C, H, W)).astype(np.float32)    # three values: ties in most voxels
        want = pred.argmax(1)
    else:
        pred = rng.integers(-2, C + 2, (n, H, W))
        want = np.where((pred >= 0) & (pred < C), pred, 255)
    inputs = dict(pred=torch.from_numpy(pred), target=torch.from_numpy(target))
    outputs = dict(lab_pred=((D, H, W), torch.uint8), lab_target=((D, H, W), torch.uint8))

    def run(x):
        hip.volume_labels(x["pred"], x["target"], C, x["lab_pred"], x["lab_target"], z0)
        torch.cuda.synchronize()

    plain, pool, guarded = pools(inputs, outputs, DEV, fill="poison")
    run(plain)
    guarded["lab_pred"].fill_(0xFF)
    guarded["lab_target"].fill_(0xFF)
    with LaunchLog(pool) as log:
        run(guarded)
    pool.assert_clean("volume_labels entry")
    pool.assert_inputs_unchanged()
    assert log.names == ["volume_labels"]
    got = {e[0]: e[2] for e in pool.entries}
    assert got == {k: v.numel() * v.element_size() for k, v in plain.items()} and got["lab_pred"] == D * H * W
    for k, w in (("lab_pred", want), ("lab_target", np.where((target >= 0) & (target < C), target, 255))):
        assert torch.equal(plain[k], guarded[k])
        g = guarded[k].cpu().numpy()
        assert np.array_equal(g[z0:], w) and (g[:z0] == 0xFF).all(), k   # the slices before z0 keep their fill


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_volume_dist_entry(shape):
    from lm_net_amd import hip
    D, H, W = shape
    C, spacing = 4, (3, 1, 2)
    classes = [1, 2, 3]
    pred, target = R.ellipsoid_case(D, H, W, C)
    ws_bytes = hip.volume_workspace(D, H, W, len(classes))
    inputs = dict(lab_pred=torch.from_numpy(pred.astype(np.uint8)), lab_target=torch.from_numpy(target.astype(np.uint8)))
    outputs = dict(workspace=((ws_bytes,), torch.uint8), stats_i=((len(classes), 9), torch.int64), stats_f=((len(classes), 2), torch.float64))

    def run(x):
        hip.volume_dist(x["lab_pred"], x["lab_target"], C, classes, spacing, x["workspace"], x["stats_i"], x["stats_f"])
        torch.cuda.synchronize()

    plain, pool, guarded = pools(inputs, outputs, DEV, fill="poison")
    run(plain)
    with LaunchLog(pool) as log:
        run(guarded)
    pool.assert_clean("volume_dist entry")
    pool.assert_inputs_unchanged()
    assert log.names == ["volume_dist"]
    got = {e[0]: e[2] for e in pool.entries}
    assert got == {k: v.numel() * v.element_size() for k, v in plain.items()}     # exact sizes: nothing is rounded up
    assert got["workspace"] == ws_bytes and got["stats_i"] == 72 * len(classes) and got["stats_f"] == 16 * len(classes)
    assert torch.equal(plain["stats_i"], guarded["stats_i"])                     # identical to ordinary allocations, poisoned scratch or not
    assert torch.equal(plain["stats_f"].view(torch.int64), guarded["stats_f"].view(torch.int64))
    # ... and the right values, so that the guarded run is the real one
    si, sf, _ = R.case_stats(pred, target, classes, spacing)
    assert (si[:, 0] > 0).all() and (si[:, 1] > 0).all()
    assert np.array_equal(guarded["stats_i"].cpu().numpy(), si)
    assert np.allclose(guarded["stats_f"].cpu().numpy(), sf, rtol=1e-9, atol=0)

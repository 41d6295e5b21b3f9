"""GPU: the three entries of include/distmap/lmnet_distmap.h that write device memory -- lmn_dist_map, lmn_dist_loss_fwd,
lmn_dist_loss_bwd -- inside guard bands (tests/guard.py): the guard manifest's tests of these entries.  Every buffer -- the source,
the workspace at exactly lmn_dist_workspace bytes, sd2, flags, the sums, the loss and dlogits -- is carved from a GuardPool at its
exact size, canaries flush against each, and every body the entries write starts filled with junk (0xA5 bytes: a large negative int32,
a finite negative float).  The shapes are two of tests/test_distmap_kernels_gpu.py: 37 x 45 (odd tails, one column block) and
130 x 67 (three 64-row groups, a second column block of three live lanes)."""
import numpy as np
import pytest
import torch

import distmap_ref as R
from guard import LaunchLog, pools, sizes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SHAPES = [(37, 45), (130, 67)]


@pytest.mark.parametrize("source", ["labels", "softmax", "sigmoid"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dist_map_entry(shape, source):
    """The masks, the column pass and the row pass with the scratch at its exact size: the maps equal those of ordinary allocations
    and the restatement."""
    from lm_net_amd import hip
    H, W = shape
    C, classes, mask = 5, [1, 3], 0b1010
    y = R.label_batch(H, W, C, classes, seed=2)
    B, nk = y.shape[0], len(classes)
    want = R.maps(R.masks_of_labels(y, classes))
    ws_bytes = hip.dist_workspace(B, nk, H, W)
    src = torch.from_numpy(y) if source == "labels" else torch.from_numpy(R.logits_of_labels(y, C, source))
    mode = {"labels": None, "softmax": hip.DISTMAP_SOFTMAX, "sigmoid": hip.DISTMAP_SIGMOID}[source]
    thr = 0.5 if source == "softmax" else 0.0
    outputs = dict(workspace=((ws_bytes,), torch.uint8), sd2=((B, nk, H, W), torch.int32), flags=((B, nk), torch.int32))

    def run(x):
        hip.dist_map(x["src"], C, mask, x["workspace"], x["sd2"], x["flags"], mode=mode, threshold=thr)
        torch.cuda.synchronize()

    plain, pool, guarded = pools(dict(src=src), outputs, DEV, fill="junk")
    run(plain)
    with LaunchLog(pool) as log:
        run(guarded)
    pool.assert_clean("dist_map entry")
    pool.assert_inputs_unchanged()
    assert log.names == ["dist_map"]
    got = sizes(pool, plain)
    up = lambda v: (v + 255) // 256 * 256
    assert got["workspace"] == ws_bytes == up(B * nk * H * W) + up(2 * B * nk * H * W) + up(4 * B * nk)
    assert got["sd2"] == 4 * B * nk * H * W and got["flags"] == 4 * B * nk
    for name, w in zip(("sd2", "flags"), want):
        assert torch.equal(plain[name], guarded[name]), name
        assert np.array_equal(guarded[name].cpu().numpy(), w), name              # ... the right values: the guarded run is the real one
    assert sorted(set(want[1].ravel().tolist())) == [0, 1, 2]


@pytest.mark.parametrize("head,term,C", [("softmax", "boundary", 2), ("softmax", "hausdorff", 5), ("sigmoid", "hausdorff", 3),
                                         ("sigmoid", "boundary", 1)])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dist_loss_entries(shape, head, term, C):
    """Forward and backward of one term with sums, loss and dlogits at their exact sizes and junk in them: the same bits as with
    ordinary allocations (deterministic mode: the partials go through slots of the library's own scratch, not through these
    buffers), and the values of the restatement."""
    from lm_net_amd import hip
    H, W = shape
    classes = R.default_classes(C)
    mask = sum(1 << k for k in classes)
    lg, y = R.loss_inputs(2, C, H, W, head, seed=5, void=True)
    alpha = 2.0
    want, wgrad, n, mag, near = R.loss_and_grad(lg, y, head, term, classes, alpha=alpha, scale=0.5, gscale=0.37)
    assert near == 0 and n > 0
    sd2_g = torch.from_numpy(R.maps(R.target_masks(y, head, classes))[0])
    inputs = dict(logits=torch.from_numpy(lg), target=torch.from_numpy(y), sd2_g=sd2_g, gscale=torch.tensor([0.37]))
    if term == "hausdorff":
        inputs["sd2_p"] = torch.from_numpy(R.prediction_maps(lg, head, classes)[0])
    outputs = dict(sums=((hip.DISTMAP_SUMS_WORDS,), torch.int32), loss=((1,), torch.float32), dlogits=(lg.shape, torch.float32))
    hd = hip.DISTMAP_SOFTMAX if head == "softmax" else hip.DISTMAP_SIGMOID
    tm = hip.DISTMAP_BOUNDARY if term == "boundary" else hip.DISTMAP_HAUSDORFF

    def run(x):
        hip.dist_loss_fwd(x["logits"], x["target"], hd, tm, alpha, 0.5, mask, x["sd2_g"], x.get("sd2_p"), x["sums"], x["loss"])
        hip.dist_loss_bwd(x["logits"], x["target"], hd, tm, alpha, mask, x["sd2_g"], x.get("sd2_p"), x["sums"], x["gscale"], x["dlogits"])
        torch.cuda.synchronize()

    hip.set_deterministic(True)
    try:
        plain, pool, guarded = pools(inputs, outputs, DEV, fill="junk")
        run(plain)
        with LaunchLog(pool) as log:
            run(guarded)
    finally:
        hip.set_deterministic(False)
    pool.assert_clean("dist_loss entries")
    pool.assert_inputs_unchanged()
    assert log.names == ["dist_loss_fwd", "dist_loss_bwd"]
    got = sizes(pool, plain)
    assert got["sums"] == 16 and got["loss"] == 4 and got["dlogits"] == 4 * lg.size
    for name in outputs:
        assert torch.equal(plain[name].view(torch.uint8), guarded[name].view(torch.uint8)), name
    assert int(guarded["sums"][0]) == n and int(guarded["sums"][3]) == 0
    loss = float(guarded["loss"][0])
    assert abs(loss - want) < 1e-5 * (mag if term == "boundary" else abs(want)), (loss, want)
    d = guarded["dlogits"].cpu().numpy().astype(np.float64)
    assert np.abs(d - wgrad).max() < 1e-4 * np.abs(wgrad).max()

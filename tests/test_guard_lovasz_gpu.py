"""GPU: the three entries of include/lovasz/lmnet_lovasz.h that write device memory -- lmn_lovasz_order, lmn_lovasz_fwd,
lmn_lovasz_bwd -- inside guard bands (tests/guard.py): the guard manifest's tests of these entries.  Every buffer -- the keys or the
logits and the target, the workspace at exactly lmn_lovasz_workspace bytes, errors, perm, counts, coef, the sums, the loss and
dlogits -- is carved from a GuardPool at its exact size, canaries flush against each, and every body the entries write starts filled
with junk (0xA5 bytes).  The lengths straddle the sort tile: one short tile, and three tiles with a tail of 17."""
import numpy as np
import pytest
import torch

import lovasz_ref as R
from guard import LaunchLog, pools, sizes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.mark.parametrize("S,P", [(3, 257), (2, 3 * 2048 + 17)])
def test_lovasz_order_entry(S, P):
    """The twelve launches of the sort with the scratch at its exact size: the order equals that of ordinary allocations and
    np.lexsort, and the keys are not modified."""
    from lm_net_amd import hip
    rng = np.random.default_rng(S)
    keys = rng.integers(0, 1 << 32, (S, P), dtype=np.uint64).astype(np.uint32)
    keys[:, ::3] &= 0xFF00FF00                               # ties in two digits
    ws_bytes = hip.lovasz_workspace(S, P)
    outputs = dict(workspace=((ws_bytes,), torch.uint8), perm=((S, P), torch.int32))

    def run(x):
        hip.lovasz_order(x["keys"], x["workspace"], x["perm"])
        torch.cuda.synchronize()

    plain, pool, guarded = pools(dict(keys=torch.from_numpy(keys.view(np.int32))), outputs, DEV, fill="junk")
    run(plain)
    with LaunchLog(pool) as log:
        run(guarded)
    pool.assert_clean("lovasz_order entry")
    pool.assert_inputs_unchanged()
    assert log.names == ["lovasz_order"]
    got = sizes(pool, plain)
    assert got["workspace"] == ws_bytes and got["perm"] == 4 * S * P
    assert torch.equal(plain["perm"], guarded["perm"])
    idx = np.arange(P)
    want = np.stack([np.lexsort((idx, keys[s])) for s in range(S)])
    assert np.array_equal(guarded["perm"].cpu().numpy(), want)


@pytest.mark.parametrize("head,C,classes,per_image", [("softmax", 3, "present", False), ("softmax", 5, [1, 3], True), ("sigmoid", 2, "all", False),
                                                      ("sigmoid", 1, "all", True)])
@pytest.mark.parametrize("shape", [(2, 13, 19), (3, 45, 47)], ids=lambda s: "x".join(map(str, s)))
def test_lovasz_loss_entries(shape, head, C, classes, per_image):
    """Forward and backward with every buffer at its exact size and junk in it: the same bits as with ordinary allocations, and the
    values of the restatement on the device's order."""
    from lm_net_amd import hip
    B, H, W = shape
    ids, present = R.class_ids(C, head, classes)
    mask, nk = sum(1 << k for k in ids), len(ids)
    lg, y = R.inputs(B, C, H, W, head, seed=5, void=0.2)
    S, P = hip.lovasz_segments(B, nk, H, W, per_image)
    hd = hip.LOVASZ_SOFTMAX if head == "softmax" else hip.LOVASZ_SIGMOID
    inputs = dict(logits=torch.from_numpy(lg), target=torch.from_numpy(y), gscale=torch.tensor([0.5]))
    outputs = dict(workspace=((hip.lovasz_workspace(S, P),), torch.uint8), errors=((S, P), torch.float32), perm=((S, P), torch.int32),
                   counts=((S, 2), torch.int32), coef=((B, nk, H, W), torch.float32), sums=((hip.LOVASZ_SUMS_WORDS,), torch.int32),
                   loss=((1,), torch.float32), dlogits=(lg.shape, torch.float32))

    def run(x):
        hip.lovasz_fwd(x["logits"], x["target"], hd, per_image, present, mask, 0.25, x["workspace"], x["errors"], x["perm"], x["counts"],
                       x["coef"], x["sums"], x["loss"])
        hip.lovasz_bwd(x["logits"], x["target"], hd, mask, x["coef"], x["sums"], x["gscale"], x["dlogits"])
        torch.cuda.synchronize()

    plain, pool, guarded = pools(inputs, outputs, DEV, fill="junk")
    run(plain)
    with LaunchLog(pool) as log:
        run(guarded)
    pool.assert_clean("lovasz loss entries")
    pool.assert_inputs_unchanged()
    assert log.names == ["lovasz_fwd", "lovasz_bwd"]
    got = sizes(pool, plain)
    assert got["sums"] == 16 and got["loss"] == 4 and got["dlogits"] == 4 * lg.size and got["counts"] == 8 * S
    for name in outputs:
        if name != "workspace":
            assert torch.equal(plain[name].view(torch.uint8), guarded[name].view(torch.uint8)), name
    perm = guarded["perm"].cpu().numpy()
    want, wgrad, counts, _ = R.loss_and_grad(lg, y, C, head, classes, per_image, scale=0.25, gscale=0.5, order=perm)
    assert np.array_equal(guarded["counts"].cpu().numpy(), counts)
    loss = float(guarded["loss"][0])
    assert abs(loss - want) < 1e-5 * abs(want), (loss, want)
    d = guarded["dlogits"].cpu().numpy().astype(np.float64)
    assert np.abs(d - wgrad).max() < 1e-4 * np.abs(wgrad).max()

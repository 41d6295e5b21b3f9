"""GPU: the two entries of include/region/lmnet_region.h that write device memory -- lmn_region_fwd, lmn_region_bwd -- inside guard
bands (tests/guard.py): the guard manifest's test of these entries.  Every buffer -- the logits and the target, the workspace at
exactly lmn_region_workspace bytes, sums, counts, coef, per_class, the loss and dlogits -- is carved from a GuardPool at its exact size,
canaries flush against each, and every body the entries write starts filled with junk (0xA5 bytes).  The shapes are the smallest
templated one, the smallest general-C one and the scalar sigmoid one, in ordinary and in deterministic mode."""
import numpy as np
import pytest
import torch

import region_ref as R
from guard import JUNK, LaunchLog, pools, sizes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("head,shape,kind,den,classes,per_image", [
    ("softmax", (1, 2, 1, 1), "dice", "squared", None, False),                  # the smallest templated shape
    ("softmax", (2, 2, 5, 7), "tversky", "linear", [1], True),
    ("softmax", (2, 5, 3, 3), "jaccard", "squared", [1, 3], True),              # the smallest general-C shape: C = 5
    ("softmax", (2, 5, 3, 3), "generalized_dice", "linear", None, False),
    ("sigmoid", (2, 1, 5, 7), "dice", "linear", None, True),                    # odd H * W: the scalar sigmoid route
    ("sigmoid", (2, 3, 5, 7), "jaccard", "squared", [0, 2], False)])
def test_region_loss_entries(head, shape, kind, den, classes, per_image, det):
    """Forward and backward with every buffer at its exact size and junk in it: the same bits as with ordinary allocations (in
    deterministic mode; the counts in either), and the values of the restatement."""
    from lm_net_amd import hip
    from lm_net_amd.loss import _REGION_DENOMINATORS, _REGION_HEADS, _REGION_KINDS
    B, C, H, W = shape
    ids = R.class_ids(C, classes)
    mask, nk, G = sum(1 << k for k in ids), len(ids), (B if per_image else 1)
    lg, y = R.inputs(B, C, H, W, head, seed=5, void=0.2)
    hd = _REGION_HEADS[head]
    ws_bytes = hip.region_workspace(hd, B, C, H, W, mask)
    inputs = dict(logits=torch.from_numpy(lg), target=torch.from_numpy(y), gscale=torch.tensor([0.5]))
    outputs = dict(workspace=((ws_bytes,), torch.uint8), sums=((G, nk, 3), torch.float32), counts=((G, nk, 2), torch.int32),
                   coef=((G, nk, 3), torch.float32), per_class=((G, nk), torch.float32), loss=((1,), torch.float32), dlogits=(lg.shape, torch.float32))

    def run(x):
        hip.region_fwd(x["logits"], x["target"], hd, _REGION_KINDS[kind], _REGION_DENOMINATORS[den], per_image, 0.3, 0.7, 1e-5, 0.75, 0.25, mask,
                       None, x["workspace"], x["sums"], x["counts"], x["coef"], x["per_class"], x["loss"])
        hip.region_bwd(x["logits"], x["target"], hd, per_image, mask, x["coef"], x["gscale"], x["dlogits"])
        torch.cuda.synchronize()

    was = hip.get_deterministic()
    hip.set_deterministic(det)
    try:
        plain, pool, guarded = pools(inputs, outputs, DEV, fill="junk")
        run(plain)
        with LaunchLog(pool) as log:
            run(guarded)
    finally:
        hip.set_deterministic(was)
    pool.assert_clean("region loss entries")
    pool.assert_inputs_unchanged()
    assert log.names == ["region_fwd", "region_bwd"]
    got = sizes(pool, plain)
    assert got["workspace"] == ws_bytes and got["loss"] == 4 and got["dlogits"] == 4 * lg.size and got["counts"] == 8 * G * nk
    assert torch.equal(plain["counts"], guarded["counts"])
    if det:
        for name in outputs:
            if name != "workspace":
                assert torch.equal(plain[name].view(torch.uint8), guarded[name].view(torch.uint8)), name
    else:                                                  # the workspace is neither read nor written outside deterministic mode
        assert bool((guarded["workspace"] == JUNK).all())
    r = R.loss_and_grad(lg, y, C, kind=kind, head=head, classes=classes, per_image=per_image, denominator=den, smooth=1e-5, alpha=0.3, beta=0.7,
                        exponent=0.75, scale=0.25, gscale=0.5)
    assert np.array_equal(guarded["counts"].cpu().numpy(), r.counts)
    loss = float(guarded["loss"][0])
    assert abs(loss - r.loss) <= 1e-5 * abs(r.loss), (loss, r.loss)
    d = guarded["dlogits"].cpu().numpy().astype(np.float64)
    assert np.abs(d - r.grad).max() <= 1e-4 * np.abs(r.grad).max()

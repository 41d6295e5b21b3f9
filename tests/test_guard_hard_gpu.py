"""GPU: the two entries of include/hard/lmnet_hard.h that write device memory -- lmn_hard_fwd, lmn_hard_bwd -- inside guard bands
(tests/guard.py): the guard manifest's tests of these entries.  Every buffer -- the logits, the target, the class weights, the
workspace at exactly lmn_hard_workspace bytes, values, selection, terms, loss and dlogits -- is carved from a GuardPool at its exact
size, canaries flush against each, and every body the entries write starts filled with junk (0xA5 bytes; the workspace too: the entry
zeroes the tables it accumulates in).  The instances are those of tests/test_hard_kernels_gpu.py: the templated class counts 2, 3, 4
and 8, the general ones 5 and 64 (LDS-staged in the backward), the vector sigmoid route at 1 and 3 planes and the scalar one at 7 x 9; per batch and per image."""
import numpy as np
import pytest
import torch

import hard_ref as R
from guard import LaunchLog, pools

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


INSTANCES = [("softmax", (1, 2, 1, 1), dict(keep=0.5)),                       # the smallest templated shape
             ("softmax", (2, 2, 5, 7), dict(keep=0.1, min_kept=3)),
             ("softmax", (2, 3, 5, 7), dict(thresh=0.7, min_kept=5)),
             ("softmax", (2, 4, 24, 40), dict(keep=0.25)),                   # several blocks
             ("softmax", (2, 8, 5, 8), dict(min_kept=11)),
             ("softmax", (2, 5, 3, 3), dict(keep=0.3)),                      # the smallest general-C shape
             ("softmax", (1, 64, 8, 8), dict(thresh=0.05)),
             ("sigmoid", (2, 1, 4, 6), dict(keep=0.2)),                      # H * W % 4 == 0: the vector route
             ("sigmoid", (2, 3, 2, 6), dict(thresh=0.6, min_kept=4)),
             ("sigmoid", (2, 3, 7, 9), dict(keep=0.15))]                     # odd H * W: the scalar route


@pytest.mark.parametrize("per_image", [False, True], ids=["batch", "per_image"])
@pytest.mark.parametrize("head,shape,kw", INSTANCES, ids=lambda v: v if isinstance(v, str) else ("x".join(map(str, v)) if isinstance(v, tuple) else None))
def test_hard_entries(head, shape, kw, per_image):
    """Forward and backward with every buffer at its exact size and junk in it: the same bits as with ordinary allocations, the
    record numpy's own selection on the device's values, and the values of the restatement."""
    from lm_net_amd import hip
    B, C, H, W = shape
    hd = ("softmax", "sigmoid").index(head)
    lg, y = R.inputs(B, C, H, W, head, seed=5, void=0.0 if H * W == 1 else 0.2, dtype=np.uint8)
    G = B if per_image else 1
    ws_bytes = hip.hard_workspace(hd, per_image, B, C, H, W)
    weight = [1.0 + 0.5 * k for k in range(C)]
    inputs = dict(logits=torch.from_numpy(lg), target=torch.from_numpy(y), weight=torch.tensor(weight), gscale=torch.tensor([-0.5]))
    vshape = (B, H, W) if head == "softmax" else (B, C, H, W)
    outputs = dict(workspace=((ws_bytes,), torch.uint8), values=(vshape, torch.float32), selection=((G, hip.HARD_RECORD_WORDS), torch.int32),
                   terms=((G,), torch.float32), loss=((1,), torch.float32), dlogits=(lg.shape, torch.float32))
    keep, min_kept, thresh = kw.get("keep"), kw.get("min_kept", 0), kw.get("thresh")

    def run(x):
        hip.hard_fwd(x["logits"], x["target"], hd, per_image, keep or 0.0, min_kept, hip.hard_cut(thresh), 0.7, x["weight"], x["workspace"], x["values"],
                     x["selection"], x["terms"], x["loss"])
        hip.hard_bwd(x["logits"], x["target"], hd, per_image, 0.7, x["weight"], x["values"], x["selection"], x["gscale"], x["dlogits"])
        torch.cuda.synchronize()

    plain, pool, guarded = pools(inputs, outputs, DEV, fill="junk")
    run(plain)
    with LaunchLog(pool) as log:
        run(guarded)
    pool.assert_clean("hard entries")
    pool.assert_inputs_unchanged()
    assert log.names == ["hard_fwd", "hard_bwd"]
    got = {e[0]: e[2] for e in pool.entries}
    assert got == {k: v.numel() * v.element_size() for k, v in plain.items()}     # exact sizes: nothing is rounded up
    assert got["workspace"] == ws_bytes and got["selection"] == 20 * G and got["dlogits"] == 4 * lg.size and got["loss"] == 4
    for name in outputs:
        if name != "workspace":
            assert torch.equal(plain[name].view(torch.uint8), guarded[name].view(torch.uint8)), name
    vals, sel = guarded["values"].cpu().numpy(), guarded["selection"].cpu().numpy()
    r = R.loss_and_grad(lg, y, C, head=head, weight=weight, per_image=per_image, scale=0.7, gscale=-0.5, device=(vals, sel), **kw)
    assert np.array_equal(vals < 0, ~r.valid) and np.array_equal(vals[~r.valid], np.full((~r.valid).sum(), -1, np.float32))
    assert np.all(np.abs(vals - r.values)[r.valid] <= R.VALUES_BAR * np.maximum(1.0, r.values[r.valid]))
    assert np.array_equal(sel, R.record_of(vals, r.valid, per_image, **kw)), (sel, R.record_of(vals, r.valid, per_image, **kw))
    loss, d = float(guarded["loss"][0]), guarded["dlogits"].cpu().numpy().astype(np.float64)
    assert abs(loss - r.loss) <= 1e-5 * abs(r.loss), (loss, r.loss)
    assert np.abs(d - r.grad).max() <= 1e-4 * np.abs(r.grad).max()
    assert not np.signbit(d[r.grad == 0]).any() and not d[r.grad == 0].any()      # void and unselected: exactly +0 under a negative factor

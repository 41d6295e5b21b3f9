"""GPU: the entry of include/curves/lmnet_curves.h that writes device memory, lmn_curve_hist, inside guard bands (tests/guard.py): the
guard manifest's test of this entry.  Every buffer -- the values, the target, the edge table, the workspace at exactly
lmn_curve_workspace bytes and the histograms -- is carved from a GuardPool at its exact size, canaries flush against each.
(2, 3, 17, 23): HW is odd, one element per lane, and the planes end on no 16-byte boundary; (1, 2, 64, 64) runs the four-element
form, whose 16-byte loads end flush with the buffers."""
import numpy as np
import pytest
import torch

import curves_ref as R
from guard import GuardPool, LaunchLog

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.mark.parametrize("shape", [(2, 3, 17, 23), (1, 2, 64, 64)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("scores", ["sigmoid", "softmax"])
def test_curve_hist_entry(scores, shape):
    """Both score kinds; the sigmoid form against uint8 planes, the softmax form against an int64 label map; N = 65."""
    from lm_net_amd import hip
    B, C, H, W = shape
    N = 65
    kind = hip.CURVE_SOFTMAX if scores == "softmax" else hip.CURVE_RAW
    form = hip.CURVE_LABELS if scores == "softmax" else hip.CURVE_PLANES
    key = "guard_curves/%s/%d" % (scores, H)
    if scores == "softmax":
        z, _ = R.softmax_case(shape, N, key + "/z")
        t = R.label_targets((B, H, W), C, key + "/t")
    else:
        z = R.logits(shape, key + "/z")
        t = R.plane_targets(shape, key + "/t", dtype=np.uint8)
    edges = hip.curve_edges(N, "logit" if scores == "sigmoid" else "probability")
    ws_bytes = hip.curve_workspace(kind, B, H * W)
    assert ws_bytes == (4 * B * H * W if scores == "softmax" else 0)
    inputs = dict(values=torch.from_numpy(z), target=torch.from_numpy(t), edges=torch.from_numpy(edges))
    outputs = dict(hist=((B, C, 2, N + 1), torch.int64))
    if ws_bytes:
        outputs["workspace"] = ((ws_bytes,), torch.uint8)

    def run(x):
        hip.curve_hist(x["values"], x["target"], form, kind, x["edges"], x["hist"], x.get("workspace"))
        torch.cuda.synchronize()

    plain = {k: v.to(DEV) for k, v in inputs.items()}
    plain.update({k: torch.empty(s, dtype=dt, device=DEV) for k, (s, dt) in outputs.items()})
    run(plain)
    pool = GuardPool(DEV, GuardPool.size_for([v.numel() * v.element_size() for v in plain.values()]))
    guarded = {k: pool.take(k, None, None, init=v.to(DEV)) for k, v in inputs.items()}
    guarded.update({k: pool.take(k, s, dt) for k, (s, dt) in outputs.items()})
    with LaunchLog(pool) as log:
        run(guarded)
    pool.assert_clean("curve entry")
    pool.assert_inputs_unchanged()
    assert log.names == ["curve_hist"]
    got = {e[0]: e[2] for e in pool.entries}
    assert got == {k: v.numel() * v.element_size() for k, v in plain.items()}     # exact sizes: nothing is rounded up
    assert got["hist"] == B * C * 2 * (N + 1) * 8 and got["edges"] == 4 * N and got.get("workspace", 0) == ws_bytes
    assert torch.equal(plain["hist"], guarded["hist"])                           # identical to ordinary allocations
    # ... and the right values, so that the guarded run is the real one
    ref = R.hist(z, t, N, scores, "labels" if scores == "softmax" else "planes")
    assert np.array_equal(guarded["hist"].cpu().numpy(), ref)

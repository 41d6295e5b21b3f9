"""GPU: lm_net_amd.metrics.LesionMeter inside a 2D validation loop.  LM_Net(3, 2) and LM_Net(3, 4) (seeded weights, eval mode) run
a [4, 3, 32, 32] batch; the logits are pushed in two batches and the case is closed once.  The records must equal the restatement
tests/lesion_ref.py on the arg-max that lmn_volume_labels wrote for the same logits (the meter's own narrowing, called once more
here), and the same batch scored image by image must equal four one-slice cases."""
import numpy as np
import pytest
import torch

import lesion_ref as R
import volpost_ref as VR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
NAMES = ("comp_keys", "comp_sizes", "pair_keys", "pair_counts", "ctrl")


@pytest.mark.parametrize("C", [2, 4])
def test_validation_loop_pushes_logits_in_two_batches(C):
    from lm_net_amd import LM_Net, LesionMeter, hip
    from tools.detweights import det_input, fill_module
    B, H, W = 4, 32, 32
    net = LM_Net(3, C)
    fill_module(net, 7)
    net = net.to(DEV).eval()
    x = det_input((B, 3, H, W), "lesion/x").to(DEV)
    target = torch.from_numpy(VR.blob_labels((B, H, W), C, seed=2)).to(DEV)                # int64 with values outside [0, C)
    meter = LesionMeter(C, connectivity=18, max_components=2048, max_pairs=1024)
    images = LesionMeter(C, connectivity=18, max_components=2048, max_pairs=1024)
    lab_p, lab_t = (torch.empty(B, H, W, dtype=torch.uint8, device=DEV) for _ in range(2))
    with torch.no_grad():
        for z0 in (0, 3):                                              # 3 + 1 slices
            logits = net(x[z0:z0 + 3])
            assert tuple(logits.shape) == (min(3, B - z0), C, H, W)
            meter.push(logits, target[z0:z0 + 3])
            images.update_images(logits, target[z0:z0 + 3])
            hip.volume_labels(logits.float().contiguous(), target[z0:z0 + 3], C, lab_p, lab_t, z0)
    meter.close_case()
    Lp, Lt = lab_p.cpu().numpy(), lab_t.cpu().numpy()
    assert (Lt == 255).any() and len(np.unique(Lp)) >= 2                # void target voxels; the net predicts more than one class
    want = R.records(Lp, Lt, C, 18, None, 2048, 2048)
    for got, w, name in zip(meter.raw(), want, NAMES):
        assert tuple(got.shape) == (1,) + w.shape and np.array_equal(got[0].cpu().numpy(), w), name
    assert want[4][0] >= 2
    for b in range(B):
        want = R.records(Lp[b:b + 1], Lt[b:b + 1], C, 18, None, 2048, 2048)
        for got, w, name in zip(images.raw(), want, NAMES):
            assert got.shape[0] == B and np.array_equal(got[b].cpu().numpy(), w), (b, name)
    from lm_net_amd.metrics import lesion_metrics
    got, ref = meter.compute(), lesion_metrics(R.stack([R.records(Lp, Lt, C, 18, None, 2048, 2048)]), list(range(1, C)))
    for key in ("n_pred", "n_target", "det_tp", "tp", "pq", "f1"):
        assert np.array_equal(got["pooled"][key], ref["pooled"][key], equal_nan=True), key

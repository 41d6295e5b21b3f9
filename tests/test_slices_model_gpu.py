"""GPU: VolumeSlicer as the first stage of a case.  A 12 x 40 x 48 int16 phantom with labels goes through VolumeSlicer(size=(32, 32),
context=1) into LM_Net(3, 3) in eval, the arg-max back through restore() to the native grid, then through VolumePostprocess.push and
VolumeSurfaceMeter.push / close_case: shapes and dtypes, no host synchronisation in the slicer's calls, the whole chain bit-identical
over two runs in deterministic mode, and one training step on batch(z, sample(...)) with SegLoss."""
import warnings

import numpy as np
import pytest
import torch

import slices_ref as R
from helpers import no_dropout
from tools.detweights import fill_module

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
D, HS, WS, SIZE = 12, 40, 48, (32, 32)


def _phantom():
    vol, lab = R.phantom(1, D, HS, WS, seed=21)
    return torch.from_numpy(vol[0]).to(DEV), torch.from_numpy(lab).to(DEV)


def _net(train=False):
    from lm_net_amd import LM_Net
    net = LM_Net(3, 3)
    fill_module(net, 9)
    no_dropout(net)
    net = net.to(DEV)
    return net.train() if train else net.eval()


@pytest.fixture
def deterministic():
    from lm_net_amd import hip
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    yield
    hip.set_deterministic(was)


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype == torch.uint8 else t.contiguous().view(torch.int32)


def _chain(net, vol, lab):
    """the validation pass of one case, four slices at a time -> what every stage produced"""
    from lm_net_amd import VolumePostprocess, VolumeSlicer, VolumeSurfaceMeter
    s = VolumeSlicer(size=SIZE, context=1, foreground=-1000, clip=(0.5, 99.5))
    post, meter = VolumePostprocess(3, keep_largest=1), VolumeSurfaceMeter(3)
    s.open_case(vol, lab)
    kept = []
    with torch.no_grad():
        for z0 in range(0, D, 4):
            x, y = s.slices(z0, z0 + 4)
            assert tuple(x.shape) == (4, 3, 32, 32) and x.dtype == torch.float32 and tuple(y.shape) == (4, 32, 32) and y.dtype == torch.uint8
            logits = net(x)
            assert tuple(logits.shape) == (4, 3, 32, 32)
            native = s.restore(logits.argmax(1).to(torch.uint8))
            assert tuple(native.shape) == (4, HS, WS) and native.dtype == torch.uint8
            post.push(native)
            meter.push(native, lab[z0:z0 + 4])
            kept.append((x.clone(), y.clone(), logits.float().clone(), native.clone()))
    out = post.close_case()
    meter.close_case()
    assert tuple(out.labels.shape) == (D, HS, WS) and out.labels.dtype == torch.uint8
    assert tuple(s.stats.shape) == (1, 8) and s.stats.dtype == torch.int64 and tuple(s.table.shape) == (1, 4) and s.table.dtype == torch.float32
    return s, kept, out, meter.raw()


def test_validation_chain_is_bit_identical_over_two_runs(deterministic):
    vol, lab = _phantom()
    net = _net()
    a, b = _chain(net, vol, lab), _chain(net, vol, lab)
    torch.cuda.synchronize()
    assert torch.equal(a[0].stats, b[0].stats) and torch.equal(_bits(a[0].table), _bits(b[0].table))
    for ka, kb in zip(a[1], b[1]):
        for ta, tb in zip(ka, kb):
            assert torch.equal(_bits(ta), _bits(tb))
    assert torch.equal(a[2].labels, b[2].labels) and torch.equal(a[2].stats, b[2].stats)
    assert torch.equal(a[3][0], b[3][0]) and torch.equal(a[3][1].view(torch.int64), b[3][1].view(torch.int64))
    # the stages saw real work: a normalised image, all three classes in the labels, a record of the foreground only
    x, y = a[1][1][0], a[1][1][1]
    assert bool(torch.isfinite(x).all()) and float(x.std()) > 0.1 and sorted(torch.unique(y).tolist()) == [0, 1, 2]
    n_fg = int((vol > -1000).sum())
    assert a[0].stats[0, 0].item() == n_fg and 0 < n_fg < vol.numel()


def _sync_debug_works():
    """torch's sync-debug mode reports a known synchronisation (a device-to-host copy) on this device."""
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        return False
    t = torch.ones(4, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            t.sum().item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return any("synchroniz" in str(w.message).lower() for w in seen)


def test_the_slicer_does_not_synchronise():
    """open_case, slices, batch (host list and device tensor, with drawn parameters) and restore under torch's sync-debug mode
    "error"; the first round sizes the slicer's scratch and staging, the second must not allocate: the same tensors come back."""
    from lm_net_amd import VolumeSlicer
    assert _sync_debug_works(), "torch's sync-debug mode reports nothing on this device"
    vol, lab = _phantom()
    s = VolumeSlicer(size=SIZE, context=1)
    zt = torch.tensor([3, 3, 0, 11], dtype=torch.int32, device=DEV)
    net_labels = torch.zeros(4, 32, 32, dtype=torch.uint8, device=DEV)
    seen = []
    for rnd in range(2):
        params = s.sample(4, rnd)
        torch.cuda.synchronize()
        if rnd:
            torch.cuda.set_sync_debug_mode("error")
        try:
            s.open_case(vol, lab)
            x, y = s.slices(4, 8)
            xb, yb = s.batch([7, 0, 7, 11], params)
            xt, yt = s.batch(zt, params)
            native = s.restore(net_labels)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        seen.append([t.data_ptr() for t in (s.stats, s.table, x, y, xb, yb, xt, yt, native)])
    torch.cuda.synchronize()
    assert seen[0] == seen[1]
    assert bool(torch.isfinite(xt).all()) and tuple(native.shape) == (4, HS, WS)


def test_one_training_step_on_an_augmented_batch(deterministic):
    from lm_net_amd import SegLoss, VolumeSlicer
    vol, lab = _phantom()
    net = _net(train=True)
    s = VolumeSlicer(size=SIZE, context=1, label_dtype=torch.int64, border="constant", border_value=-1024, label_border=0, p_ssr=1.0)
    s.open_case(vol, lab)
    z = [5, 2, 9, 5]
    params = s.sample(len(z), 3)
    assert all(p["M"] is not None for p in params)
    x, y = s.batch(z, params)
    assert tuple(x.shape) == (4, 3, 32, 32) and y.dtype == torch.int64 and int(y.max()) <= 2
    loss = SegLoss(ce_weight=(1.0, 2.0, 4.0), dice_weight=(1.0, 2.0, 4.0)).to(DEV)(net(x), y)
    loss.backward()
    torch.cuda.synchronize()
    grads = [p.grad for p in net.parameters()]
    assert np.isfinite(float(loss.detach())) and float(loss.detach()) > 0
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and sum(float(g.abs().sum()) for g in grads) > 0

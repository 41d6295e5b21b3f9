"""GPU: the three recipes in a training step of LM_Net(3, 2, filters=[12] * 5) at 32 x 32, batch 4, in deterministic mode, with a
frozen eval-mode teacher of the same shape: DeviceMix into the model into SoftSegLoss + DistillLoss, one backward.  The flat parameter
gradient of that step is bit-identical to the one obtained by taking the criteria's dlogits on a detached copy of the logits and
calling logits.backward(dlogits), and bit-identical across two runs (every step starts from one state, as the determinism tests of
the model do): both routes feed the same bits into the same deterministic backward, so the check has no tolerance.  A CutMix batch goes through SegLoss(ignore_index=255) by target.labels, and LM_Net(3, 1)
trains against a teacher under DistillLoss(head="sigmoid")."""
import numpy as np
import pytest
import torch

from helpers import no_dropout
from tools.detweights import det_input, fill_module

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B, H, W = 4, 32, 32
VOID = 255


def _net(C, seed, train=True):
    from lm_net_amd import LM_Net
    net = LM_Net(3, C, filters=[12] * 5)
    fill_module(net, seed)
    no_dropout(net)
    net = net.to(DEV)
    if train:
        return net.train()
    for p in net.parameters():
        p.requires_grad_(False)
    return net.eval()


def _batch(C):
    x = det_input((B, 3, H, W), "soft_model/x").to(DEV)
    yy, xx = np.mgrid[0:H, 0:W]
    y = np.stack([((yy - 15) ** 2 + (xx - 10 - 3 * b) ** 2 < (6 + 2 * b) ** 2) for b in range(B)]).astype(np.int64)
    y[:, 20:22] = VOID                                               # a band that is not annotated
    return x, torch.from_numpy(y).to(DEV)


def _flat(net):
    return torch.cat([p.grad.reshape(-1) for p in net.parameters()]).clone()


@pytest.fixture
def deterministic():
    from lm_net_amd import hip
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    yield
    hip.set_deterministic(was)


def test_mixup_and_distillation_step_is_exact(deterministic):
    from lm_net_amd import DeviceMix, DistillLoss, SoftSegLoss
    net, teacher = _net(2, 7), _net(2, 8, train=False)
    x, y = _batch(2)
    mixer = DeviceMix(mixup_alpha=0.4, cutmix_alpha=1.0, generator=5)
    rows = mixer.sample(B, H, W)
    rows[0, 1], rows[1, 1] = 1, 2                                    # at least one Mixup and one CutMix row
    rows[1, 4:] = (4, 6, 20, 30)
    soft, kd = SoftSegLoss(2, ce_weight=(1.0, 4.0), dice_weight=(1.0, 4.0), label_smoothing=0.1).to(DEV), DistillLoss(2, temperature=4.0, scale=0.5)

    state = {k: v.clone() for k, v in net.state_dict().items()}

    def step(direct):
        net.load_state_dict(state)                                   # every step from one state, the BatchNorm buffers included
        net.zero_grad(set_to_none=True)
        xm, target = mixer.mix(x, y, rows=rows)
        with torch.no_grad():
            zt = teacher(xm)
        logits = net(xm)
        if direct:
            loss = soft(logits, target) + kd(logits, zt, target.ya)
            loss.backward()
        else:                                                        # the criteria's dlogits on a detached copy, fed to the model
            z = logits.detach().clone().requires_grad_(True)
            loss = soft(z, target) + kd(z, zt, target.ya)
            loss.backward()
            logits.backward(z.grad)
        torch.cuda.synchronize()
        return float(loss.detach()), _flat(net)

    l1, g1 = step(True)
    l2, g2 = step(False)
    l3, g3 = step(True)
    assert np.isfinite(l1) and l1 > 0 and bool(torch.isfinite(g1).all()) and float(g1.abs().sum()) > 0
    assert l1 == l2 == l3
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32)), float((g1 - g2).abs().max())
    assert torch.equal(g1.view(torch.int32), g3.view(torch.int32)), float((g1 - g3).abs().max())
    assert float(soft.terms[0]) > 0 and float(kd.terms[1]) > 0 and int(soft.counts[0]) == int(kd.counts[0]) > 0


def test_cutmix_batch_through_segloss(deterministic):
    """mixup_alpha = 0: the mixed target is a hard label map, void band included, that SegLoss takes as it is."""
    from lm_net_amd import DeviceMix, SegLoss
    net = _net(2, 7)
    x, y = _batch(2)
    xm, target = DeviceMix(mixup_alpha=0.0, cutmix_alpha=1.0, generator=3).mix(x, y)
    seg = SegLoss(ignore_index=VOID).to(DEV)
    loss = seg(net(xm), target.labels)
    loss.backward()
    torch.cuda.synchronize()
    g = _flat(net)
    assert float(loss.detach()) > 0 and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0
    assert bool((target.labels == VOID).any()) and bool((target.lam == 1).all()) and tuple(xm.shape) == tuple(x.shape)


def test_sigmoid_head_distillation_step(deterministic):
    from lm_net_amd import DistillLoss, SigmoidSegLoss
    net, teacher = _net(1, 7), _net(1, 8, train=False)
    x, y = _batch(1)
    with torch.no_grad():
        zt = teacher(x)
    logits = net(x)
    assert tuple(logits.shape) == (B, 1, H, W)
    kd = DistillLoss(1, temperature=2.0, head="sigmoid")
    loss = SigmoidSegLoss().to(DEV)(logits, y) + kd(logits, zt.to(torch.bfloat16), y)
    loss.backward()
    torch.cuda.synchronize()
    g = _flat(net)
    assert float(loss.detach()) > 0 and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0
    assert int(kd.counts[0]) == int((y != VOID).sum()) and float(kd.terms[1]) > 0

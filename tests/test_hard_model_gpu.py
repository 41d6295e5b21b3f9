"""GPU: nnU-Net's DC_and_topk_loss in training steps of LM_Net(3, 2) at 64 x 64, batch 2, in deterministic mode:
RegionLoss(2, classes=[1]) + HardPixelLoss(2, keep=0.1), three SGD steps from one saved state (every run starts from that state, the
BatchNorm buffers included, as tests/test_soft_model_gpu.py does).  The gradients are finite and non-zero, two runs are bit-identical
in every loss, gradient and parameter, and the flat parameter gradient of a step equals, bit for bit, the one obtained by taking the
criteria's dlogits on a detached copy of the logits and calling logits.backward(dlogits) -- both routes feed the same bits into the
same deterministic backward, so those checks have no tolerance.  With keep=1.0 the step is the SegLoss(None, None, dice_scale=0) +
RegionLoss step: two kernel families, so the bars are the project's loss and gradient bars, 1e-5 |ref| for the loss and 1e-4 max |ref|
for the flat parameter gradient (the model's backward is one fixed linear map of dlogits in deterministic mode, and the two dlogits
agree to fp32 rounding)."""
import numpy as np
import pytest
import torch

from helpers import no_dropout
from tools.detweights import det_input, fill_module

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B, H, W = 2, 64, 64
VOID = 255


def _net(seed=7):
    from lm_net_amd import LM_Net
    net = LM_Net(3, 2)
    fill_module(net, seed)
    no_dropout(net)
    return net.to(DEV).train()


def _batch():
    x = det_input((B, 3, H, W), "hard_model/x").to(DEV)
    yy, xx = np.mgrid[0:H, 0:W]
    y = np.stack([((yy - 30) ** 2 + (xx - 20 - 9 * b) ** 2 < (7 + 3 * b) ** 2) for b in range(B)]).astype(np.int64)
    y[:, 40:43] = VOID                                               # a band that is not annotated
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


def test_dc_and_topk_steps_are_reproducible(deterministic):
    from lm_net_amd import HardPixelLoss, RegionLoss
    net = _net()
    x, y = _batch()
    dice, topk = RegionLoss(2, classes=[1]).to(DEV), HardPixelLoss(2, keep=0.1).to(DEV)
    state = {k: v.clone() for k, v in net.state_dict().items()}

    def train(steps=3, lr=0.05):
        net.load_state_dict(state)
        out = []
        for _ in range(steps):
            net.zero_grad(set_to_none=True)
            logits = net(x)
            loss = dice(logits, y) + topk(logits, y)
            loss.backward()
            g = _flat(net)
            with torch.no_grad():
                for p in net.parameters():
                    p.add_(p.grad, alpha=-lr)
            out.append((loss.detach().clone(), g, topk.selection.clone()))
        torch.cuda.synchronize()
        return out, torch.cat([p.detach().reshape(-1) for p in net.parameters()]).clone()

    a, pa = train()
    b, pb = train()
    n_valid = int((y != VOID).sum())
    for (la, ga, sa), (lb, gb, sb) in zip(a, b):
        assert np.isfinite(float(la)) and float(la) > 0 and bool(torch.isfinite(ga).all()) and float(ga.abs().sum()) > 0
        assert torch.equal(la.view(torch.int32), lb.view(torch.int32)) and torch.equal(ga.view(torch.int32), gb.view(torch.int32)) and torch.equal(sa, sb)
        N, K = int(sa[0, 0]), int(sa[0, 1])
        assert N == n_valid and K == int(np.floor(np.float64(np.float32(0.1)) * N))          # the kept fraction, read after the fact
    assert torch.equal(pa.view(torch.int32), pb.view(torch.int32))
    assert float(a[0][0]) != float(a[-1][0])                                                 # the steps moved the model


def test_step_equals_the_criteria_dlogits_fed_to_the_model(deterministic):
    from lm_net_amd import HardPixelLoss, RegionLoss
    net = _net()
    x, y = _batch()
    dice, topk = RegionLoss(2, classes=[1]).to(DEV), HardPixelLoss(2, keep=0.1).to(DEV)
    state = {k: v.clone() for k, v in net.state_dict().items()}

    def step(direct):
        net.load_state_dict(state)
        net.zero_grad(set_to_none=True)
        logits = net(x)
        if direct:
            loss = dice(logits, y) + topk(logits, y)
            loss.backward()
        else:
            z = logits.detach().clone().requires_grad_(True)
            loss = dice(z, y) + topk(z, y)
            loss.backward()
            logits.backward(z.grad)
        torch.cuda.synchronize()
        return float(loss.detach()), _flat(net)

    l1, g1 = step(True)
    l2, g2 = step(False)
    assert l1 == l2 and torch.equal(g1.view(torch.int32), g2.view(torch.int32)), float((g1 - g2).abs().max())
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().sum()) > 0


def test_keep_one_step_is_the_segloss_step(deterministic):
    from lm_net_amd import HardPixelLoss, RegionLoss, SegLoss
    net = _net()
    x, y = _batch()
    dice = RegionLoss(2, classes=[1]).to(DEV)
    hard, seg = HardPixelLoss(2, keep=1.0).to(DEV), SegLoss(None, None, dice_scale=0).to(DEV)
    state = {k: v.clone() for k, v in net.state_dict().items()}

    def step(ce):
        net.load_state_dict(state)
        net.zero_grad(set_to_none=True)
        logits = net(x)
        loss = ce(logits, y) + dice(logits, y)
        loss.backward()
        torch.cuda.synchronize()
        return float(loss.detach()), _flat(net).double()

    lh, gh = step(hard)
    ls, gs = step(seg)
    print("keep=1.0 against SegLoss: loss %.9g / %.9g, max |dg| %.3e of max |g| %.3e" % (lh, ls, float((gh - gs).abs().max()), float(gs.abs().max())))
    assert abs(lh - ls) <= 1e-5 * abs(ls), (lh, ls)
    assert float((gh - gs).abs().max()) <= 1e-4 * float(gs.abs().max())
    assert int(hard.selection[0, 0]) == int(hard.selection[0, 1]) == int((y != VOID).sum())

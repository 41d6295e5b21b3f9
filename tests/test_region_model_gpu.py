"""GPU: RegionLoss in a training step of LM_Net(3, 2) (softmax head, SegLoss) and LM_Net(3, 1) (one-logit sigmoid head,
SigmoidSegLoss) at 64 x 64, batch 2, in deterministic mode.  The objective is the regional loss + a per-image Tversky term; one
backward reaches every parameter.  The parameter gradients of that step equal those obtained by feeding the model the float64
restatement's dlogits (tests/region_ref.py) in place of the criterion's own, and the criterion's value and dlogits on the model's
logits keep the bars of tests/test_region_kernels_gpu.py: |L - ref| <= 1e-5 |ref|, max |d - ref| <= 1e-4 max |ref|."""
import numpy as np
import pytest
import torch

import region_ref as R
from helpers import no_dropout
from tools.detweights import det_input, fill_module

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
H = W = 64
VOID = 255


def _case(C):
    from lm_net_amd import LM_Net
    net = LM_Net(3, C)
    fill_module(net, 7)
    no_dropout(net)
    net = net.to(DEV).train()
    x = det_input((2, 3, H, W), "region_model/%d/x" % C).to(DEV)
    yy, xx = np.mgrid[0:H, 0:W]
    y_np = np.stack([((yy - 30) ** 2 + (xx - 24 - 10 * b) ** 2 < (14 + 4 * b) ** 2) for b in range(2)]).astype(np.int64)
    y_np[:, 20:23] = VOID                                             # a band that is not annotated
    return net, x, y_np


@pytest.fixture
def deterministic():
    from lm_net_amd import hip
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    yield
    hip.set_deterministic(was)


def test_training_step_with_a_tversky_term(deterministic):
    from lm_net_amd import RegionLoss, SegLoss
    net, x, y_np = _case(2)
    y = torch.from_numpy(y_np).to(DEV)
    seg = SegLoss(ignore_index=VOID).to(DEV)
    kw = dict(kind="tversky", alpha=0.3, beta=0.7, per_image=True)
    reg = RegionLoss(2, **kw)

    logits = net(x)
    logits.retain_grad()
    (seg(logits, y) + reg(logits, y)).backward()
    torch.cuda.synchronize()
    step = [p.grad.detach().clone() for p in net.parameters()]
    assert all(bool(torch.isfinite(g).all()) for g in step) and sum(float(g.abs().sum()) for g in step) > 0

    # the criterion alone on the model's logits
    z = logits.detach().clone().requires_grad_(True)
    loss = reg(z, y)
    loss.backward()
    r = R.loss_and_grad(z.detach().cpu().numpy(), y_np, 2, **kw)
    got, d = float(loss.detach()), z.grad.cpu().numpy().astype(np.float64)
    print("loss %.9g ref %.9g; dlogits max err %.3e of %.3e" % (got, r.loss, np.abs(d - r.grad).max(), np.abs(r.grad).max()))
    assert np.array_equal(reg.counts.cpu().numpy(), r.counts) and r.counts[0, 0, 1] == int((y_np[0] != VOID).sum())
    assert r.loss > 0 and abs(got - r.loss) <= 1e-5 * abs(r.loss)
    assert np.abs(d - r.grad).max() <= 1e-4 * np.abs(r.grad).max()

    # the same step of a second, identically filled model with the restatement's dlogits in place of the criterion's
    twin, _, _ = _case(2)
    again = twin(x)
    z2 = again.detach().clone().requires_grad_(True)
    seg(z2, y).backward()
    r2 = R.loss_and_grad(again.detach().cpu().numpy(), y_np, 2, **kw)
    again.backward(z2.grad + torch.from_numpy(r2.grad).float().to(DEV))
    torch.cuda.synchronize()
    ref = [p.grad for p in twin.parameters()]
    top = max(float(g.abs().max()) for g in ref)
    err = max(float((a - b).abs().max()) for a, b in zip(step, ref))
    print("parameter gradients: max err %.3e of %.3e" % (err, top))
    assert top > 0 and err <= 1e-4 * top


def test_sigmoid_head_step_and_a_rising_scale(deterministic):
    """LM_Net(3, 1) takes one step with head="sigmoid"; a rising `scale` between two calls changes the loss accordingly, without
    reconstruction."""
    from lm_net_amd import RegionLoss, SigmoidSegLoss
    net, x, y_np = _case(1)
    y = torch.from_numpy(y_np).to(DEV)
    seg = SigmoidSegLoss().to(DEV)
    kw = dict(kind="tversky", head="sigmoid", alpha=0.3, beta=0.7, per_image=True, exponent=0.75)
    reg = RegionLoss(1, scale=0.5, **kw)
    logits = net(x)
    (seg(logits, y) + reg(logits, y)).backward()
    torch.cuda.synchronize()
    assert tuple(logits.shape) == (2, 1, H, W)
    grads = [p.grad for p in net.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and sum(float(g.abs().sum()) for g in grads) > 0

    z = logits.detach().clone().requires_grad_(True)
    half = reg(z, y)
    half.backward()
    r = R.loss_and_grad(z.detach().cpu().numpy(), y_np[:, None], 1, scale=0.5, **kw)
    d = z.grad.cpu().numpy().astype(np.float64)
    assert r.loss > 0 and abs(float(half.detach()) - r.loss) <= 1e-5 * abs(r.loss)
    assert np.abs(d - r.grad).max() <= 1e-4 * np.abs(r.grad).max()
    reg.scale = 1.0                                                   # per epoch: a host float, no rebuild
    z.grad = None
    full = reg(z, y)
    full.backward()
    assert float(full.detach()) == 2.0 * float(half.detach())         # (a power of two: exact)
    assert np.array_equal(z.grad.cpu().numpy().astype(np.float64), 2.0 * d)


def test_scratch_is_not_a_registered_buffer(deterministic):
    """After a step the module that holds the criterion has exactly its registered buffer, the class weight, in its state_dict and still
    moves: the scratch of the geometry is kept outside torch.nn.Module's registries, and it is reused: a second forward gives the same
    bits."""
    from lm_net_amd import RegionLoss
    g = torch.Generator().manual_seed(3)
    z = torch.randn(2, 3, 5, 7, generator=g).to(DEV).requires_grad_(True)
    y = torch.randint(0, 3, (2, 5, 7), generator=g).to(DEV)
    crit = RegionLoss(3, weight=[1.0, 2.0, 3.0])
    first = crit(z, y)
    first.backward()
    holder = torch.nn.ModuleList([crit])
    assert list(holder.state_dict()) == ["0.weight"] and list(crit.state_dict()) == ["weight"]
    assert holder.to(DEV) is holder
    second = crit(z.detach(), y)
    torch.cuda.synchronize()
    assert float(first.detach()) > 0 and bool(torch.isfinite(z.grad).all()) and float(z.grad.abs().max()) > 0
    assert first.detach().view(torch.int32).item() == second.view(torch.int32).item()

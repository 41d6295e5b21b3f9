"""GPU: LovaszLoss in a training step of LM_Net(3, 2) (softmax head, SegLoss) and LM_Net(3, 1) (one-logit sigmoid head,
SigmoidSegLoss) at 64 x 64, batch 2.  The objective is the regional loss + LovaszLoss; one backward reaches every parameter.  The
criterion's value and its dlogits on the model's own logits are compared with the float64 restatement (tests/lovasz_ref.py) on the
device's order, with the bars of tests/test_lovasz_kernels_gpu.py: |L - ref| < 1e-5 |ref|, max |d - ref| < 1e-4 max |ref|."""
import numpy as np
import pytest
import torch

import lovasz_ref as R
from helpers import no_dropout
from tools.detweights import det_input, fill_module

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
H = W = 64
VOID = 255


@pytest.mark.parametrize("C", [2, 1])
def test_training_step_with_lovasz(C):
    from lm_net_amd import LM_Net, LovaszLoss, SegLoss, SigmoidSegLoss
    net = LM_Net(3, C)
    fill_module(net, 7)
    no_dropout(net)
    net = net.to(DEV).train()
    x = det_input((2, 3, H, W), "lovasz_model/%d/x" % C).to(DEV)
    yy, xx = np.mgrid[0:H, 0:W]
    y_np = np.stack([((yy - 30) ** 2 + (xx - 24 - 10 * b) ** 2 < (14 + 4 * b) ** 2) for b in range(2)]).astype(np.int64)
    y_np[:, 20:23] = VOID                                             # a band that is not annotated
    y = torch.from_numpy(y_np).to(DEV)
    head = "softmax" if C > 1 else "sigmoid"
    seg = (SegLoss(ignore_index=VOID) if C > 1 else SigmoidSegLoss()).to(DEV)
    lov = LovaszLoss(C, head=head, scale=0.5)

    logits = net(x)
    logits.retain_grad()
    (seg(logits, y) + lov(logits, y)).backward()
    torch.cuda.synchronize()
    assert tuple(logits.shape) == (2, C, H, W)
    grads = [p.grad for p in net.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and sum(float(g.abs().sum()) for g in grads) > 0

    # the criterion alone on the model's logits
    z = logits.detach().clone().requires_grad_(True)
    loss = lov(z, y)
    loss.backward()
    order = lov.ranks[1].cpu().numpy()
    y_ref = y_np if C > 1 else y_np[:, None]
    want, wgrad, counts, _ = R.loss_and_grad(z.detach().cpu().numpy(), y_ref, C, head, "present", False, scale=0.5, order=order)
    assert np.array_equal(lov.ranks[2].cpu().numpy(), counts) and counts[0, 0] == int((y_np != VOID).sum())
    got, d = float(loss.detach()), z.grad.cpu().numpy().astype(np.float64)
    print("loss %.9g ref %.9g; dlogits max err %.3e of %.3e" % (got, want, np.abs(d - wgrad).max(), np.abs(wgrad).max()))
    assert want > 0 and abs(got - want) < 1e-5 * abs(want)
    assert np.abs(d - wgrad).max() < 1e-4 * np.abs(wgrad).max()
    # the step's dlogits is the sum of the two criteria's
    z2 = logits.detach().clone().requires_grad_(True)
    seg(z2, y).backward()
    both = (z2.grad + z.grad - logits.grad).abs().max()
    assert float(both) <= 1e-5 * float(logits.grad.abs().max())


def test_scratch_is_not_a_registered_buffer():
    """After a step the module that holds the criterion still has a state_dict and still moves: the scratch of the geometry is kept
    outside torch.nn.Module's registries, and it is reused: a second forward gives the same bits."""
    from lm_net_amd import LovaszLoss
    g = torch.Generator().manual_seed(3)
    z = torch.randn(2, 3, 5, 7, generator=g).to(DEV).requires_grad_(True)
    y = torch.randint(0, 3, (2, 5, 7), generator=g).to(DEV)
    crit = LovaszLoss(3)
    first = crit(z, y)
    first.backward()
    holder = torch.nn.ModuleList([crit])
    assert list(holder.state_dict()) == [] and list(crit.state_dict()) == []
    assert holder.to(DEV) is holder
    second = crit(z.detach(), y)
    torch.cuda.synchronize()
    assert float(first.detach()) > 0 and bool(torch.isfinite(z.grad).all()) and float(z.grad.abs().max()) > 0
    assert first.detach().view(torch.int32).item() == second.view(torch.int32).item()

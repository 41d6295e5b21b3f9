"""GPU: BoundaryLoss and HausdorffDTLoss in a training step of LM_Net(3, 2) (softmax head, SegLoss) and LM_Net(3, 1) (one-logit
sigmoid head, SigmoidSegLoss) at 64 x 96.  The objective is the regional loss + BoundaryLoss + HausdorffDTLoss; one backward.  The
parameter gradients are compared with the same composition where the two new terms are computed by the float64 restatement
(tests/distmap_ref.py) on the model's own logits and fed back through autograd as a linear surrogate with the restatement's
gradient.  Tolerance: that of tests/test_distmap_kernels_gpu.py for dlogits, max |d - ref| < 1e-4 max |ref|, at the logits and --
the parameter gradients being linear in dlogits -- over the whole parameter-gradient vector.  Between the forward of the criteria and
the end of their backward nothing synchronises with the host (torch's sync-debug mode; skipped where the device lacks it)."""
import warnings

import numpy as np
import pytest
import torch

import distmap_ref as R
from helpers import no_dropout
from tools.detweights import det_input, fill_module

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
H, W = 64, 96


def _setup(C):
    from lm_net_amd import LM_Net, BoundaryLoss, HausdorffDTLoss, SegLoss, SigmoidSegLoss
    net = LM_Net(3, C)
    fill_module(net, 7)
    no_dropout(net)
    net = net.to(DEV).train()
    x = det_input((2, 3, H, W), "distmap_model/%d/x" % C).to(DEV)
    rng = np.random.default_rng(C)
    y = np.stack([R.blobs(H, W, rng, 3) for _ in range(2)]).astype(np.int64)
    y[:, 20:23] = R.VOID                                              # a band that is not annotated
    head = "softmax" if C > 1 else "sigmoid"
    seg = (SegLoss(ignore_index=R.VOID) if C > 1 else SigmoidSegLoss()).to(DEV)
    return net, x, y, head, seg, BoundaryLoss(C, head=head, scale=0.5), HausdorffDTLoss(C, head=head, scale=0.01)


@pytest.mark.parametrize("C", [2, 1])
def test_parameter_gradients_against_the_restatement(C):
    net, x, y_np, head, seg, bl, hd = _setup(C)
    y = torch.from_numpy(y_np).to(DEV)
    classes = R.default_classes(C)

    def step(new_terms):
        net.zero_grad(set_to_none=True)
        logits = net(x)
        logits.retain_grad()
        (seg(logits, y) + new_terms(logits)).backward()
        torch.cuda.synchronize()
        return logits.detach(), logits.grad.clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}

    maps = bl.target_maps(y)                                          # computed once for both terms
    logits, dl, got = step(lambda z: bl(z, y, maps) + hd(z, y, maps))
    assert tuple(logits.shape) == (2, C, H, W)
    lg_np = logits.cpu().numpy()
    b = R.loss_and_grad(lg_np, y_np, head, "boundary", classes, scale=0.5)
    h = R.loss_and_grad(lg_np, y_np, head, "hausdorff", classes, scale=0.01)
    assert h[4] == 0, "%d logits within %g of the threshold: the prediction's mask is not decided in fp32" % (h[4], R.MARGIN)
    assert b[2] == h[2] == int((y_np != R.VOID).sum()) * len(classes)
    wgrad = torch.from_numpy(b[1] + h[1]).float().to(DEV)
    assert float(wgrad.abs().max()) > 0
    logits2, dl2, want = step(lambda z: (z * wgrad).sum())           # the surrogate: its gradient at the logits is the restatement's
    assert float((logits - logits2).abs().max()) <= 1e-5 * float(logits.abs().max())      # (the same forward, up to its own atomics)
    err, top = float((dl - dl2).abs().max()), float(dl2.abs().max())
    print("dlogits: max |d - ref| %.3g of max |ref| %.3g" % (err, top))
    assert err < 1e-4 * top
    gmax = max(float(g.abs().max()) for g in want.values())
    worst = max(float((got[k] - want[k]).abs().max()) for k in want)
    print("parameters: max |d - ref| %.3g of max |ref| %.3g" % (worst, gmax))
    assert worst < 1e-4 * gmax and all(bool(torch.isfinite(g).all()) for g in got.values())
    # the two terms as values
    assert abs(float(bl(logits, y)) - b[0]) < 1e-5 * b[3] and abs(float(hd(logits, y)) - h[0]) < 1e-5 * abs(h[0])


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


@pytest.mark.parametrize("C", [2, 1])
def test_no_host_synchronisation_between_forward_and_backward(C):
    if not _sync_debug_works():
        pytest.skip("torch's sync-debug mode reports nothing on this device")
    net, x, y_np, head, seg, bl, hd = _setup(C)
    y = torch.from_numpy(y_np).to(DEV)
    with torch.no_grad():
        logits = net(x)
    one = torch.ones((), device=DEV)
    for _ in range(2):                                                # (the first round loads the library and sizes the allocator)
        z = logits.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            total = seg(z, y) + bl(z, y) + hd(z, y)
            total.backward(one)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(z.grad).all()) and float(z.grad.abs().max()) > 0


def test_the_last_maps_are_not_registered_buffers():
    """After a step the module that holds the criteria still has an empty state_dict and still moves: the maps the criteria keep are
    plain attributes outside torch.nn.Module's registries.  A second forward gives the same bits (deterministic mode)."""
    from lm_net_amd import BoundaryLoss, HausdorffDTLoss, hip
    g = torch.Generator().manual_seed(3)
    y = torch.randint(0, 3, (2, 5, 7), generator=g).to(DEV)
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    try:
        for cls in (BoundaryLoss, HausdorffDTLoss):
            z = torch.randn(2, 3, 5, 7, generator=g).to(DEV).requires_grad_(True)
            crit = cls(3)
            first = crit(z, y)
            first.backward()
            holder = torch.nn.ModuleList([crit])
            assert list(holder.state_dict()) == [] and list(crit.state_dict()) == []
            assert holder.to(DEV) is holder
            second = crit(z.detach(), y)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(z.grad).all()) and float(z.grad.abs().max()) > 0
            assert first.detach().view(torch.int32).item() == second.view(torch.int32).item()
    finally:
        hip.set_deterministic(was)

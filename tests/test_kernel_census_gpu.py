"""GPU: the census.  Every kernel INSTANCE a training step (and a deploy-mode forward) launches has an owner in
tests/kernel_forms.py -- a check or test that compares that instance with a high-precision reference and proves that it launches it.

The whole-model goldens hold gradients to 4e-3 ... 2.5e-2 of a tensor's largest element and the bench-size tests compare the product
with itself, so an instance that only the step reaches, and that is slightly wrong, would otherwise be caught by nothing tighter.  There is
no exemption list: a new instance that reaches the step fails here until it gets an owner (list what a call launches with
kernel_forms.launched)."""
import pytest
import torch

from helpers import no_dropout
from kernel_forms import OWNED, launched
from tools.detweights import det_input, disc_labels, fill_module

pytestmark = pytest.mark.gpu


def _model():
    from lm_net_amd import LM_Net
    m = LM_Net(3, 2)
    fill_module(m, 43)
    no_dropout(m)
    return m


def _train(B, H, W, det=False, dtype="fp32", steps=2):
    """The training step of tests/test_bench_size_gpu.py::_train (fused loss, FusedAdamW as bench.py uses them) on a fresh model: host
    launches, no plans, no graphs."""
    from lm_net_amd.loss import SegLoss
    from lm_net_amd.optim import FusedAdamW
    x, y = det_input((B, 3, H, W), "census/x").cuda(), disc_labels(B, H, W).cuda()
    m = _model().cuda().train()
    m.deterministic = det
    m.compute_dtype = dtype
    crit = SegLoss(label_smoothing=1e-3).cuda()
    opt = FusedAdamW(m, lr=1e-3, weight_decay=1e-4)
    for _ in range(steps):
        loss = crit(m(x), y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss.detach()))


def _deploy(B, H, W):
    x = det_input((B, 3, H, W), "census/x").cuda()
    m = _model()
    m.eval()
    m.structural_reparam()
    m = m.cuda().eval()
    with torch.no_grad():
        y = m(x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())


CONFIGS = {
    "fp32-352": lambda: _train(8, 352, 352),
    "fp32-deterministic-352": lambda: _train(8, 352, 352, det=True),
    "bf16-352": lambda: _train(8, 352, 352, dtype="bf16"),
    "fp32-64x96": lambda: _train(2, 64, 96),          # the size of the model goldens: small maps select other instances
    "deploy-eval-352": lambda: _deploy(8, 352, 352),
}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_every_launched_instance_has_an_owner(config):
    from lm_net_amd import hip
    try:
        _, names = launched(CONFIGS[config])
    finally:
        hip.set_deterministic(False)
    print("census %s: %d distinct kernel instances" % (config, len(names)))
    assert len(names) > 30, names          # (the timer saw the pass)
    unowned = sorted(names - set(OWNED))
    assert not unowned, "%d of the %d kernel instances of `%s` have no owner in tests/kernel_forms.py:\n  %s" % (
        len(unowned), len(names), config, "\n  ".join(unowned))

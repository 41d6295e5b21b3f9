"""GPU: the census of the supported envelope.  tests/test_kernel_census_gpu.py gives every kernel instance of the DEFAULT model's
step an owner; the wide variants (filters up to 4x), 1..16 input channels / up to 64 classes, na_kernel_size 5 / 7, the "bf16-mma"
precision and 512^2 inputs select other instances -- na_any_*, the VALU gattn_*_kernel<64|128>, ln_*_wide_kernel, na_*_gen_kernel,
other conv / weight-gradient / depthwise template arguments.  Every one of them has an owner in tests/kernel_forms.py too: same
step, same rule, no exemption list (list what a call launches with kernel_forms.launched).

The configurations are small on purpose (64x64, batch 2) except where the map size is what selects the instance."""
import pytest
import torch

from helpers import no_dropout
from kernel_forms import OWNED, launched
from test_wide_model_gpu import WIDE
from tools.detweights import det_input, disc_labels, fill_module

pytestmark = pytest.mark.gpu
DEFAULT = [12, 24, 48, 96, 192]


def _model(filters, K, cin, ncls):
    from lm_net_amd import LM_Net
    m = LM_Net(cin, ncls, filters=filters, na_kernel_size=K)
    fill_module(m, 43)
    no_dropout(m)
    return m


def _labels(B, H, W, ncls):
    if ncls == 2:
        return disc_labels(B, H, W)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")     # every class present, blocks of 4 x 4 pixels
    return torch.stack([(yy // 4 * 5 + xx // 4 + i) % ncls for i in range(B)]).long()


def _train(B, H, W, filters=DEFAULT, det=False, dtype="fp32", K=3, cin=3, ncls=2, steps=2):
    """The step of tests/test_kernel_census_gpu.py::_train on a fresh model of the given variant: host launches, no plans, no graphs."""
    from lm_net_amd.loss import SegLoss
    from lm_net_amd.optim import FusedAdamW
    x, y = det_input((B, cin, H, W), "census/x").cuda(), _labels(B, H, W, ncls).cuda()
    m = _model(filters, K, cin, ncls).cuda().train()
    m.deterministic = det
    m.compute_dtype = dtype
    crit = (SegLoss(label_smoothing=1e-3) if ncls == 2 else SegLoss(None, None, label_smoothing=1e-3)).cuda()
    opt = FusedAdamW(m, lr=1e-3, weight_decay=1e-4)
    for _ in range(steps):
        loss = crit(m(x), y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss.detach()))


def _eval(B, H, W, reparam, dtype="fp32"):
    """reparam=False: the eval forward of a training-mode model (BatchNorm running statistics); True: the deploy forward."""
    x = det_input((B, 3, H, W), "census/x").cuda()
    m = _model(DEFAULT, 3, 3, 2)
    m.eval()
    if reparam:
        m.structural_reparam()
    m = m.cuda().eval()
    m.compute_dtype = dtype
    with torch.no_grad():
        y = m(x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())


CONFIGS = {
    "W2-fp32": lambda: _train(2, 64, 64, WIDE["W2"]),
    "W3-fp32": lambda: _train(2, 64, 64, WIDE["W3"]),
    "W4-fp32": lambda: _train(2, 64, 64, WIDE["W4"]),
    "Wodd-fp32": lambda: _train(2, 64, 64, WIDE["Wodd"]),
    "W3-bf16": lambda: _train(2, 64, 64, WIDE["W3"], dtype="bf16"),
    "Wodd-bf16": lambda: _train(2, 64, 64, WIDE["Wodd"], dtype="bf16"),
    "W3-fp32-deterministic": lambda: _train(2, 64, 64, WIDE["W3"], det=True),
    "W2-fp32-352": lambda: _train(2, 352, 352, WIDE["W2"]),                    # large maps select other conv forms
    "K5-fp32": lambda: _train(2, 64, 64, K=5),
    "K7-fp32": lambda: _train(2, 64, 64, K=7),
    "K5-bf16": lambda: _train(2, 64, 64, K=5, dtype="bf16"),
    "K7-bf16": lambda: _train(2, 64, 64, K=7, dtype="bf16"),
    "W3-K5-fp32": lambda: _train(2, 64, 64, WIDE["W3"], K=5),
    "bf16-mma-352": lambda: _train(8, 352, 352, dtype="bf16-mma"),
    "fp32-512": lambda: _train(2, 512, 512),                                   # global attention over N = 1024 tokens
    "gray-9-classes": lambda: _train(2, 64, 64, cin=1, ncls=9),                # padded stem, segloss_*<K>
    "16-channels-64-classes": lambda: _train(2, 64, 64, cin=16, ncls=64),      # padded stem and head, segloss_*_gen_kernel
    "eval-running-stats": lambda: _eval(2, 64, 64, reparam=False),
    "deploy-bf16": lambda: _eval(2, 64, 64, reparam=True, dtype="bf16"),
}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_every_launched_instance_of_the_envelope_has_an_owner(config):
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

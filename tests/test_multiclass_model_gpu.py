"""GPU: LM_Net at other input-channel / class counts (README "Input channels and classes": 1 <= channel <= 16, 1 <= n_classes <= 64)
through whole passes.

Each fp32 training step (batch-statistics BatchNorm, dropout off) is checked against float64 goldens of the REAL reference
(tests/golden/mc_c*_k*.npz, tools/make_golden_multiclass.py) with the tolerances of tests/test_wide_model_gpu.py: logits, every
parameter gradient, the input gradient and the BatchNorm running statistics.  (16, 64) and a wide width at (1, 9) are checked against
the CPU oracle; then bf16 against the fp32 HIP path, eval and structural_reparam against the oracle, plan replay against host launch
(deterministic mode), an enable_graphs step, the grayscale / class-id pipeline end to end, and the envelope check.
"""
import numpy as np
import pytest
import torch

from helpers import load_golden, no_dropout, rel_err
from tools.detweights import det_input, fill_module

pytestmark = pytest.mark.gpu
TOL = 1e-4
W2 = [24, 48, 96, 192, 384]


def _pair(channel, n_classes, seed, filters=(12, 24, 48, 96, 192)):
    from lm_net_amd import LM_Net
    from oracle.lmnet_ref import LM_Net as Oracle
    ora = Oracle(channel, n_classes, filters=list(filters))
    fill_module(ora, seed)
    no_dropout(ora)
    m = LM_Net(channel, n_classes, filters=list(filters))
    fill_module(m, seed)
    no_dropout(m)
    return ora, m.cuda()


def _golden_train_step(channel, n_classes, size, B, tol_g=4e-3, tol_affine=2.5e-2):
    """One training step against tests/golden/mc_c<channel>_k<n_classes>_<size>_b<B>.npz, checked as tests/test_wide_model_gpu.py
    checks its goldens."""
    from lm_net_amd import LM_Net
    from tools.make_golden_f64 import sample_index
    key = "mc_c%d_k%d_%d_b%d" % (channel, n_classes, size, B)
    g = load_golden(key + ".npz")
    size, B, seed, ch, nc = (int(v) for v in g["meta"])
    assert (ch, nc) == (channel, n_classes)
    m = LM_Net(channel, n_classes)
    fill_module(m, seed)
    no_dropout(m)
    m = m.cuda().train()
    x = det_input((B, channel, size, size), key + "/x").cuda().requires_grad_(True)
    y = m(x)
    assert y.shape == (B, n_classes, size, size)
    yf = y.detach().flatten().cpu().double()
    ys = yf[torch.from_numpy(sample_index(yf.numel(), 32768))].numpy()
    assert float(np.abs(ys - g["logits/sample"]).max()) < TOL * float(g["logits/stat"][0]), key
    assert abs(float(yf.norm()) - float(g["logits/stat"][1])) < TOL * float(g["logits/stat"][1]), key
    (y * det_input(tuple(y.shape), key + "/G").cuda()).sum().backward()
    torch.cuda.synchronize()
    gmax = max(float(g["gstat/" + k][0]) for k, _ in m.named_parameters())

    def check(tag, grad, stat, samp):
        gf = grad.detach().flatten().cpu().double()
        gs = gf[torch.from_numpy(sample_index(gf.numel()))].numpy()
        err = float(np.abs(gs - samp).max())
        if err < 2e-5 * gmax:          # pre-BatchNorm biases (exact gradient 0) and other tiny tensors: absolute scale
            return
        assert err < (tol_affine if grad.dim() == 1 else tol_g) * float(stat[0]), (key, tag, err, float(stat[0]))
        assert abs(float(gf.norm()) - float(stat[1])) < 2e-3 * float(stat[1]), (key, tag, float(gf.norm()), float(stat[1]))

    check("input", x.grad, g["gx/stat"], g["gx/sample"])
    for k, p in m.named_parameters():
        check(k, p.grad, g["gstat/" + k], g["gsamp/" + k])
    for k, v in m.state_dict().items():
        if "running_" in k:
            assert rel_err(v, g["state/" + k]) < 1e-4, (key, k)


@pytest.mark.parametrize("channel, n_classes", [(1, 2), (1, 9), (4, 4), (3, 14)])
def test_train_step_64_batch2_vs_reference_f64(channel, n_classes):
    _golden_train_step(channel, n_classes, 64, 2)


def test_train_step_352_batch2_c1_k9_vs_reference_f64():
    _golden_train_step(1, 9, 352, 2)


def _oracle_step(channel, n_classes, seed, filters, size=64):
    """fp32 train step of the HIP path against the CPU oracle on the same weights: logits, input gradient, every parameter gradient."""
    ora, m = _pair(channel, n_classes, seed, filters)
    ora.train()
    m.train()
    x = det_input((2, channel, size, size), "mc_ora/x%d" % channel)
    G = det_input((2, n_classes, size, size), "mc_ora/G%d" % n_classes)
    xo = x.clone().requires_grad_(True)
    yo = ora(xo)
    (yo * G).sum().backward()
    xg = x.cuda().requires_grad_(True)
    yg = m(xg)
    (yg * G.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert rel_err(yg, yo) < TOL, rel_err(yg, yo)
    assert rel_err(xg.grad, xo.grad) < 2e-3, rel_err(xg.grad, xo.grad)
    go = dict(ora.named_parameters())
    gmax = max(float(p.grad.abs().max()) for p in go.values())
    for k, p in m.named_parameters():
        ref = go[k].grad
        err = float((p.grad.cpu() - ref).abs().max())
        if err < 2e-5 * gmax:
            continue
        assert err < (2.5e-2 if p.dim() == 1 else 4e-3) * float(ref.abs().max()), (k, err, float(ref.abs().max()))


def test_c16_k64_train_step_vs_oracle():
    _oracle_step(16, 64, 21, (12, 24, 48, 96, 192))


def test_wide_c1_k9_train_step_vs_oracle():
    _oracle_step(1, 9, 23, W2)


@pytest.mark.parametrize("channel, n_classes", [(1, 9), (16, 64)])
def test_bf16_vs_fp32_path(channel, n_classes):
    """bf16 storage (and bf16-mma, and autocast) against the fp32 HIP path of the same model, with the distances of
    tests/test_wide_model_gpu.py."""
    def l2(a, b):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return float((a - b).norm() / (b.norm() + 1e-30))

    x = det_input((2, channel, 64, 64), "mc_bf16/x").cuda()
    G = det_input((2, n_classes, 64, 64), "mc_bf16/G").cuda()

    def run(mode):
        _, m = _pair(channel, n_classes, 9)
        m.compute_dtype = mode
        m.eval()
        with torch.no_grad():
            ye = m(x)
        m.train()
        xg = x.clone().requires_grad_(True)
        yt = m(xg)
        (yt * G).sum().backward()
        torch.cuda.synchronize()
        return ye, yt.detach(), xg.grad, [(k, p.grad) for k, p in m.named_parameters()]

    ref = run("fp32")
    for mode in ("bf16", "bf16-mma"):
        ye, yt, gx, grads = run(mode)
        assert 2e-4 < rel_err(ye, ref[0]) < 4e-2 and l2(ye, ref[0]) < 1.6e-2, (mode, rel_err(ye, ref[0]))
        assert rel_err(yt, ref[1]) < 5e-2 and l2(yt, ref[1]) < 3e-2, (mode, rel_err(yt, ref[1]))
        assert l2(gx, ref[2]) < 0.1, mode
        # (at one input channel the stem's expand-conv weight gradient is a heavily cancelling sum over every pixel of a
        #  single channel: its bf16 distance runs 0.3-0.5, so it gets a bound of its own)
        stem = "conv1.0.expand_conv.0.weight" if channel == 1 else None
        errs = sorted((l2(g, gr), k) for (k, g), (_, gr) in zip(grads, ref[3]) if float(gr.abs().max()) > 0 and
                      not (k.endswith("expand_conv.0.bias") or k.endswith("fuse_conv.0.bias")) and k != stem)
        assert errs[len(errs) // 2][0] < 0.1 and errs[-1][0] < 0.4, (mode, errs[len(errs) // 2], errs[-1])
        if stem:
            d = dict((k, l2(g, gr)) for (k, g), (_, gr) in zip(grads, ref[3]))[stem]
            assert d < 0.8, (mode, stem, d)
    _, m = _pair(channel, n_classes, 9)
    m.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ya = m(x)
    assert 2e-4 < rel_err(ya, ref[0]) < 4e-2


@pytest.mark.parametrize("channel, n_classes, filters", [(1, 2, None), (4, 4, None), (3, 14, None), (16, 64, None), (1, 9, W2)])
def test_eval_and_structural_reparam_vs_oracle(channel, n_classes, filters):
    ora, m = _pair(channel, n_classes, 11, filters or (12, 24, 48, 96, 192))
    ora.eval()
    m.eval()
    x = det_input((2, channel, 64, 96), "mc_eval/x")
    with torch.no_grad():
        yo = ora(x)
        yg = m(x.cuda())
    assert rel_err(yg, yo) < TOL, rel_err(yg, yo)
    ora.structural_reparam()
    m.structural_reparam()
    with torch.no_grad():
        yo2 = ora(x)
        yg2 = m(x.cuda())
    assert rel_err(yg2, yo2) < TOL, rel_err(yg2, yo2)
    assert rel_err(yo2, yo) < 1e-4


@pytest.mark.parametrize("channel, n_classes", [(1, 9), (16, 64)])
def test_plan_replay_equals_host_launch_deterministic_and_graph_step(channel, n_classes):
    from lm_net_amd import hip
    x = det_input((2, channel, 64, 64), "mc_plan/x").cuda()
    G = det_input((2, n_classes, 64, 64), "mc_plan/G").cuda()

    def step(m):
        m.zero_grad(set_to_none=True)
        y = m(x)
        (y * G).sum().backward()
        torch.cuda.synchronize()
        return y.detach().clone(), [p.grad.detach().clone() for p in m.parameters()]

    hip.set_deterministic(True)
    try:
        _, m = _pair(channel, n_classes, 13)
        m.train()
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        host = step(m)
        m.load_state_dict(sd)
        m.enable_plans(True)
        runs = []
        for _ in range(4):                   # two sizing passes, one recording, one replay
            m.load_state_dict(sd)
            runs.append(step(m))
        for y, gr in runs[2:]:
            assert torch.equal(y, host[0])
            assert all(torch.equal(u, v) for u, v in zip(gr, host[1]))
        m.enable_plans(False)
    finally:
        hip.set_deterministic(False)
    _, m = _pair(channel, n_classes, 13)
    m.train()
    ref = step(m)
    m.enable_graphs(True)
    for _ in range(3):
        yg, gg = step(m)
    assert rel_err(yg, ref[0]) < 1e-3
    assert torch.isfinite(yg).all()


def test_grayscale_labels_end_to_end():
    """DevicePreprocess(channels=1, mask_mode="labels") -> LM_Net(1, 9) -> SegLoss(None, None) -> backward -> ConfusionMeter(9):
    runs, and the loss and the confusion matrix match their CPU restatements on the same logits."""
    import torch.nn.functional as F
    from lm_net_amd import LM_Net
    from lm_net_amd.data import DevicePreprocess
    from lm_net_amd.loss import SegLoss
    from lm_net_amd.metrics import ConfusionMeter
    rng = np.random.default_rng(3)
    B, C = 2, 9
    img = torch.from_numpy(rng.integers(0, 256, (B, 90, 120), dtype=np.uint8)).cuda()
    mask = torch.from_numpy(rng.integers(0, C, (B, 90, 120), dtype=np.uint8)).cuda()
    x, y = DevicePreprocess((64, 96), mean=(0.5,), std=(0.25,), channels=1, mask_mode="labels")(img, mask)
    assert x.shape == (B, 1, 64, 96) and int(y.max()) <= C - 1
    m = LM_Net(1, C)
    fill_module(m, 4)
    no_dropout(m)
    m = m.cuda().train()
    out = m(x)
    loss = SegLoss(None, None)(out, y)
    loss.backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    lo = out.detach().double()
    ce = F.cross_entropy(lo, y)
    p = torch.softmax(lo, 1)
    dice = sum(1 - (2 * (p[:, c] * (y == c)).sum() + 1e-5) / ((p[:, c] ** 2).sum() + (y == c).sum() + 1e-5) for c in range(C)) / C
    assert abs(float(loss) - float(ce + dice)) < 1e-5 * float(ce + dice)
    meter = ConfusionMeter(C)
    meter.update(out.detach(), y)
    r = meter.compute()
    pred, gt = out.detach().argmax(1).cpu().numpy().ravel(), y.cpu().numpy().ravel()
    ref = np.bincount(C * gt + pred, minlength=C * C).reshape(C, C)
    assert np.array_equal(np.array(r["confusion"]), ref)
    assert "Mean_Intersection_over_Union" in r and "Frequency_Weighted_Intersection_over_Union" in r


@pytest.mark.parametrize("channel, n_classes, words", [(17, 2, ["channel = 17", "16"]), (3, 65, ["n_classes = 65", "64"])])
def test_outside_envelope_raises_before_launch(channel, n_classes, words):
    from lm_net_amd import LM_Net, hip
    m = LM_Net(channel, n_classes).cuda()          # construction stays possible
    x = torch.zeros(1, channel, 64, 64, device="cuda")
    hip.prof_begin()
    with pytest.raises(ValueError) as e:
        m(x)
    assert hip.prof_end() == {}                   # nothing was launched
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_default_step_launch_list_unchanged_by_class_dispatch():
    """The default LM_Net(3, 2) loss step still runs the 2-class templated loss kernels and no general-C kernel."""
    from lm_net_amd import LM_Net, hip
    from lm_net_amd.loss import SegLoss
    from tools.detweights import disc_labels
    m = LM_Net(3, 2)
    fill_module(m, 2)
    m = m.cuda().train()
    x = det_input((2, 3, 64, 64), "mc_def/x").cuda()
    y = disc_labels(2, 64, 64).cuda()
    SegLoss(label_smoothing=1e-3).cuda()(m(x), y).backward()
    torch.cuda.synchronize()
    hip.prof_begin()
    SegLoss(label_smoothing=1e-3).cuda()(m(x), y).backward()
    names = list(hip.prof_end())
    assert not any("segloss_sums_gen" in n or "segloss_bwd_gen" in n for n in names), names
    assert any("segloss_sums_kernel<2>" in n for n in names) and any("segloss_bwd_kernel<2>" in n for n in names), names

"""GPU: the general-class-count kernels of csrc/rows.hip (loss) and csrc/metrics.hip (confusion), and the ABI 15 input pipeline entry.

  * fused loss (lmn_segloss_fwd / _bwd) at C outside {2, 3, 4, 8}: loss and dlogits against a float64 torch restatement and against
    the reference DiceLoss + CrossEntropyLoss goldens (tests/golden/mc_loss_metrics.npz, tools/make_golden_multiclass.py);
    deterministic mode bit-identical; C in {2, 3, 4, 8} still run the kernels templated on C;
  * confusion matrix (lmn_confusion) at 5 <= C <= 64: exact against np.bincount with out-of-range labels and forced ties, and the
    Evaluator metrics of ConfusionMeter.compute() against the reference golden;
  * lmn_preprocess_u8_ex: grayscale frames and class-id masks bit-exact against the composed oracle functions, and the 3-channel
    binary mode equal to lmn_preprocess_u8.
"""
import math

import numpy as np
import pytest
import torch

from helpers import load_golden
from oracle import preprocess_ref as P
from tools.detweights import det_input, uniform

pytestmark = pytest.mark.gpu


def _labels(B, H, W, C, key):
    u = uniform(key, B * H * W)
    return torch.from_numpy(np.minimum((u * C).astype(np.int64), C - 1).reshape(B, H, W))


def _loss_f64(lg, y, wce, wdice, eps, smooth=1e-5):
    """CrossEntropyLoss(weight=wce, label_smoothing=eps) + DiceLoss(C)(softmax, one-hot, weight=wdice), float64 torch."""
    import torch.nn.functional as F
    C = lg.shape[1]
    ce = F.cross_entropy(lg, y, weight=wce, label_smoothing=eps)
    p = torch.softmax(lg, 1)
    dice = 0.0
    for c in range(C):
        t = (y == c).double()
        dice = dice + wdice[c] * (1 - (2 * (p[:, c] * t).sum() + smooth) / ((p[:, c] ** 2).sum() + (t * t).sum() + smooth))
    return ce + dice / C


def _run_loss(lg, y, wce, wdice, eps, gscale=None):
    from lm_net_amd import hip
    B, C = lg.shape[:2]
    sums = torch.empty(3 + 3 * C, device="cuda")
    coef = torch.empty(3 + 2 * C, device="cuda")
    loss = torch.empty(1, device="cuda")
    hip.segloss_fwd(lg, y, wce, wdice, eps, 1e-5, sums, coef, loss)
    d = torch.empty_like(lg)
    hip.segloss_bwd(lg, y, wce, coef, gscale, d)
    torch.cuda.synchronize()
    return loss.clone(), d


@pytest.mark.parametrize("C", [5, 6, 7, 9, 14, 33, 64])
def test_general_c_loss_vs_f64(C):
    from kernel_forms import launched, owned_by
    B, H, W = 2, 37, 45                              # 1665 pixels per image: not a multiple of 64 or 256
    for eps in (0.0, 1e-3):
        key = "mc_k/%d/%g" % (C, eps)
        lg = (det_input((B, C, H, W), key + "/lg") * 2.5).cuda()
        y = _labels(B, H, W, C, key + "/y").cuda()
        wce = torch.from_numpy(0.25 + 2 * uniform(key + "/wce", C)).float().cuda()
        wdice = torch.from_numpy(0.25 + 2 * uniform(key + "/wdice", C)).float().cuda()
        l64 = lg.double().requires_grad_(True)
        ref = _loss_f64(l64, y, wce.double(), wdice.double(), eps)
        ref.backward()
        g_ref = l64.grad
        for gs in (None, 0.37):                      # (the second call gets sums / coef workspaces that held other values)
            gst = None if gs is None else torch.tensor([gs], device="cuda")
            (loss, d), names = launched(lambda: _run_loss(lg, y, wce, wdice, eps, gst))
            # (the general-C kernels of a step with other class counts than 2: this test owns them, tests/kernel_forms.py)
            assert {"segloss_sums_gen_kernel", "segloss_bwd_gen_kernel"} <= owned_by("tests/test_multiclass_kernels_gpu.py::test_general_c_loss_vs_f64") <= names, names
            assert abs(float(loss) - float(ref)) < 1e-5 * abs(float(ref)), (C, eps, float(loss), float(ref))
            expect = g_ref * (1.0 if gs is None else gs)
            err = float((d.double() - expect).abs().max())
            assert err < 1e-4 * float(expect.abs().max()), (C, eps, gs, err)


def test_two_class_loss_vs_f64_owns_the_step_kernels():
    """C = 2, the class count of the training step and of bench.py: the kernels templated on C against the same float64 restatement,
    at the tolerances of the general-C test above, and (tests/kernel_forms.py) proof that this test launches the instances it owns."""
    from kernel_forms import launched, owned_by
    C, B, H, W = 2, 2, 37, 45
    for eps in (0.0, 1e-3):
        key = "mc_k/2/%g" % eps
        lg = (det_input((B, C, H, W), key + "/lg") * 2.5).cuda()
        y = _labels(B, H, W, C, key + "/y").cuda()
        wce = torch.from_numpy(0.25 + 2 * uniform(key + "/wce", C)).float().cuda()
        wdice = torch.from_numpy(0.25 + 2 * uniform(key + "/wdice", C)).float().cuda()
        l64 = lg.double().requires_grad_(True)
        ref = _loss_f64(l64, y, wce.double(), wdice.double(), eps)
        ref.backward()
        gst = torch.tensor([0.37], device="cuda")
        (loss, d), names = launched(lambda: _run_loss(lg, y, wce, wdice, eps, gst))
        assert owned_by("tests/test_multiclass_kernels_gpu.py::test_two_class_loss_vs_f64_owns_the_step_kernels") <= names, names
        assert abs(float(loss) - float(ref)) < 1e-5 * abs(float(ref)), (eps, float(loss), float(ref))
        expect = l64.grad * 0.37
        assert float((d.double() - expect).abs().max()) < 1e-4 * float(expect.abs().max()), eps


@pytest.mark.parametrize("tag", ["k9", "k33"])
def test_general_c_loss_vs_reference_golden(tag):
    """SegLoss at C = 9 / 33 with the golden's class weights against the reference DiceLoss + CrossEntropyLoss (float64)."""
    from lm_net_amd.loss import SegLoss
    g = load_golden("mc_loss_metrics.npz")
    C, B, H, W, scale = g[tag + "/meta"]
    C, B, H, W = int(C), int(B), int(H), int(W)
    lg = (det_input((B, C, H, W), "mc_loss/%s" % tag) * float(scale)).cuda().requires_grad_(True)
    y = _labels(B, H, W, C, "mc_loss/%s/y" % tag).cuda()
    crit = SegLoss(g[tag + "/wce"].tolist(), g[tag + "/wdice"].tolist(), label_smoothing=0.001).cuda()
    loss = crit(lg, y)
    loss.backward()
    ref = float(g[tag + "/loss"][0])
    assert abs(float(loss.detach()) - ref) < 1e-5 * abs(ref), (tag, float(loss.detach()), ref)
    gr = torch.from_numpy(g[tag + "/dlogits"]).double()
    assert float((lg.grad.cpu().double() - gr).abs().max()) < 1e-4 * float(gr.abs().max()), tag


def test_segloss_none_weights_are_all_ones():
    from lm_net_amd import hip
    from lm_net_amd.loss import SegLoss
    C, B, H, W = 9, 2, 32, 48
    lg = det_input((B, C, H, W), "mc_ones/lg").cuda()
    y = _labels(B, H, W, C, "mc_ones/y").cuda()
    hip.set_deterministic(True)                      # (fixed reduction order: the two losses compare bit for bit)
    try:
        a = SegLoss(None, None)(lg, y)
        b = SegLoss([1.0] * C, [1.0] * C).cuda()(lg, y)
    finally:
        hip.set_deterministic(False)
    assert torch.equal(a, b)
    ref = _loss_f64(lg.double(), y, torch.ones(C, dtype=torch.float64, device="cuda"), [1.0] * C, 0.0)
    assert abs(float(a) - float(ref)) < 1e-5 * abs(float(ref))


@pytest.mark.parametrize("C", [9, 64])
def test_general_c_loss_deterministic_bit_identical(C):
    from lm_net_amd import hip
    B, H, W = 2, 96, 80
    lg = (det_input((B, C, H, W), "mc_det/%d" % C) * 3).cuda()
    y = _labels(B, H, W, C, "mc_det/y%d" % C).cuda()
    wce = torch.from_numpy(0.5 + uniform("mc_det/w", C)).float().cuda()
    hip.set_deterministic(True)
    try:
        runs = [_run_loss(lg, y, wce, wce, 1e-3) for _ in range(2)]
    finally:
        hip.set_deterministic(False)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    ref = _loss_f64(lg.double(), y, wce.double(), wce.double(), 1e-3)
    assert abs(float(runs[0][0]) - float(ref)) < 1e-5 * abs(float(ref))


@pytest.mark.parametrize("C", [2, 3, 4, 8, 9])
def test_loss_dispatch_by_class_count(C):
    """C in {2, 3, 4, 8} keep the kernels templated on C; every other C runs the general-C kernels."""
    from lm_net_amd import hip
    B, H, W = 1, 32, 32
    lg = det_input((B, C, H, W), "mc_disp/%d" % C).cuda()
    y = _labels(B, H, W, C, "mc_disp/y%d" % C).cuda()
    w = torch.ones(C, device="cuda")
    torch.cuda.synchronize()
    hip.prof_begin("segloss")
    _run_loss(lg, y, w, w, 0.0)
    names = set(hip.prof_end())

    def has(k):
        return any(k in n for n in names)
    if C in (2, 3, 4, 8):
        assert has("segloss_sums_kernel<%d>" % C) and has("segloss_bwd_kernel<%d>" % C), names
        assert not has("segloss_sums_gen") and not has("segloss_bwd_gen"), names
    else:
        assert has("segloss_sums_gen_kernel") and has("segloss_bwd_gen_kernel"), names
        assert not has("segloss_sums_kernel<") and not has("segloss_bwd_kernel<"), names


@pytest.mark.parametrize("C", [5, 9, 33, 64])
def test_general_c_confusion_exact(C):
    from lm_net_amd import hip
    B, H, W = 3, 41, 57
    lg = det_input((B, C, H, W), "mc_conf/%d" % C).cuda()
    lg = torch.round(lg * 2) / 2                     # coarse values: many ties
    lg[:, C - 1, :5] = lg[:, 0, :5]                  # forced ties between the first and the last class
    lg[0, :, 7, :] = 0.25                            # a row where every class ties
    y = _labels(B, H, W, C, "mc_conf/y%d" % C)
    y.view(-1)[::31] = 255
    y.view(-1)[3::37] = -1
    counts = torch.zeros(C, C, device="cuda")
    hip.confusion(lg.contiguous(), y.cuda(), counts)
    pred = lg.argmax(1).cpu().numpy().reshape(-1)    # torch.argmax: the first maximum
    gt = y.numpy().reshape(-1)
    keep = (gt >= 0) & (gt < C)
    ref = np.bincount(C * gt[keep] + pred[keep], minlength=C * C).reshape(C, C)
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), ref)


def test_general_c_confusion_dispatch():
    from lm_net_amd import hip
    lg = det_input((1, 9, 32, 32), "mc_cd").cuda()
    y = _labels(1, 32, 32, 9, "mc_cd/y").cuda()
    hip.prof_begin("confusion")
    hip.confusion(lg, y, torch.zeros(9, 9, device="cuda"))
    names = list(hip.prof_end())
    assert len(names) == 1 and "confusion_gen_kernel" in names[0], names


@pytest.mark.parametrize("tag", ["k9", "k33"])
def test_confusion_meter_evaluator_keys_vs_reference(tag):
    """ConfusionMeter(C) on the golden's logits and labels (255 / -1 included): the matrix equals the reference Evaluator's, and
    every Evaluator metric compute() reports equals the value the reference method returned (NaN for NaN)."""
    from lm_net_amd.metrics import ConfusionMeter
    g = load_golden("mc_loss_metrics.npz")
    C, B, H, W, scale = g[tag + "/meta"]
    C, B, H, W = int(C), int(B), int(H), int(W)
    lg = (det_input((B, C, H, W), "mc_loss/%s" % tag) * float(scale)).cuda()
    gt = torch.from_numpy(g[tag + "/labels"].astype(np.int64)).cuda()
    m = ConfusionMeter(C)
    m.update(lg[:1], gt[:1])
    m.update(lg[1:], gt[1:])
    r = m.compute()
    assert np.array_equal(np.array(r["confusion"], dtype=np.float64), g[tag + "/confusion"])
    for k in ("Mean_Accuracy", "Mean_Recall", "Precision", "Recall", "Specificity", "Mean_Dice", "Mean_Intersection_over_Union",
              "Frequency_Weighted_Intersection_over_Union"):
        ref = float(g["%s/ev/%s" % (tag, k)][0])
        assert (math.isnan(r[k]) and math.isnan(ref)) or abs(r[k] - ref) < 1e-12, (tag, k, r[k], ref)
    assert abs(r["accuracy"] - float(g[tag + "/ev/Accuracy"][0])) < 1e-12


def _oracle_gray(img, mask, size, flips, mean, std, labels):
    H, W = size
    xs, ys = [], []
    for b in range(img.shape[0]):
        im = P.resize_linear_u8(img[b].reshape(img.shape[1], img.shape[2], 1), H, W)
        mk = mask[b] if labels else (mask[b] > 127).astype(np.uint8)
        mk = P.resize_nearest(mk, H, W)
        fl = int(flips[b]) if flips is not None else 0
        if fl & 1:
            im, mk = im[:, ::-1], mk[:, ::-1]
        if fl & 2:
            im, mk = im[::-1], mk[::-1]
        xs.append(P.normalize(np.ascontiguousarray(im), mean, std).transpose(2, 0, 1))
        ys.append(mk.astype(np.int64))
    return np.stack(xs), np.stack(ys)


@pytest.mark.parametrize("B,hs,ws,h,w", [(3, 37, 53, 32, 48), (2, 100, 80, 352, 352), (2, 530, 622, 256, 256)])
def test_grayscale_and_label_masks_match_oracle(B, hs, ws, h, w):
    from lm_net_amd.data import DevicePreprocess
    rng = np.random.default_rng(B * 100 + hs)
    img = rng.integers(0, 256, (B, hs, ws), dtype=np.uint8)
    mask = rng.integers(0, 14, (B, hs, ws), dtype=np.uint8)
    flips = rng.integers(0, 4, (B,), dtype=np.uint8)
    mean, std = (0.3,), (0.2,)
    for labels in (True, False):
        xr, yr = _oracle_gray(img, mask if labels else mask * 18, (h, w), flips, mean, std, labels)
        p = DevicePreprocess((h, w), mean, std, channels=1, mask_mode="labels" if labels else "binary")
        mk = torch.from_numpy(mask if labels else mask * 18).cuda()
        for shape in ((B, hs, ws), (B, hs, ws, 1)):             # both grayscale layouts
            x, y = p(torch.from_numpy(img.reshape(shape)).cuda(), mk, torch.from_numpy(flips).cuda())
            assert x.shape == (B, 1, h, w) and y.shape == (B, h, w) and y.dtype == torch.int64
            assert np.array_equal(x.cpu().numpy(), xr)
            assert np.array_equal(y.cpu().numpy(), yr)
    # no flips, masks only
    none, y2 = DevicePreprocess((h, w), mean, std, channels=1, mask_mode="labels")(None, torch.from_numpy(mask).cuda())
    assert none is None
    assert np.array_equal(y2.cpu().numpy(), np.stack([P.resize_nearest(mask[b], h, w) for b in range(B)]).astype(np.int64))


def test_label_masks_three_channel_and_binary_entry_equal():
    """3-channel frames: mask_mode="labels" passes ids through the new entry; binary mode through lmn_preprocess_u8_ex equals
    lmn_preprocess_u8 bit for bit."""
    from lm_net_amd import hip
    from lm_net_amd.data import DevicePreprocess
    rng = np.random.default_rng(7)
    B, hs, ws, h, w = 2, 90, 120, 64, 96
    img = torch.from_numpy(rng.integers(0, 256, (B, hs, ws, 3), dtype=np.uint8)).cuda()
    mask = torch.from_numpy(rng.integers(0, 256, (B, hs, ws), dtype=np.uint8)).cuda()
    flips = torch.from_numpy(np.array([1, 2], dtype=np.uint8)).cuda()
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    x0, y0 = DevicePreprocess((h, w))(img, mask, flips)
    x1 = torch.empty_like(x0)
    y1 = torch.empty_like(y0)
    hip.preprocess_u8_ex(img, mask, flips, x1, y1, mean, std, 3, 0)
    assert torch.equal(x0, x1) and torch.equal(y0, y1)
    x2, y2 = DevicePreprocess((h, w), mask_mode="labels")(img, mask, flips)
    assert torch.equal(x2, x0)
    mk = mask.cpu().numpy()
    fl = flips.cpu().numpy()
    for b in range(B):
        ref = P.resize_nearest(mk[b], h, w)
        if fl[b] & 1:
            ref = ref[:, ::-1]
        if fl[b] & 2:
            ref = ref[::-1]
        assert np.array_equal(y2[b].cpu().numpy(), ref.astype(np.int64))

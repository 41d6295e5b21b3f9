"""GPU: the loss with void labels and the focal term (lmn_segloss_ex_fwd / _bwd, include/lmnet_loss.h) against the float64
restatement of tests/void_ref.py and the reference goldens (tests/golden/void_loss_stats.npz).

Tolerances: the project's own for this loss family (tests/test_multiclass_kernels_gpu.py): |loss - ref| < 1e-5 |ref| for the total
and each term (a term whose reference is 0 must be exactly 0), max |dlogits - ref| < 1e-4 max |ref|.  Exact conditions: dlogits is
bitwise +0 at every void pixel; an all-void batch gives a finite loss and an all-zero gradient."""
import numpy as np
import pytest
import torch

import void_ref as V
from helpers import load_golden

pytestmark = pytest.mark.gpu

TEMPLATED, GENERAL = (2, 3, 4, 8), (5, 9, 33, 64)
# (eps, ce_scale, dice_scale, focal_scale, gamma, alpha)
PARAMS = {
    "plain": (0.0, 1.0, 1.0, 0.0, 2.0, 0.25),
    "smoothed": (1e-3, 1.0, 1.0, 0.0, 2.0, 0.25),
    "focal_alone": (0.0, 0.0, 0.0, 1.0, 2.0, 0.25),
    "focal_gamma0": (1e-3, 0.0, 0.0, 1.0, 0.0, 0.25),
    "all_terms": (1e-3, 0.7, 1.3, 0.5, 1.5, -1.0),
}


def _pattern(name, B, H, W, C, key):
    """-> (labels int64 [B,H,W], ignore_index)"""
    y = V.labels(B, H, W, C, key + "/y")
    if name == "void20":
        return V.with_void(y, key + "/v", 255), 255
    if name == "void20_neg":
        return V.with_void(y, key + "/v", -100), -100
    if name == "run64":                                           # one whole wave of the first block is void
        y.view(-1)[128:192] = 255
        return y, 255
    if name == "image_void":
        y[B - 1] = 255
        return y, 255
    if name == "batch_void":
        return torch.full_like(y, 255), 255
    if name == "class_absent":
        y[y == C - 1] = 0
        return V.with_void(y, key + "/v", 255), 255
    if name == "stray77":                                         # 77 is void although it is not ignore_index (C = 64: 77 >= C too)
        y = V.with_void(y, key + "/v", 255, frac=0.05)
        y.view(-1)[min(1000, y.numel() - 1)] = 77
        return y, 255
    raise KeyError(name)


def _run(lg, y, wce, wdice, ignore_index, par, gscale=None):
    from lm_net_amd import hip
    eps, cs, ds, fs, gamma, alpha = par
    C = lg.shape[1]
    p = hip.loss_param(ignore_index, eps, 1e-5, cs, ds, fs, gamma, alpha)
    sums = torch.empty(hip.loss_sums_floats(C), device="cuda")
    coef = torch.empty(hip.loss_coef_floats(C), device="cuda")
    loss4 = torch.empty(4, device="cuda")
    hip.segloss_ex_fwd(lg, y, wce, wdice, p, sums, coef, loss4)
    d = torch.empty_like(lg)
    hip.segloss_ex_bwd(lg, y, wce, coef, None if gscale is None else torch.tensor([gscale], device="cuda"), p, d)
    torch.cuda.synchronize()
    return loss4.cpu().double(), d


def _ref(lg, y, wce, wdice, ignore_index, par):
    eps, cs, ds, fs, gamma, alpha = par
    return V.loss_and_grad(lg, y, wce, wdice, eps=eps, ignore_index=ignore_index, ce_scale=cs, dice_scale=ds, focal_scale=fs, gamma=gamma,
                           alpha=alpha)


def _check(tag, loss4, d, terms, grad, y, C, gs=1.0):
    for k, name in enumerate(("total", "ce", "dice", "focal")):
        got, ref = float(loss4[k]), terms[k]
        print("%s %s: got %.9g ref %.9g" % (tag, name, got, ref))
        assert np.isfinite(got), (tag, name)
        if ref == 0.0:
            assert got == 0.0, (tag, name, got)
        else:
            assert abs(got - ref) < 1e-5 * abs(ref), (tag, name, got, ref)
    expect = grad * gs
    err, scale = float((d.cpu().double() - expect).abs().max()), float(expect.abs().max())
    print("%s dlogits: err %.3e of %.3e" % (tag, err, scale))
    assert err < 1e-4 * scale or (scale == 0.0 and err == 0.0), (tag, err, scale)
    void = ((y < 0) | (y >= C)).cpu()
    at_void = d.cpu().permute(0, 2, 3, 1)[void]
    assert int(at_void.view(torch.int32).abs().max()) == 0 if at_void.numel() else True, tag      # bitwise +0


@pytest.mark.parametrize("C", TEMPLATED + GENERAL)
def test_loss_and_gradient_vs_f64(C):
    B, H, W = 2, 37, 45                                           # 1665 pixels per image: a multiple of neither 64 nor 256
    key = "void_gpu/%d" % C
    lg = V.det_input((B, C, H, W), key + "/lg") * 2.5
    wce, wdice = V.weights(key + "/wce", C), V.weights(key + "/wdice", C)
    lgd, wced, wdiced = lg.cuda(), wce.cuda(), wdice.cuda()
    for i, pat in enumerate(("void20", "void20_neg", "run64", "image_void", "batch_void", "class_absent", "stray77")):
        y, ii = _pattern(pat, B, H, W, C, key + "/" + pat)
        for j, (pname, par) in enumerate(PARAMS.items()):
            terms, grad = _ref(lg, y, wce, wdice, ii, par)
            gs = None if (i + j) % 2 == 0 else 0.37               # (both on every pattern and every parameter set)
            loss4, d = _run(lgd, y.cuda(), wced, wdiced, ii, par, gs)
            _check("C=%d %s %s gs=%s" % (C, pat, pname, gs), loss4, d, terms, grad, y, C, 1.0 if gs is None else gs)
            if pat == "batch_void":
                assert all(t == 0.0 for t in terms) and int(d.view(torch.int32).abs().max()) == 0


@pytest.mark.parametrize("C", [2, 8, 9, 64])
def test_less_than_one_wave(C):
    B, H, W = 1, 5, 7
    key = "void_gpu/tiny/%d" % C
    lg = V.det_input((B, C, H, W), key + "/lg") * 2.5
    wce, wdice = V.weights(key + "/wce", C), V.weights(key + "/wdice", C)
    for pat in ("void20", "batch_void", "stray77"):
        y, ii = _pattern(pat, B, H, W, C, key + "/" + pat)
        for pname in ("smoothed", "all_terms"):
            terms, grad = _ref(lg, y, wce, wdice, ii, PARAMS[pname])
            loss4, d = _run(lg.cuda(), y.cuda(), wce.cuda(), wdice.cuda(), ii, PARAMS[pname], 0.37)
            _check("tiny C=%d %s %s" % (C, pat, pname), loss4, d, terms, grad, y, C, 0.37)


@pytest.mark.parametrize("C", [3, 9])
def test_void_image_equals_the_other_image_alone(C):
    B, H, W = 2, 37, 45
    key = "void_gpu/alone/%d" % C
    lg = (V.det_input((B, C, H, W), key + "/lg") * 2.5).cuda()
    wce, wdice = V.weights(key + "/wce", C).cuda(), V.weights(key + "/wdice", C).cuda()
    y, ii = _pattern("image_void", B, H, W, C, key)
    y = y.cuda()
    par = PARAMS["all_terms"]
    l2, d2 = _run(lg, y, wce, wdice, ii, par)
    l1, d1 = _run(lg[:1].contiguous(), y[:1].contiguous(), wce, wdice, ii, par)
    for k in range(4):
        assert abs(float(l2[k]) - float(l1[k])) < 1e-5 * abs(float(l1[k])), (k, float(l2[k]), float(l1[k]))
    assert float((d2[:1] - d1).abs().max()) < 1e-4 * float(d1.abs().max())
    assert int(d2[1].view(torch.int32).abs().max()) == 0


@pytest.mark.parametrize("tag", ["k2", "k9", "f3"])
def test_modules_through_autograd_vs_reference_golden(tag):
    """SegLoss(ignore_index=255) against F.cross_entropy(ignore_index=255) + the reference DiceLoss(ignore=...), FocalLoss against
    the reference FocalLoss (float64 goldens)."""
    from lm_net_amd import FocalLoss, SegLoss
    g = load_golden("void_loss_stats.npz")
    lg, y, wce, wdice, kw = V.loss_case(tag)
    lg = lg.cuda().requires_grad_(True)
    if tag == "f3":
        crit = FocalLoss(lg.shape[1])
    else:
        crit = SegLoss(wce.tolist(), wdice.tolist(), label_smoothing=kw["eps"], ignore_index=kw["ignore_index"]).cuda()
    loss = crit(lg, y.cuda())
    (loss * 0.37).backward()
    ref = float(g[tag + "/loss"][0])
    got = float(loss.detach())
    print("%s: got %.9g ref %.9g" % (tag, got, ref))
    assert abs(got - ref) < 1e-5 * abs(ref)
    terms = crit.terms.cpu()
    assert terms.shape == (4,) and float(terms[0]) == got
    assert float(terms[3 if tag == "f3" else 1]) > 0 and float(terms[1 if tag == "f3" else 3]) == 0.0
    gr = torch.from_numpy(g[tag + "/dlogits"]).double() * 0.37
    err = float((lg.grad.cpu().double() - gr).abs().max())
    print("%s dlogits: err %.3e of %.3e" % (tag, err, float(gr.abs().max())))
    assert err < 1e-4 * float(gr.abs().max())


@pytest.mark.parametrize("C", [2, 9, 64])
def test_agrees_with_the_old_entries_and_is_deterministic(C):
    """Focal off, unit scales, no void label: the new entries against lmn_segloss_fwd / _bwd on the same inputs; in deterministic mode
    two runs of the new entries (here and with void labels and every term on) are bit-identical."""
    from lm_net_amd import hip
    B, H, W = 2, 37, 45
    key = "void_gpu/old/%d" % C
    lg = (V.det_input((B, C, H, W), key + "/lg") * 2.5).cuda()
    y = V.labels(B, H, W, C, key + "/y").cuda()
    wce, wdice = V.weights(key + "/wce", C).cuda(), V.weights(key + "/wdice", C).cuda()
    sums, coef, loss = torch.empty(3 + 3 * C, device="cuda"), torch.empty(3 + 2 * C, device="cuda"), torch.empty(1, device="cuda")
    hip.segloss_fwd(lg, y, wce, wdice, 1e-3, 1e-5, sums, coef, loss)
    d_old = torch.empty_like(lg)
    hip.segloss_bwd(lg, y, wce, coef, None, d_old)
    l4, d_new = _run(lg, y, wce, wdice, None, PARAMS["smoothed"])
    assert abs(float(l4[0]) - float(loss)) < 1e-5 * abs(float(loss)) and float(l4[3]) == 0.0
    assert float((d_new - d_old).abs().max()) < 1e-4 * float(d_old.abs().max())
    yv = V.with_void(y.cpu(), key + "/v").cuda()
    hip.set_deterministic(True)
    try:
        runs = [_run(lg, y, wce, wdice, None, PARAMS["smoothed"]) for _ in range(2)]
        runs_v = [_run(lg, yv, wce, wdice, 255, PARAMS["all_terms"], 0.37) for _ in range(2)]
    finally:
        hip.set_deterministic(False)
    for a, b in (runs, runs_v):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert abs(float(runs[0][0][0]) - float(l4[0])) < 1e-5 * abs(float(l4[0]))


@pytest.mark.parametrize("C", [2, 3, 4, 8, 5, 9])
def test_dispatch_by_class_count(C):
    """C in {2, 3, 4, 8} run the new kernels templated on C, the others the general ones; focal off runs the instance without it."""
    from lm_net_amd import hip
    lg = V.det_input((1, C, 32, 32), "void_gpu/disp/%d" % C).cuda()
    y = V.labels(1, 32, 32, C, "void_gpu/disp/y%d" % C).cuda()
    w = torch.ones(C, device="cuda")
    for focal, par in ((False, PARAMS["smoothed"]), (True, PARAMS["all_terms"])):
        torch.cuda.synchronize()
        hip.prof_begin("segloss")
        _run(lg, y, w, w, 255, par)
        names = set(hip.prof_end())
        f = "true" if focal else "false"
        if C in TEMPLATED:
            want = {"segloss_ex_sums_kernel<%d, %s>" % (C, f), "segloss_ex_bwd_kernel<%d, %s>" % (C, f), "segloss_ex_finish_kernel"}
        else:
            want = {"segloss_ex_sums_gen_kernel<%s>" % f, "segloss_ex_bwd_gen_kernel<%s>" % f, "segloss_ex_finish_kernel"}
        assert names == want, (C, focal, names)


def test_default_segloss_runs_only_the_old_kernels():
    from lm_net_amd import SegLoss, hip
    lg = V.det_input((2, 2, 32, 32), "void_gpu/default").cuda().requires_grad_(True)
    y = V.labels(2, 32, 32, 2, "void_gpu/default/y").cuda()
    torch.cuda.synchronize()
    hip.prof_begin("segloss")
    crit = SegLoss().cuda()
    crit(lg, y).backward()
    names = set(hip.prof_end())
    assert names == {"segloss_sums_kernel<2>", "segloss_finish_kernel", "segloss_bwd_kernel<2>"}, names
    assert crit.terms is None


def test_training_step_with_void_labels():
    from lm_net_amd import LM_Net, SegLoss
    from lm_net_amd.optim import FusedAdamW
    torch.manual_seed(0)
    x = V.det_input((2, 3, 32, 32), "void_gpu/step/x").cuda()
    y = V.with_void(V.labels(2, 32, 32, 3, "void_gpu/step/y"), "void_gpu/step/v").cuda()
    m = LM_Net(3, 3, filters=[12] * 5).cuda().train()
    opt = FusedAdamW(m, lr=1e-3)
    crit = SegLoss(None, None, label_smoothing=1e-3, ignore_index=255, focal_scale=0.5)
    loss = crit(m(x), y)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and bool(torch.isfinite(crit.terms).all()) and float(crit.terms[3]) > 0
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())

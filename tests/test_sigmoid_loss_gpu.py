"""GPU: the sigmoid-head loss (lmn_sigloss_fwd / _bwd, include/lmnet_sigmoid.h) against the float64 restatement of
tests/sigmoid_ref.py on the same fp32 inputs, and against the reference goldens (tests/golden/sigmoid_loss_stats.npz).

Tolerances: the project's own for this loss family (tests/test_void_loss_gpu.py): |term - ref| < 1e-5 |ref| for the total and each
term (a term whose reference is 0 must be exactly 0), max |dlogits - ref| < 1e-4 max |ref|.  Exact conditions: dlogits is bitwise +0
at every void element; an all-void image has an all-zero gradient."""
import numpy as np
import pytest
import torch

import sigmoid_ref as S
import void_ref as V
from helpers import load_golden

pytestmark = pytest.mark.gpu

# (bce_scale, dice_scale, focal_scale, gamma, alpha, drawn weights)
PARAMS = {
    "default": (1.0, 1.0, 0.0, 2.0, 0.25, False),
    "weighted": (1.0, 1.0, 0.0, 2.0, 0.25, True),
    "focal_g0_a": (0.0, 0.0, 1.0, 0.0, 0.25, False),
    "focal_g0_na": (0.0, 0.0, 1.0, 0.0, -1.0, False),
    "focal_g15_a": (0.0, 0.0, 1.0, 1.5, 0.25, False),
    "focal_g15_na": (0.0, 0.0, 1.0, 1.5, -1.0, True),
    "focal_g2_a": (0.0, 0.0, 1.0, 2.0, 0.25, True),
    "focal_g2_na": (0.0, 0.0, 1.0, 2.0, -1.0, False),
    "all_terms": (0.7, 1.3, 0.5, 1.5, 0.25, True),
}


def _weights(C, key, drawn):
    if not drawn:
        return torch.ones(C), torch.ones(C), torch.ones(C)
    return tuple(S.weights("%s/%s" % (key, n), C) for n in ("wbce", "pw", "wdice"))


def _kw(par):
    bs, ds, fs, gamma, alpha, _ = par
    return dict(bce_scale=bs, dice_scale=ds, focal_scale=fs, gamma=gamma, alpha=alpha)


def _run(lg, t, w, par, gscale=None):
    """-> (loss4 float64 on the host, dlogits on the device) of device logits / target and host weight vectors."""
    from lm_net_amd import hip
    bs, ds, fs, gamma, alpha, _ = par
    C = lg.shape[1]
    wb, pw, wd = (v.cuda() for v in w)
    p = hip.sig_param(1e-5, bs, ds, fs, gamma, alpha, hip.sig_target_kind(t))
    sums = torch.empty(hip.sig_sums_words(C), device="cuda", dtype=torch.int32)
    coef = torch.empty(hip.sig_coef_floats(C), device="cuda")
    loss4 = torch.empty(4, device="cuda")
    hip.sigloss_fwd(lg, t, wb, pw, wd, p, sums, coef, loss4)
    d = torch.empty_like(lg)
    hip.sigloss_bwd(lg, t, pw, coef, None if gscale is None else torch.tensor([gscale], device="cuda"), p, d)
    torch.cuda.synchronize()
    return loss4.cpu().double(), d


def _check(tag, loss4, d, terms, grad, t, gs=1.0):
    for k, name in enumerate(("total", "bce", "dice", "focal")):
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
    void = ~((t == 0) | (t == 1)).cpu().reshape(d.shape)
    if int(void.sum()):
        assert int(d.cpu()[void].view(torch.int32).abs().max()) == 0, tag      # bitwise +0


def _sweep(C, B, H, W, key, names):
    """Every parameter set of `names` x {no void, 20 % void} x {int64, uint8} on one shape; gscale alternates between None and 0.37."""
    lg = S.logits((B, C, H, W), key + "/lg")
    lgd = lg.cuda()
    n = 0
    for void in (False, True):
        t = S.targets((B, C, H, W), key + "/t", key + "/v" if void else None)
        tds = {"int64": t.cuda(), "uint8": t.to(torch.uint8).cuda()}
        for pname in names:
            par = PARAMS[pname]
            w = _weights(C, key + "/" + pname, par[5])
            terms, grad = S.loss_and_grad(lg, t, *w, **_kw(par))
            for dt, td in tds.items():
                gs = None if n % 2 == 0 else 0.37
                n += 1
                loss4, d = _run(lgd, td, w, par, gs)
                _check("C=%d %dx%d void=%s %s %s gs=%s" % (C, H, W, void, pname, dt, gs), loss4, d, terms, grad, t, 1.0 if gs is None else gs)


@pytest.mark.parametrize("H, W", [(37, 45), (36, 44)])
@pytest.mark.parametrize("C", [1, 2, 3, 5, 64])
def test_loss_and_gradient_vs_f64(C, H, W):
    """37x45: HW = 1665 is odd, the one-element form and its tail (1665 = 6 * 256 + 129); 36x44: HW = 1584 = 4 * 396, the four-element
    form and its tail (396 = 256 + 140)."""
    _sweep(C, 2, H, W, "sig_gpu/%d/%dx%d" % (C, H, W), list(PARAMS))


@pytest.mark.parametrize("H, W, pname", [(149, 221, "default"), (149, 221, "all_terms"), (150, 220, "all_terms")])
def test_many_blocks_and_loop_trips(H, W, pname):
    """B = 2, C = 64: 128 planes, so the sums pass runs 2048 / 128 = 16 blocks per plane and the gradient pass 4096 / 128 = 32.
    149x221 = 32929 elements (odd: one element per lane) are 129 trips of 256 lanes: 8-9 per block forward, 4-5 backward;
    150x220 = 33000 (four elements per lane) are 8250 quads, 33 trips of 256 lanes: 2-3 per block forward, 1-2 backward."""
    _sweep(64, 2, H, W, "sig_gpu/big/%dx%d" % (H, W), [pname])


@pytest.mark.parametrize("C", [1, 3, 64])
def test_less_than_one_wave(C):
    _sweep(C, 1, 5, 7, "sig_gpu/tiny/%d" % C, ["default", "weighted", "all_terms"])


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8])
def test_one_fully_void_class(dtype):
    """Class 1 of 3 is not annotated at all: it adds 0 to the bce and focal terms, smooth / smooth - 1 = 0 to Dice, and has no gradient."""
    B, C, H, W = 2, 3, 37, 45
    key = "sig_gpu/voidclass"
    lg = S.logits((B, C, H, W), key + "/lg")
    t = S.targets((B, C, H, W), key + "/t", key + "/v")
    t[:, 1] = 255
    par = PARAMS["all_terms"]
    w = _weights(C, key, True)
    terms, grad = S.loss_and_grad(lg, t, *w, **_kw(par))
    loss4, d = _run(lg.cuda(), t.to(dtype).cuda(), w, par)
    _check("void class", loss4, d, terms, grad, t)
    assert int(d[:, 1].view(torch.int32).abs().max()) == 0


@pytest.mark.parametrize("C", [1, 3])
def test_void_image_equals_the_other_image_alone(C):
    """The valid counts N and N_c and every per-class sum are those of the first image, so nothing changes but the all-zero gradient
    of the second."""
    B, H, W = 2, 37, 45
    key = "sig_gpu/alone/%d" % C
    lg = S.logits((B, C, H, W), key + "/lg").cuda()
    t = S.targets((B, C, H, W), key + "/t", key + "/v")
    t[1] = 255
    t = t.cuda()
    par = PARAMS["all_terms"]
    w = _weights(C, key, True)
    l2, d2 = _run(lg, t, w, par)
    l1, d1 = _run(lg[:1].contiguous(), t[:1].contiguous(), w, par)
    terms, grad = S.loss_and_grad(lg.cpu(), t.cpu(), *w, **_kw(par))
    _check("image + void image", l2, d2, terms, grad, t)
    for k in range(4):
        assert abs(float(l2[k]) - float(l1[k])) < 1e-5 * abs(float(l1[k])), (k, float(l2[k]), float(l1[k]))
    assert float((d2[:1] - d1).abs().max()) < 1e-4 * float(d1.abs().max())
    assert int(d2[1].view(torch.int32).abs().max()) == 0


def test_all_void_batch():
    lg = S.logits((2, 3, 9, 11), "sig_gpu/allvoid").cuda()
    t = torch.full((2, 3, 9, 11), 255, dtype=torch.uint8, device="cuda")
    loss4, d = _run(lg, t, _weights(3, "", False), PARAMS["all_terms"], 0.37)
    assert [float(v) for v in loss4] == [0.0, 0.0, 0.0, 0.0]       # (dice: 1 - smooth / smooth)
    assert int(d.view(torch.int32).abs().max()) == 0


@pytest.mark.parametrize("C", [2, 9])
def test_focal_term_equals_the_softmax_route_focal_loss(C):
    """SigmoidSegLoss(focal alone) on the one-hot planes of a label map against the shipped FocalLoss(C) on the label map."""
    from lm_net_amd import FocalLoss, SigmoidSegLoss
    B, H, W = 2, 37, 45
    lg = S.logits((B, C, H, W), "sig_gpu/cross/%d" % C).cuda()
    y = V.labels(B, H, W, C, "sig_gpu/cross/y%d" % C).cuda()
    planes = torch.nn.functional.one_hot(y, C).permute(0, 3, 1, 2).contiguous()
    a = lg.clone().requires_grad_(True)
    b = lg.clone().requires_grad_(True)
    mine = SigmoidSegLoss(bce_scale=0.0, dice_scale=0.0, focal_scale=1.0)(a, planes)
    ref = FocalLoss(C)(b, y)
    mine.backward()
    ref.backward()
    print("C=%d sigmoid %.9g softmax-route %.9g" % (C, float(mine), float(ref)))
    assert abs(float(mine) - float(ref)) < 1e-5 * abs(float(ref))
    assert float((a.grad - b.grad).abs().max()) < 1e-4 * float(b.grad.abs().max())


@pytest.mark.parametrize("tag", list(S.LOSS_TAGS))
def test_module_through_autograd_vs_reference_golden(tag):
    from lm_net_amd import SigmoidSegLoss
    g = load_golden("sigmoid_loss_stats.npz")
    lg, t, w_bce, pw, w_dice, kw = S.loss_case(tag)
    kw = {{"gamma": "focal_gamma", "alpha": "focal_alpha"}.get(k, k): v for k, v in kw.items()}
    crit = SigmoidSegLoss(w_bce.tolist(), pw.tolist(), w_dice.tolist(), **kw).cuda()
    lg = lg.cuda().requires_grad_(True)
    if tag == "b1":                                               # the [B, H, W] mask of a binary pipeline, as it is
        t = t[:, 0]
    loss = crit(lg, t.cuda())
    (loss * 0.37).backward()
    ref = g[tag + "/loss4"]
    terms = crit.terms.cpu()
    assert terms.shape == (4,) and float(terms[0]) == float(loss.detach())
    for k in range(4):
        print("%s term %d: got %.9g ref %.9g" % (tag, k, float(terms[k]), float(ref[k])))
        assert (float(terms[k]) == 0.0) if ref[k] == 0.0 else abs(float(terms[k]) - ref[k]) < 1e-5 * abs(ref[k])
    grad = lg.grad.cpu().double().numpy() / 0.37
    dig = g[tag + "/grad_digest"]
    err = float(np.abs(S.grad_sample(grad) - g[tag + "/grad_sample"]).max())
    print("%s dlogits sample: err %.3e of %.3e" % (tag, err, dig[3]))
    assert err < 1e-4 * dig[3]
    assert abs(float(np.abs(grad).max()) - dig[3]) < 1e-4 * dig[3]


@pytest.mark.parametrize("C, H, W", [(1, 37, 45), (5, 36, 44), (64, 37, 45)])
def test_deterministic_mode(C, H, W):
    """Two runs in deterministic mode are bit-identical (loss4 and dlogits); the ordinary mode agrees within the tolerances."""
    from lm_net_amd import hip
    key = "sig_gpu/det/%d" % C
    lg = S.logits((2, C, H, W), key + "/lg").cuda()
    t = S.targets((2, C, H, W), key + "/t", key + "/v").cuda()
    w = _weights(C, key, True)
    par = PARAMS["all_terms"]
    plain = _run(lg, t, w, par, 0.37)
    hip.set_deterministic(True)
    try:
        runs = [_run(lg, t, w, par, 0.37) for _ in range(2)]
    finally:
        hip.set_deterministic(False)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    for k in range(4):
        assert abs(float(plain[0][k]) - float(runs[0][0][k])) < 1e-5 * abs(float(runs[0][0][k])), k
    assert float((plain[1] - runs[0][1]).abs().max()) < 1e-4 * float(runs[0][1].abs().max())


@pytest.mark.parametrize("dtype, H, W", [(torch.int64, 32, 32), (torch.uint8, 32, 32), (torch.int64, 37, 45)])
def test_kernel_dispatch(dtype, H, W):
    """The default route launches the instances without the focal term; focal_scale > 0 launches the ones with it.  The template
    arguments are <target kind, four elements per lane, focal>."""
    from lm_net_amd import hip
    lg = S.logits((2, 3, H, W), "sig_gpu/disp").cuda()
    t = S.targets((2, 3, H, W), "sig_gpu/disp/t").to(dtype).cuda()
    kind, vec = (1 if dtype == torch.int64 else 0), ("true" if (H * W) % 4 == 0 else "false")
    for focal, pname in ((False, "default"), (True, "all_terms")):
        torch.cuda.synchronize()
        hip.prof_begin("sigloss")
        _run(lg, t, _weights(3, "", False), PARAMS[pname])
        names = set(hip.prof_end())
        f = "true" if focal else "false"
        want = {"sigloss_sums_kernel<%d, %s, %s>" % (kind, vec, f), "sigloss_bwd_kernel<%d, %s, %s>" % (kind, vec, f), "sigloss_finish_kernel"}
        assert names == want, (focal, names)


def test_plain_segloss_still_runs_only_its_kernels():
    """A plain SegLoss step launches what tests/test_void_loss_gpu.py::test_default_segloss_runs_only_the_old_kernels expects, and
    nothing of this file's entries."""
    from lm_net_amd import SegLoss, hip
    lg = V.det_input((2, 2, 32, 32), "sig_gpu/plain").cuda().requires_grad_(True)
    y = V.labels(2, 32, 32, 2, "sig_gpu/plain/y").cuda()
    torch.cuda.synchronize()
    hip.prof_begin("segloss|sigloss|sigmoid")
    SegLoss().cuda()(lg, y).backward()
    names = set(hip.prof_end())
    assert names == {"segloss_sums_kernel<2>", "segloss_finish_kernel", "segloss_bwd_kernel<2>"}, names

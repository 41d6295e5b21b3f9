"""GPU: the kernels of include/region/lmnet_region.h (lm_net_amd/csrc/region.hip) behind RegionLoss and region_sums, against the
float64 restatement tests/region_ref.py on the same fp32 inputs, with the bars of tests/test_distmap_kernels_gpu.py:
|L - ref| <= 1e-5 |ref|, max |dlogits - ref| <= 1e-4 max |ref|, per_class held to the loss bar element by element,
counts exactly equal.  The shapes are the smallest that reach every instance and every boundary: the templated class counts, general
C below and above one pixel group per wave and at 64, one pixel, odd sizes, several blocks per image, the vector and the scalar
sigmoid route.  kernel_forms.launched asserts which instance ran."""
import numpy as np
import pytest
import torch

import region_ref as R
from kernel_forms import launched

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

SOFTMAX = [(1, 2, 1, 1), (2, 3, 5, 7), (3, 4, 16, 16), (2, 8, 24, 40), (2, 5, 9, 11), (2, 9, 32, 36), (1, 64, 8, 8), (2, 2, 96, 100)]
SIGMOID = [(2, 1, 5, 7), (2, 3, 16, 20), (2, 9, 33, 31), (1, 64, 8, 8), (2, 1, 96, 100)]
KINDS = [("dice", "squared"), ("dice", "linear"), ("jaccard", "squared"), ("jaccard", "linear"), ("tversky", "linear"), ("generalized_dice", "linear")]


def _run(crit, lg, y, gscale=1.0):
    """(loss, dlogits float64, per_class, counts) of one forward + backward"""
    z = torch.from_numpy(lg).to(DEV).requires_grad_(True)
    loss = crit(z, torch.from_numpy(y).to(DEV))
    (loss * gscale).backward()
    return float(loss.detach()), z.grad.cpu().numpy().astype(np.float64), crit.per_class.cpu().numpy().astype(np.float64), crit.counts.cpu().numpy()


def _compare(got, r, what):
    loss, d, per_class, counts = got
    assert np.array_equal(counts, r.counts), what
    assert abs(loss - r.loss) <= 1e-5 * abs(r.loss), (what, loss, r.loss)
    assert np.all(np.abs(per_class - r.per_class) <= 1e-5 * np.abs(r.per_class)), (what, per_class, r.per_class)
    assert np.abs(d - r.grad).max() <= 1e-4 * np.abs(r.grad).max(), (what, np.abs(d - r.grad).max(), np.abs(r.grad).max())


def _expected_forms(head, C, H, W, den, dtype):
    """(prefixes that must be launched, prefixes that must not)"""
    sq, kind = "true" if den == "squared" else "false", "0" if dtype == np.uint8 else "1"
    if head == "softmax":
        if C in (2, 3, 4, 8):
            return (["rg_softmax_sums_kernel<%d, %s, %s>" % (C, sq, kind), "rg_softmax_bwd_kernel<%d, %s>" % (C, kind), "rg_finish_kernel"],
                    ["rg_softmax_sums_gen_kernel<", "rg_softmax_bwd_gen_kernel<", "rg_sigmoid_"])
        return (["rg_softmax_sums_gen_kernel<%s, %s>" % (sq, kind), "rg_softmax_bwd_gen_kernel<%s>" % kind, "rg_finish_kernel"],
                ["rg_softmax_sums_kernel<", "rg_softmax_bwd_kernel<", "rg_sigmoid_"])
    vec = "true" if H * W % 4 == 0 else "false"
    return (["rg_sigmoid_sums_kernel<%s, %s, %s>" % (vec, sq, kind), "rg_sigmoid_bwd_kernel<%s, %s>" % (vec, kind), "rg_finish_kernel"],
            ["rg_softmax_", "rg_sigmoid_sums_kernel<%s" % ("false" if vec == "true" else "true")])


@pytest.mark.parametrize("head,shape", [("softmax", s) for s in SOFTMAX] + [("sigmoid", s) for s in SIGMOID],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_loss_and_gradient_vs_f64(head, shape):
    """Every kind and denominator, per batch and per image, on inputs with 20 % void; the class subset, the weights, the exponent and
    the target type take both their values across the twelve combinations, in an order that differs from shape to shape.  The
    instance that ran is asserted: templated against general C, vector against scalar, and no P2 for the linear kinds."""
    from lm_net_amd import RegionLoss
    B, C, H, W = shape
    salt = (SOFTMAX + SIGMOID).index(shape)
    n = 0
    for per_image in (False, True):
        for kind, den in KINDS:
            bits = (5 * n + salt) % 16
            n += 1
            subset, weighted, frac, u8 = bits & 1, (bits >> 1) & 1, (bits >> 2) & 1, (bits >> 3) & 1
            classes = None if not subset or C == 1 else ([C - 1] if C == 2 else [1, C - 1])
            nk = len(R.class_ids(C, classes))
            weight = [1.0 + 1.5 * k for k in range(nk)] if weighted and kind != "generalized_dice" else None
            kw = dict(kind=kind, head=head, classes=classes, weight=weight, per_image=per_image, denominator=den, smooth=1e-5, alpha=0.3, beta=0.7,
                      exponent=0.75 if frac else 1.0, scale=0.7)
            dtype = np.uint8 if u8 else np.int64
            lg, y = R.inputs(B, C, H, W, head, seed=100 + n, void=0.2, dtype=dtype)
            if shape[2:] == (1, 1):
                y[:] = 1                                   # (one pixel: keep it valid)
            crit = RegionLoss(C, **kw).to(DEV)
            got, names = launched(lambda: _run(crit, lg, y, gscale=0.5))
            what = "%s %s %s" % (head, shape, kw)
            _compare(got, R.loss_and_grad(lg, y, C, gscale=0.5, **kw), what)
            want, never = _expected_forms(head, C, H, W, den, dtype)
            hit = lambda p: any(nm.startswith(p) for nm in names)
            assert all(hit(p) for p in want) and not any(hit(p) for p in never), (what, sorted(names))


@pytest.mark.parametrize("head,shape", [("softmax", (2, 3, 5, 7)), ("softmax", (2, 9, 32, 36)), ("sigmoid", (2, 3, 16, 20))],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_all_void_image_inside_a_batch(head, shape):
    """One all-void image inside a batch: its gradient is exactly +0 in every class (the sign bit is checked), per batch and per
    image, and the values still equal the restatement."""
    from lm_net_amd import RegionLoss
    B, C, H, W = shape
    lg, y = R.inputs(B, C, H, W, head, seed=3, void=0.2)
    y[1] = R.VOID
    for kind, den in KINDS:
        for per_image in (False, True):
            kw = dict(kind=kind, head=head, per_image=per_image, denominator=den, exponent=0.75)
            crit = RegionLoss(C, **kw).to(DEV)
            got = _run(crit, lg, y, gscale=-2.0)           # (a negative factor: -0 would show)
            _compare(got, R.loss_and_grad(lg, y, C, gscale=-2.0, **kw), (kind, den, per_image))
            d = got[1][1]
            assert not d.any() and not np.signbit(d).any()
            if per_image:
                assert not got[2][1].any() and not got[3][1].any()


@pytest.mark.parametrize("head", ["softmax", "sigmoid"])
def test_saturated_logits_stay_finite(head):
    """Logits of +-100 on a full-foreground plane under exponent = 0.75: p rounds to exactly 1 (or 0) in fp32, u <= 0 where the plane
    is matched, and loss and gradient stay finite."""
    from lm_net_amd import RegionLoss
    B, C, H, W = 2, 2, 8, 8
    for sign in (100.0, -100.0):
        lg = np.full((B, C, H, W), -sign, dtype=np.float32)
        lg[:, 1] = sign
        y = np.ones((B, H, W) if head == "softmax" else (B, C, H, W), dtype=np.int64)
        for kind, den in KINDS:
            for per_image in (False, True):
                crit = RegionLoss(C, kind=kind, head=head, classes=[1], per_image=per_image, denominator=den, exponent=0.75)
                got = _run(crit, lg, y)
                loss, d, per_class, counts = got
                assert np.isfinite(loss) and np.isfinite(d).all() and np.isfinite(per_class).all(), (kind, den, sign)
                r = R.loss_and_grad(lg, y, C, kind=kind, head=head, classes=[1], per_image=per_image, denominator=den, exponent=0.75)
                if sign > 0:                               # matched: u <= 0, the loss and every coefficient are 0
                    assert loss == 0.0 and not d.any(), (kind, den, loss)
                    _compare(got, r, (kind, den, sign, per_image))
                else:                                      # missed: u is 1 up to the smoothing; the gradient is p (1 - p) d with p ~ 1e-44
                    assert 0.99 < loss <= 1.0 and abs(loss - r.loss) <= 1e-5 * abs(r.loss) and np.abs(d).max() < 1e-30, (kind, den, loss, r.loss)


@pytest.mark.parametrize("head,shape", [("softmax", (2, 2, 96, 100)), ("softmax", (2, 9, 32, 36)), ("sigmoid", (2, 3, 16, 20)), ("sigmoid", (2, 1, 5, 7))],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_deterministic_mode_is_bit_identical(head, shape):
    """Two calls in deterministic mode agree bit for bit in loss, per_class and dlogits; the counts agree between the two modes; the
    deterministic values keep the bars."""
    from lm_net_amd import RegionLoss, hip
    B, C, H, W = shape
    lg, y = R.inputs(B, C, H, W, head, seed=17, void=0.2)
    was = hip.get_deterministic()
    try:
        for kind, den in (("dice", "squared"), ("tversky", "linear"), ("generalized_dice", "linear")):
            for per_image in (False, True):
                kw = dict(kind=kind, head=head, per_image=per_image, denominator=den, exponent=0.75)
                crit = RegionLoss(C, **kw).to(DEV)
                hip.set_deterministic(False)
                plain = _run(crit, lg, y)
                hip.set_deterministic(True)
                a, b = _run(crit, lg, y), _run(crit, lg, y)
                assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
                assert np.array_equal(a[3], plain[3]) and np.array_equal(a[3], b[3])
                _compare(a, R.loss_and_grad(lg, y, C, **kw), (kind, per_image))
    finally:
        hip.set_deterministic(was)


@pytest.mark.parametrize("C,weight", [(2, (1.0, 4.0)), (9, (1.0,) * 9)])
def test_dice_term_of_segloss(C, weight):
    """RegionLoss(C, weight=w) -- dice, squared, per batch, smooth 1e-5 -- is the Dice term of SegLoss: the two kernel families agree
    within the loss and gradient bars at (2, C, 32, 36), and both with the restatement."""
    from lm_net_amd import RegionLoss, SegLoss
    lg, y = R.inputs(2, C, 32, 36, seed=23, void=0.2)
    reg = RegionLoss(C, weight=weight).to(DEV)
    seg = SegLoss(ce_weight=weight, dice_weight=weight, ce_scale=0.0).to(DEV)
    got = _run(reg, lg, y)
    z = torch.from_numpy(lg).to(DEV).requires_grad_(True)
    ls = seg(z, torch.from_numpy(y).to(DEV))
    ls.backward()
    want, wd = float(ls.detach()), z.grad.cpu().numpy().astype(np.float64)
    assert abs(got[0] - want) <= 1e-5 * abs(want), (got[0], want)
    assert np.abs(got[1] - wd).max() <= 1e-4 * np.abs(wd).max()
    _compare(got, R.loss_and_grad(lg, y, C, weight=weight), C)


@pytest.mark.parametrize("head,shape", [("softmax", (2, 4, 16, 16)), ("sigmoid", (2, 3, 16, 20))], ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_region_sums(head, shape):
    """region_sums: the soft overlaps I, P1, P2 within 1e-5 of float64 and T, N exactly, per batch and per image, on a class subset."""
    from lm_net_amd import region_sums
    B, C, H, W = shape
    lg, y = R.inputs(B, C, H, W, head, seed=29, void=0.2, dtype=np.uint8)
    for per_image in (False, True):
        sums, counts = region_sums(torch.from_numpy(lg).to(DEV), torch.from_numpy(y).to(DEV), C, head=head, classes=[1, C - 1], per_image=per_image)
        r = R.loss_and_grad(lg, y, C, head=head, classes=[1, C - 1], per_image=per_image)
        assert np.array_equal(counts.cpu().numpy(), r.counts)
        assert np.abs(sums.cpu().numpy() - r.sums).max() <= 1e-5 * np.abs(r.sums).max()

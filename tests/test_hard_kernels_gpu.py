"""GPU: the kernels of include/hard/lmnet_hard.h (lm_net_amd/csrc/hard.hip) behind HardPixelLoss and hard_pixel_values.

Selection is EXACT: on the device's own fp32 values, N, K, n_gt, n_eq and the bits of tau equal numpy's (np.partition and counts on
the same array, tests/hard_ref.record_of) -- at the templated class counts 2, 3, 4, 8 and the general ones 5 and 64, on 2 x 24 x 40
and on 2 x 96 x 96 (several blocks per group), under sigmoid heads at 1 and 3 planes with H * W % 4 == 0 and at 7 x 9 (scalar loads),
in every mode, per batch and per image, with 20 % void, an all-void group, K = 1 and keep = 1.0, and on logits built so that the values
differ only in the low 10, the middle 11 or the top 11 key bits (every digit, every digit boundary) or not at all (the tie rule).

Values, loss and gradient against the float64 restatement tests/hard_ref.py, every element compared:
  values   |v - l| <= hard_ref.VALUES_BAR * max(1, l) = 4.36e-6: 8 x the largest deviation measured on an MI355X over the shapes
           of this file, 5.452e-07 (softmax head, 64 classes, 2 x 96 x 96, logits of scale 3); every test prints its own figure
  loss     |L - ref| <= 1e-5 |ref|                   the bars of tests/test_region_kernels_gpu.py
  dlogits  max |d - ref| <= 1e-4 max |ref|           the gradient taken on the device's own selection
kernel_forms.launched asserts which instance ran."""
import numpy as np
import pytest
import torch

import hard_ref as R
from kernel_forms import launched

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

SOFTMAX = [(2, 2, 24, 40), (2, 3, 24, 40), (2, 4, 24, 40), (2, 8, 24, 40), (2, 5, 24, 40), (2, 64, 24, 40), (2, 2, 96, 96), (2, 3, 96, 96), (2, 4, 96, 96),
           (2, 8, 96, 96), (2, 5, 96, 96), (2, 64, 96, 96), (1, 2, 1, 1), (3, 3, 5, 7)]
SIGMOID = [(2, 1, 24, 40), (2, 3, 24, 40), (2, 1, 96, 96), (2, 3, 96, 96), (2, 1, 7, 9), (2, 3, 7, 9), (1, 64, 8, 8)]
MODES = [dict(keep=0.1), dict(min_kept=100), dict(thresh=0.7), dict(thresh=0.7, min_kept=300), dict(keep=0.05, thresh=0.3), dict(keep=0.2, min_kept=50, thresh=0.9),
         dict(keep=1.0), dict(keep=1e-9), dict(min_kept=10 ** 9)]
IDS = lambda v: v if isinstance(v, str) else ("x".join(map(str, v)) if isinstance(v, tuple) else None)
ALL = [("softmax", s) for s in SOFTMAX] + [("sigmoid", s) for s in SIGMOID]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _values(lg, y, C, head, **kw):
    from lm_net_amd import hard_pixel_values
    v, s = hard_pixel_values(_dev(lg), _dev(y), C, head=head, **kw)
    return v.cpu().numpy(), s.cpu().numpy()


def _run(crit, lg, y, gscale=1.0):
    """(loss, dlogits float64, values, selection, terms) of one forward + backward"""
    z = _dev(lg).requires_grad_(True)
    loss = crit(z, _dev(y))
    (loss * gscale).backward()
    return (float(loss.detach()), z.grad.cpu().numpy().astype(np.float64), crit.values.cpu().numpy(), crit.selection.cpu().numpy(),
            crit.terms.cpu().numpy().astype(np.float64))


def _check_selection(vals, sel, valid, per_image, kw, what):
    assert np.array_equal(vals >= 0, valid) and (vals[~valid] == -1).all(), what
    want = R.record_of(vals, valid, per_image, **kw)
    assert sel.dtype == np.int32 and np.array_equal(sel, want), (what, sel, want)


def _compare(got, r, what):
    loss, d, vals, sel, terms = got
    dev = np.abs(vals - r.values)[r.valid] / np.maximum(1.0, r.values[r.valid]) if r.valid.any() else np.zeros(1)
    print("hard values %s: max deviation %.3e of max(1, l) (bar %.1e)" % (what, dev.max(), R.VALUES_BAR))
    assert dev.max() <= R.VALUES_BAR, (what, dev.max())
    assert abs(loss - r.loss) <= 1e-5 * abs(r.loss), (what, loss, r.loss)
    assert np.all(np.abs(terms - r.terms) <= 1e-5 * np.abs(r.terms)), (what, terms, r.terms)
    assert d.shape == r.grad.shape and np.abs(d - r.grad).max() <= 1e-4 * np.abs(r.grad).max(), (what, np.abs(d - r.grad).max(), np.abs(r.grad).max())
    assert not d[r.grad == 0].any() and not np.signbit(d[r.grad == 0]).any(), what           # void and unselected: exactly +0
    return dev.max()


def _expected_forms(head, C, H, W, per_image, B):
    M = (1 if per_image else B) * (C if head == "sigmoid" else 1) * H * W
    lv = "true" if M % 4 == 0 else "false"
    levels = ["hp_level_kernel<%d, %s>" % (k, lv) for k in (2, 3, 4)] + ["hp_finish_kernel"]
    if head == "softmax":
        ct = C if C in (2, 3, 4, 8) else 0
        return ["hp_softmax_values_kernel<%d>" % ct, "hp_softmax_bwd_kernel<%d>" % ct] + levels, ["hp_sigmoid_"]
    vec = "true" if H * W % 4 == 0 else "false"
    return ["hp_sigmoid_values_kernel<%s>" % vec, "hp_sigmoid_bwd_kernel<%s>" % vec] + levels, ["hp_softmax_", "hp_sigmoid_values_kernel<%s>" % ("false" if vec == "true" else "true")]


@pytest.mark.parametrize("head,shape", ALL, ids=IDS)
def test_selection_is_exact(head, shape):
    """Every mode, per batch and per image, 20 % void and image 1 entirely void in every other combination: the record is numpy's
    selection on the device's own values."""
    B, C, H, W = shape
    salt = ALL.index((head, shape))
    n = 0
    for per_image in (False, True):
        for kw in MODES:
            n += 1
            lg, y = R.inputs(B, C, H, W, head, seed=1000 * salt + n, void=0.0 if H * W == 1 else 0.2, dtype=np.uint8 if n % 2 else np.int64, scale=1.0 + (n % 3))
            if n % 2 == 0 and B > 1:
                y[1] = R.VOID
            weight = [0.5 + 0.5 * k for k in range(C)] if n % 3 == 0 else None
            vals, sel = _values(lg, y, C, head, weight=weight, per_image=per_image, **kw)
            _, valid, _ = R.values(lg, y, head)
            what = "%s %s per_image=%s %s" % (head, shape, per_image, kw)
            _check_selection(vals, sel, valid, per_image, kw, what)
            N, K = sel[:, 0], sel[:, 1]
            assert ((K >= 1) == (N > 0)).all() and (K <= N).all() and (sel[:, 2] < np.maximum(K, 1)).all() and (sel[:, 2] + sel[:, 3] >= K).all(), what
            if kw == dict(keep=1.0) or kw == dict(min_kept=10 ** 9):
                assert np.array_equal(K, N), what
            if kw == dict(keep=1e-9):
                assert (K == (N > 0)).all(), what
            if n % 2 == 0 and B > 1 and per_image:
                assert not sel[1].any(), what                # the all-void group: an all-zero record


def _bits_to_logits(bits, shape, rng):
    """sigmoid-head logits [B, 1, H, W] whose value against target 0 is the logit itself: softplus(z) == z in fp32 from z = 32 on"""
    z = np.asarray(bits, np.uint32).view(np.float32)
    assert (z >= 32.0).all() and np.isfinite(z).all()
    return rng.permutation(z).reshape(shape).copy()


@pytest.mark.parametrize("digit", ["low10", "middle11", "top11", "equal"])
def test_selection_digit_by_digit(digit):
    """Values that differ in one digit of the key only, every pattern repeated (so the cutoffs are tied), at ranks that put tau on
    the first, the second, an inner, the last but one and the last bin of that digit; and a batch whose values are all equal."""
    from lm_net_amd import HardPixelLoss
    B, H, W = 2, 32, 48
    n = B * H * W
    rng = np.random.default_rng(7)
    j = np.arange(n, dtype=np.uint64)
    if digit == "low10":
        bits, distinct = 0x42000000 + (j % 1024), 1024
    elif digit == "middle11":
        bits, distinct = 0x42000000 + ((j % 1024) * 2 + (j // 1024) % 2 << 10), 2048
    elif digit == "top11":
        bits, distinct = ((0x420 >> 1) + 1 + (j % 480) << 21) | 0x12345, 480
    else:
        bits, distinct = np.full(n, 0x42280000, np.uint64), 1
    lg = _bits_to_logits(bits.astype(np.uint32), (B, 1, H, W), rng)
    y = np.zeros((B, 1, H, W), np.uint8)
    y[rng.random(y.shape) < 0.1] = R.VOID
    valid = y == 0
    for per_image in (False, True):
        Nmin = int(R.grouped(valid, per_image).sum(1).min())
        for K in (1, 2, 3, 4, 7, Nmin // 2, Nmin - 7, Nmin - 3, Nmin - 1, Nmin):
            vals, sel = _values(lg, y, 1, "sigmoid", per_image=per_image, min_kept=K)
            assert np.array_equal(vals[valid].view(np.uint32), lg[valid].view(np.uint32))      # the keys are the logits' bits
            _check_selection(vals, sel, valid, per_image, dict(min_kept=K), (digit, per_image, K))
            assert (sel[:, 1] == K).all()
        if digit == "equal":
            assert (sel[:, 2] == 0).all() and np.array_equal(sel[:, 3], sel[:, 0])
    assert len(np.unique(lg)) == distinct
    # the tie rule in the gradient: sigmoid(z) = 1 at these logits, so dlogits is the gradient weight itself
    crit = HardPixelLoss(1, head="sigmoid", min_kept=Nmin // 2, per_image=True)
    loss, d, vals, sel, terms = _run(crit, lg, y)
    r = R.loss_and_grad(lg, y, 1, head="sigmoid", min_kept=Nmin // 2, per_image=True, device=(vals, sel))
    assert np.abs(d - r.grad).max() <= 1e-4 * np.abs(r.grad).max() and abs(loss - r.loss) <= 1e-5 * abs(r.loss)
    wsum = R.grouped(d, True).sum(1) * B
    assert np.all(np.abs(wsum - 1.0) <= 1e-5), wsum                                         # the weights of a group sum to 1
    tau = sel[:, 4].copy().view(np.float32)
    for g in range(B):
        tied = d[g][(vals[g] == tau[g])]
        assert tied.size == sel[g, 3] and len(np.unique(tied)) == 1 and (tied > 0).all()     # tied elements carry one weight
        assert not d[g][vals[g] < tau[g]].any()


@pytest.mark.parametrize("head,shape", ALL, ids=IDS)
def test_values_loss_and_gradient_vs_f64(head, shape):
    """Three modes per shape, per batch and per image, with class weights in every other combination; the gradient is taken on the
    device's own selection and every element is compared.  The instance that ran is asserted."""
    from lm_net_amd import HardPixelLoss
    B, C, H, W = shape
    salt = ALL.index((head, shape))
    n, worst = 0, 0.0
    for per_image in (False, True):
        for kw in (MODES[(salt + i) % len(MODES)] for i in (0, 3, 6)):
            n += 1
            lg, y = R.inputs(B, C, H, W, head, seed=2000 * salt + n, void=0.0 if H * W == 1 else 0.2, dtype=np.uint8 if n % 2 else np.int64, scale=1.0 + 2.0 * (n % 2))
            weight = [0.5 + 0.5 * k for k in range(C)] if n % 2 == 0 else None
            crit = HardPixelLoss(C, head=head, weight=weight, per_image=per_image, scale=0.7, **kw).to(DEV)
            got, names = launched(lambda: _run(crit, lg, y, gscale=-0.5))
            what = "%s %s per_image=%s %s weight=%s" % (head, shape, per_image, kw, weight is not None)
            r = R.loss_and_grad(lg, y, C, head=head, weight=weight, per_image=per_image, scale=0.7, gscale=-0.5, device=(got[2], got[3]), **kw)
            _check_selection(got[2], got[3], r.valid, per_image, kw, what)
            worst = max(worst, _compare(got, r, what))
            if "thresh" not in kw:                         # without thresh K is integer arithmetic: the restatement's own selection agrees in K
                own = R.loss_and_grad(lg, y, C, head=head, weight=weight, per_image=per_image, scale=0.7, **kw)
                assert np.array_equal(own.record[:, :2], got[3][:, :2]) and abs(got[0] - own.loss) <= 1e-5 * abs(own.loss), what
            want, never = _expected_forms(head, C, H, W, per_image, B)
            hit = lambda p: any(nm.startswith(p) for nm in names)
            assert all(hit(p) for p in want) and not any(hit(p) for p in never), (what, sorted(names))
    print("hard values %s %s: worst deviation %.3e" % (head, shape, worst))


@pytest.mark.parametrize("C", [2, 5])
def test_keep_one_is_the_cross_entropy_of_segloss(C):
    """HardPixelLoss(C, keep=1.0) is SegLoss(None, None, dice_scale=0): the mean cross entropy over the valid pixels; the two kernel
    families agree within the loss and gradient bars at (2, C, 32, 36)."""
    from lm_net_amd import HardPixelLoss, SegLoss
    lg, y = R.inputs(2, C, 32, 36, seed=23, void=0.2)
    got = _run(HardPixelLoss(C, keep=1.0).to(DEV), lg, y)
    z = _dev(lg).requires_grad_(True)
    ls = SegLoss(None, None, dice_scale=0).to(DEV)(z, _dev(y))
    ls.backward()
    want, wd = float(ls.detach()), z.grad.cpu().numpy().astype(np.float64)
    assert abs(got[0] - want) <= 1e-5 * abs(want), (got[0], want)
    assert np.abs(got[1] - wd).max() <= 1e-4 * np.abs(wd).max()
    _compare(got, R.loss_and_grad(lg, y, C, keep=1.0, device=(got[2], got[3])), C)


@pytest.mark.parametrize("head,shape", [("softmax", (2, 2, 96, 96)), ("softmax", (2, 5, 24, 40)), ("sigmoid", (2, 3, 24, 40)), ("sigmoid", (2, 1, 7, 9))], ids=IDS)
def test_two_calls_are_bit_identical_in_both_modes(head, shape):
    """No float atomics: loss, terms, record, values and dlogits are bit-identical from call to call with deterministic mode off and
    on, and between the two modes."""
    from lm_net_amd import HardPixelLoss, hip
    B, C, H, W = shape
    lg, y = R.inputs(B, C, H, W, head, seed=17, void=0.2)
    was = hip.get_deterministic()
    try:
        for kw in (dict(keep=0.1), dict(thresh=0.7, min_kept=100, per_image=True)):
            crit = HardPixelLoss(C, head=head, **kw).to(DEV)
            runs = []
            for det in (False, False, True, True):
                hip.set_deterministic(det)
                runs.append(_run(crit, lg, y))
            for other in runs[1:]:
                assert other[0] == runs[0][0] and all(a.tobytes() == b.tobytes() for a, b in zip(other[1:], runs[0][1:])), kw
    finally:
        hip.set_deterministic(was)


@pytest.mark.parametrize("head,shape", [("softmax", (2, 3, 24, 40)), ("sigmoid", (2, 3, 7, 9))], ids=IDS)
def test_scale_and_upstream_factor_are_linear(head, shape):
    """`scale` (read at every call) and an upstream gradient factor scale loss and gradient linearly; void and unselected positions
    stay exactly +0 under a negative factor; an all-void batch gives loss 0 and an all-zero gradient, never NaN."""
    from lm_net_amd import HardPixelLoss
    B, C, H, W = shape
    lg, y = R.inputs(B, C, H, W, head, seed=31, void=0.2)
    crit = HardPixelLoss(C, head=head, keep=0.2).to(DEV)
    base = _run(crit, lg, y)
    crit.scale = -3.0
    scaled = _run(crit, lg, y, gscale=0.25)
    assert abs(scaled[0] + 3.0 * base[0]) <= 1e-6 * abs(base[0]) and np.array_equal(scaled[3], base[3])
    assert np.abs(scaled[1] + 0.75 * base[1]).max() <= 1e-6 * np.abs(base[1]).max()
    zero = base[1] == 0
    assert zero.any() and not scaled[1][zero].any() and not np.signbit(scaled[1][zero]).any()
    void = np.full_like(y, R.VOID)
    loss, d, vals, sel, terms = _run(crit, lg, void)
    assert loss == 0.0 and not d.any() and not np.signbit(d).any() and not sel.any() and (vals == -1).all() and not terms.any()
    sat = np.where(np.arange(C)[None, :, None, None] == 0, 100.0, -100.0).astype(np.float32) * np.ones_like(lg)
    loss, d, vals, sel, terms = _run(crit, sat, y)              # saturated logits stay finite
    assert np.isfinite(loss) and np.isfinite(d).all() and np.isfinite(vals).all()

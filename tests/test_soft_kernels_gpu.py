"""GPU: the kernels of include/soft/lmnet_soft.h (lm_net_amd/csrc/soft.hip) behind SoftSegLoss and DistillLoss, against the float64
restatement tests/soft_ref.py on the same inputs, with the bars of tests/test_distmap_kernels_gpu.py: |L - ref| <= 1e-5 |ref| for
total, ce and dice, max |dlogits - ref| <= 1e-4 max |ref|, N exactly equal.  For the distillation term the loss bar is 1e-5 *
magnitude: the divergence is a difference of two sums of that size (soft_ref.distill), and a plain fp32 evaluation on the CPU
already misses 1e-5 |ref| at one pixel and T = 4.  The shapes are the siblings': every templated class count, general C on both sides
of a wave's pixel group and at 64, one pixel, odd sizes, several blocks per image, the vector and the scalar routes.
kernel_forms.launched asserts which instance ran: templated against general, vector against scalar, the reader."""
import numpy as np
import pytest
import torch

import soft_ref as R
from kernel_forms import launched

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

SOFTMAX, SIGMOID, TEMPERATURES = R.SOFTMAX, R.SIGMOID, R.TEMPERATURES
ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _t(a, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(torch.bfloat16) if bf16 else t


def _target(r, reader):
    from lm_net_amd import MixedTarget
    return _t(r.q) if reader == "probs" else MixedTarget(_t(r.ya), _t(r.yb), _t(r.lam))


def _run(crit, r, reader, gscale=1.0):
    """(terms float64 [3], dlogits float64, N) of one forward + backward"""
    z = _t(r.lg).requires_grad_(True)
    if reader in ("probs", "pair"):
        loss = crit(z, _target(r, reader))
    else:
        loss = crit(z, _t(r.zt, reader == "teacher_bf16"), None if r.valid is None else _t(r.valid))
    (loss * gscale).backward()
    terms = crit.terms.cpu().numpy().astype(np.float64)
    assert float(loss.detach()) == terms[0]
    return terms, z.grad.cpu().numpy().astype(np.float64), int(crit.counts.cpu()[0])


def _compare_seg(got, ref, what, ce_scale=1.0, dice_scale=1.0):
    terms, d, N = got
    print(what, "terms", terms, "ref", (ref.loss, ref.ce, ref.dice), "grad err", np.abs(d - ref.grad).max(), "of", np.abs(ref.grad).max())
    assert N == ref.N, what
    for g, want in zip(terms, (ref.loss, ref.ce, ref.dice)):
        assert abs(g - want) <= 1e-5 * abs(want), (what, terms, (ref.loss, ref.ce, ref.dice))
    assert np.abs(d - ref.grad).max() <= 1e-4 * np.abs(ref.grad).max(), (what, np.abs(d - ref.grad).max(), np.abs(ref.grad).max())


def _compare_kd(got, ref, what, scale=1.0):
    terms, d, N = got
    print(what, "terms", terms, "ref", (ref.loss, ref.kd), "magnitude", ref.magnitude, "grad err", np.abs(d - ref.grad).max(), "of",
          np.abs(ref.grad).max())
    assert N == ref.N, what
    assert abs(terms[1] - ref.kd) <= 1e-5 * ref.magnitude and abs(terms[0] - ref.loss) <= 1e-5 * abs(scale) * ref.magnitude, (what, terms, ref.loss, ref.kd)
    assert terms[2] == 0.0
    assert np.abs(d - ref.grad).max() <= 1e-4 * np.abs(ref.grad).max(), (what, np.abs(d - ref.grad).max(), np.abs(ref.grad).max())


def _forms(names, want, never, what):
    hit = lambda p: any(nm.startswith(p) for nm in names)
    assert all(hit(p) for p in want) and not any(hit(p) for p in never), (what, want, sorted(names))


def _softmax_forms(C, H, W, reader):
    ct = C if C in (2, 3, 4, 8) else 0
    e = 4 if reader == "teacher_bf16" and H * W % 4 == 0 else 1
    inst = "<%d, %d, %d>" % (ct, R.READERS.index(reader), e)
    other = ["sf_softmax_sums_kernel<%d," % k for k in (0, 2, 3, 4, 8) if k != ct]
    return ["sf_softmax_sums_kernel" + inst, "sf_softmax_bwd_kernel" + inst, "sf_finish_kernel"], other + ["sf_sigmoid_"]


@pytest.mark.parametrize("shape", SOFTMAX, ids=ids)
def test_softmax_head_vs_f64(shape):
    """Every reader on inputs with 20 % void (soft_ref.softmax_cases: the label type, the weights, the smoothing, the temperature and
    the sign of the incoming gradient vary in an order that differs from shape to shape).  The instance that ran is asserted."""
    from lm_net_amd import DistillLoss, SoftSegLoss
    B, C, H, W = shape
    for k in R.softmax_cases(shape):
        if k.reader in ("probs", "pair"):
            kw = dict(w_ce=[1.0 + 1.5 * c for c in range(C)] if k.weighted else None, w_dice=[2.0 - 0.5 * (c % 3) for c in range(C)] if k.weighted else None,
                      eps=k.eps, ce_scale=0.7, dice_scale=1.3)
            crit = SoftSegLoss(C, ce_weight=kw["w_ce"], dice_weight=kw["w_dice"], label_smoothing=k.eps, ce_scale=0.7, dice_scale=1.3).to(DEV)
            got, names = launched(lambda: _run(crit, k.r, k.reader, k.gscale))
            _compare_seg(got, R.loss_and_grad(k.r, k.reader, gscale=k.gscale, **kw), k.what)
        else:
            crit = DistillLoss(C, temperature=k.T, scale=0.6)
            got, names = launched(lambda: _run(crit, k.r, k.reader, k.gscale))
            _compare_kd(got, R.loss_and_grad(k.r, k.reader, T=k.T, scale=0.6, gscale=k.gscale), k.what, 0.6)
        _forms(names, *_softmax_forms(C, H, W, k.reader), k.what)


@pytest.mark.parametrize("shape", SIGMOID, ids=ids)
def test_sigmoid_head_vs_f64(shape):
    """Both teacher readers under the sigmoid head, with and without the valid planes (soft_ref.sigmoid_cases)."""
    from lm_net_amd import DistillLoss
    B, C, H, W = shape
    for k in R.sigmoid_cases(shape):
        crit = DistillLoss(C, temperature=k.T, head="sigmoid", scale=0.6)
        got, names = launched(lambda: _run(crit, k.r, k.reader, k.gscale))
        _compare_kd(got, R.loss_and_grad(k.r, k.reader, "sigmoid", T=k.T, scale=0.6, gscale=k.gscale), k.what, 0.6)
        inst = "<%s, %s>" % ("true" if H * W % 4 == 0 else "false", "true" if k.reader == "teacher_bf16" else "false")
        _forms(names, ["sf_sigmoid_sums_kernel" + inst, "sf_sigmoid_bwd_kernel" + inst, "sf_finish_kernel"], ["sf_softmax_"], k.what)


def _void_image(r, reader, head, b):
    if reader == "probs":
        r.q[b, 0] = np.nan
    elif reader == "pair":
        r.ya[b] = R.VOID
    else:
        r.valid[b] = R.VOID


def _crit(reader, head, C, T=4.0):
    from lm_net_amd import DistillLoss, SoftSegLoss
    if reader in ("probs", "pair"):
        return SoftSegLoss(C, label_smoothing=0.1).to(DEV), dict(eps=0.1)
    return DistillLoss(C, temperature=T, head=head), dict(T=T)


CASES = [("softmax", (2, 3, 5, 7)), ("softmax", (2, 9, 32, 36)), ("sigmoid", (2, 3, 16, 20))]


@pytest.mark.parametrize("head,shape", CASES, ids=ids)
def test_all_void_image_inside_a_batch_and_all_void_input(head, shape):
    """One all-void image inside a batch: its gradient is exactly +0 in every class (the sign bit is checked under a negative incoming
    gradient) and the values still equal the restatement.  An all-void input: every term 0, no gradient bit set."""
    B, C, H, W = shape
    for reader in (R.READERS if head == "softmax" else R.READERS[2:]):
        r = R.inputs(B, C, H, W, reader, head, seed=3, void=0.2)
        _void_image(r, reader, head, 1)
        crit, kw = _crit(reader, head, C)
        got = _run(crit, r, reader, gscale=-2.0)
        ref = R.loss_and_grad(r, reader, head, gscale=-2.0, **kw)
        (_compare_seg if reader in ("probs", "pair") else _compare_kd)(got, ref, (head, reader))
        assert not got[1][1].any() and not np.signbit(got[1][1]).any()
        _void_image(r, reader, head, 0)
        terms, d, N = _run(crit, r, reader, gscale=-2.0)
        assert N == 0 and not terms.any() and not d.any() and not np.signbit(d).any(), (reader, terms)


@pytest.mark.parametrize("head,C", [("softmax", 2), ("softmax", 5), ("sigmoid", 2)], ids=ids)
def test_saturated_logits_stay_finite(head, C):
    """Logits and teacher logits of +-100, agreeing and opposed, at every temperature: loss and gradient are finite and keep the bars."""
    from lm_net_amd import DistillLoss, SoftSegLoss
    B, H, W = 2, 8, 8
    sign = np.where(np.arange(C)[None, :, None, None] % 2 == 0, 100.0, -100.0) * np.where(np.arange(W) % 2 == 0, 1.0, -1.0)
    lg = np.broadcast_to(sign, (B, C, H, W)).astype(np.float32).copy()
    zt = lg * np.where(np.arange(H)[:, None] % 2 == 0, 1.0, -1.0).astype(np.float32)
    for T in TEMPERATURES:
        for reader in ("teacher_f32", "teacher_bf16"):
            r = R.SimpleNamespace(lg=lg, zt=zt, valid=None)
            terms, d, N = got = _run(DistillLoss(C, temperature=T, head=head), r, reader)
            assert np.isfinite(terms).all() and np.isfinite(d).all() and terms[0] > 0, (head, reader, T, terms)
            _compare_kd(got, R.distill(lg, zt, head, None, T), (head, reader, T))
    if head == "softmax":
        q = np.random.default_rng(0).random((B, C, H, W)).astype(np.float32)
        r = R.SimpleNamespace(lg=lg, q=q)
        got = _run(SoftSegLoss(C).to(DEV), r, "probs")
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        _compare_seg(got, R.loss_and_grad(r, "probs"), (head, "probs"))


@pytest.mark.parametrize("head,shape", [("softmax", (2, 3, 5, 7)), ("softmax", (2, 8, 24, 40)), ("softmax", (2, 9, 32, 36)), ("softmax", (2, 5, 9, 11)),
                                        ("sigmoid", (2, 3, 16, 20)), ("sigmoid", (2, 9, 33, 31))], ids=ids)
def test_teacher_equal_to_the_student_gives_exactly_zero(head, shape):
    """log q and log p come from one device routine: teacher logits bitwise equal to the student's (bf16-representable values for the
    bf16 reader) give loss == 0.0 and an all-zero gradient, at every temperature."""
    from lm_net_amd import DistillLoss
    B, C, H, W = shape
    lg = R.bf16_round(3.0 * R.inputs(B, C, H, W, "teacher_f32", head, seed=41).lg)
    for T in TEMPERATURES:
        for reader in ("teacher_f32", "teacher_bf16"):
            r = R.SimpleNamespace(lg=lg, zt=lg.copy(), valid=None)
            terms, d, N = _run(DistillLoss(C, temperature=T, head=head), r, reader, gscale=3.0)
            assert N == B * H * W * (C if head == "sigmoid" else 1)
            assert terms[0] == 0.0 and terms[1] == 0.0 and not d.any(), (head, reader, T, terms, np.abs(d).max())


@pytest.mark.parametrize("head,shape", [("softmax", (2, 2, 96, 100)), ("softmax", (2, 9, 32, 36)), ("sigmoid", (2, 3, 16, 20)), ("sigmoid", (2, 1, 5, 7))], ids=ids)
def test_deterministic_mode_is_bit_identical(head, shape):
    """Two calls in deterministic mode agree bit for bit in loss, terms and dlogits; N agrees between the two modes; the deterministic
    values keep the bars."""
    from lm_net_amd import hip
    B, C, H, W = shape
    was = hip.get_deterministic()
    try:
        for reader in (R.READERS if head == "softmax" else R.READERS[2:]):
            r = R.inputs(B, C, H, W, reader, head, seed=17, void=0.2)
            crit, kw = _crit(reader, head, C)
            hip.set_deterministic(False)
            plain = _run(crit, r, reader)
            hip.set_deterministic(True)
            a, b = _run(crit, r, reader), _run(crit, r, reader)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] == plain[2], (head, reader)
            ref = R.loss_and_grad(r, reader, head, **kw)
            (_compare_seg if reader in ("probs", "pair") else _compare_kd)(a, ref, (head, reader, "deterministic"))
    finally:
        hip.set_deterministic(was)


@pytest.mark.parametrize("C", [2, 9])
def test_one_hot_targets_agree_with_segloss(C):
    """SoftSegLoss on a one-hot q with unit weights, and on a Mixup pair with lam = 1, is SegLoss(None, None) on the label map: the two
    kernel families agree within the loss and gradient bars, void pixels included."""
    from lm_net_amd import MixedTarget, SegLoss, SoftSegLoss
    B, H, W = 2, 32, 36
    r = R.inputs(B, C, H, W, "teacher_f32", seed=23, void=0.2)
    y = r.valid
    z = _t(r.lg).requires_grad_(True)
    seg = SegLoss(ce_weight=None, dice_weight=None, ignore_index=R.VOID).to(DEV)
    ls = seg(z, _t(y))
    ls.backward()
    want, wd = seg.terms.cpu().numpy().astype(np.float64)[:3], z.grad.cpu().numpy().astype(np.float64)
    q = (y[:, None] == np.arange(C)[None, :, None, None]).astype(np.float32)
    q[np.broadcast_to((y == R.VOID)[:, None], q.shape)] = np.nan
    crit = SoftSegLoss(C).to(DEV)
    for reader, rr in (("probs", R.SimpleNamespace(lg=r.lg, q=q)),
                       ("pair", R.SimpleNamespace(lg=r.lg, ya=y, yb=np.where(y == R.VOID, y, (y + 1) % C), lam=np.ones(B, dtype=np.float32)))):
        terms, d, N = _run(crit, rr, reader)
        assert N == int((y != R.VOID).sum())
        assert np.all(np.abs(terms - want) <= 1e-5 * np.abs(want)), (reader, terms, want)
        assert np.abs(d - wd).max() <= 1e-4 * np.abs(wd).max(), reader

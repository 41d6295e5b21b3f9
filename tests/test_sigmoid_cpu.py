"""CPU: the sigmoid-head restatements (tests/sigmoid_ref.py) against the real reference code where the reference tree exists and
against tests/golden/sigmoid_loss_stats.npz everywhere; known answers; the exports of include/lmnet_sigmoid.h, the argument checks of
its entries (rejected before any HIP call) and the Python-side checks of SigmoidSegLoss / SigmoidStatsMeter (no GPU needed)."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

import sigmoid_ref as S
import void_ref as V
from helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not S.reference_available(), reason="the reference tree is not on this machine")
GOLDEN = "sigmoid_loss_stats.npz"


def _close(a, b, tol):
    return (np.isnan(a) and np.isnan(b)) or a == b or abs(a - b) <= tol * max(abs(b), 1e-300)


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


# ---------------------------------------------------------------- restatement vs the real reference
@needs_reference
def test_dice_restatement_equals_reference():
    ref_loss, _ = S.reference_modules()
    C = 3
    shape = (2, C, 13, 17)
    z = S.logits(shape, "sig_loss/lg").double()
    t = S.targets(shape, "sig_loss/t", "sig_loss/void")
    valid = (t == 0) | (t == 1)
    mod = ref_loss.DiceLoss(C)
    for c in range(C):
        w = torch.zeros(C)
        w[c] = 1.0                                                # class c alone: C * dice term = its _dice_loss
        a = z.clone().requires_grad_(True)
        b = z.clone().requires_grad_(True)
        mine = S.loss_terms(a, t, w_dice=w, bce_scale=0.0)[2] * C
        ref = mod._dice_loss(torch.sigmoid(b[:, c]), (t[:, c] == 1), (~valid[:, c]).long())
        mine.backward()
        ref.backward()
        assert _rel(mine.detach(), ref.detach()) < 1e-12
        assert float((a.grad - b.grad).abs().max()) < 1e-12 * float(b.grad.abs().max())
        assert float(a.grad[:, c][~valid[:, c]].abs().max()) == 0.0


@needs_reference
@pytest.mark.parametrize("C", [2, 3, 9])
def test_focal_restatement_equals_reference(C):
    """The reference FocalLoss(C) on a label map against the restatement on its one-hot planes, no void element.  The reference casts
    its one-hot targets to float32 and binary_cross_entropy_with_logits then returns float32 elements: 2^-23 on the loss, 2^-22 on the
    gradient (tests/test_void_cpu.py::test_focal_restatement_equals_reference); in float64 throughout the same formula agrees to
    1e-12."""
    ref_loss, _ = S.reference_modules()
    z = (V.det_input((2, C, 11, 9), "sig_cpu/focal/%d" % C) * 4).double()
    y = V.labels(2, 11, 9, C, "sig_cpu/focal/y%d" % C)
    planes = torch.nn.functional.one_hot(y, C).permute(0, 3, 1, 2).contiguous()
    a = z.clone().requires_grad_(True)
    b = z.clone().requires_grad_(True)
    mine = S.loss_terms(a, planes, bce_scale=0.0, dice_scale=0.0, focal_scale=1.0)[0]
    ref = ref_loss.FocalLoss(num_classes=C)(b, y)
    mine.backward()
    ref.backward()
    assert _rel(mine.detach(), ref.detach()) < 2.0 ** -23
    assert float((a.grad - b.grad).abs().max()) < 2.0 ** -22 * float(b.grad.abs().max())
    f64 = sum(V.sigmoid_focal_loss(z[:, c], (y == c).double(), reduction="mean") for c in range(C))
    assert _rel(mine.detach(), f64) < 1e-12


@pytest.mark.parametrize("C", [1, 3])
def test_bce_restatement_equals_torch(C):
    shape = (2, C, 13, 17)
    z = S.logits(shape, "sig_cpu/bce/%d" % C).double()
    t = S.targets(shape, "sig_cpu/bce/t%d" % C)
    w, pw = S.weights("sig_cpu/bce/w", C), S.weights("sig_cpu/bce/pw", C)
    a = z.clone().requires_grad_(True)
    b = z.clone().requires_grad_(True)
    mine = S.loss_terms(a, t, w_bce=w, pos_weight=pw, dice_scale=0.0)[1]
    ref = torch.nn.functional.binary_cross_entropy_with_logits(b, t.double(), weight=w.double().view(1, C, 1, 1).expand_as(b),
                                                               pos_weight=pw.double().view(1, C, 1, 1))
    mine.backward()
    ref.backward()
    assert _rel(mine.detach(), ref.detach()) < 1e-12
    assert float((a.grad - b.grad).abs().max()) < 1e-12 * float(b.grad.abs().max())


@needs_reference
@pytest.mark.parametrize("C", S.STATS_C)
def test_stats_and_metrics_equal_reference(C):
    from lm_net_amd.metrics import stats_score
    _, ref_fn = S.reference_modules()
    lg, t = S.stats_case(C, void=False)
    cw = S.stats_class_weights(C)
    for thr in S.STATS_THR:
        lt = S.logit_threshold(thr)
        assert (lt == 0.0) if thr == 0.5 else (lt < 0)
        assert float((lg.double() - float(lt)).abs().min()) >= 1e-6   # exact equality needs every logit away from the threshold
        tp, fp, fn, tn = ref_fn.get_stats(torch.sigmoid(lg), t, mode="binary" if C == 1 else "multilabel", threshold=thr)
        st = S.stats(lg.numpy(), t.numpy(), thr)
        assert np.array_equal(st, torch.stack([tp, fp, fn, tn], -1).numpy())
        if thr == 0.5:                                            # the reference's tp is the z >= 0 rule
            assert np.array_equal(st[..., 0], ((lg >= 0) & (t == 1)).flatten(2).sum(2).numpy())
        st[1] = 0                                                 # (one image without a valid element: 0/0 in every imagewise score)
        tp, fp, fn, tn = (torch.from_numpy(st[..., i]).double() for i in range(4))
        for m in S.METRICS:
            name, kw = S.REFERENCE_NAMES.get(m, (m, {}))
            pname, pkw = S.PRODUCT_NAMES.get(m, (m, {}))
            for r in S.REDUCTIONS:
                w = cw if "weighted" in r else None
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    ref = float(getattr(ref_fn, name)(tp, fp, fn, tn, reduction=r, class_weights=w, **kw))
                assert _close(S.score(st, m, r, w), ref, 1e-12), (m, r)
                assert _close(stats_score(st[..., 0], st[..., 1], st[..., 2], st[..., 3], pname, r, w, **pkw), ref, 1e-12), (m, r)


# ---------------------------------------------------------------- restatement vs the committed golden
@pytest.mark.parametrize("tag", list(S.LOSS_TAGS))
def test_loss_restatement_equals_golden(tag):
    g = load_golden(GOLDEN)
    lg, t, w_bce, pw, w_dice, kw = S.loss_case(tag)
    terms, grad = S.loss_and_grad(lg, t, w_bce, pw, w_dice, **kw)
    for k in range(4):
        ref = float(g[tag + "/loss4"][k])
        assert terms[k] == ref == 0.0 or _rel(terms[k], ref) < 1e-12, (k, terms[k], ref)
    assert abs(terms[0] - (terms[1] + terms[2] + terms[3])) < 1e-15 * abs(terms[0])
    dig, ref = S.grad_digest(grad.numpy()), g[tag + "/grad_digest"]
    assert float(np.abs(dig - ref).max()) < 1e-12 * float(np.abs(ref).max())
    assert float(np.abs(S.grad_sample(grad.numpy()) - g[tag + "/grad_sample"]).max()) < 1e-12 * float(ref[3])
    void = ~((t == 0) | (t == 1))
    assert int(void.sum()) > 0 and float(grad[void].abs().max()) == 0.0


@pytest.mark.parametrize("C", S.STATS_C)
def test_stats_restatement_and_product_scores_equal_golden(C):
    from lm_net_amd.metrics import stats_score
    g = load_golden(GOLDEN)
    cw = S.stats_class_weights(C)
    for void in (False, True):
        lg, t = S.stats_case(C, void)
        n_valid = ((t == 0) | (t == 1)).flatten(2).sum(2).numpy()
        for thr in S.STATS_THR:
            key = "%d/%s/%g" % (C, "void" if void else "full", thr)
            st = S.stats(lg.numpy(), t.numpy(), thr)
            assert np.array_equal(st, g["stats/" + key]), key
            assert np.array_equal(st.sum(-1), n_valid), key
            for i, m in enumerate(S.METRICS):
                pname, pkw = S.PRODUCT_NAMES.get(m, (m, {}))
                for j, r in enumerate(S.REDUCTIONS):
                    w = cw if "weighted" in r else None
                    ref = float(g["s64/" + key][i, j])
                    assert _close(S.score(st, m, r, w), ref, 1e-12), (key, m, r)
                    assert _close(stats_score(st[..., 0], st[..., 1], st[..., 2], st[..., 3], pname, r, w, **pkw), ref, 1e-12), (key, m, r)


# ---------------------------------------------------------------- known answers
def test_known_answers():
    # one pixel, t = 1, z = 0: bce = log 2
    z = torch.zeros(1, 1, 1, 1, dtype=torch.float64)
    t = S.loss_terms(z, torch.ones(1, 1, 1, 1, dtype=torch.long), dice_scale=0.0)
    assert abs(float(t[1]) - np.log(2.0)) < 1e-15 and float(t[0]) == float(t[1])
    # an all-void target: [0, dice, dice, 0], finite, a zero gradient
    lg = S.logits((2, 3, 5, 7), "sig_cpu/allvoid")
    terms, grad = S.loss_and_grad(lg, torch.full((2, 3, 5, 7), 255), focal_scale=1.0)
    assert all(np.isfinite(terms)) and terms[1] == 0.0 and terms[3] == 0.0 and terms[0] == terms[2]
    assert float(grad.abs().max()) == 0.0
    # gamma = 0, alpha < 0: the focal term is the bce with unit weights, class by class (N_c differ between the classes)
    tt = S.targets((2, 3, 5, 7), "sig_cpu/g0/t", "sig_cpu/g0/v")
    for c in range(3):
        f = S.loss_terms(lg[:, c:c + 1].double(), tt[:, c:c + 1], bce_scale=0.0, dice_scale=0.0, focal_scale=1.0, gamma=0.0, alpha=-1.0)[3]
        b = S.loss_terms(lg[:, c:c + 1].double(), tt[:, c:c + 1], dice_scale=0.0)[1]
        assert abs(float(f) - float(b)) < 1e-15 * float(b)
    f = S.loss_terms(lg.double(), tt, bce_scale=0.0, dice_scale=0.0, focal_scale=1.0, gamma=0.0, alpha=-1.0)[3]
    per = sum(float(S.loss_terms(lg[:, c:c + 1].double(), tt[:, c:c + 1], dice_scale=0.0)[1]) for c in range(3))
    assert abs(float(f) - per) < 1e-14 * per
    # a stray target value 7 is void: same loss as with 255 there, no gradient, counted nowhere
    t7, t255 = tt.clone(), tt.clone()
    t7[0, 1, 2, 3], t255[0, 1, 2, 3] = 7, 255
    a, ga = S.loss_and_grad(lg, t7, focal_scale=0.5)
    b, gb = S.loss_and_grad(lg, t255, focal_scale=0.5)
    assert a == b and torch.equal(ga, gb) and float(ga[0, 1, 2, 3]) == 0.0
    assert np.array_equal(S.stats(lg.numpy(), t7.numpy()), S.stats(lg.numpy(), t255.numpy()))
    s = S.stats(np.array([[[[0.5, -0.5, 0.0, 2.0, -1.0]]]], dtype=np.float32), np.array([[[[1, 1, 0, 7, 0]]]]))
    assert s.tolist() == [[[1, 1, 1, 1]]]                         # (z = 0 at thr = 0.5 is predicted on)
    assert S.labels(np.array([0.0, -1e-30, 1e-30], dtype=np.float32)).tolist() == [1, 0, 1]


# ---------------------------------------------------------------- ABI and argument checks
def test_exports_and_struct_size():
    from lm_net_amd import hip
    lib = hip.load()
    assert hip.SYMBOLS_SIGMOID == ["lmn_sizeof_sig_param", "lmn_sigloss_fwd", "lmn_sigloss_bwd", "lmn_sigmoid_stats"]
    assert hip.HEADERS["lmnet_sigmoid.h"] is hip.SYMBOLS_SIGMOID   # (the header / export / layout checks: tests/test_host_cpu.py)
    header = open(os.path.join(ROOT, "include", "lmnet_sigmoid.h")).read()
    assert lib.lmn_sizeof_sig_param() == ctypes.sizeof(hip.SigParam) == 64 and hip.ABI_VERSION == 15
    m = re.search(r"#define LMN_SIG_SUMS_WORDS\(C\) \((\d+) \* \(C\)\)", header)
    n = re.search(r"#define LMN_SIG_COEF_FLOATS\(C\) \((\d+) \* \(C\)\)", header)
    assert m and n
    for C in (1, 9, 64):                                          # the workspace sizes of the header, mirrored in Python
        assert hip.sig_sums_words(C) == int(m.group(1)) * C and hip.sig_coef_floats(C) == int(n.group(1)) * C
    assert re.search(r"#define LMN_SIG_T_U8 0\b", header) and re.search(r"#define LMN_SIG_T_I64 1\b", header)
    assert (hip.SIG_T_U8, hip.SIG_T_I64) == (0, 1)
    assert hip.sig_logit_threshold(0.5) == 0.0 and hip.sig_logit_threshold(0.3) == float(S.logit_threshold(0.3))


def _loss_entry(which, B=2, C=3, HW=35, null=None, **kw):
    """lmn_sigloss_fwd / _bwd with fake device pointers: every case here must be rejected before any HIP call."""
    from lm_net_amd import hip
    lib = hip.load()
    fake = ctypes.c_void_p(0x1000)
    p = hip.sig_param(**kw)
    if which == "fwd":
        a = dict(logits=fake, target=fake, w_bce=fake, pos_weight=fake, w_dice=fake, param=ctypes.byref(p), sums=fake, coef=fake, loss4=fake)
        if null:
            a[null] = None
        rc = lib.lmn_sigloss_fwd(a["logits"], a["target"], a["w_bce"], a["pos_weight"], a["w_dice"], B, C, ctypes.c_int64(HW), a["param"],
                                 a["sums"], a["coef"], a["loss4"], None)
    else:
        a = dict(logits=fake, target=fake, pos_weight=fake, coef=fake, param=ctypes.byref(p), dlogits=fake)
        if null:
            a[null] = None
        rc = lib.lmn_sigloss_bwd(a["logits"], a["target"], a["pos_weight"], a["coef"], None, B, C, ctypes.c_int64(HW), a["param"],
                                 a["dlogits"], None)
    return rc, lib.lmn_last_error().decode()


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_loss_entries_reject_bad_arguments(which):
    names = ("logits", "target", "w_bce", "pos_weight", "w_dice", "param", "sums", "coef", "loss4") if which == "fwd" else \
        ("logits", "target", "pos_weight", "coef", "param", "dlogits")
    for n in names:
        rc, err = _loss_entry(which, null=n)
        assert rc == -1 and "null pointer" in err, (n, err)
    for C in (0, 65, -3):
        rc, err = _loss_entry(which, C=C)
        assert rc == -1 and "not in [1, 64]" in err, (C, err)
    rc, err = _loss_entry(which, focal_gamma=-0.5)
    assert rc == -1 and "focal_gamma" in err
    rc, err = _loss_entry(which, focal_alpha=1.25)
    assert rc == -1 and "focal_alpha" in err
    for k in ("bce_scale", "dice_scale", "focal_scale"):
        rc, err = _loss_entry(which, **{k: -1.0})
        assert rc == -1 and "negative scale" in err, k
    rc, err = _loss_entry(which, smooth=-1.0)
    assert rc == -1 and "smooth" in err
    for kind in (2, -1):
        rc, err = _loss_entry(which, target_kind=kind)
        assert rc == -1 and "target_kind" in err, kind
    for kw in (dict(HW=1 << 31), dict(HW=0), dict(B=0), dict(B=1024, C=64), dict(B=3, HW=1 << 30)):   # the limits of the header
        rc, err = _loss_entry(which, **kw)
        assert rc == -1 and "2^31" in err and "65535" in err, (kw, err)


def test_sigmoid_stats_rejects_bad_arguments():
    from lm_net_amd import hip
    lib = hip.load()
    fake = ctypes.c_void_p(0x1000)

    def call(logits=fake, target=fake, kind=1, thr=0.0, B=2, C=3, HW=35, stats=fake, labels=fake):
        rc = lib.lmn_sigmoid_stats(logits, target, kind, ctypes.c_float(thr), B, C, ctypes.c_int64(HW), stats, labels, None)
        return rc, lib.lmn_last_error().decode()
    for kw, msg in ((dict(logits=None), "null pointer"), (dict(stats=None, labels=None), "at least one"),
                    (dict(target=None), "stats needs a target"), (dict(kind=2), "target_kind"), (dict(kind=-1), "target_kind"),
                    (dict(C=0), "not in [1, 64]"), (dict(C=65), "not in [1, 64]"), (dict(HW=1 << 31), "2^31"),
                    (dict(B=1024, C=64), "65535"), (dict(B=0), "B=0"), (dict(thr=float("nan")), "NaN")):
        rc, err = call(**kw)
        assert rc == -1 and msg in err, (kw, err)


# ---------------------------------------------------------------- Python side
def test_python_value_errors():
    from lm_net_amd import SigmoidSegLoss, SigmoidStatsMeter
    from lm_net_amd.metrics import sigmoid_labels
    for kw in (dict(focal_gamma=-1.0), dict(bce_scale=-1.0), dict(dice_scale=-0.5), dict(focal_scale=-2.0), dict(focal_alpha=1.5),
               dict(smooth=-1.0), dict(pos_weight=[1.0] * 65)):
        with pytest.raises(ValueError):
            SigmoidSegLoss(**kw)
    z1, z3 = torch.zeros(2, 1, 4, 4), torch.zeros(2, 3, 4, 4)
    crit = SigmoidSegLoss()
    with pytest.raises(ValueError, match="soft"):
        crit(z1, torch.zeros(2, 1, 4, 4))                         # floating-point target
    with pytest.raises(ValueError, match="does not match"):
        crit(z3, torch.zeros(2, 4, 4, dtype=torch.long))          # [B, H, W] only when C = 1
    with pytest.raises(ValueError, match="does not match"):
        crit(z1, torch.zeros(2, 1, 4, 5, dtype=torch.long))
    with pytest.raises(ValueError, match=r"1\.\.64"):
        crit(torch.zeros(1, 65, 2, 2), torch.zeros(1, 65, 2, 2, dtype=torch.long))
    with pytest.raises(ValueError, match="int32"):
        crit(z1, torch.zeros(2, 1, 4, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="3 classes in the logits, 1 pos"):
        SigmoidSegLoss(pos_weight=[4.0])(z3, torch.zeros(2, 3, 4, 4, dtype=torch.long))
    for t in (torch.zeros(2, 4, 4, dtype=torch.long), torch.zeros(2, 1, 4, 4, dtype=torch.uint8), torch.zeros(2, 1, 4, 4, dtype=torch.bool)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            crit(z1, t)
    for kw in (dict(n_classes=0), dict(n_classes=65), dict(n_classes=1, threshold=0.0), dict(n_classes=1, threshold=1.0)):
        with pytest.raises(ValueError):
            SigmoidStatsMeter(**kw)
    with pytest.raises(ValueError):
        sigmoid_labels(z1, threshold=1.5)
    m = SigmoidStatsMeter(3, device="cpu")
    with pytest.raises(ValueError, match="n_classes = 3"):
        m.update(z1, torch.zeros(2, 1, 4, 4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.update(z3, torch.zeros(2, 3, 4, 4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.labels(z3)
    with pytest.raises(ValueError):
        m.score("iou", "weighted")                                # class weights are required


def test_meter_shares_the_scores_of_image_stats_meter():
    from lm_net_amd import ImageStatsMeter, SigmoidStatsMeter
    from lm_net_amd import metrics
    for name in ("add_raw", "raw", "stats", "score", "per_image", "reset"):
        assert getattr(SigmoidStatsMeter, name) is getattr(ImageStatsMeter, name), name     # shared, not copied
    assert "SigmoidStatsMeter" in metrics.__dict__ and "sigmoid_labels" in metrics.__dict__
    g = load_golden(GOLDEN)
    st = g["stats/5/void/0.3"]
    m = SigmoidStatsMeter(5, threshold=0.3, device="cpu")
    assert m.raw().shape == (0, 5, 4) and m.logit_threshold == float(S.logit_threshold(0.3))
    m.add_raw(torch.from_numpy(st[:2]))
    m.add_raw(torch.from_numpy(st[2:]))
    tp, fp, fn, tn = m.stats()
    assert tp.shape == (3, 5) and np.array_equal(torch.stack([tp, fp, fn, tn], -1).numpy(), st)
    cw = S.stats_class_weights(5)
    for i, mname in enumerate(S.METRICS):
        pname, pkw = S.PRODUCT_NAMES.get(mname, (mname, {}))
        for j, r in enumerate(S.REDUCTIONS):
            assert _close(m.score(pname, r, cw if "weighted" in r else None, **pkw), float(g["s64/5/void/0.3"][i, j]), 1e-12), (mname, r)
    per = m.per_image("f1")
    assert per.shape == (3, 5)
    m.reset()
    assert m.raw().shape == (0, 5, 4)
    with pytest.raises(ValueError, match="SigmoidStatsMeter.add_raw"):
        m.add_raw(torch.zeros(2, 4, 4, dtype=torch.int64))

"""CPU: the void-label restatements (tests/void_ref.py) against the real reference classes where the reference tree exists and against
tests/golden/void_loss_stats.npz everywhere; lm_net_amd.metrics.stats_score against the same golden; the exports of
include/lmnet_loss.h, the argument checks of its entries (rejected before any HIP call) and the Python-side checks and routing of
SegLoss / FocalLoss / ImageStatsMeter (no GPU needed)."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

import void_ref as V
from helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not V.reference_available(), reason="the reference tree is not on this machine")


def _close(a, b, tol):
    return (np.isnan(a) and np.isnan(b)) or a == b or abs(a - b) <= tol * max(abs(b), 1e-300)


# ---------------------------------------------------------------- restatement vs the real reference
@needs_reference
@pytest.mark.parametrize("C", [2, 3, 5, 9])
@pytest.mark.parametrize("ignore_index", [255, -100])
def test_loss_restatement_equals_reference(C, ignore_index):
    ref_loss, _ = V.reference_modules()
    B, H, W = 2, 13, 17
    key = "void_cpu/%d/%d" % (C, ignore_index)
    lg = (V.det_input((B, C, H, W), key) * 2.5).double()
    y = V.with_void(V.labels(B, H, W, C, key + "/y"), key + "/v", void=ignore_index)
    wce, wdice = V.weights(key + "/wce", C), V.weights(key + "/wdice", C)
    for eps in (0.0, 1e-3):
        a = lg.clone().requires_grad_(True)
        b = lg.clone().requires_grad_(True)
        mine = V.loss_terms(a, y, wce, wdice, eps=eps, ignore_index=ignore_index)[0]
        ref = V.reference_loss(ref_loss, b, y, wce, wdice, eps, ignore_index)
        mine.backward()
        ref.backward()
        assert abs(float(mine.detach()) - float(ref.detach())) < 1e-13 * abs(float(ref.detach()))
        assert float((a.grad - b.grad).abs().max()) < 1e-13 * float(b.grad.abs().max())
        assert float(a.grad.permute(0, 2, 3, 1)[y == ignore_index].abs().max()) == 0.0


@needs_reference
@pytest.mark.parametrize("C", [2, 3, 9])
def test_focal_restatement_equals_reference(C):
    """The reference casts its one-hot targets to float32, and binary_cross_entropy_with_logits then returns float32 elements whatever
    the logits' type: every element of its sum carries one float32 rounding (2^-24 relative), and its gradient a second one on the way
    back.  Hence 2^-23 on the loss and 2^-22 on the gradient here, not the 1e-13 of the other terms; with float64 targets the same
    formula agrees with the restatement to 1e-15 (checked below through the stand-in for torchvision's function)."""
    ref_loss, _ = V.reference_modules()
    lg = (V.det_input((2, C, 11, 9), "void_cpu/focal/%d" % C) * 4).double()
    y = V.labels(2, 11, 9, C, "void_cpu/focal/y%d" % C)
    a = lg.clone().requires_grad_(True)
    b = lg.clone().requires_grad_(True)
    mine = V.loss_terms(a, y, torch.ones(C), torch.ones(C), ce_scale=0.0, dice_scale=0.0, focal_scale=1.0)[0]
    ref = ref_loss.FocalLoss(num_classes=C)(b, y)
    mine.backward()
    ref.backward()
    assert abs(float(mine.detach()) - float(ref.detach())) < 2.0 ** -23 * abs(float(ref.detach()))
    assert float((a.grad - b.grad).abs().max()) < 2.0 ** -22 * float(b.grad.abs().max())
    f64 = sum(V.sigmoid_focal_loss(lg[:, c], (y == c).double(), reduction="mean") for c in range(C))
    assert abs(float(mine.detach()) - float(f64)) < 1e-15 * abs(float(f64))


@needs_reference
@pytest.mark.parametrize("C", [2, 5])
def test_stats_and_metrics_equal_reference(C):
    from lm_net_amd.metrics import stats_score
    _, ref_fn = V.reference_modules()
    lg, y = V.stats_case(C)
    pred = lg.argmax(1)
    assert np.array_equal(V.argmax_first(lg.numpy()), pred.numpy())
    tp, fp, fn, tn = ref_fn.get_stats(pred, y, mode="multiclass", ignore_index=255, num_classes=C)
    stats = V.image_stats(pred.numpy(), y.numpy(), C)
    assert np.array_equal(stats, torch.stack([tp, fp, fn, tn], -1).numpy())
    stats[1] = 0                                                  # (one image without a valid pixel: 0/0 in every imagewise score)
    tp, fp, fn, tn = (torch.from_numpy(stats[..., i]).double() for i in range(4))
    cw = V.stats_class_weights(C)
    for m in V.METRICS:
        name, kw = V.REFERENCE_NAMES.get(m, (m, {}))
        pname, pkw = V.PRODUCT_NAMES.get(m, (m, {}))
        for r in V.REDUCTIONS:
            w = cw if "weighted" in r else None
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                ref = float(getattr(ref_fn, name)(tp, fp, fn, tn, reduction=r, class_weights=w, **kw))
            assert _close(V.score(stats, m, r, w), ref, 1e-13), (m, r)
            assert _close(stats_score(stats[..., 0], stats[..., 1], stats[..., 2], stats[..., 3], pname, r, w, **pkw), ref, 1e-13), (m, r)


# ---------------------------------------------------------------- restatement vs the committed golden
@pytest.mark.parametrize("tag", ["k2", "k9", "f3"])
def test_loss_restatement_equals_golden(tag):
    g = load_golden("void_loss_stats.npz")
    lg, y, wce, wdice, kw = V.loss_case(tag)
    terms, grad = V.loss_and_grad(lg, y, wce, wdice, **kw)
    ref = float(g[tag + "/loss"][0])
    # (f3: the reference's focal loss sums float32 elements, see test_focal_restatement_equals_reference)
    assert abs(terms[0] - ref) < (2.0 ** -23 if tag == "f3" else 1e-13) * abs(ref)
    gr = torch.from_numpy(g[tag + "/dlogits"]).double()           # (stored as float32: 2^-24, plus the 2^-22 above for f3)
    assert float((grad - gr).abs().max()) < (2.0 ** -21 if tag == "f3" else 1e-7) * float(gr.abs().max())
    assert abs(terms[0] - (terms[1] + terms[2] + terms[3])) < 1e-15 * abs(ref)


@pytest.mark.parametrize("C", V.STATS_C)
def test_stats_restatement_and_product_scores_equal_golden(C):
    """Every metric / reduction pair: 1e-12 against the goldens made from float64 statistics, 1e-6 against those made from the int64
    statistics (the reference's arithmetic is float32 on those: every pair of the "s32" table)."""
    from lm_net_amd.metrics import stats_score
    g = load_golden("void_loss_stats.npz")
    lg, y = V.stats_case(C)
    stats = V.image_stats(V.argmax_first(lg.numpy()), y.numpy(), C)
    assert np.array_equal(stats, g["stats/%d" % C])
    assert np.array_equal(stats.sum(-1), np.repeat(((y >= 0) & (y < C)).sum((1, 2)).numpy()[:, None], C, 1))
    cw = V.stats_class_weights(C)
    for i, m in enumerate(V.METRICS):
        pname, pkw = V.PRODUCT_NAMES.get(m, (m, {}))
        for j, r in enumerate(V.REDUCTIONS):
            w = cw if "weighted" in r else None
            mine = V.score(stats, m, r, w)
            prod = stats_score(stats[..., 0], stats[..., 1], stats[..., 2], stats[..., 3], pname, r, w, **pkw)
            assert _close(mine, float(g["s64/%d" % C][i, j]), 1e-12) and _close(prod, float(g["s64/%d" % C][i, j]), 1e-12), (m, r)
            assert _close(mine, float(g["s32/%d" % C][i, j]), 1e-6), (m, r)


def test_restatement_hand_cases():
    # two pixels, C = 2, one void: cross entropy of the valid pixel alone; the void pixel has no gradient
    lg = torch.tensor([[[[0.3, 5.0]], [[-0.2, -7.0]]]], dtype=torch.float64, requires_grad=True)
    y = torch.tensor([[[1, 255]]])
    t = V.loss_terms(lg, y, torch.ones(2), torch.ones(2), ignore_index=255, dice_scale=0.0)
    assert abs(float(t[0]) - float(np.log1p(np.exp(0.5)))) < 1e-15
    t[0].backward()
    assert float(lg.grad[0, :, 0, 1].abs().max()) == 0.0
    # no valid pixel: finite, all terms 0 (dice: smooth / smooth)
    t = V.loss_terms(lg.detach(), torch.full((1, 1, 2), 255), torch.ones(2), torch.ones(2), ignore_index=255, focal_scale=1.0)
    assert [float(v) for v in t] == [0.0, 0.0, 0.0, 0.0]
    # gamma = 0, alpha < 0: the focal term is the plain sum of binary cross entropies
    z = torch.tensor([[[[1.5]], [[-0.5]]]], dtype=torch.float64)
    f = V.loss_terms(z, torch.tensor([[[0]]]), torch.ones(2), torch.ones(2), ce_scale=0.0, dice_scale=0.0, focal_scale=1.0, gamma=0.0, alpha=-1.0)[3]
    assert abs(float(f) - (np.log1p(np.exp(-1.5)) + np.log1p(np.exp(-0.5)))) < 1e-15
    # statistics: a stray label (77) and a "no class" prediction (255)
    s = V.image_stats(np.array([[[0, 1, 255, 1]]]), np.array([[[0, 0, 1, 77]]]), 2)
    assert s.tolist() == [[[1, 0, 1, 1], [0, 1, 1, 1]]]


# ---------------------------------------------------------------- ABI and argument checks
def test_exports_and_struct_size():
    from lm_net_amd import hip
    lib = hip.load()
    assert hip.SYMBOLS_LOSS == ["lmn_sizeof_loss_param", "lmn_segloss_ex_fwd", "lmn_segloss_ex_bwd", "lmn_image_stats"]
    assert hip.HEADERS["lmnet_loss.h"] is hip.SYMBOLS_LOSS         # (the header / export / layout checks: tests/test_host_cpu.py)
    header = open(os.path.join(ROOT, "include", "lmnet_loss.h")).read()
    assert lib.lmn_sizeof_loss_param() == ctypes.sizeof(hip.LossParam) == 64 and hip.ABI_VERSION == 15
    for C in (2, 9, 64):                                          # the workspace sizes of the header, mirrored in Python
        assert hip.loss_sums_floats(C) == 4 + 3 * C and hip.loss_coef_floats(C) == 4 + 2 * C
    assert re.search(r"#define LMN_LOSS_SUMS_FLOATS\(C\) \(4 \+ 3 \* \(C\)\)", header)
    assert re.search(r"#define LMN_LOSS_COEF_FLOATS\(C\) \(4 \+ 2 \* \(C\)\)", header)


def _loss_entry(which, C=3, null=None, **kw):
    """lmn_segloss_ex_fwd / _bwd with fake device pointers: every case here must be rejected before any HIP call."""
    from lm_net_amd import hip
    lib = hip.load()
    fake = ctypes.c_void_p(0x1000)
    p = hip.loss_param(**kw)
    if which == "fwd":
        a = dict(logits=fake, target=fake, w_ce=fake, w_dice=fake, param=ctypes.byref(p), sums=fake, coef=fake, loss4=fake)
        if null:
            a[null] = None
        rc = lib.lmn_segloss_ex_fwd(a["logits"], a["target"], a["w_ce"], a["w_dice"], 2, C, ctypes.c_int64(35), a["param"], a["sums"],
                                    a["coef"], a["loss4"], None)
    else:
        a = dict(logits=fake, target=fake, w_ce=fake, coef=fake, param=ctypes.byref(p), dlogits=fake)
        if null:
            a[null] = None
        rc = lib.lmn_segloss_ex_bwd(a["logits"], a["target"], a["w_ce"], a["coef"], None, 2, C, ctypes.c_int64(35), a["param"],
                                    a["dlogits"], None)
    return rc, lib.lmn_last_error().decode()


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_loss_entries_reject_bad_arguments(which):
    names = ("logits", "target", "w_ce", "w_dice", "param", "sums", "coef", "loss4") if which == "fwd" else \
        ("logits", "target", "w_ce", "coef", "param", "dlogits")
    for n in names:
        rc, err = _loss_entry(which, null=n)
        assert rc == -1 and "null pointer" in err, (n, err)
    for C in (1, 65, 0, -3):
        rc, err = _loss_entry(which, C=C)
        assert rc == -1 and "not in [2, 64]" in err, (C, err)
    for ii in (0, 2):
        rc, err = _loss_entry(which, C=3, ignore_index=ii)
        assert rc == -1 and "ignore_index" in err and "inside" in err, (ii, err)
    rc, err = _loss_entry(which, focal_gamma=-0.5)
    assert rc == -1 and "focal_gamma" in err
    rc, err = _loss_entry(which, focal_alpha=1.25)
    assert rc == -1 and "focal_alpha" in err
    for k in ("ce_scale", "dice_scale", "focal_scale"):
        rc, err = _loss_entry(which, **{k: -1.0})
        assert rc == -1 and "negative scale" in err, k
    assert "label_smoothing" in _loss_entry(which, label_smoothing=1.5)[1] and "smooth" in _loss_entry(which, smooth=-1.0)[1]


def test_image_stats_rejects_bad_arguments():
    from lm_net_amd import hip
    lib = hip.load()
    fake = ctypes.c_void_p(0x1000)

    def call(logits=fake, pred=None, target=fake, B=2, C=3, HW=35, has=1, ii=255, stats=fake):
        rc = lib.lmn_image_stats(logits, pred, target, B, C, ctypes.c_int64(HW), has, ctypes.c_int64(ii), stats, None)
        return rc, lib.lmn_last_error().decode()
    for kw, msg in ((dict(logits=fake, pred=fake), "exactly one"), (dict(logits=None, pred=None), "exactly one"),
                    (dict(target=None), "null pointer"), (dict(stats=None), "null pointer"), (dict(C=1), "not in [2, 64]"),
                    (dict(C=65), "not in [2, 64]"), (dict(ii=1), "ignore_index"), (dict(ii=0), "ignore_index"),
                    (dict(HW=1 << 31), "HW"), (dict(B=65536), "B=")):
        rc, err = call(**kw)
        assert rc == -1 and msg in err, (kw, err)


# ---------------------------------------------------------------- Python side
def test_python_value_errors():
    from lm_net_amd import FocalLoss, ImageStatsMeter, SegLoss
    for kw in (dict(ignore_index=1), dict(ignore_index=0), dict(focal_gamma=-1.0), dict(ce_scale=-1.0), dict(dice_scale=-0.5),
               dict(focal_scale=-2.0), dict(focal_alpha=1.5)):
        with pytest.raises(ValueError):
            SegLoss(**kw)
    with pytest.raises(ValueError):
        SegLoss(None, None, ignore_index=5)(torch.zeros(1, 9, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long))   # inside [0, 9)
    with pytest.raises(ValueError):
        FocalLoss(3, ignore_index=2)
    with pytest.raises(ValueError):
        FocalLoss(3, gamma=-1.0)
    with pytest.raises(ValueError):
        ImageStatsMeter(4, ignore_index=3)
    with pytest.raises(ValueError):
        ImageStatsMeter(65)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SegLoss(ignore_index=255)(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FocalLoss(2)(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ImageStatsMeter(2).update(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long))
    m = ImageStatsMeter(3, ignore_index=255, device="cpu")
    with pytest.raises(ValueError):
        m.score("iou", "weighted")                                # class weights are required
    with pytest.raises(ValueError):
        m.score("no_such_metric")


def test_default_segloss_keeps_the_old_entries(monkeypatch):
    """With every new argument at its default SegLoss calls hip.segloss_fwd / segloss_bwd and never the new wrappers; any new
    argument routes to the new ones."""
    from lm_net_amd import SegLoss, hip
    calls = []

    class FakeCuda(torch.Tensor):
        is_cuda = True

    def rec(name, fill):
        def f(*a):
            calls.append(name)
            if fill is not None:
                a[fill].zero_()
        return f
    monkeypatch.setattr(hip, "segloss_fwd", rec("segloss_fwd", 8))
    monkeypatch.setattr(hip, "segloss_bwd", rec("segloss_bwd", 5))
    monkeypatch.setattr(hip, "segloss_ex_fwd", rec("segloss_ex_fwd", 7))
    monkeypatch.setattr(hip, "segloss_ex_bwd", rec("segloss_ex_bwd", 6))
    y = torch.zeros(1, 4, 4, dtype=torch.long)
    lg = torch.zeros(1, 2, 4, 4).as_subclass(FakeCuda).requires_grad_(True)
    crit = SegLoss()
    assert crit.extended is False
    crit(lg, y).backward()
    assert calls == ["segloss_fwd", "segloss_bwd"] and crit.terms is None
    for kw in (dict(ignore_index=255), dict(focal_scale=0.5), dict(ce_scale=0.7), dict(dice_scale=0.0), dict(focal_gamma=1.5),
               dict(focal_alpha=-1.0), dict(ignore_index=-100)):
        del calls[:]
        crit = SegLoss(**kw)
        assert crit.extended is True
        crit(lg, y).backward()
        assert calls == ["segloss_ex_fwd", "segloss_ex_bwd"] and crit.terms.shape == (4,), kw


def test_meter_scores_raw_statistics_on_the_host():
    from lm_net_amd import ImageStatsMeter
    g = load_golden("void_loss_stats.npz")
    m = ImageStatsMeter(5, ignore_index=255, device="cpu")
    assert m.raw().shape == (0, 5, 4)
    m.add_raw(torch.from_numpy(g["stats/5"][:2]))
    m.add_raw(torch.from_numpy(g["stats/5"][2:]))
    tp, fp, fn, tn = m.stats()
    assert tp.shape == (3, 5) and tp.dtype == torch.int64 and np.array_equal(torch.stack([tp, fp, fn, tn], -1).numpy(), g["stats/5"])
    i, j = list(V.METRICS).index("f1"), V.REDUCTIONS.index("macro-imagewise")
    assert _close(m.score("f1", "macro-imagewise"), float(g["s64/5"][i, j]), 1e-12)
    per = m.per_image("f1")
    assert per.shape == (3, 5) and _close(float(per.mean()), float(g["s64/5"][i, j]), 1e-12)
    m.reset()
    assert m.raw().shape == (0, 5, 4)

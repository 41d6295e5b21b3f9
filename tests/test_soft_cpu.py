"""CPU: the host side of the soft-target criteria and the batch mixer (include/soft/lmnet_soft.h; lm_net_amd.loss.SoftSegLoss,
DistillLoss, MixedTarget, lm_net_amd.data.DeviceMix): registry and header agree, the
argument checks of the four C entries (rejected before any HIP call, with fake device pointers), the workspace formula, the classes'
refusals, the sampler, and the restatement tests/soft_ref.py: against F.cross_entropy's probability-target form, F.kl_div, the
reference's own DiceLoss._dice_loss on float targets (tests/golden/soft_ref.npz, written by tools/make_golden_soft.py from the real
code), float64 autograd and finite differences.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import soft_ref as R
from lm_net_amd import DeviceMix, DistillLoss, MixedTarget, SoftSegLoss, hip  # noqa: F401  (every test of this file belongs to the feature)

assert callable(hip.soft_fwd) and callable(hip.mix_batch)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_ENTRIES = ["lmn_soft_fwd", "lmn_soft_bwd", "lmn_mix_batch"]


# ---------------------------------------------------------------- ABI
def test_registry_and_header_agree():
    """The feature's own part of the registry: the literal list, its place in hip.HEADERS, the number of #defines, the header's
    citations and the package's exports.  (Header / export / layout / return-type / constants checks: tests/test_host_cpu.py.)"""
    assert hip.SYMBOLS_SOFT == ["lmn_soft_workspace"] + DEVICE_ENTRIES
    assert hip.HEADERS["soft/lmnet_soft.h"] is hip.SYMBOLS_SOFT
    header = open(os.path.join(ROOT, "include", "soft", "lmnet_soft.h")).read()
    assert "struct" not in header.replace("no struct", "")
    assert len(re.findall(r"^#define LMN_(?:SOFT|MIX)_\w+ \d+\b", header, re.M)) == 13
    for cite in ("USED AS GIVEN", "DIVIDES BY THE PIXEL COUNT", "q' = (1 - eps) q + eps / C", "(2 I_c + s) / (Z_c + Y_c + s)", "kd   = T^2 / N * sum KL(q || p)",
                 "scale T (p - q) / N", "COME FROM THE SAME DEVICE FUNCTION", "0 * log 0 is 0", "EVERY VOID POSITION GETS GRADIENT +0", "never NaN",
                 "GIVES A RATIO OF 1", "UNFUSED", "soft_workspace: ", "soft_fwd: ", "soft_bwd: ", "mix_batch: "):
        assert cite in header, cite
    import lm_net_amd
    from lm_net_amd import data, loss
    for name, mod in (("SoftSegLoss", loss), ("DistillLoss", loss), ("MixedTarget", loss), ("DeviceMix", data)):
        assert getattr(lm_net_amd, name) is getattr(mod, name) and name in lm_net_amd.__all__
    for cls, words in ((SoftSegLoss, ("Deliberate difference", "soft BCE", "per-image Dice", "bf16 probability targets")),
                       (DistillLoss, ("Deliberate difference", "Dice against the teacher", "batchmean"))):
        assert all(w in cls.__doc__ for w in words), cls


# ---------------------------------------------------------------- argument checks of the C entries
FAKE = ctypes.c_void_p(0x1000)
FAKE2 = ctypes.c_void_p(0x40000000)


def _soft(which, **kw):
    """lmn_soft_fwd / _bwd with fake device pointers: every case here must be rejected before any HIP call."""
    lib = hip.load()
    g = dict(logits=FAKE, reader=0, head=0, target=FAKE, ya=None, yb=None, kind=0, lam=None, T=1.0, eps=0.0, smooth=1e-5, ce_scale=1.0,
             dice_scale=1.0, B=3, C=4, H=33, W=65, w_ce=None, w_dice=None, workspace=FAKE, ws_bytes=1 << 40, sums=FAKE, counts=FAKE, coef=FAKE,
             terms=FAKE, dlogits=FAKE)
    g.update(kw)
    f = ctypes.c_float
    if which == "fwd":
        rc = lib.lmn_soft_fwd(g["logits"], g["reader"], g["head"], g["target"], g["ya"], g["yb"], g["kind"], g["lam"], f(g["T"]), f(g["eps"]),
                              f(g["smooth"]), f(g["ce_scale"]), f(g["dice_scale"]), g["B"], g["C"], g["H"], g["W"], g["w_ce"], g["w_dice"],
                              g["workspace"], ctypes.c_int64(g["ws_bytes"]), g["sums"], g["counts"], g["coef"], g["terms"], None)
    else:
        rc = lib.lmn_soft_bwd(g["logits"], g["reader"], g["head"], g["target"], g["ya"], g["yb"], g["kind"], g["lam"], f(g["T"]), f(g["eps"]),
                              g["B"], g["C"], g["H"], g["W"], g["w_ce"], g["coef"], None, g["dlogits"], None)
    return rc, lib.lmn_last_error().decode()


PAIR = dict(reader=hip.SOFT_PAIR, target=None, ya=FAKE, yb=FAKE, lam=FAKE)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_loss_entries_reject_bad_arguments(which):
    pre = "soft_%s: " % which
    for name in (("logits", "sums", "counts", "coef", "terms") if which == "fwd" else ("logits", "coef", "dlogits")):
        rc, err = _soft(which, **{name: None})
        assert rc == -1 and err == pre + "null pointer", (name, err)
    cases = [(dict(reader=4), "unknown reader 4"), (dict(reader=-1), "unknown reader -1"), (dict(head=2), "unknown head 2"),
             (dict(head=1), "reader 0 needs a softmax head"), (dict(head=1, **PAIR), "reader 1 needs a softmax head"),
             (dict(B=0), "B=0 not in [1, 65535]"), (dict(B=65536, C=2, H=1, W=1), "B=65536 not in"), (dict(C=65), "C=65 not in [1, 64]"),
             (dict(C=1), "C=1 needs a sigmoid head"), (dict(H=0), "size 0x65 below 1"), (dict(W=-1), "size 33x-1"), (dict(kind=7), "unknown label kind 7"),
             (dict(B=600, C=4, H=1024, W=1024), "B * C * H * W = 2516582400 not below 2^31"),
             (dict(target=None), "takes a target"), (dict(yb=FAKE), "neither yb nor lam"), (dict(lam=FAKE), "neither yb nor lam"),
             (dict(ya=FAKE), "the probability reader takes no label map"), (dict(PAIR, target=FAKE), "the pair reader takes ya, yb and lam and no target"),
             (dict(PAIR, yb=None), "the pair reader takes"), (dict(PAIR, lam=None), "the pair reader takes"),
             (dict(reader=2, T=0.0), "temperature=0 must be finite and > 0"), (dict(reader=3, T=-1.0), "temperature=-1"),
             (dict(reader=2, T=float("inf")), "temperature=inf"), (dict(reader=2, T=float("nan")), "must be finite and > 0"),
             (dict(T=2.0), "temperature=2 without a teacher"), (dict(eps=-0.1), "eps=-0.1 not in [0, 1]"), (dict(eps=1.5), "eps=1.5"),
             (dict(reader=2, w_ce=FAKE), "the teacher readers take no class weight")]
    if which == "fwd":
        cases += [(dict(smooth=-1e-3), "smooth=-0.001"), (dict(smooth=float("inf")), "smooth=inf"), (dict(ce_scale=float("inf")), "is not finite"),
                  (dict(dice_scale=float("nan")), "is not finite"), (dict(reader=3, w_dice=FAKE), "the teacher readers take no class weight"),
                  (dict(ws_bytes=100), "workspace of 100 bytes too small")]
    for kw, msg in cases:
        rc, err = _soft(which, **kw)
        assert rc == -1 and msg in err and err.startswith(pre), (kw, err)
    if which == "fwd":                                     # the bounds themselves pass: the last check, of the workspace, is reached
        for kw in (dict(reader=2, head=1, B=1, C=1, H=1, W=1), dict(reader=3, B=2, C=64, H=5, W=7, T=0.5), dict(PAIR, B=65535, C=2, H=1, W=1, eps=1.0)):
            need = hip.soft_workspace(kw["reader"], kw.get("head", 0), kw["B"], kw["C"], kw["H"], kw["W"])
            rc, err = _soft(which, ws_bytes=need - 1, **kw)
            assert rc == -1 and "workspace of %d bytes too small, %d needed" % (need - 1, need) in err, err


def test_deterministic_mode_needs_the_workspace():
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    try:
        rc, err = _soft("fwd", workspace=None)
    finally:
        hip.set_deterministic(was)
    assert rc == -1 and err == "soft_fwd: deterministic mode needs the workspace"


def test_workspace_is_host_arithmetic():
    up = lambda v: (v + 255) // 256 * 256
    cdiv = lambda a, b: (a + b - 1) // b
    for reader, head, B, C, H, W in ((0, 0, 1, 2, 1, 1), (0, 0, 8, 2, 352, 352), (1, 0, 8, 9, 352, 352), (2, 0, 8, 9, 352, 352), (3, 0, 8, 9, 352, 352),
                                     (3, 0, 2, 3, 5, 7), (3, 0, 2000, 3, 40, 40), (2, 1, 2, 1, 5, 7), (3, 1, 8, 9, 352, 352), (2, 1, 1, 64, 8, 8)):
        hw = H * W
        if head == 0:
            items = hw // 4 if reader == 3 and hw % 4 == 0 else hw
            cap = max(1, 1024 // B)
            nbx = max(1, min(cdiv(items, 256), cap)) if C in (2, 3, 4, 8) else max(1, min(cdiv(items, 64), 4 * cap))
            slots = B * nbx
        else:
            slots = B * C * max(1, min(cdiv(hw // 4 if hw % 4 == 0 else hw, 256), max(1, 2048 // (B * C))))
        assert hip.soft_workspace(reader, head, B, C, H, W) == up(4 * slots * (1 if reader >= 2 else 1 + 3 * C)), (reader, head, B, C, H, W)
    for args, msg in (((0, 0, 0, 2, 8, 8), "B=0"), ((0, 0, 2, 1, 8, 8), "C=1 needs a sigmoid head"), ((0, 1, 2, 3, 8, 8), "needs a softmax head"),
                      ((4, 0, 2, 3, 8, 8), "unknown reader"), ((0, 0, 70000, 2, 1, 1), "B=70000"), ((2, 1, 600, 4, 1024, 1024), "not below 2^31")):
        with pytest.raises(ValueError, match="soft_workspace"):
            hip.soft_workspace(*args)
        assert msg in hip.load().lmn_last_error().decode()


def _mix(rows, B=2, Cin=3, H=8, W=8, **kw):
    lib = hip.load()
    g = dict(x=FAKE, y=FAKE, kind=0, rows_dev=FAKE, x_out=FAKE2, ya=FAKE2, yb=FAKE2, lam=FAKE)
    g.update(kw)
    rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
    rp = None if rows is None else rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    rc = lib.lmn_mix_batch(g["x"], g["y"], g["kind"], rp, g["rows_dev"], B, Cin, H, W, g["x_out"], g["ya"], g["yb"], g["lam"], None)
    return rc, lib.lmn_last_error().decode()


def test_mix_entry_rejects_bad_arguments():
    ok = hip.mix_rows([1, 0], [R.MIXUP, R.CUTMIX], [0.25, 1.0], [(0, 0, 0, 0), (2, 3, 8, 8)])
    for name in ("x", "y", "rows_dev", "x_out", "ya", "lam"):
        rc, err = _mix(ok, **{name: None})
        assert rc == -1 and err == "mix_batch: null pointer", name
    assert _mix(None)[1] == "mix_batch: null pointer"

    def row(b, **kw):
        r = ok.copy()
        for k, v in kw.items():
            r[b, ("partner", "mode", "lam", "oml", "y0", "x0", "y1", "x1").index(k)] = v
        return r
    bits = lambda v: int(np.float32(v).view(np.int32))
    cases = [(dict(kind=3), ok, "unknown label kind 3"), (dict(B=0), ok, "B=0 not in"), (dict(Cin=0), ok, "Cin=0 not in [1, 64]"), (dict(Cin=65), ok, "Cin=65"),
             (dict(H=0), ok, "size 0x8 below 1"), (dict(B=2, Cin=64, H=4096, W=4096), ok, "B * Cin * H * W = 2147483648 not below 2^31"),
             (dict(x_out=FAKE), ok, "x_out overlaps x"), (dict(x_out=ctypes.c_void_p(0x1000 + 4 * 2 * 3 * 64 - 4)), ok, "x_out overlaps x"),
             (dict(ya=FAKE), ok, "ya_out or yb_out overlaps y"), (dict(yb=ctypes.c_void_p(0x1000 + 127)), ok, "ya_out or yb_out overlaps y"),
             (dict(), row(0, partner=2), "row 0: partner 2 not in [0, 2)"), (dict(), row(1, partner=-1), "row 1: partner -1"),
             (dict(), row(1, mode=3), "row 1: unknown mode 3"), (dict(), row(0, lam=bits(1.5), oml=bits(-0.5)), "row 0: lam=1.5 not in [0, 1]"),
             (dict(), row(0, lam=bits(float("nan"))), "not in [0, 1]"), (dict(), row(0, oml=bits(0.5)), "row 0: the fourth word 0.5 is not 1 - lam in fp32"),
             (dict(), row(1, y1=9), "row 1: box [2, 9) x [3, 8) outside 8x8"), (dict(), row(1, x0=-1), "outside 8x8"), (dict(), row(1, y0=8, y1=7), "outside 8x8"),
             (dict(yb=None), ok, "row 0 is a mixup row and yb_out is NULL")]
    for kw, rows, msg in cases:
        rc, err = _mix(rows, **kw)
        assert rc == -1 and msg in err and err.startswith("mix_batch: "), (kw, err)


# ---------------------------------------------------------------- the classes refuse what they cannot run
def test_python_refuses_what_it_cannot_run():
    """In the words of the shared front end (_check_n_classes, _check_head, _check_scale, _check_pair) where the fault is the same."""
    z, q = torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4)
    y = torch.zeros(2, 4, 4, dtype=torch.uint8)
    for make, msg in ((lambda: SoftSegLoss(65), r"n_classes = 65 outside \[1, 64\]"), (lambda: SoftSegLoss(1), "a softmax head needs n_classes >= 2"),
                      (lambda: SoftSegLoss(3, label_smoothing=1.5), "label_smoothing"), (lambda: SoftSegLoss(3, smooth=-1), "smooth"),
                      (lambda: SoftSegLoss(3, ce_weight=[1, 2]), "ce_weight needs 3 finite values"), (lambda: SoftSegLoss(3, dice_weight=[1, 2, float("nan")]), "dice_weight"),
                      (lambda: DistillLoss(0), "n_classes = 0 outside"), (lambda: DistillLoss(1), "a softmax head needs n_classes >= 2"),
                      (lambda: DistillLoss(3, head="tanh"), "expected 'softmax' or 'sigmoid'"), (lambda: DistillLoss(3, temperature=0.0), "temperature = 0.0 must be finite and > 0"),
                      (lambda: DistillLoss(3, temperature=-2), "temperature"), (lambda: DistillLoss(3, temperature=float("inf")), "temperature"),
                      (lambda: DeviceMix(mixup_alpha=-1), "mixup_alpha"), (lambda: DeviceMix(prob=1.5), "prob"), (lambda: DeviceMix(partner="next"), "partner"),
                      (lambda: DeviceMix(generator="seed"), "generator must be None, an int seed")):
        with pytest.raises(ValueError, match=msg):
            make()
    assert DistillLoss(1, head="sigmoid").n_classes == 1
    crit, kd = SoftSegLoss(3), DistillLoss(3)
    bad = [(lambda: crit(torch.zeros(2, 4, 4, 4), q), r"logits must be floating point \[B, 3, H, W\]"), (lambda: crit(z.long(), q), "logits must be floating point"),
           (lambda: crit(z, q[:, :2]), "does not match logits"), (lambda: crit(z, y), "floating-point tensor"), (lambda: crit(z, q.double()), "must be fp32"),
           (lambda: crit(z, q.bfloat16()), "bf16 probability targets are out of scope"),
           (lambda: crit(z, MixedTarget(y, y.float(), torch.ones(2))), "target must be uint8, bool or int64"),
           (lambda: crit(z, MixedTarget(y, y[:, :2], torch.ones(2))), "does not match logits"),
           (lambda: crit(torch.zeros(65536, 3, 1, 1), torch.zeros(65536, 3, 1, 1)), "above the limit 65535"),
           (lambda: crit(torch.zeros(2, 3, 0, 4), torch.zeros(2, 3, 0, 4)), r"outside the limit \[1, 2\^31\)"),
           (lambda: crit(torch.zeros(1, 3, 1, 1).expand(4, 3, 32768, 8192), q), r"B \* C \* H \* W = 3221225472 outside the limit"),
           (lambda: kd(z, q[:, :2]), "teacher_logits .* does not match logits"), (lambda: kd(z, y), "teacher_logits must be a floating-point tensor"),
           (lambda: kd(z, q, y.float()), "target must be uint8, bool or int64"), (lambda: kd(z, q, y[:1]), "does not match logits"),
           (lambda: kd(torch.zeros(1, 3, 1, 1).expand(4, 3, 32768, 8192), q), "outside the limit")]
    for call, msg in bad:
        with pytest.raises(ValueError, match=msg):
            call()
    crit.ce_scale = float("inf")
    with pytest.raises(ValueError, match="scale = inf is not finite"):
        crit(z, q)
    kd.scale = float("nan")
    with pytest.raises(ValueError, match="is not finite"):
        kd(z, q)
    mixer = DeviceMix()
    for call, msg in ((lambda: mixer.mix(z.double(), y), "x must be an fp32 tensor"), (lambda: mixer.mix(z, y.float()), "uint8 or int64 label map"),
                      (lambda: mixer.mix(z, y[:1]), "label map"), (lambda: mixer.mix(torch.zeros(2, 65, 4, 4), y), "outside the limits")):
        with pytest.raises(ValueError, match=msg):
            call()
    # CPU tensors: "no CPU fallback", after every check that needs no device
    for call in (lambda: SoftSegLoss(3)(z, q), lambda: SoftSegLoss(3)(z, MixedTarget(y, y, torch.ones(2))), lambda: DistillLoss(3)(z, q),
                 lambda: DistillLoss(3)(z, q.bfloat16(), y), lambda: mixer.mix(z, y)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    t = MixedTarget(y, y, torch.ones(2))
    assert t.ya is y and tuple(t) == (y, y, t.lam)
    with pytest.raises(ValueError, match="can draw Mixup"):
        t.labels
    t.hard = True
    assert t.labels is y


# ---------------------------------------------------------------- the sampler
def test_sampler():
    B, H, W = 64, 24, 40
    a, b = DeviceMix(0.4, 0.3, generator=5).sample(B, H, W), DeviceMix(0.4, 0.3, generator=5).sample(B, H, W)
    assert a.dtype == np.int32 and a.shape == (B, hip.MIX_ROW_WORDS) and np.array_equal(a, b)          # a seed reproduces the rows
    assert not np.array_equal(a, DeviceMix(0.4, 0.3, generator=6).sample(B, H, W))
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    assert np.array_equal(DeviceMix(0.4, 0.3, generator=g1).sample(B, H, W), DeviceMix(0.4, 0.3, generator=g2).sample(B, H, W))
    assert np.array_equal(DeviceMix(0.4, 0.3, generator=np.random.default_rng(5)).sample(B, H, W), a)
    rows = np.concatenate([DeviceMix(0.4, 0.2, partner="perm", generator=s).sample(B, H, W) for s in range(8)])
    lam, oml = rows[:, 2].copy().view(np.float32), rows[:, 3].copy().view(np.float32)
    assert (lam >= 0).all() and (lam <= 1).all() and np.array_equal(oml, np.float32(1) - lam)
    assert set(rows[:, 1]) == {R.MIXUP, R.CUTMIX}
    y0, x0, y1, x1 = rows[:, 4:].T
    assert (0 <= y0).all() and (y0 <= y1).all() and (y1 <= H).all() and (0 <= x0).all() and (x0 <= x1).all() and (x1 <= W).all()
    cut = rows[:, 1] == R.CUTMIX
    area = (y1 - y0) * (x1 - x0)
    assert (area[cut] == 0).any() and ((area[cut] > 0) & (area[cut] < H * W)).any()                    # empty boxes occur
    tiny = np.concatenate([DeviceMix(0.0, 1e-3, generator=s).sample(B, 2, 2) for s in range(4)])       # lam is 0 or 1 up to rounding
    tarea = (tiny[:, 6] - tiny[:, 4]) * (tiny[:, 7] - tiny[:, 5])
    assert (tarea == 0).any() and (tarea == 4).any() and (tiny[:, 4:6] >= 0).all() and (tiny[:, 6:] <= 2).all()      # and so do full ones
    # (that the entry takes them is shown on the device: tests/test_soft_mix_gpu.py mixes with empty and full boxes)
    assert np.allclose(lam[cut], 1.0 - area[cut] / (H * W), atol=1e-6) and not area[~cut].any()
    for chunk in rows.reshape(8, B, -1):
        assert sorted(chunk[:, 0]) == list(range(B))                                                   # a permutation
    assert np.array_equal(a[:, 0], np.arange(B)[::-1])                                                 # flip
    ident = DeviceMix(0.4, 0.3, prob=0.0, generator=1).sample(B, H, W)
    assert not ident[:, 1].any() and (ident[:, 2].copy().view(np.float32) == 1).all() and not ident[:, 4:].any()
    assert not DeviceMix(0.0, 0.0, generator=1).sample(B, H, W)[:, 1].any()
    assert set(DeviceMix(0.0, 1.0, generator=1).sample(B, H, W)[:, 1]) == {R.CUTMIX} and set(DeviceMix(0.5, 0.0, generator=1).sample(B, H, W)[:, 1]) == {R.MIXUP}
    one = DeviceMix(0.4, 0.3, per_sample=False, generator=2).sample(B, H, W)
    assert (one[:, 1:] == one[0, 1:]).all()                                                            # one draw for the batch


def test_mix_restatement():
    """The numpy fp32 restatement itself: mode none copies, Mixup is the unfused expression, CutMix pastes pixels and labels."""
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal((3, 2, 4, 6)).astype(np.float32), rng.integers(0, 4, (3, 4, 6)).astype(np.uint8)
    rows = hip.mix_rows([2, 0, 1], [R.MIXUP, R.CUTMIX, R.NONE], [0.3, 0.5, 0.7], [(0, 0, 0, 0), (1, 2, 3, 6), (0, 0, 4, 6)])
    xo, ya, yb, lam = R.mix(x, y, rows)
    l = np.float32(0.3)
    assert np.array_equal(xo[0], l * x[0] + (np.float32(1) - l) * x[2]) and xo.dtype == np.float32
    assert np.array_equal(ya[0], y[0]) and np.array_equal(yb[0], y[2]) and lam.tolist() == [l, 1.0, 1.0]
    assert np.array_equal(xo[1, :, 1:3, 2:6], x[0, :, 1:3, 2:6]) and np.array_equal(xo[1, :, 0], x[1, :, 0]) and np.array_equal(ya[1, 1:3, 2:6], y[0, 1:3, 2:6])
    assert np.array_equal(ya[1], yb[1]) and np.array_equal(ya[1, 0], y[1, 0])
    assert np.array_equal(xo[2], x[2]) and np.array_equal(ya[2], y[2]) and np.array_equal(yb[2], y[2])


# ---------------------------------------------------------------- the restatement against torch
W3 = [1.0, 2.5, 4.0]


def _q_clean(r, C):
    """(q float64 with 0 at void pixels, valid) of a probs or pair case"""
    if r.q is not None:
        valid = R.probs_valid(r.q)
        return np.where(valid[:, None], r.q.astype(np.float64), 0.0), valid
    return R.pair_q(r.ya, r.yb, r.lam, C)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("weight", [None, W3])
def test_ce_equals_torch_probability_target_form(weight, eps):
    """F.cross_entropy(logits, q, weight, label_smoothing) on the valid pixels: torch divides by the pixel count, not the weight sum."""
    r = R.inputs(3, 3, 5, 7, "probs", seed=2, void=0.2)
    q, valid = _q_clean(r, 3)
    z = torch.from_numpy(r.lg).double()
    zv, qv = z.permute(0, 2, 3, 1)[torch.from_numpy(valid)], torch.from_numpy(q).permute(0, 2, 3, 1)[torch.from_numpy(valid)]
    want = F.cross_entropy(zv, qv, weight=None if weight is None else torch.tensor(weight, dtype=torch.float64), label_smoothing=eps)
    got = R.loss_and_grad(r, "probs", w_ce=weight, eps=eps, dice_scale=0.0)
    assert 0 < valid.sum() < valid.size and abs(got.ce - float(want)) <= 1e-12 * abs(float(want)) and got.loss == got.ce


@pytest.mark.parametrize("T", R.TEMPERATURES)
def test_kd_equals_torch_kl_div(T):
    r = R.inputs(3, 4, 5, 7, "teacher_f32", seed=3, void=0.2)
    valid = torch.from_numpy(r.valid != R.VOID)
    z, zt = (torch.from_numpy(a).double().permute(0, 2, 3, 1)[valid] for a in (r.lg, r.zt))
    want = F.kl_div(F.log_softmax(z / T, 1), F.softmax(zt / T, 1), reduction="sum") / int(valid.sum()) * T * T
    got = R.loss_and_grad(r, "teacher_f32", T=T)
    assert abs(got.kd - float(want)) <= 1e-12 * abs(float(want)) and got.N == int(valid.sum())
    # the Bernoulli form against the binary cross entropies
    r = R.inputs(3, 2, 5, 7, "teacher_f32", "sigmoid", seed=4, void=0.2)
    m = torch.from_numpy((r.valid == 0) | (r.valid == 1))
    z, zt = torch.from_numpy(r.lg).double()[m] / T, torch.from_numpy(r.zt).double()[m] / T
    q = torch.sigmoid(zt)
    want = (F.binary_cross_entropy_with_logits(z, q, reduction="sum") - F.binary_cross_entropy_with_logits(zt, q, reduction="sum")) / int(m.sum()) * T * T
    got = R.loss_and_grad(r, "teacher_f32", "sigmoid", T=T)
    assert abs(got.kd - float(want)) <= 1e-12 * got.magnitude and got.kd > 0


def test_pair_equals_probs_of_the_same_q():
    r = R.inputs(3, 4, 5, 7, "pair", seed=5, void=0.2)
    q, valid = R.pair_q(r.ya, r.yb, r.lam, 4)
    q32 = np.where(valid[:, None], q, np.nan)
    kw = dict(w_ce=[1.0, 2.0, 0.5, 1.5], w_dice=[1.0, 0.5, 2.0, 1.5], eps=0.1)
    a, b = R.loss_and_grad(r, "pair", **kw), R.segloss(r.lg, q32, R.probs_valid(q32), **kw)
    assert a.N == b.N and abs(a.loss - b.loss) < 1e-14 and abs(a.ce - b.ce) < 1e-14 and abs(a.dice - b.dice) < 1e-14 and np.abs(a.grad - b.grad).max() < 1e-15


@pytest.mark.parametrize("C", [2, 4])
def test_one_hot_q_is_the_index_target_loss(C):
    """One-hot q with unit weights: the index-target cross entropy of torch plus the reference's Dice (region_ref: dice, squared, per
    batch, smooth 1e-5), void pixels included."""
    import region_ref
    lg, y = region_ref.inputs(3, C, 5, 7, seed=7, void=0.2)
    q = (y[:, None] == np.arange(C)[None, :, None, None]).astype(np.float32)
    q[np.broadcast_to((y == R.VOID)[:, None], q.shape)] = np.nan
    got = R.segloss(lg, q, R.probs_valid(q))
    z = torch.from_numpy(lg).double().requires_grad_(True)
    ce = F.cross_entropy(z, torch.from_numpy(y), ignore_index=R.VOID)
    ce.backward()
    reg = region_ref.loss_and_grad(lg, y, C)
    assert abs(got.ce - float(ce.detach())) < 1e-12 and abs(got.dice - reg.loss) < 1e-12
    assert np.abs(got.grad - (z.grad.numpy() + reg.grad)).max() < 1e-12
    lam1 = R.SimpleNamespace(lg=lg, ya=y, yb=np.where(y == R.VOID, y, (y + 1) % C), lam=np.ones(3, np.float32))
    pair = R.loss_and_grad(lam1, "pair")
    assert abs(pair.loss - got.loss) < 1e-14 and np.abs(pair.grad - got.grad).max() < 1e-15


# ---------------------------------------------------------------- the Dice term against the reference's own code
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "soft_ref.npz"))


def _close(got, want, rel=1e-12):
    return np.abs(np.asarray(got) - np.asarray(want)).max() <= rel * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("reader", ["probs", "pair"])
@pytest.mark.parametrize("C", [2, 4])
def test_dice_equals_the_reference_dice_loss(C, reader):
    """DiceLoss._dice_loss of the reference's utils/loss.py on float targets, recorded by tools/make_golden_soft.py in float64."""
    from tools.make_golden_soft import case, weights
    r, q, valid = case(C, reader)
    assert 0 < valid.sum() < valid.size
    got = R.loss_and_grad(r, reader, w_dice=weights(C), ce_scale=0.0)
    assert got.loss == got.dice and _close(got.dice, GOLDEN["dice_%s/%d/loss" % (reader, C)][0]) and _close(got.grad, GOLDEN["dice_%s/%d/dlogits" % (reader, C)])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "soft_ref.npz")) < 16384


@pytest.mark.skipif(not __import__("void_ref").reference_available(), reason="the reference tree is not on this machine")
def test_golden_is_what_the_reference_computes():
    """Where the reference tree exists, the golden is recomputed from its code (tools/make_golden_soft.py) and must not have moved."""
    from tools.make_golden_soft import compute
    live = compute()
    assert sorted(live) == sorted(GOLDEN.files)
    for name, want in live.items():
        assert _close(GOLDEN[name], want, 1e-14), name


# ---------------------------------------------------------------- gradients: float64 autograd and finite differences
def _torch_seg(lg, q, valid, w_ce, w_dice, eps, smooth, ce_scale, dice_scale):
    z = torch.tensor(np.asarray(lg, dtype=np.float64), requires_grad=True)
    C = z.shape[1]
    m = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(valid[:, None], z.shape))).double()
    qt = torch.from_numpy(q)
    w = torch.ones(C, dtype=torch.float64) if w_ce is None else torch.tensor(w_ce, dtype=torch.float64)
    v = torch.ones(C, dtype=torch.float64) if w_dice is None else torch.tensor(w_dice, dtype=torch.float64)
    lp = torch.log_softmax(z, 1)
    p = lp.exp()
    ce = -(w[None, :, None, None] * ((1 - eps) * qt + eps / C) * lp * m).sum() / valid.sum()
    I, Z, Y = (p * qt * m).sum((0, 2, 3)), (p * p * m).sum((0, 2, 3)), (qt * qt * m).sum((0, 2, 3))
    dice = (v * (1 - (2 * I + smooth) / (Z + Y + smooth))).mean()
    loss = ce_scale * ce + dice_scale * dice
    loss.backward()
    return float(loss.detach()), z.grad.numpy()


@pytest.mark.parametrize("reader", ["probs", "pair"])
@pytest.mark.parametrize("C", [2, 5])
def test_seg_gradient_equals_torch_autograd(C, reader):
    r = R.inputs(3, C, 5, 7, reader, seed=9, void=0.2)
    q, valid = _q_clean(r, C)
    kw = dict(w_ce=[1.0 + 0.5 * c for c in range(C)], w_dice=[2.0 - 0.25 * c for c in range(C)], eps=0.1, smooth=1e-5, ce_scale=0.7, dice_scale=1.3)
    want, wgrad = _torch_seg(r.lg, q, valid, **kw)
    got = R.loss_and_grad(r, reader, **kw)
    assert want > 0 and abs(got.loss - want) < 1e-10 and np.abs(got.grad - wgrad).max() < 1e-10
    void = ~np.broadcast_to(valid[:, None], got.grad.shape)
    assert void.any() and not got.grad[void].any() and not np.signbit(got.grad[void]).any()              # +0 at every void position


@pytest.mark.parametrize("head,C", [("softmax", 2), ("softmax", 5), ("sigmoid", 1), ("sigmoid", 3)])
@pytest.mark.parametrize("T", R.TEMPERATURES)
def test_kd_gradient_equals_torch_autograd(head, C, T):
    r = R.inputs(3, C, 5, 7, "teacher_f32", head, seed=10, void=0.2)
    z = torch.tensor(r.lg.astype(np.float64), requires_grad=True)
    zt = torch.from_numpy(r.zt.astype(np.float64))
    if head == "softmax":
        m = torch.from_numpy(r.valid != R.VOID)[:, None].expand_as(z)
        kl = (torch.softmax(zt / T, 1) * (torch.log_softmax(zt / T, 1) - torch.log_softmax(z / T, 1)))
        N = int(m[:, 0].sum())
    else:
        m = torch.from_numpy((r.valid == 0) | (r.valid == 1))
        q = torch.sigmoid(zt / T)
        kl = q * (F.logsigmoid(zt / T) - F.logsigmoid(z / T)) + (1 - q) * (F.logsigmoid(-zt / T) - F.logsigmoid(-z / T))
        N = int(m.sum())
    loss = 0.6 * T * T * (kl * m).sum() / N
    loss.backward()
    got = R.loss_and_grad(r, "teacher_f32", head, T=T, scale=0.6)
    assert got.N == N and abs(got.loss - float(loss.detach())) < 1e-10 and np.abs(got.grad - z.grad.numpy()).max() < 1e-10
    void = ~m.numpy()
    assert void.any() and not got.grad[void].any() and not np.signbit(got.grad[void]).any()


@pytest.mark.parametrize("reader,head", [("probs", "softmax"), ("pair", "softmax"), ("teacher_f32", "softmax"), ("teacher_bf16", "sigmoid")])
def test_gradient_equals_finite_differences(reader, head):
    r = R.inputs(2, 3, 4, 5, reader, head, seed=7, void=0.15)
    r.lg = r.lg.astype(np.float64)
    kw = dict(w_ce=W3, w_dice=W3[::-1], eps=0.1) if reader in ("probs", "pair") else dict(T=4.0, scale=0.6)
    full = R.loss_and_grad(r, reader, head, gscale=2.0, **kw)
    h = 1e-6
    rng = np.random.default_rng(0)
    base = r.lg
    for _ in range(12):
        at = tuple(rng.integers(0, n) for n in base.shape)
        vals = []
        for s in (h, -h):
            r.lg = base.copy()
            r.lg[at] += s
            vals.append(R.loss_and_grad(r, reader, head, **kw).loss)
        fd = 2.0 * (vals[0] - vals[1]) / (2 * h)
        assert abs(fd - full.grad[at]) < 1e-6 * max(abs(fd), np.abs(full.grad).max()), (at, fd, full.grad[at])


# ---------------------------------------------------------------- edge rules
def test_edge_rules():
    """No valid pixel: every term 0 and no gradient bit set.  A Dice denominator that is exactly 0 (smooth = 0, q = 0 and p = 0 on a
    class): ratio 1.  A teacher equal to the student: exactly 0."""
    for reader, head in (("probs", "softmax"), ("pair", "softmax"), ("teacher_f32", "softmax"), ("teacher_f32", "sigmoid")):
        r = R.inputs(2, 3, 4, 5, reader, head, seed=1, void=0.2)
        if reader == "probs":
            r.q[:, 1] = -1.0
        elif reader == "pair":
            r.ya[:] = R.VOID
        else:
            r.valid[:] = R.VOID
        got = R.loss_and_grad(r, reader, head)
        assert got.N == 0 and got.loss == 0.0 and not got.grad.any() and not np.signbit(got.grad).any()
    lg = np.zeros((1, 2, 2, 2), np.float32)
    lg[:, 1] = -1e4                                        # p_1 underflows to exactly 0
    q = np.zeros((1, 2, 2, 2), np.float32)
    q[:, 0] = 1.0
    got = R.segloss(lg, q, R.probs_valid(q), smooth=0.0)
    assert got.sums[1][1] == 0.0 and got.sums[2][1] == 0.0 and got.dice == 0.0 and np.isfinite(got.grad).all()
    r = R.inputs(2, 3, 4, 5, "teacher_f32", seed=2)
    for head in ("softmax", "sigmoid"):
        same = R.distill(r.lg, r.lg, head, None, 4.0)
        assert same.kd == 0.0 and not same.grad.any()


# ---------------------------------------------------------------- the preconditions of the GPU tests
def test_busy_subjects_discriminate():
    import busy
    import soft_busy_cases as S
    subjects = S.subjects()
    assert sorted(subjects) == sorted(S.NAMES + [S.MIX_NAME])
    for s in subjects.values():
        busy.check_discrimination(s)


def test_magnitude_bounds_every_teacher_case_of_the_gpu_tests():
    """The loss bar of the distillation term is 1e-5 * magnitude: for every teacher case of tests/test_soft_kernels_gpu.py the
    divergence is non-negative and no larger than the magnitude."""
    n = 0
    for head, shapes, cases in (("softmax", R.SOFTMAX, R.softmax_cases), ("sigmoid", R.SIGMOID, R.sigmoid_cases)):
        for shape in shapes:
            for k in cases(shape):
                if k.reader.startswith("teacher"):
                    ref = R.loss_and_grad(k.r, k.reader, head, T=k.T)
                    assert ref.magnitude >= ref.kd >= 0.0 and ref.N > 0, k.what
                    n += 1
    assert n == 2 * 2 * len(R.SOFTMAX) + 6 * len(R.SIGMOID)


def test_plain_fp32_misses_the_relative_bar_and_keeps_the_magnitude_bar():
    """Why the bar is of the magnitude: KL is a difference of two sums of that size, so an fp32 evaluation of one pixel at T = 4 is
    already outside 1e-5 |ref| for some draws while it stays orders of magnitude inside 1e-5 * magnitude."""
    worst_rel, worst_mag = 0.0, 0.0
    for seed in range(200):
        r = R.inputs(1, 4, 1, 1, "teacher_f32", seed=seed, void=0.0)
        ref = R.distill(r.lg, r.zt, T=4.0)
        z, zt = torch.from_numpy(r.lg) / 4.0, torch.from_numpy(r.zt) / 4.0
        lq, lp = torch.log_softmax(zt, 1), torch.log_softmax(z, 1)
        kd32 = 16.0 * float((lq.exp() * (lq - lp)).sum())
        worst_rel, worst_mag = max(worst_rel, abs(kd32 - ref.kd) / ref.kd), max(worst_mag, abs(kd32 - ref.kd) / ref.magnitude)
    assert worst_rel > 1e-5 and worst_mag < 1e-7, (worst_rel, worst_mag)

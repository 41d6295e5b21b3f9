"""CPU: the host side of the region-overlap losses (include/region/lmnet_region.h; lm_net_amd.loss.RegionLoss, region_sums): registry
and header agree, the argument checks of the three C entries (rejected before any HIP call,
with fake device pointers), the workspace formula, the classes' ValueErrors, and the restatement tests/region_ref.py: against the
reference's own DiceLoss, BCEDiceLoss and offical_DiceLoss (tests/golden/region_ref.npz, written by tools/make_golden_region.py from
the real code), against a plain torch float64 autograd composition, against finite differences, and on the edge rules.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import region_ref as R
from lm_net_amd import RegionLoss, hip, region_sums  # noqa: F401  (every test of this file belongs to the feature)

assert callable(hip.region_fwd)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_ENTRIES = ["lmn_region_fwd", "lmn_region_bwd"]


# ---------------------------------------------------------------- ABI
def test_registry_and_header_agree():
    """The feature's own part of the registry: the literal list, its place in hip.HEADERS, the number of #defines, the header's
    citations and the package's exports.  (Header / export / layout / return-type / constants checks: tests/test_host_cpu.py.)"""
    from lm_net_amd import hip
    assert hip.SYMBOLS_REGION == ["lmn_region_workspace"] + DEVICE_ENTRIES
    assert hip.HEADERS["region/lmnet_region.h"] is hip.SYMBOLS_REGION
    header = open(os.path.join(ROOT, "include", "region", "lmnet_region.h")).read()
    assert len(re.findall(r"^#define LMN_REGION_\w+ \d+\b", header, re.M)) == 11
    for cite in ("R = (2 I + s) / (D + s)", "R = (I + s) / (D - I + s)", "R = (I + s) / (I + alpha FP + beta FN + s)",
                 "R_g = (2 sum_k v_k I_k + s) / (sum_k v_k (P1_k + T_k) + s)", "v_k = 1 / T_k^2", "MONAI's rule",
                 "A DENOMINATOR THAT IS EXACTLY 0 GIVES R = 1", "L = 0 WITH A ZERO DERIVATIVE FOR u <= 0", "never NaN",
                 "EVERY VOID POSITION GETS GRADIENT +0", "d_k = a_gk t + b_gk + c_gk p", "ONLY WITHOUT VOID", "that quirk is not reproduced",
                 "region_workspace: ", "region_fwd: ", "region_bwd: "):
        assert cite in header, cite
    import lm_net_amd
    from lm_net_amd import loss
    for name in ("RegionLoss", "region_sums"):
        assert getattr(lm_net_amd, name) is getattr(loss, name) and name in lm_net_amd.__all__
    assert "Deliberate difference" in loss.RegionLoss.__doc__


# ---------------------------------------------------------------- argument checks
FAKE = ctypes.c_void_p(0x1000)
FWD_POINTERS = ("logits", "target", "sums", "counts", "coef", "per_class", "loss")
BWD_POINTERS = ("logits", "target", "coef", "dlogits")


def _entry(which, null=(), **kw):
    """lmn_region_fwd / _bwd with fake device pointers: every case here must be rejected before any HIP call."""
    from lm_net_amd import hip
    lib = hip.load()
    a = {k: FAKE for k in (FWD_POINTERS if which == "fwd" else BWD_POINTERS)}
    a.update(weight=None, workspace=FAKE)
    for k in null:
        a[k] = None
    g = dict(dict(tk=1, head=0, kind=0, den=1, per_image=0, alpha=0.5, beta=0.5, smooth=1e-5, exponent=1.0, scale=1.0, B=3, C=4, H=33, W=65,
                  class_mask=0b1110, ws_bytes=1 << 40, weight=None), **kw)
    if "weight" in kw:
        a["weight"] = kw["weight"]
    cm = ctypes.c_uint64(g["class_mask"])
    f = ctypes.c_float
    if which == "fwd":
        rc = lib.lmn_region_fwd(a["logits"], a["target"], g["tk"], g["head"], g["kind"], g["den"], g["per_image"], f(g["alpha"]), f(g["beta"]),
                                f(g["smooth"]), f(g["exponent"]), f(g["scale"]), g["B"], g["C"], g["H"], g["W"], cm, a["weight"], a["workspace"],
                                ctypes.c_int64(g["ws_bytes"]), a["sums"], a["counts"], a["coef"], a["per_class"], a["loss"], None)
    else:
        rc = lib.lmn_region_bwd(a["logits"], a["target"], g["tk"], g["head"], g["per_image"], g["B"], g["C"], g["H"], g["W"], cm, a["coef"], None,
                                a["dlogits"], None)
    return rc, lib.lmn_last_error().decode()


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_loss_entries_reject_bad_arguments(which):
    from lm_net_amd import hip
    pre = "region_%s: " % which
    for name in (FWD_POINTERS if which == "fwd" else BWD_POINTERS):
        rc, err = _entry(which, null=(name,))
        assert rc == -1 and err == pre + "null pointer", (name, err)
    cases = [(dict(head=2), "unknown head 2"), (dict(B=0), "B=0 not in [1, 65535]"), (dict(B=65536, C=2, H=1, W=1, class_mask=1), "B=65536 not in"),
             (dict(C=65), "C=65 not in [1, 64]"), (dict(C=0, class_mask=1), "C=0"), (dict(C=1, class_mask=1), "C=1 needs a sigmoid head"),
             (dict(H=0), "size 0x65 below 1"), (dict(W=-1), "size 33x-1"), (dict(class_mask=0), "class_mask is empty"),
             (dict(class_mask=1 << 4), "a class >= C=4"), (dict(tk=7), "unknown label kind 7"),
             (dict(B=600, C=4, H=1024, W=1024, class_mask=2), "B * C * H * W")]
    if which == "fwd":
        cases += [(dict(kind=4), "unknown kind 4"), (dict(kind=-1), "unknown kind -1"), (dict(den=2), "unknown denominator 2"),
                  (dict(kind=hip.REGION_TVERSKY, den=hip.REGION_SQUARED), "squared denominator exists for dice and jaccard only"),
                  (dict(kind=hip.REGION_GDICE, den=hip.REGION_SQUARED), "squared denominator exists for dice and jaccard only"),
                  (dict(alpha=-0.1), "alpha=-0.1"), (dict(beta=-1.0), "beta=-1"), (dict(alpha=float("nan")), "must be finite and >= 0"),
                  (dict(smooth=-1e-3), "smooth=-0.001"), (dict(smooth=float("inf")), "smooth=inf"),
                  (dict(exponent=0.0), "exponent=0 not in (0, 8]"), (dict(exponent=8.5), "exponent=8.5 not in (0, 8]"),
                  (dict(exponent=float("nan")), "not in (0, 8]"), (dict(scale=float("inf")), "scale=inf is not finite"),
                  (dict(scale=float("nan")), "is not finite"), (dict(kind=hip.REGION_GDICE, den=0, weight=FAKE), "takes no class weight"),
                  (dict(ws_bytes=100), "workspace of 100 bytes too small")]
    for kw, msg in cases:
        rc, err = _entry(which, **kw)
        assert rc == -1 and msg in err and err.startswith(pre), (kw, err)
    if which == "fwd":                                     # the bounds themselves pass: the last check, of the workspace, is reached
        for kw in (dict(B=1, C=1, H=1, W=1, class_mask=1, head=hip.REGION_SIGMOID, den=0, kind=hip.REGION_TVERSKY, alpha=0.0, beta=0.0, smooth=0.0),
                   dict(B=2, C=64, H=5, W=7, class_mask=1 << 63, exponent=8.0), dict(B=65535, C=2, H=1, W=1, class_mask=3, per_image=1, exponent=1e-3)):
            need = hip.region_workspace(kw.get("head", 0), kw["B"], kw["C"], kw["H"], kw["W"], kw["class_mask"])
            rc, err = _entry(which, ws_bytes=need - 1, **kw)
            assert rc == -1 and "workspace of %d bytes too small, %d needed" % (need - 1, need) in err, err


def test_deterministic_mode_needs_the_workspace():
    """The slots are the caller's: without a workspace the forward is refused in deterministic mode, before any HIP call."""
    from lm_net_amd import hip
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    try:
        rc, err = _entry("fwd", null=("workspace",))
    finally:
        hip.set_deterministic(was)
    assert rc == -1 and err == "region_fwd: deterministic mode needs the workspace"


def test_workspace_is_host_arithmetic():
    from lm_net_amd import hip
    up = lambda v: (v + 255) // 256 * 256
    cdiv = lambda a, b: (a + b - 1) // b
    for head, B, C, H, W, mask in ((0, 1, 2, 1, 1, 3), (0, 8, 2, 352, 352, 3), (0, 8, 9, 352, 352, 0b110), (0, 2000, 3, 40, 40, 7), (1, 2, 1, 5, 7, 1),
                                   (1, 8, 9, 352, 352, 0x1ff), (1, 2, 3, 16, 20, 5), (1, 1, 64, 8, 8, (1 << 64) - 1)):
        nk, hw = bin(mask).count("1"), H * W
        if head == 0:
            nbx = max(1, min(cdiv(hw, 256), max(1, 1024 // B)))
        else:
            nbx = max(1, min(cdiv(hw // 4 if hw % 4 == 0 else hw, 256), max(1, 2048 // (B * C))))
        assert hip.region_workspace(head, B, C, H, W, mask) == up(4 * B * nbx * nk * 3), (head, B, C, H, W)
    for args, msg in (((0, 0, 2, 8, 8, 3), "B=0"), ((0, 2, 1, 8, 8, 1), "C=1 needs a sigmoid head"), ((1, 2, 3, 8, 8, 8), "a class >= C=3"),
                      ((2, 2, 3, 8, 8, 1), "unknown head"), ((0, 70000, 2, 1, 1, 1), "B=70000")):
        with pytest.raises(ValueError, match="region_workspace"):
            hip.region_workspace(*args)
        assert msg in hip.load().lmn_last_error().decode()


def test_python_refuses_what_it_cannot_run():
    """The family's own rules; what it shares with the other criteria (class count, class list, head, logits, target, scale, "no CPU
    fallback") is in tests/test_criteria_cpu.py."""
    from lm_net_amd import RegionLoss
    for kw, msg in ((dict(n_classes=3, classes="present"), "None or a list"), (dict(n_classes=3, kind="lovasz"), "kind"),
                    (dict(n_classes=3, denominator="cubed"), "denominator"), (dict(n_classes=3, kind="tversky", denominator="squared"), "dice and jaccard only"),
                    (dict(n_classes=3, kind="generalized_dice", denominator="squared"), "dice and jaccard only"),
                    (dict(n_classes=3, kind="generalized_dice", weight=[1, 1, 1]), "no class weight"), (dict(n_classes=3, weight=[1, 2]), "one per scored class"),
                    (dict(n_classes=3, classes=[1], weight=[1, 2, 3]), "one per scored class"), (dict(n_classes=3, alpha=-1), "alpha"),
                    (dict(n_classes=3, beta=float("inf")), "beta"), (dict(n_classes=3, smooth=-1), "smooth"), (dict(n_classes=3, exponent=0), "exponent"),
                    (dict(n_classes=3, exponent=9), "exponent")):
        with pytest.raises(ValueError, match=msg):
            RegionLoss(**kw)
    with pytest.raises(ValueError, match="above the limit 65535"):
        RegionLoss(3)(torch.zeros(65536, 3, 1, 1), torch.zeros(65536, 1, 1, dtype=torch.uint8))
    assert (RegionLoss(4, classes=[3, 1]).classes, RegionLoss(4, classes=[3, 1]).class_mask) == ([1, 3], 0b1010)
    assert RegionLoss(4).denominator == "squared" and RegionLoss(4, "jaccard").denominator == "squared"
    assert RegionLoss(4, "tversky").denominator == "linear" and RegionLoss(4, "generalized_dice").denominator == "linear"


# ---------------------------------------------------------------- the restatement against the reference's classes
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "region_ref.npz"))


def _close(got, want, rel=1e-12):
    return np.abs(np.asarray(got) - np.asarray(want)).max() <= rel * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("C", [2, 4])
def test_restatement_equals_the_reference_classes(C):
    """DiceLoss (weights; with and without void), BCEDiceLoss and offical_DiceLoss of the reference's utils/loss.py, recorded by
    tools/make_golden_region.py in float64.  offical_DiceLoss is compared without void labels only: its denominator ignores the
    valid mask."""
    w = [1.0 + 1.5 * k for k in range(C)]
    B = 3
    for tag, void in (("", 0.0), ("_void", 0.2)):
        lg, y = R.inputs(B, C, 5, 7, seed=11 + C, void=void)
        assert (y == R.VOID).any() == bool(void)
        r = R.loss_and_grad(lg, y, C, weight=w)                                       # dice, squared, batch, smooth 1e-5
        assert _close(r.loss, GOLDEN["dice%s/%d/loss" % (tag, C)][0]) and _close(r.grad, GOLDEN["dice%s/%d/dlogits" % (tag, C)])
    lg, y = R.inputs(B, C, 5, 7, seed=11 + C)
    z = torch.from_numpy(lg).double().requires_grad_(True)
    ce = torch.nn.functional.cross_entropy(z, torch.from_numpy(y))
    ce.backward()
    r = R.loss_and_grad(lg, y, C, per_image=True, denominator="linear", smooth=1e-7)
    assert _close(0.4 * float(ce.detach()) + 0.6 * r.loss, GOLDEN["bcedice/%d/loss" % C][0])
    assert _close(0.4 * z.grad.numpy() + 0.6 * r.grad, GOLDEN["bcedice/%d/dlogits" % C])
    r = R.loss_and_grad(lg, y, C, per_image=True, smooth=1.0)
    assert _close(B * r.loss, GOLDEN["offical/%d/loss" % C][0]) and _close(B * r.grad, GOLDEN["offical/%d/dlogits" % C])


@pytest.mark.skipif(not __import__("void_ref").reference_available(), reason="the reference tree is not on this machine")
def test_golden_is_what_the_reference_computes():
    """Where the reference tree exists, the golden is recomputed from its code (tools/make_golden_region.py) and must not have moved."""
    from tools.make_golden_region import compute
    live = compute()
    assert sorted(live) == sorted(GOLDEN.files)
    for name, want in live.items():
        assert _close(GOLDEN[name], want, 1e-14), name


# ---------------------------------------------------------------- the restatement against a torch float64 composition
def _torch_loss(lg, y, C, kind, head, classes, weight, per_image, denominator, smooth, alpha, beta, exponent, scale):
    """The same losses as a plain torch composition: softmax / sigmoid, masked sums, the ratio, (1 - R) ** exponent, a mean."""
    z = torch.tensor(np.asarray(lg, dtype=np.float64), requires_grad=True)
    t, valid = (torch.from_numpy(np.ascontiguousarray(a)) for a in R.targets(y, C, head))
    m = valid.double()
    p = torch.softmax(z, 1) if head == "softmax" else torch.sigmoid(z)
    ids = R.class_ids(C, classes)
    dims = (2, 3) if per_image else (0, 2, 3)
    red = lambda a: a[:, ids].sum(dims).reshape(-1, len(ids))
    I, P1, P2, T = red(p * t * m), red(p * m), red(p * p * m), red(t * m)
    D = (P2 if denominator == "squared" else P1) + T
    if kind == "dice":
        R_ = (2 * I + smooth) / (D + smooth)
    elif kind == "jaccard":
        R_ = (I + smooth) / (D - I + smooth)
    elif kind == "tversky":
        R_ = (I + smooth) / (I + alpha * (P1 - I) + beta * (T - I) + smooth)
    else:
        v = torch.where(T > 0, 1.0 / (T * T).clamp_min(1e-300), torch.zeros_like(T))
        v = torch.where(T > 0, v, v.max(1, keepdim=True).values.expand_as(v))
        R_ = ((2 * (v * I).sum(1) + smooth) / ((v * (P1 + T)).sum(1) + smooth))[:, None].expand_as(I)
    w = torch.ones(len(ids), dtype=torch.float64) if weight is None else torch.tensor(weight, dtype=torch.float64)
    loss = scale * ((1 - R_) ** exponent * w).mean()
    loss.backward()
    return float(loss.detach()), z.grad.numpy()


CONFIGS = [dict(kind="tversky", alpha=0.3, beta=0.7), dict(kind="tversky", alpha=0.7, beta=0.3, exponent=0.75, per_image=True, weight=True),
           dict(kind="jaccard"), dict(kind="jaccard", denominator="linear", per_image=True, exponent=2.0, weight=True),
           dict(kind="generalized_dice"), dict(kind="generalized_dice", per_image=True, exponent=0.75, smooth=0.0),
           dict(kind="dice", denominator="linear", classes=True), dict(kind="dice", per_image=True, classes=True, weight=True, smooth=1.0)]


def _config(cfg, C, head):
    kw = dict(kind="dice", head=head, classes=None, weight=None, per_image=False, denominator=None, smooth=1e-5, alpha=0.5, beta=0.5, exponent=1.0,
              scale=0.7)
    kw.update(cfg)
    if kw["denominator"] is None:
        kw["denominator"] = "squared" if kw["kind"] in ("dice", "jaccard") else "linear"
    if kw["classes"] is True:
        kw["classes"] = [C - 1] if C < 3 else [1, C - 1]
    if kw["weight"] is True:
        kw["weight"] = [1.0 + 0.5 * k for k in range(len(R.class_ids(C, kw["classes"])))]
    return kw


@pytest.mark.parametrize("head,C", [("softmax", 2), ("softmax", 4), ("sigmoid", 1), ("sigmoid", 3)])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join("%s" % v for v in c.values()))
def test_restatement_equals_torch_autograd(cfg, head, C):
    kw = _config(cfg, C, head)
    lg, y = R.inputs(3, C, 5, 7, head, seed=5, void=0.2)
    want, wgrad = _torch_loss(lg, y, C, **kw)
    r = R.loss_and_grad(lg, y, C, **kw)
    assert want > 0 and abs(r.loss - want) < 1e-10 and np.abs(r.grad - wgrad).max() < 1e-10
    t, valid = R.targets(y, C, head)
    assert (~valid).any() and not r.grad[~valid].any() and not np.signbit(r.grad[~valid]).any()          # +0 at every void position


@pytest.mark.parametrize("head,C", [("softmax", 3), ("sigmoid", 2)])
@pytest.mark.parametrize("per_image", [False, True])
def test_identities(head, C, per_image):
    lg, y = R.inputs(3, C, 5, 7, head, seed=9, void=0.2)
    kw = dict(head=head, per_image=per_image, weight=[1.0, 4.0, 2.0][:C])
    for s in (0.0, 1e-5, 1.0):
        a = R.loss_and_grad(lg, y, C, kind="tversky", alpha=0.5, beta=0.5, smooth=s, **kw)
        b = R.loss_and_grad(lg, y, C, kind="dice", denominator="linear", smooth=2 * s, **kw)
        assert abs(a.loss - b.loss) < 1e-12 and np.abs(a.grad - b.grad).max() < 1e-12
        a = R.loss_and_grad(lg, y, C, kind="tversky", alpha=1.0, beta=1.0, smooth=s, **kw)
        b = R.loss_and_grad(lg, y, C, kind="jaccard", denominator="linear", smooth=s, **kw)
        assert abs(a.loss - b.loss) < 1e-12 and np.abs(a.grad - b.grad).max() < 1e-12


# ---------------------------------------------------------------- finite differences
@pytest.mark.parametrize("head,C", [("softmax", 3), ("sigmoid", 2)])
@pytest.mark.parametrize("cfg", [dict(kind="dice"), dict(kind="jaccard", per_image=True), dict(kind="tversky", alpha=0.3, beta=0.7, exponent=0.75),
                                 dict(kind="tversky", alpha=0.3, beta=0.7, exponent=0.75, per_image=True, weight=True),
                                 dict(kind="generalized_dice", exponent=0.75), dict(kind="generalized_dice", per_image=True)],
                         ids=lambda c: "-".join("%s" % v for v in c.values()))
def test_gradient_equals_finite_differences(cfg, head, C):
    """Central differences of the restatement itself, on random logits of unit scale, for which u >= 0.05 everywhere: exponent = 0.75
    is tested away from its singular point."""
    kw = _config(cfg, C, head)
    lg, y = R.inputs(2, C, 4, 5, head, seed=7, void=0.15)
    lg = lg.astype(np.float64)
    r = R.loss_and_grad(lg, y, C, gscale=2.0, **kw)
    assert r.u.min() >= 0.05, r.u
    h = 1e-6
    rng = np.random.default_rng(0)
    for _ in range(12):
        at = tuple(rng.integers(0, n) for n in lg.shape)
        hi, lo = lg.copy(), lg.copy()
        hi[at] += h
        lo[at] -= h
        fd = 2.0 * (R.loss_and_grad(hi, y, C, **kw).loss - R.loss_and_grad(lo, y, C, **kw).loss) / (2 * h)
        assert abs(fd - r.grad[at]) < 1e-6 * max(abs(fd), np.abs(r.grad).max()), (at, fd, r.grad[at])


# ---------------------------------------------------------------- edge rules
KINDS = [("dice", "squared"), ("dice", "linear"), ("jaccard", "squared"), ("jaccard", "linear"), ("tversky", "linear"), ("generalized_dice", "linear")]


@pytest.mark.parametrize("kind,den", KINDS)
@pytest.mark.parametrize("head", ["softmax", "sigmoid"])
def test_all_void_image_and_batch(kind, den, head):
    C = 3
    lg, y = R.inputs(2, C, 4, 5, head, seed=3)
    full = R.loss_and_grad(lg[:1], y[:1], C, kind=kind, head=head, denominator=den, per_image=True, exponent=0.75)
    y[1] = R.VOID                                         # one all-void image: it counts in the mean with L = 0
    for s in (0.0, 1e-5):
        r = R.loss_and_grad(lg, y, C, kind=kind, head=head, denominator=den, per_image=True, smooth=s, exponent=0.75)
        assert not r.per_class[1].any() and not r.coef[1].any() and not r.counts[1].any()
        assert not r.grad[1].any() and not np.signbit(r.grad[1]).any() and np.isfinite(r.loss)
        if s:
            assert abs(r.loss - 0.5 * full.loss) < 1e-12 and np.abs(r.grad[0] - 0.5 * full.grad[0]).max() < 1e-12
        y2 = np.full_like(y, R.VOID)                      # an all-void batch: 0, no gradient bit set
        for per_image in (False, True):
            r = R.loss_and_grad(lg, y2, C, kind=kind, head=head, denominator=den, per_image=per_image, smooth=s, exponent=0.75)
            assert r.loss == 0.0 and not r.grad.any() and not np.signbit(r.grad).any() and not r.coef.any() and not r.counts.any()


@pytest.mark.parametrize("absent", [[2], [1, 3], [0, 1, 2, 3]])
def test_generalized_dice_with_absent_classes(absent):
    """A class with T_k = 0 takes the largest finite v of its group; 0 when the group has none (every T_k = 0)."""
    C = 4
    lg, y = R.inputs(2, C, 6, 7, "sigmoid", seed=4)
    y[:, absent] = 0
    r = R.loss_and_grad(lg, y, C, kind="generalized_dice", head="sigmoid", smooth=1e-5)
    T = r.counts[0, :, 0].astype(np.float64)
    assert sorted(np.flatnonzero(T == 0)) == absent
    if len(absent) == C:
        assert abs(r.loss - 0.0) < 1e-12 and not r.coef.any()          # v = 0 everywhere: R = s / s = 1
        assert R.loss_and_grad(lg, y, C, kind="generalized_dice", head="sigmoid", smooth=0.0).loss == 0.0      # 0 / 0: R = 1
        return
    v = np.where(T > 0, 1.0 / np.maximum(T, 1) ** 2, (1.0 / T[T > 0] ** 2).max())
    I, P1 = r.sums[0, :, 0], r.sums[0, :, 1]
    want = 1.0 - (2 * (v * I).sum() + 1e-5) / ((v * (P1 + T)).sum() + 1e-5)
    assert abs(r.loss - want) < 1e-12 and np.all(r.per_class == r.per_class[0, 0])
    wl, wg = _torch_loss(lg, y, C, "generalized_dice", "sigmoid", None, None, False, "linear", 1e-5, 0.5, 0.5, 1.0, 1.0)
    assert abs(r.loss - wl) < 1e-10 and np.abs(r.grad - wg).max() < 1e-10


@pytest.mark.parametrize("kind,den", KINDS)
def test_empty_class_without_smoothing(kind, den):
    """s = 0 and a class without a foreground element: the ratio is 0 over a positive denominator (L = 1) while p > 0; with p = 0 on the
    whole plane too the denominator is exactly 0: R = 1, the loss is 0 and its coefficients are 0."""
    C = 2
    lg, y = R.inputs(2, C, 4, 5, "sigmoid", seed=6)
    y[:, 1] = 0
    r = R.loss_and_grad(lg, y, C, kind=kind, head="sigmoid", denominator=den, smooth=0.0)
    assert np.isfinite(r.loss) and np.isfinite(r.grad).all()
    if kind != "generalized_dice":
        assert r.per_class[0, 1] == 1.0
    p = R.probabilities(lg, "sigmoid")
    p[:, 1] = 0.0
    r = R.loss_and_grad(lg, y, C, kind=kind, head="sigmoid", denominator=den, smooth=0.0, classes=[1], p=p)
    assert r.loss == 0.0 and not r.coef.any() and not r.per_class.any()


@pytest.mark.parametrize("kind,den", KINDS)
def test_saturated_foreground_under_a_fractional_exponent(kind, den):
    """p exactly 1 on a full-foreground plane: u <= 0, so exponent = 0.75 gives loss 0 and coefficients 0 instead of 0 ** -0.25."""
    C = 2
    lg, y = R.inputs(2, C, 4, 5, "sigmoid", seed=8)
    y[:] = 1
    p = np.ones_like(lg, dtype=np.float64)
    for s in (0.0, 1e-5):
        r = R.loss_and_grad(lg, y, C, kind=kind, head="sigmoid", denominator=den, smooth=s, exponent=0.75, per_image=True, p=p)
        assert r.u.max() <= 0.0 and r.loss == 0.0 and not r.coef.any() and not r.grad.any()
    r = R.loss_and_grad(lg, y, C, kind=kind, head="sigmoid", denominator=den, exponent=1.0, p=p)
    assert abs(r.loss) < 1e-15 and r.coef.any()           # exponent 1 keeps L = u and its derivative

"""CPU: the host side of the Lovasz losses (include/lovasz/lmnet_lovasz.h; lm_net_amd.loss.LovaszLoss, lovasz_ranks): registry and
header agree, the argument checks of the four C entries (rejected before any HIP call,
with fake device pointers), the workspace formula, the classes' ValueErrors, and the restatement tests/lovasz_ref.py: its closed-form
coefficients against Berman's cumsum form, the whole of it against a direct torch.sort transcription of lovasz_softmax_flat /
lovasz_hinge_flat, its gradients against finite differences, and the edge cases.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lovasz_ref as R
from lm_net_amd import LovaszLoss, hip, lovasz_ranks  # noqa: F401  (every test of this file belongs to the feature)

assert callable(hip.lovasz_order)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_ENTRIES = ["lmn_lovasz_order", "lmn_lovasz_fwd", "lmn_lovasz_bwd"]


# ---------------------------------------------------------------- ABI
def test_registry_and_header_agree():
    """The feature's own part of the registry: the literal list, its place in hip.HEADERS, the number of #defines, the header's
    citations and the package's exports.  (Header / export / layout / return-type / constants checks: tests/test_host_cpu.py.)"""
    from lm_net_amd import hip
    assert hip.SYMBOLS_LOVASZ == ["lmn_lovasz_workspace"] + DEVICE_ENTRIES
    assert hip.HEADERS["lovasz/lmnet_lovasz.h"] is hip.SYMBOLS_LOVASZ
    header = open(os.path.join(ROOT, "include", "lovasz", "lmnet_lovasz.h")).read()
    assert len(re.findall(r"^#define LMN_LOVASZ_\w+ \d+\b", header, re.M)) == 8
    assert hip.LOVASZ_TILE % 256 == 0 and hip.LOVASZ_SUMS_WORDS == 4
    for cite in ("TIES BY ELEMENT INDEX ASCENDING", "g_r = 1 / (G + m_r)", "(G - n_r) / ((G + m_r - 1) (G + m_r))", "g_0 = 1", "never NaN",
                 "NO FLOAT ATOMICS", "NO KERNEL WAITS ON ANOTHER BLOCK", "every loop of every kernel is bounded", "lovasz_order: ",
                 "lovasz_fwd: ", "lovasz_bwd: ", "keys (uint32 [S, P]) is not modified"):
        assert cite in header, cite
    import lm_net_amd
    from lm_net_amd import loss
    for name in ("LovaszLoss", "lovasz_ranks"):
        assert getattr(lm_net_amd, name) is getattr(loss, name) and name in lm_net_amd.__all__
    assert "Deliberate difference" in loss.LovaszLoss.__doc__


# ---------------------------------------------------------------- argument checks
FAKE = ctypes.c_void_p(0x1000)
BIG = ctypes.c_int64(1 << 40)


def _order(null=(), S=3, P=100, ws_bytes=1 << 40):
    from lm_net_amd import hip
    lib = hip.load()
    a = dict(keys=FAKE, workspace=FAKE, perm=FAKE)
    for k in null:
        a[k] = None
    rc = lib.lmn_lovasz_order(a["keys"], S, ctypes.c_int64(P), a["workspace"], ctypes.c_int64(ws_bytes), a["perm"], None)
    return rc, lib.lmn_last_error().decode()


def test_order_rejects_bad_arguments():
    from lm_net_amd import hip
    for name in ("keys", "workspace", "perm"):
        rc, err = _order(null=(name,))
        assert rc == -1 and err == "lovasz_order: null pointer", (name, err)
    for kw in (dict(S=0), dict(S=65536), dict(P=0), dict(S=2, P=1 << 30), dict(S=-1)):
        rc, err = _order(**kw)
        assert rc == -1 and err.startswith("lovasz_order: S=") and "outside 1 <= S <= 65535, P >= 1, S * P < 2^31" in err, (kw, err)
    for S, P in ((1, 1), (3, 100), (65535, 7), (1, (1 << 31) - 1)):
        need = hip.lovasz_workspace(S, P)
        rc, err = _order(S=S, P=P, ws_bytes=need - 1)
        assert rc == -1 and "workspace of %d bytes too small, %d needed" % (need - 1, need) in err, err


FWD_POINTERS = ("logits", "target", "workspace", "errors", "perm", "counts", "coef", "sums", "loss")
BWD_POINTERS = ("logits", "target", "coef", "sums", "dlogits")


def _loss(which, null=(), **kw):
    """lmn_lovasz_fwd / _bwd with fake device pointers: every case here must be rejected before any HIP call."""
    from lm_net_amd import hip
    lib = hip.load()
    a = {k: FAKE for k in (FWD_POINTERS if which == "fwd" else BWD_POINTERS)}
    for k in null:
        a[k] = None
    g = dict(dict(kind=1, head=0, per_image=0, present=1, scale=1.0, B=3, C=4, H=33, W=65, class_mask=0b1110, ws_bytes=1 << 40), **kw)
    cm = ctypes.c_uint64(g["class_mask"])
    if which == "fwd":
        rc = lib.lmn_lovasz_fwd(a["logits"], a["target"], g["kind"], g["head"], g["per_image"], g["present"], ctypes.c_float(g["scale"]), g["B"],
                                g["C"], g["H"], g["W"], cm, a["workspace"], ctypes.c_int64(g["ws_bytes"]), a["errors"], a["perm"], a["counts"],
                                a["coef"], a["sums"], a["loss"], None)
    else:
        rc = lib.lmn_lovasz_bwd(a["logits"], a["target"], g["kind"], g["head"], g["B"], g["C"], g["H"], g["W"], cm, a["coef"], a["sums"], None,
                                a["dlogits"], None)
    return rc, lib.lmn_last_error().decode()


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_loss_entries_reject_bad_arguments(which):
    from lm_net_amd import hip
    pre = "lovasz_%s: " % which
    for name in (FWD_POINTERS if which == "fwd" else BWD_POINTERS):
        rc, err = _loss(which, null=(name,))
        assert rc == -1 and err == pre + "null pointer", (name, err)
    cases = [(dict(head=2), "unknown head 2"), (dict(B=0), "B=0 < 1"), (dict(C=65), "C=65 not in [1, 64]"), (dict(C=0, class_mask=1), "C=0"),
             (dict(C=1, class_mask=1), "C=1 needs a sigmoid head"), (dict(H=0), "size 0x65 below 1"), (dict(W=-1), "size 33x-1"),
             (dict(class_mask=0), "class_mask is empty"), (dict(class_mask=1 << 4), "a class >= C=4"), (dict(kind=7), "unknown label kind 7"),
             (dict(B=600, C=4, H=1024, W=1024, class_mask=2), "B * C * H * W")]
    if which == "fwd":
        cases += [(dict(scale=float("inf")), "scale=inf is not finite"), (dict(scale=float("nan")), "is not finite"),
                  (dict(B=30000, C=3, H=2, W=2, class_mask=0b111, per_image=1), "90000 segments above 65535"),
                  (dict(ws_bytes=1000), "workspace of 1000 bytes too small")]
    for kw, msg in cases:
        rc, err = _loss(which, **kw)
        assert rc == -1 and msg in err and err.startswith(pre), (kw, err)
    if which == "fwd":                                     # the bounds themselves pass: the last check, of the workspace, is reached
        for kw, (S, P) in ((dict(B=1, C=1, H=1, W=1, class_mask=1, head=hip.LOVASZ_SIGMOID), (1, 1)),
                           (dict(B=2, C=64, H=5, W=7, class_mask=1 << 63), (1, 70)),
                           (dict(B=2, C=64, H=5, W=7, class_mask=(1 << 64) - 1, per_image=1), (128, 35))):
            need = hip.lovasz_workspace(S, P)
            rc, err = _loss(which, ws_bytes=need - 1, **kw)
            assert rc == -1 and "workspace of %d bytes too small, %d needed" % (need - 1, need) in err, err


def test_workspace_is_host_arithmetic():
    from lm_net_amd import hip
    up = lambda v: (v + 255) // 256 * 256
    T = hip.LOVASZ_TILE
    for S, P in ((1, 1), (3, 1920), (2, 8 * 352 * 352), (72, 352 * 352), (17, 3 * T + 17), (1, T), (1, T + 1), (65535, 100)):
        nb = (P + T - 1) // T
        assert hip.lovasz_workspace(S, P) == 4 * up(4 * S * P) + up(4 * S * 256 * nb) + up(4 * S * 256) + 2 * up(4 * S * nb) + up(4 * S)
    assert hip.lovasz_workspace(1, 1) == 4 * 256 + 1024 + 1024 + 3 * 256
    for args, msg in (((0, 8), "S=0"), ((65536, 8), "S=65536"), ((1, 0), "P=0"), ((2, 1 << 30), "P=1073741824")):
        with pytest.raises(ValueError, match="lovasz_workspace"):
            hip.lovasz_workspace(*args)
        assert msg in hip.load().lmn_last_error().decode()


def test_python_refuses_what_it_cannot_run():
    """The family's own rules; what it shares with the other criteria (class count, class list, head, logits, target, scale, "no CPU
    fallback") is in tests/test_criteria_cpu.py."""
    from lm_net_amd import LovaszLoss
    with pytest.raises(ValueError, match="'present', 'all'"):
        LovaszLoss(n_classes=3, classes="some")
    with pytest.raises(ValueError, match="segments above the limit"):
        LovaszLoss(3, per_image=True)(torch.zeros(30000, 3, 1, 1), torch.zeros(30000, 1, 1, dtype=torch.uint8))
    assert (LovaszLoss(4, classes=[3, 1]).classes, LovaszLoss(4, classes=[3, 1]).class_mask, LovaszLoss(4, classes=[3, 1]).present) == ([1, 3], 0b1010, False)
    assert LovaszLoss(4).present and not LovaszLoss(4, classes="all").present and not LovaszLoss(4, head="sigmoid").present


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("P", [1, 2, 5, 1000])
@pytest.mark.parametrize("frac", [0.0, 0.3, 1.0])
def test_closed_form_equals_cumsum_form(P, frac):
    rng = np.random.default_rng(P)
    fg = rng.random(P) < frac if 0.0 < frac < 1.0 else np.full(P, frac == 1.0)
    a, b = R.coefficients(fg, P), R.coefficients_cumsum(fg)
    assert np.abs(a - b).max() < 1e-12, (P, frac)
    assert abs(a.sum() - 1.0) < 1e-12                       # the Jaccard loss of the whole segment is 1 at the last rank
    V = P // 2                                              # void ranks: the valid prefix alone counts
    a = R.coefficients(fg, V)
    assert np.all(a[V:] == 0) and (V == 0 or np.abs(a[:V] - R.coefficients_cumsum(fg[:V])).max() < 1e-12)


def _berman_grad(gt_sorted):
    gts = gt_sorted.sum()
    intersection = gts - gt_sorted.cumsum(0)
    union = gts + (1 - gt_sorted).cumsum(0)
    jaccard = 1.0 - intersection / union
    if len(gt_sorted) > 1:
        jaccard[1:] = jaccard[1:] - jaccard[:-1].clone()
    return jaccard


def _berman_softmax_flat(probas, labels, classes):
    """lovasz_softmax_flat of the paper's reference code: probas [P, C], labels [P]."""
    losses = []
    for c in (range(probas.shape[1]) if classes in ("all", "present") else classes):
        fg = (labels == c).double()
        if classes == "present" and fg.sum() == 0:
            continue
        errors = (fg - probas[:, c]).abs()
        errors_sorted, perm = torch.sort(errors, dim=0, descending=True, stable=True)
        losses.append(torch.dot(errors_sorted, _berman_grad(fg[perm])))
    return sum(losses) / len(losses) if losses else probas.sum() * 0.0


def _berman_hinge_flat(logits, labels):
    signs = 2.0 * labels.double() - 1.0
    errors = 1.0 - logits * signs
    errors_sorted, perm = torch.sort(errors, dim=0, descending=True, stable=True)
    return torch.dot(torch.relu(errors_sorted), _berman_grad(labels.double()[perm]))


def _berman(logits, y, head, classes, per_image):
    """The transcription over a batch: void elements removed first, as the reference code's flatten_probas does."""
    z = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    B, C = z.shape[:2]
    t = torch.as_tensor(y.astype(np.int64))
    groups = [[b] for b in range(B)] if per_image else [list(range(B))]
    total = 0.0
    for grp in groups:
        if head == "softmax":
            p = torch.softmax(z[grp], 1).permute(0, 2, 3, 1).reshape(-1, C)
            lab = t[grp].reshape(-1)
            keep = lab < C
            total = total + _berman_softmax_flat(p[keep], lab[keep], classes)
        else:
            planes = 0.0
            for c in range(C):
                zz, lab = z[grp][:, c].reshape(-1), t[grp][:, c].reshape(-1)
                keep = lab <= 1
                planes = planes + (_berman_hinge_flat(zz[keep], lab[keep]) if keep.any() else zz.sum() * 0.0)
            total = total + planes / C
    total = total / len(groups)
    total.backward()
    return float(total.detach()), z.grad.numpy()


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("head,C,classes", [("softmax", 2, "present"), ("softmax", 4, "present"), ("softmax", 4, "all"), ("softmax", 5, [1, 3]),
                                            ("sigmoid", 1, "all"), ("sigmoid", 3, "all")])
def test_restatement_equals_berman(head, C, classes, per_image):
    """Tie-free inputs (continuous logits) with 20 % void and, at C = 4, a class that is absent from the second image."""
    lg, y = R.inputs(2, C, 9, 11, head, seed=3, void=0.2)
    if head == "softmax" and C == 4:
        y[1][y[1] == 2] = 0
    want, wgrad = _berman(lg, y, head, classes, per_image)
    loss, grad, counts, _ = R.loss_and_grad(lg, y, C, head, classes, per_image)
    assert abs(loss - want) < 1e-12 * max(1.0, abs(want)) and want > 0
    assert np.abs(grad - wgrad).max() < 1e-12
    void = (y >= C) if head == "softmax" else (y > 1)
    at_void = grad[np.broadcast_to(void[:, None] if head == "softmax" else void, grad.shape)]
    assert at_void.size and not at_void.any() and not np.signbit(at_void).any()                      # +0 at every void position
    assert counts[:, 0].min() > 0


@pytest.mark.parametrize("head,C,classes,per_image", [("softmax", 3, "present", False), ("softmax", 3, "all", True), ("sigmoid", 2, "all", False)])
def test_gradient_equals_finite_differences(head, C, classes, per_image):
    """Away from ties the order is locally constant, so the loss is differentiable: central differences of the restatement itself."""
    lg, y = R.inputs(2, C, 4, 5, head, seed=7, void=0.15)
    lg = lg.astype(np.float64)
    loss, grad, _, perm = R.loss_and_grad(lg, y, C, head, classes, per_image, scale=0.5, gscale=2.0)
    h = 1e-6
    rng = np.random.default_rng(0)
    for _ in range(12):
        at = tuple(rng.integers(0, n) for n in lg.shape)
        hi, lo = lg.copy(), lg.copy()
        hi[at] += h
        lo[at] -= h
        fh, _, _, ph = R.loss_and_grad(hi, y, C, head, classes, per_image, scale=0.5)
        fl, _, _, pl = R.loss_and_grad(lo, y, C, head, classes, per_image, scale=0.5)
        assert np.array_equal(ph, perm) and np.array_equal(pl, perm)             # (no tie was crossed)
        assert abs(2.0 * (fh - fl) / (2 * h) - grad[at]) < 1e-6, at


def test_edge_cases():
    # P = 1, G = P: the loss is the one error; G = 0 ("all"): the largest error, "present": nothing to average, 0
    z = np.array([[[[0.3]], [[-0.2]]]])
    p = np.exp(z[0, :, 0, 0]) / np.exp(z[0, :, 0, 0]).sum()
    loss, grad, counts, _ = R.loss_and_grad(z, np.array([[[1]]]), 2, classes=[1])
    assert abs(loss - (1 - p[1])) < 1e-15 and counts.tolist() == [[1, 1]]
    loss, _, counts, _ = R.loss_and_grad(z, np.array([[[0]]]), 2, classes=[1])
    assert abs(loss - p[1]) < 1e-15 and counts.tolist() == [[1, 0]]
    z2 = np.random.default_rng(1).standard_normal((1, 3, 2, 3))
    y2 = np.zeros((1, 2, 3), dtype=np.uint8)
    pk = torch.softmax(torch.tensor(z2), 1).numpy()
    loss, _, _, _ = R.loss_and_grad(z2, y2, 3, classes=[2])
    assert abs(loss - pk[0, 2].max()) < 1e-15
    loss, grad, _, _ = R.loss_and_grad(z2, np.full((1, 2, 3), 7, dtype=np.uint8), 3, classes="present")
    assert loss == 0.0 and not grad.any() and not np.signbit(grad).any()
    # all void: 0 in every reduction, no gradient bit set
    for head, classes, per_image in (("softmax", "all", False), ("softmax", "present", True), ("sigmoid", "all", True)):
        yv = np.full((1, 2, 3) if head == "softmax" else (1, 3, 2, 3), 255, dtype=np.uint8)
        loss, grad, counts, _ = R.loss_and_grad(z2, yv, 3, head, classes, per_image)
        assert loss == 0.0 and not grad.any() and not np.signbit(grad).any() and not counts.any()
    # exact ties: equal errors keep their index order, void goes last
    e = np.array([[0.5, 0.25, 0.5, 0.0, 0.25, 0.5]])
    v = np.array([[True, True, True, False, True, True]])
    assert R.stable_order(e, v).tolist() == [[0, 2, 5, 1, 4, 3]]
    # the hinge on tied integer logits: constant logits, the order is the index order among equal errors
    zt = np.zeros((1, 1, 2, 2))
    loss, grad, counts, perm = R.loss_and_grad(zt, np.array([[[[1, 0], [0, 1]]]], dtype=np.uint8), 1, "sigmoid")
    assert perm.tolist() == [[0, 1, 2, 3]] and counts.tolist() == [[4, 2]] and abs(loss - 1.0) < 1e-15
    assert np.allclose(grad.ravel(), -np.array([1, -1, -1, 1]) * R.coefficients([True, False, False, True], 4))

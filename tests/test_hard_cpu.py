"""CPU: the host side of the hard-pixel criterion (include/hard/lmnet_hard.h; lm_net_amd.loss.HardPixelLoss, hard_pixel_values):
registry and header agree, the argument checks of the three C entries (rejected before any
HIP call, with fake device pointers), the workspace formula, the classes' refusals, and the restatement tests/hard_ref.py: against
torch.topk over F.cross_entropy / F.binary_cross_entropy_with_logits in float64, float64 autograd, finite differences, tied inputs,
an explicit OHEM loop and the boundaries of the K formula.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hard_ref as R
from lm_net_amd import HardPixelLoss, hard_pixel_values, hip  # noqa: F401  (every test of this file belongs to the feature)

assert callable(hip.hard_fwd) and callable(hip.hard_bwd)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_ENTRIES = ["lmn_hard_fwd", "lmn_hard_bwd"]


# ---------------------------------------------------------------- ABI
def test_registry_and_header_agree():
    """The feature's own part of the registry: the literal list, its place in hip.HEADERS, the number of #defines, the header's
    citations and the package's exports.  (Header / export / layout / return-type / constants checks: tests/test_host_cpu.py.)"""
    assert hip.SYMBOLS_HARD == ["lmn_hard_workspace"] + DEVICE_ENTRIES
    assert hip.HEADERS["hard/lmnet_hard.h"] is hip.SYMBOLS_HARD
    header = open(os.path.join(ROOT, "include", "hard", "lmnet_hard.h")).read()
    assert "struct" not in header.replace("no struct", "")
    assert len(re.findall(r"^#define LMN_HARD_\w+ \d+\b", header, re.M)) == 9
    for cite in ("THE STORED VALUE IS CLAMPED TO >= +0", "order-preserving unsigned key", "A VOID ELEMENT STORES", "K = min(N, max(1, Kkeep, min_kept, Nhard))",
                 "floor((double)keep * N)", "(sum_{l > tau} l + (K - n_gt) * tau) / K", "(K - n_gt) / (n_eq * K)", "TIED ELEMENTS AT",
                 "A GROUP WITH N = 0 CONTRIBUTES 0", "never NaN", "GETS GRADIENT +0", "No float atomics", "BIT-IDENTICAL FROM CALL TO CALL",
                 "hard_workspace: ", "hard_fwd: ", "hard_bwd: "):
        assert cite in header, cite
    import lm_net_amd
    from lm_net_amd import loss
    for name in ("HardPixelLoss", "hard_pixel_values"):
        assert getattr(lm_net_amd, name) is getattr(loss, name) and name in lm_net_amd.__all__
    for words in ("Deliberate difference", "no longer a pure probability threshold", "DC_and_topk_loss", "at most 1024 images", "is not pinned"):
        assert words in HardPixelLoss.__doc__, words


# ---------------------------------------------------------------- argument checks of the C entries
FAKE = ctypes.c_void_p(0x1000)


def _hard(which, **kw):
    """lmn_hard_fwd / _bwd with fake device pointers: every case here must be rejected before any HIP call."""
    lib = hip.load()
    g = dict(logits=FAKE, target=FAKE, kind=0, head=0, per_image=0, keep=0.1, min_kept=0, cut=-1.0, scale=1.0, B=3, C=4, H=33, W=65, weight=None,
             workspace=FAKE, ws_bytes=1 << 40, values=FAKE, selection=FAKE, terms=FAKE, loss=FAKE, dlogits=FAKE)
    g.update(kw)
    if which == "fwd":
        rc = lib.lmn_hard_fwd(g["logits"], g["target"], g["kind"], g["head"], g["per_image"], g["keep"], g["min_kept"], g["cut"], g["scale"], g["B"],
                              g["C"], g["H"], g["W"], g["weight"], g["workspace"], g["ws_bytes"], g["values"], g["selection"], g["terms"], g["loss"], None)
    else:
        rc = lib.lmn_hard_bwd(g["logits"], g["target"], g["kind"], g["head"], g["per_image"], g["scale"], g["B"], g["C"], g["H"], g["W"], g["weight"],
                              g["values"], g["selection"], None, g["dlogits"], None)
    return rc, lib.lmn_last_error().decode()


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_loss_entries_reject_bad_arguments(which):
    pre = "hard_%s: " % which
    for name in (("logits", "target", "workspace", "values", "selection", "terms", "loss") if which == "fwd" else ("logits", "target", "values", "selection", "dlogits")):
        rc, err = _hard(which, **{name: None})
        assert rc == -1 and err == pre + "null pointer", (name, err)
    cases = [(dict(head=2), "unknown head 2"), (dict(head=-1), "unknown head -1"), (dict(per_image=2), "per_image=2 is neither 0 nor 1"),
             (dict(B=0), "B=0 not in [1, 65535]"), (dict(B=65536, C=2, H=1, W=1), "B=65536 not in"), (dict(C=65), "C=65 not in [1, 64]"), (dict(C=0), "C=0 not in"),
             (dict(C=1), "C=1 needs a sigmoid head"), (dict(H=0), "size 0x65 below 1"), (dict(W=-1), "size 33x-1"), (dict(kind=7), "unknown label kind 7"),
             (dict(B=600, C=4, H=1024, W=1024), "B * C * H * W = 2516582400 not below 2^31"),
             (dict(per_image=1, B=1025, C=2, H=4, W=4), "per_image: B=1025 groups above the limit 1024"),
             (dict(scale=float("inf")), "scale=inf is not finite"), (dict(scale=float("nan")), "is not finite")]
    if which == "fwd":
        cases += [(dict(keep=-0.1), "keep=-0.1 not in [0, 1]"), (dict(keep=1.5), "keep=1.5 not in"), (dict(keep=float("nan")), "not in [0, 1]"),
                  (dict(min_kept=-1), "min_kept=-1 is negative"), (dict(cut=float("inf")), "cut=inf is not finite"), (dict(cut=float("nan")), "is not finite"),
                  (dict(keep=0.0), "none of keep, min_kept and cut is given"), (dict(ws_bytes=100), "workspace of 100 bytes too small"),
                  (dict(workspace=ctypes.c_void_p(0x1004)), "the workspace is not 8-byte aligned")]
    for kw, msg in cases:
        rc, err = _hard(which, **kw)
        assert rc == -1 and msg in err and err.startswith(pre), (kw, err)
    if which == "fwd":                                     # the bounds themselves pass: the last size check, of the workspace, is reached
        for kw in (dict(head=1, B=1, C=1, H=1, W=1), dict(B=2, C=64, H=5, W=7, keep=0.0, min_kept=1 << 40), dict(per_image=1, B=1024, C=2, H=1, W=1, keep=1.0),
                   dict(B=65535, C=2, H=1, W=1, keep=0.0, cut=0.0)):
            need = hip.hard_workspace(kw.get("head", 0), kw.get("per_image", 0), kw["B"], kw["C"], kw["H"], kw["W"])
            rc, err = _hard(which, **dict(kw, ws_bytes=need - 1))
            assert rc == -1 and "workspace of %d bytes too small, %d needed" % (need - 1, need) in err, err


def test_workspace_is_host_arithmetic():
    up = lambda v: (v + 255) // 256 * 256
    cdiv = lambda a, b: (a + b - 1) // b
    for head, per_image, B, C, H, W in ((0, 0, 1, 2, 1, 1), (0, 0, 8, 2, 352, 352), (0, 1, 8, 9, 352, 352), (1, 0, 8, 9, 352, 352), (1, 1, 8, 9, 352, 352),
                                        (0, 1, 2, 3, 5, 7), (0, 1, 9, 3, 5, 7), (0, 1, 16, 3, 5, 7), (0, 1, 17, 2, 8, 8), (0, 1, 33, 2, 8, 8), (0, 1, 1024, 3, 40, 40), (1, 0, 2, 1, 5, 7), (1, 1, 2, 1, 7, 9), (1, 0, 1, 64, 8, 8)):
        G = B if per_image else 1
        M = (1 if per_image else B) * (C if head else 1) * H * W
        nbx = max(1, min(cdiv(M // 4 if M % 4 == 0 else M, 256), max(1, 1024 // G)))
        copies = 8 if G <= 8 else 4 if G <= 16 else 2 if G <= 32 else 1          # of the first histogram
        want = up(4 * G * ((copies + 1) * hip.HARD_BINS_HIGH + hip.HARD_BINS_LOW + 16)) + up(8 * G * nbx)
        assert hip.hard_workspace(head, per_image, B, C, H, W) == want, (head, per_image, B, C, H, W)
    for args, msg in (((0, 0, 0, 2, 8, 8), "B=0"), ((0, 0, 2, 1, 8, 8), "C=1 needs a sigmoid head"), ((2, 0, 2, 3, 8, 8), "unknown head"),
                      ((0, 0, 70000, 2, 1, 1), "B=70000"), ((0, 1, 1025, 2, 1, 1), "groups above the limit 1024"), ((1, 0, 600, 4, 1024, 1024), "not below 2^31")):
        with pytest.raises(ValueError, match="hard_workspace"):
            hip.hard_workspace(*args)
        assert msg in hip.load().lmn_last_error().decode()
    assert hip.hard_cut(None) == -1.0 and hip.hard_cut(1.0) == 0.0 and not np.signbit(hip.hard_cut(1.0))
    assert hip.hard_cut(0.7) == float(np.float32(-np.log(0.7))) == float(R.cut_of(0.7))


# ---------------------------------------------------------------- the classes refuse what they cannot run
def test_python_refuses_what_it_cannot_run():
    """In the words of the shared front end (_check_n_classes, _check_head, _check_scale, _check_pair, _check_elements) where the fault
    is the same."""
    z, y = torch.zeros(2, 3, 4, 4), torch.zeros(2, 4, 4, dtype=torch.uint8)
    for make, msg in ((lambda: HardPixelLoss(65, keep=0.1), r"n_classes = 65 outside \[1, 64\]"), (lambda: HardPixelLoss(1, keep=0.1), "a softmax head needs n_classes >= 2"),
                      (lambda: HardPixelLoss(3, head="tanh", keep=0.1), "expected 'softmax' or 'sigmoid'"), (lambda: HardPixelLoss(3), "one of keep, min_kept > 0 and thresh must be given"),
                      (lambda: HardPixelLoss(3, keep=0.0), r"keep = 0.0 outside \(0, 1\]"), (lambda: HardPixelLoss(3, keep=1.5), "keep = 1.5 outside"),
                      (lambda: HardPixelLoss(3, keep=float("nan")), "keep = nan outside"), (lambda: HardPixelLoss(3, min_kept=-1), "min_kept = -1 must be an integer >= 0"),
                      (lambda: HardPixelLoss(3, min_kept=2.5), "min_kept = 2.5 must be an integer"), (lambda: HardPixelLoss(3, thresh=0.0), r"thresh = 0.0 outside \(0, 1\]"),
                      (lambda: HardPixelLoss(3, thresh=1.2), "thresh = 1.2 outside"), (lambda: HardPixelLoss(3, keep=0.1, weight=[1, 2]), "weight needs 3 finite values >= 0"),
                      (lambda: HardPixelLoss(3, keep=0.1, weight=[1, 2, -1]), "finite values >= 0"), (lambda: HardPixelLoss(3, keep=0.1, weight=[1, 2, float("inf")]), "finite values >= 0"),
                      (lambda: hard_pixel_values(z, y, 3), "hard_pixel_values: one of keep, min_kept > 0 and thresh must be given"),
                      (lambda: hard_pixel_values(z, y, 0, keep=0.5), "n_classes = 0 outside")):
        with pytest.raises(ValueError, match=msg):
            make()
    assert HardPixelLoss(1, head="sigmoid", min_kept=5).n_classes == 1
    crit, img = HardPixelLoss(3, keep=0.1), HardPixelLoss(3, keep=0.1, per_image=True)
    bad = [(lambda: crit(torch.zeros(2, 4, 4, 4), y), r"logits must be floating point \[B, 3, H, W\]"), (lambda: crit(z.long(), y), "logits must be floating point"),
           (lambda: crit(z, y.float()), "target must be uint8, bool or int64"), (lambda: crit(z, y[:1]), "does not match logits .* under a softmax head"),
           (lambda: HardPixelLoss(3, head="sigmoid", keep=0.1)(z, y), "under a sigmoid head"),
           (lambda: crit(torch.zeros(65536, 3, 1, 1), torch.zeros(65536, 1, 1, dtype=torch.uint8)), "B = 65536 above the limit 65535"),
           (lambda: img(torch.zeros(1025, 3, 1, 1), torch.zeros(1025, 1, 1, dtype=torch.uint8)), "per_image: B = 1025 groups above the limit 1024"),
           (lambda: crit(torch.zeros(2, 3, 0, 4), y), r"outside the limit \[1, 2\^31\)"),
           (lambda: crit(torch.zeros(1, 3, 1, 1).expand(4, 3, 32768, 8192), y), r"B \* C \* H \* W = 3221225472 outside the limit"),
           (lambda: hard_pixel_values(z, y[:1], 3, keep=0.5), "hard_pixel_values: target .* does not match logits")]
    for call, msg in bad:
        with pytest.raises(ValueError, match=msg):
            call()
    crit.scale = float("inf")
    with pytest.raises(ValueError, match="HardPixelLoss: scale = inf is not finite"):
        crit(z, y)
    for call in (lambda: img(z, y), lambda: HardPixelLoss(3, head="sigmoid", thresh=0.7)(z, torch.zeros(2, 3, 4, 4, dtype=torch.int64)),
                 lambda: hard_pixel_values(z, y, 3, min_kept=4)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert "weight" in img.state_dict() or img.weight is None
    assert "_scratch" not in HardPixelLoss(3, keep=0.5, weight=[1, 2, 3]).state_dict() and list(HardPixelLoss(3, keep=0.5, weight=[1, 2, 3]).state_dict()) == ["weight"]


# ---------------------------------------------------------------- the restatement
CASES = [("softmax", (2, 5, 9, 11), dict(keep=0.1), True), ("softmax", (3, 2, 8, 8), dict(keep=0.37, per_image=True), False),
         ("softmax", (2, 4, 6, 10), dict(min_kept=17), True), ("softmax", (2, 3, 7, 9), dict(thresh=0.6, min_kept=5, per_image=True), True),
         ("sigmoid", (2, 3, 6, 10), dict(keep=0.2), True), ("sigmoid", (3, 1, 7, 9), dict(thresh=0.55, per_image=True), False),
         ("sigmoid", (2, 4, 5, 5), dict(keep=0.05, min_kept=9, thresh=0.4), True)]


def _weights(C, weighted):
    return [0.5 + 0.75 * k for k in range(C)] if weighted else None


def _torch_values(lg, y, head, weight):
    """(float64 per-element loss tensor with grad, valid mask) from torch's own reduction='none' losses"""
    z = torch.from_numpy(lg).double().requires_grad_(True)
    yt = torch.from_numpy(y.astype(np.int64))
    C = z.shape[1]
    w = None if weight is None else torch.tensor(weight, dtype=torch.float64)
    if head == "softmax":
        valid = (yt >= 0) & (yt < C)
        l = F.cross_entropy(z, torch.where(valid, yt, torch.zeros_like(yt)), weight=w, reduction="none")
    else:
        valid = (yt == 0) | (yt == 1)
        l = F.binary_cross_entropy_with_logits(z, torch.where(valid, yt, torch.zeros_like(yt)).double(), reduction="none")
        if w is not None:
            l = l * w[None, :, None, None]
    return z, l, valid


def _torch_loss(lg, y, head, weight, per_image, record, scale=1.0):
    """scale / G * sum_g torch.topk(l_g[valid], K_g).values.mean() with K from the restatement's record"""
    z, l, valid = _torch_values(lg, y, head, weight)
    G = lg.shape[0] if per_image else 1
    lg_, vg = l.reshape(G, -1), valid.reshape(G, -1)
    total = 0.0
    for g in range(G):
        K = int(record[g, 1])
        if K:
            total = total + torch.topk(lg_[g][vg[g]], K).values.mean()
    return z, scale * total / G


@pytest.mark.parametrize("head,shape,kw,weighted", CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_restatement_is_topk_of_torchs_losses(head, shape, kw, weighted):
    """The loss equals the mean of torch.topk over F.cross_entropy(reduction="none") (the BCE analogue likewise) to 1e-12, with
    weights and 20 % void, and the gradient float64 autograd to 1e-10 (random inputs: the cutoff is not tied)."""
    B, C, H, W = shape
    lg, y = R.inputs(B, C, H, W, head, seed=sum(shape), void=0.2)
    weight = _weights(C, weighted)
    r = R.loss_and_grad(lg, y, C, head=head, weight=weight, scale=0.7, gscale=1.0, **kw)
    assert (r.record[:, 3] == 1).all() and (r.record[:, 1] >= 1).all() and (r.record[:, 0] < lg[0, 0].size * B * C).all()
    z, loss = _torch_loss(lg, y, head, weight, kw.get("per_image", False), r.record, scale=0.7)
    assert abs(float(loss.detach()) - r.loss) <= 1e-12 * max(1.0, abs(r.loss)), (float(loss.detach()), r.loss)
    loss.backward()
    assert np.abs(z.grad.numpy() - r.grad).max() <= 1e-10
    G = r.record.shape[0]
    assert np.allclose(R.grouped(r.weights, kw.get("per_image", False)).sum(1), 1.0, atol=1e-12) and r.terms.shape == (G,)
    _, valid, _ = R.values(lg, y, head)
    assert not r.grad[np.broadcast_to(~valid[:, None] if head == "softmax" else ~valid, r.grad.shape)].any()


def test_gradient_is_the_finite_difference():
    for head, shape, kw, weighted in CASES[:2] + CASES[4:5]:
        B, C, H, W = shape
        lg, y = R.inputs(B, C, H, W, head, seed=5, void=0.2)
        weight = _weights(C, weighted)
        r = R.loss_and_grad(lg, y, C, head=head, weight=weight, **kw)
        rng = np.random.default_rng(1)
        d = rng.standard_normal(lg.shape)
        h = 1e-6
        f = lambda s: R.loss_and_grad(lg.astype(np.float64) + s * h * d, y, C, head=head, weight=weight, **kw).loss
        fd = (f(1.0) - f(-1.0)) / (2 * h)
        assert abs(fd - (r.grad * d).sum()) <= 1e-6 * max(1.0, abs(fd)), (head, fd, (r.grad * d).sum())


def test_ties_share_the_remaining_weight():
    """All-equal logits, and duplicated pixels that straddle the cutoff: the loss is still topk's mean, the gradient weights of a group
    sum to 1, tied elements carry equal weights, and nothing depends on an order among the ties."""
    B, C, H, W = 2, 3, 4, 6
    y = np.random.default_rng(0).integers(0, C, (B, H, W))
    y[0, 0, :2] = R.VOID
    lg = np.zeros((B, C, H, W), np.float32)
    for per_image in (False, True):
        r = R.loss_and_grad(lg, y, C, keep=0.3, per_image=per_image)
        N = r.record[:, 0]
        assert (r.record[:, 2] == 0).all() and (r.record[:, 3] == N).all() and np.allclose(r.terms, np.log(3.0), atol=1e-12)
        assert np.allclose(R.grouped(r.weights, per_image).sum(1), 1.0, atol=1e-12)
        valid = r.valid
        assert np.allclose(r.weights[valid], (1.0 / N)[np.nonzero(valid)[0]] if per_image else 1.0 / N[0], atol=1e-15)
    # duplicated pixels: 6 distinct pixel kinds, each 4 times; K = 10 cuts through the third kind
    rng = np.random.default_rng(3)
    kinds = rng.standard_normal((6, C)).astype(np.float32)
    lg = np.repeat(kinds, 4, axis=0).T.reshape(1, C, 4, 6).copy()
    y = np.zeros((1, 4, 6), np.int64)
    r = R.loss_and_grad(lg, y, C, min_kept=10)
    z, l, valid = _torch_values(lg, y, "softmax", None)
    want = torch.topk(l.flatten(), 10).values.mean()
    assert abs(float(want.detach()) - r.loss) <= 1e-12 and tuple(r.record[0]) == (24, 10, 8, 4)
    assert np.isclose(r.weights.sum(), 1.0, atol=1e-12) and sorted(set(np.round(r.weights.ravel(), 12))) == [0.0, 0.05, 0.1]
    perm = rng.permutation(24)                              # a permutation of the pixels permutes the gradient and nothing else
    lp = lg.reshape(C, 24)[:, perm].reshape(1, C, 4, 6)
    rp = R.loss_and_grad(lp, y, C, min_kept=10)
    assert rp.loss == pytest.approx(r.loss, abs=1e-15) and np.allclose(rp.grad.reshape(C, 24), r.grad.reshape(C, 24)[:, perm], atol=1e-15)


def test_ohem_form_is_the_explicit_loop():
    """thresh and min_kept with unit weights: keep every pixel whose true-class probability is below thresh, at least min_kept."""
    B, C, H, W = 2, 4, 9, 11
    lg, y = R.inputs(B, C, H, W, seed=9, void=0.2, scale=2.0)
    for thresh, min_kept in ((0.7, 0), (0.7, 60), (0.2, 150), (0.999, 3), (0.01, 0)):
        p_true = []
        for b in range(B):
            for i in range(H):
                for j in range(W):
                    if 0 <= y[b, i, j] < C:
                        z = lg[b, :, i, j].astype(np.float64)
                        p_true.append(np.exp(z[y[b, i, j]] - z.max()) / np.exp(z - z.max()).sum())
        p_true = np.sort(np.asarray(p_true))
        cut = np.float64(R.cut_of(thresh))
        n_keep = min(len(p_true), max(1, min_kept, int((-np.log(p_true) > cut).sum())))
        want = -np.log(p_true[:n_keep]).mean()
        r = R.loss_and_grad(lg, y, C, thresh=thresh, min_kept=min_kept)
        assert r.record[0, 1] == n_keep and abs(r.loss - want) <= 1e-12 * max(1.0, want), (thresh, min_kept, r.loss, want)


def test_count_formula_at_its_boundaries():
    f32 = lambda v: float(np.float32(v))
    assert R.count(0, keep=0.5, min_kept=3, nhard=0) == 0                   # N = 0
    assert R.count(10, min_kept=50) == 10 and R.count(10, keep=1.0) == 10   # min_kept > N; keep = 1
    assert R.count(10, keep=0.01) == 1 and R.count(10, nhard=4, keep=0.2, min_kept=3) == 4
    # keep rounded to fp32 just below / above a decimal: 0.1f > 0.1, 0.7f < 0.7
    assert f32(0.1) > 0.1 and R.count(10, keep=0.1) == 1 and R.count(10 ** 7, keep=0.1) == 10 ** 6 and R.count(10 ** 9, keep=0.1) == 100000001
    assert f32(0.7) < 0.7 and R.count(10, keep=0.7) == 6 and R.count(100, keep=0.7) == 69
    assert R.count(8, keep=0.5) == 4 and R.count(9, keep=0.5) == 4 and R.count(3, keep=0.25) == 1
    for N, keep in ((991232, 0.1), (123904, 0.05), (2 ** 31 - 1, 1.0), (2 ** 31 - 1, 0.3)):
        assert R.count(N, keep=keep) == int(np.floor(np.float64(np.float32(keep)) * N))
    lg, y = R.inputs(2, 3, 4, 5, seed=2, void=0.2)
    y[1] = R.VOID                                                            # an all-void image
    r = R.loss_and_grad(lg, y, 3, keep=0.5, per_image=True)
    assert tuple(r.record[1]) == (0, 0, 0, 0) and r.terms[1] == 0.0 and not r.grad[1].any() and np.isfinite(r.loss)
    rec = R.record_of(np.where(r.valid, r.values, -1).astype(np.float32), r.valid, True, keep=0.5)
    assert rec.shape == (2, R.WORDS) and not rec[1].any() and rec[0, 1] == r.record[0, 1]


# ---------------------------------------------------------------- the preconditions of the GPU tests
def test_busy_subjects_discriminate():
    import busy
    import hard_busy_cases as S
    subjects = S.subjects()
    assert sorted(subjects) == sorted(S.NAMES + [S.VALUES_NAME])
    for s in subjects.values():
        busy.check_discrimination(s)


def test_values_bar_is_at_most_1e_5():
    assert 0 < R.VALUES_BAR <= 1e-5

"""Restatements for the void-label loss and the per-image statistics (include/lmnet_loss.h), written from the formulas and checked
against the real reference classes where the reference tree exists (tests/test_void_cpu.py) and against
tests/golden/void_loss_stats.npz everywhere:

  * loss_terms: float64 torch, differentiable: cross entropy with class weights, label smoothing and void pixels; the reference's
    Dice loss with its `ignore` mask; a per-class sigmoid focal loss averaged over the valid pixels;
  * image_stats / score: numpy, exact integers / float64: tp, fp, fn, tn per image and class over the valid pixels and the metric
    reductions of the reference's utils/functional.py.

valid(i): 0 <= y_i < C.  ignore_index lies outside [0, C), so it needs no test of its own here.  The case builders below are shared
by the golden generator (tools/make_golden_void.py) and the tests: inputs are tools/detweights recipes, only keys are stored."""
import os
import sys
import types

import numpy as np
import torch

from tools.detweights import det_input, uniform

REFERENCE_ROOT = os.environ.get("LMNET_REFERENCE_ROOT", "/root/reference")


# ---------------------------------------------------------------------------------------------------------------- inputs
def labels(B, H, W, C, key):
    u = uniform(key, B * H * W)
    return torch.from_numpy(np.minimum((u * C).astype(np.int64), C - 1).reshape(B, H, W))


def with_void(y, key, void=255, frac=0.2):
    """y with `void` wherever uniform(key) < frac."""
    m = torch.from_numpy(uniform(key, y.numel()) < frac).reshape(y.shape)
    return torch.where(m, torch.full_like(y, void), y)


def weights(key, C):
    return torch.from_numpy(0.25 + 2 * uniform(key, C)).float()


def loss_case(tag):
    """The golden loss cases: (logits fp32 [B,C,H,W], labels, w_ce, w_dice, kwargs of loss_terms)."""
    C = {"k2": 2, "k9": 9, "f3": 3}[tag]
    B, H, W = 2, 37, 45
    lg = det_input((B, C, H, W), "void_loss/%s/lg" % tag) * 2.5
    y = labels(B, H, W, C, "void_loss/%s/y" % tag)
    if tag == "f3":                                   # the reference FocalLoss: no void labels, torchvision's defaults
        return lg, y, torch.ones(C), torch.ones(C), dict(ce_scale=0.0, dice_scale=0.0, focal_scale=1.0, gamma=2.0, alpha=0.25)
    y = with_void(y, "void_loss/%s/void" % tag)
    return lg, y, weights("void_loss/%s/wce" % tag, C), weights("void_loss/%s/wdice" % tag, C), dict(eps=1e-3, ignore_index=255)


STATS_C = (2, 4, 5, 64)


def stats_case(C):
    """The golden statistics cases: logits fp32 [3,C,37,45] and labels with 20 % void (255)."""
    B, H, W = 3, 37, 45
    lg = det_input((B, C, H, W), "void_stats/%d/lg" % C)
    y = with_void(labels(B, H, W, C, "void_stats/%d/y" % C), "void_stats/%d/void" % C)
    return lg, y


def stats_class_weights(C):
    return 0.5 + uniform("void_stats/cw", C)


# ---------------------------------------------------------------------------------------------------------------- loss
def loss_terms(lg, y, wce, wdice, eps=0.0, smooth=1e-5, ignore_index=None, ce_scale=1.0, dice_scale=1.0, focal_scale=0.0, gamma=2.0,
               alpha=0.25):
    """(total, ce, dice, focal) as float64 tensors of float64 logits [B,C,H,W]; empty sums give 0, not NaN."""
    B, C = lg.shape[:2]
    assert ignore_index is None or not 0 <= ignore_index < C
    z = lg.double().permute(0, 2, 3, 1).reshape(-1, C)
    yf = y.reshape(-1)
    valid = (yf >= 0) & (yf < C)
    z, t = z[valid], torch.nn.functional.one_hot(yf[valid], C).double()
    wce, wdice = wce.double(), torch.as_tensor(wdice).double()
    zero = lg.sum() * 0
    logp = torch.log_softmax(z, 1)
    p = logp.exp()
    s_w = (t * wce).sum()
    ce = zero
    if float(s_w) > 0:
        ce = ce_scale * ((1 - eps) * -(t * wce * logp).sum() + (eps / C) * -(wce * logp).sum()) / s_w
    i_c, z_c, y_c = (p * t).sum(0), (p * p).sum(0), t.sum(0)
    dice = dice_scale * (wdice * (1 - (2 * i_c + smooth) / (z_c + y_c + smooth))).sum() / C
    focal = zero
    if focal_scale and z.shape[0] > 0:
        s = z * (2 * t - 1)                                           # q_t = sigmoid(s)
        bce = -torch.nn.functional.logsigmoid(s)                      # -log q_t  (softplus would cut off at its threshold of 20)
        mod = torch.exp(gamma * torch.nn.functional.logsigmoid(-s))   # (1 - q_t)^gamma
        a_t = alpha * t + (1 - alpha) * (1 - t) if alpha >= 0 else 1.0
        focal = focal_scale * (a_t * mod * bce).sum() / z.shape[0]
    return ce + dice + focal, ce, dice, focal


def loss_and_grad(lg, y, wce, wdice, **kw):
    """-> ([total, ce, dice, focal] floats, d total / d logits float64)."""
    l64 = lg.detach().double().cpu().requires_grad_(True)
    terms = loss_terms(l64, y.cpu(), wce.cpu(), wdice.cpu() if torch.is_tensor(wdice) else wdice, **kw)
    terms[0].backward()
    return [float(v.detach()) for v in terms], l64.grad


# ---------------------------------------------------------------------------------------------------------------- statistics
def argmax_first(lg):
    """arg-max over dim 1, the first maximum wins (numpy's rule)."""
    return np.argmax(np.asarray(lg), axis=1)


def image_stats(pred, y, C):
    """int64 [B, C, 4] = tp, fp, fn, tn over the valid pixels; pred: integer label map, values outside [0, C) mean no class."""
    pred, y = np.asarray(pred).astype(np.int64), np.asarray(y).astype(np.int64)
    out = np.zeros((y.shape[0], C, 4), dtype=np.int64)
    for b in range(y.shape[0]):
        v = (y[b] >= 0) & (y[b] < C)
        pb, yb = pred[b][v], y[b][v]
        for c in range(C):
            tp = int(((pb == c) & (yb == c)).sum())
            fp, fn = int((pb == c).sum()) - tp, int((yb == c).sum()) - tp
            out[b, c] = tp, fp, fn, int(v.sum()) - tp - fp - fn
    return out


def _ratio(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(a, dtype=np.float64) / np.asarray(b, dtype=np.float64)


METRICS = {
    "f1": lambda tp, fp, fn, tn: _ratio(2 * tp, 2 * tp + fn + fp),
    "f2": lambda tp, fp, fn, tn: _ratio(5 * tp, 5 * tp + 4 * fn + fp),
    "iou": lambda tp, fp, fn, tn: _ratio(tp, tp + fp + fn),
    "accuracy": lambda tp, fp, fn, tn: _ratio(tp + tn, tp + fp + fn + tn),
    "precision": lambda tp, fp, fn, tn: _ratio(tp, tp + fp),
    "recall": lambda tp, fp, fn, tn: _ratio(tp, tp + fn),
    "sensitivity": lambda tp, fp, fn, tn: _ratio(tp, tp + fn),
    "specificity": lambda tp, fp, fn, tn: _ratio(tn, tn + fp),
    "balanced_accuracy": lambda tp, fp, fn, tn: (_ratio(tp, tp + fn) + _ratio(tn, tn + fp)) / 2,
    "npv": lambda tp, fp, fn, tn: _ratio(tn, tn + fn),
    "fnr": lambda tp, fp, fn, tn: _ratio(fn, fn + tp),
    "fpr": lambda tp, fp, fn, tn: _ratio(fp, fp + tn),
    "fdr": lambda tp, fp, fn, tn: 1 - _ratio(tp, tp + fp),
    "for": lambda tp, fp, fn, tn: 1 - _ratio(tn, tn + fn),
    "positive_likelihood_ratio": lambda tp, fp, fn, tn: _ratio(_ratio(tp, tp + fn), _ratio(fp, fp + tn)),
    "negative_likelihood_ratio": lambda tp, fp, fn, tn: _ratio(_ratio(fn, fn + tp), _ratio(tn, tn + fp)),
}
# name here -> (function of utils/functional.py, extra keyword arguments); (name of lm_net_amd.metrics, extra keyword arguments)
REFERENCE_NAMES = {"f1": ("f1_score", {}), "f2": ("fbeta_score", {"beta": 2.0}), "iou": ("iou_score", {}), "npv": ("negative_predictive_value", {}),
                   "fnr": ("false_negative_rate", {}), "fpr": ("false_positive_rate", {}), "fdr": ("false_discovery_rate", {}),
                   "for": ("false_omission_rate", {})}
PRODUCT_NAMES = {"f2": ("fbeta", {"beta": 2.0})}
REDUCTIONS = ("micro", "macro", "weighted", "micro-imagewise", "macro-imagewise", "weighted-imagewise", "none")


def score(stats, metric, reduction, class_weights=None, zero_division=1.0):
    """One metric under one reduction of stats [N, C, 4], float64.  The reference's rules: only 0/0 becomes zero_division ("micro"
    keeps it NaN); class weights are normalised to sum 1 and the weighted scores are then averaged over classes; "none" is the sum
    over images of the class-mean score."""
    s = np.asarray(stats, dtype=np.int64)
    f = METRICS[metric]

    def fixed(x):
        return np.where(np.isnan(x), zero_division, x)
    cw = 1.0 if class_weights is None else np.asarray(class_weights, dtype=np.float64) / np.sum(class_weights)
    if reduction == "micro":
        return float(f(*s.sum((0, 1))))
    if reduction in ("macro", "weighted"):
        return float(np.mean(fixed(f(*s.sum(0).T)) * cw))
    if reduction == "micro-imagewise":
        return float(np.mean(fixed(f(*s.sum(1).T))))
    per = fixed(f(s[..., 0], s[..., 1], s[..., 2], s[..., 3]))
    if reduction in ("macro-imagewise", "weighted-imagewise"):
        return float(np.mean(per.mean(0) * cw))
    assert reduction == "none", reduction
    return float(per.mean(1).sum())


# ---------------------------------------------------------------------------------------------------------------- the reference
def reference_available():
    return os.path.isfile(os.path.join(REFERENCE_ROOT, "utils", "loss.py"))


def sigmoid_focal_loss(inputs, targets, alpha=0.25, gamma=2.0, reduction="none"):
    """torchvision.ops.sigmoid_focal_loss restated from its documented formula (torchvision is not installed where the goldens are
    made; parity with torchvision's own code is not pinned): BCE-with-logits times (1 - p_t)^gamma, times alpha_t when alpha >= 0."""
    p = torch.sigmoid(inputs)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
    p_t = p * targets + (1 - p) * (1 - targets)
    loss = ce * (1 - p_t) ** gamma
    if alpha >= 0:
        loss = (alpha * targets + (1 - alpha) * (1 - targets)) * loss
    return loss.mean() if reduction == "mean" else loss.sum() if reduction == "sum" else loss


def reference_modules():
    """(utils.loss, utils.functional) of the reference tree, with the third-party import it cannot satisfy here stubbed."""
    added = [n for n in ("torchvision", "torchvision.ops", "torchvision.ops.focal_loss") if n not in sys.modules]
    for name in added:
        sys.modules[name] = types.ModuleType(name)
    if "torchvision.ops.focal_loss" in added:
        sys.modules["torchvision.ops.focal_loss"].sigmoid_focal_loss = sigmoid_focal_loss
    sys.path.insert(0, REFERENCE_ROOT)
    try:
        import utils.functional as ref_functional
        import utils.loss as ref_loss
    finally:                                          # (leave no stub or path behind for the other tests of the session)
        sys.path.remove(REFERENCE_ROOT)
        for name in added:
            del sys.modules[name]
    return ref_loss, ref_functional


def reference_loss(ref_loss, lg, y, wce, wdice, eps, ignore_index):
    """F.cross_entropy(..., ignore_index) + the real DiceLoss(..., ignore=...) on float64 logits."""
    C = lg.shape[1]
    ii = -100 if ignore_index is None else ignore_index
    ce = torch.nn.functional.cross_entropy(lg, y, weight=wce.double(), label_smoothing=eps, ignore_index=ii)
    ignore = (y == ii) if ignore_index is not None else None
    if ignore is None:
        ignore = torch.zeros_like(y, dtype=torch.bool)
    dice = ref_loss.DiceLoss(C)(lg, y.unsqueeze(1).float(), weight=[float(v) for v in wdice], ignore=ignore)
    return ce + dice

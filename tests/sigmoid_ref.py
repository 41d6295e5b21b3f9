"""Restatements for the sigmoid-head loss and statistics (include/lmnet_sigmoid.h), written from the formulas and checked against the
real reference code where the reference tree exists (tests/test_sigmoid_cpu.py) and against tests/golden/sigmoid_loss_stats.npz
everywhere:

  * loss_terms: float64 torch, differentiable: per-class binary cross entropy with class weights and pos_weight, the reference's Dice
    loss on sigmoid probabilities with a per-class `ignore` mask, a per-class sigmoid focal loss, each over the valid elements;
  * stats / labels: numpy, exact: the fp32 compare `z >= logit_threshold` and tp, fp, fn, tn per (image, class) plane over the valid
    elements.  The metric reductions are tests/void_ref.py's (score, METRICS, REDUCTIONS), not restated here.

valid(b, c, i): the target is 0 or 1.  The case builders below are shared by the golden generator (tools/make_golden_sigmoid.py) and
the tests: inputs are tools/detweights recipes, only keys are stored."""
import numpy as np
import torch

from tools.detweights import det_input, uniform
from void_ref import METRICS, PRODUCT_NAMES, REDUCTIONS, REFERENCE_NAMES, reference_available, reference_modules, score  # noqa: F401

VOID = 255


# ---------------------------------------------------------------------------------------------------------------- inputs
def logits(shape, key):
    return det_input(shape, key) * 2.5


def targets(shape, key, void_key=None, void=VOID, frac=0.2, dtype=torch.int64):
    """1 where uniform(key) < 0.3, else 0; `void` wherever a second uniform(void_key) < frac.  Classes are independent: planes overlap."""
    n = int(np.prod(shape))
    t = torch.from_numpy((uniform(key, n) < 0.3).astype(np.int64)).reshape(shape)
    if void_key is not None:
        m = torch.from_numpy(uniform(void_key, n) < frac).reshape(shape)
        t = torch.where(m, torch.full_like(t, void), t)
    return t.to(dtype)          # (uint8: -100 would wrap, the callers pass 255 there)


def weights(key, C):
    return torch.from_numpy(0.25 + 2 * uniform(key, C)).float()


def logit_threshold(thr):
    """log(thr / (1 - thr)) in float64, rounded to fp32 (exactly 0 at 0.5)."""
    return np.float32(np.log(np.float64(thr) / (1.0 - np.float64(thr))))


LOSS_TAGS = {"b1": 1, "m3": 3, "f5": 5}


def loss_case(tag):
    """The golden loss cases: (logits fp32 [B,C,H,W], target int64, w_bce, pos_weight, w_dice, kwargs of loss_terms)."""
    C = LOSS_TAGS[tag]
    shape = (2, C, 37, 45)
    lg = logits(shape, "sig_loss/%s/lg" % tag)
    t = targets(shape, "sig_loss/%s/t" % tag, "sig_loss/%s/void" % tag)
    if tag == "b1":                                   # the binary head as a user trains it: BCE + Dice, a positive weight
        return lg, t, torch.ones(C), torch.tensor([4.0]), torch.ones(C), {}
    w = [weights("sig_loss/%s/%s" % (tag, n), C) for n in ("wbce", "pw", "wdice")]
    if tag == "m3":
        return lg, t, w[0], w[1], w[2], {}
    return lg, t, w[0], w[1], w[2], dict(bce_scale=0.7, dice_scale=1.3, focal_scale=0.5, gamma=1.5, alpha=0.25)


STATS_C = (1, 2, 5, 64)
STATS_THR = (0.5, 0.3)


def stats_case(C, void=True):
    """The statistics cases: logits fp32 [3,C,37,45] and int64 targets, with 20 % void (255) or none."""
    shape = (3, C, 37, 45)
    lg = logits(shape, "sig_stats/%d/lg" % C)
    t = targets(shape, "sig_stats/%d/t" % C, "sig_stats/%d/void" % C if void else None)
    return lg, t


def stats_class_weights(C):
    return 0.5 + uniform("sig_stats/cw", C)


# ---------------------------------------------------------------------------------------------------------------- loss
def loss_terms(lg, t, w_bce=None, pos_weight=None, w_dice=None, smooth=1e-5, bce_scale=1.0, dice_scale=1.0, focal_scale=0.0, gamma=2.0,
               alpha=0.25):
    """(total, bce, dice, focal) as float64 tensors of logits [B,C,...] and an integer target of the same size ([B,...] when C = 1);
    empty sums give 0, not NaN."""
    B, C = lg.shape[:2]
    z = lg.double().reshape(B, C, -1)
    ti = t.reshape(B, C, -1).long()
    valid = ((ti == 0) | (ti == 1)).double()
    tt = (ti == 1).double()
    ones = torch.ones(C, dtype=torch.float64)
    w_bce = ones if w_bce is None else torch.as_tensor(w_bce).double()
    pos_weight = ones if pos_weight is None else torch.as_tensor(pos_weight).double()
    w_dice = ones if w_dice is None else torch.as_tensor(w_dice).double()
    sp_pos = -torch.nn.functional.logsigmoid(-z)                      # softplus(z)  = -log(1 - p)   (no threshold cut-off)
    sp_neg = -torch.nn.functional.logsigmoid(z)                       # softplus(-z) = -log p
    p = torch.sigmoid(z)
    n_c = valid.sum((0, 2))
    n = n_c.sum()
    zero = z.sum() * 0
    bce = zero
    if bce_scale and float(n) > 0:
        elem = pos_weight.view(1, C, 1) * tt * sp_neg + (1 - tt) * sp_pos
        bce = bce_scale * (w_bce * (elem * valid).sum((0, 2))).sum() / n
    i_c, z_c, y_c = (p * tt * valid).sum((0, 2)), (p * p * valid).sum((0, 2)), (tt * valid).sum((0, 2))
    dice = zero
    if dice_scale:
        dice = dice_scale * (w_dice * (1 - (2 * i_c + smooth) / (z_c + y_c + smooth))).sum() / C
    focal = zero
    if focal_scale:
        s = z * (2 * tt - 1)                                          # q_t = sigmoid(s)
        ce = -torch.nn.functional.logsigmoid(s)
        mod = torch.exp(gamma * torch.nn.functional.logsigmoid(-s))   # (1 - q_t)^gamma
        a_t = alpha * tt + (1 - alpha) * (1 - tt) if alpha >= 0 else 1.0
        per_class = (a_t * mod * ce * valid).sum((0, 2))
        focal = focal_scale * torch.where(n_c > 0, per_class / n_c.clamp_min(1), torch.zeros_like(n_c)).sum()
    return bce + dice + focal, bce, dice, focal


def loss_and_grad(lg, t, w_bce=None, pos_weight=None, w_dice=None, **kw):
    """-> ([total, bce, dice, focal] floats, d total / d logits float64)."""
    l64 = lg.detach().double().cpu().requires_grad_(True)
    terms = loss_terms(l64, t.cpu(), *(None if w is None else w.cpu() for w in (w_bce, pos_weight, w_dice)), **kw)
    terms[0].backward()
    return [float(v.detach()) for v in terms], l64.grad


def grad_digest(grad):
    """[sum, sum of |.|, sum of squares, max |.|] of a gradient: the golden's check of the whole tensor."""
    g = np.asarray(grad, dtype=np.float64).ravel()
    return np.array([g.sum(), np.abs(g).sum(), (g * g).sum(), np.abs(g).max()])


def grad_sample(grad, step=97):
    return np.asarray(grad, dtype=np.float64).ravel()[::step].copy()


# ---------------------------------------------------------------------------------------------------------------- statistics
def labels(lg, thr=0.5):
    """uint8, the logits' shape: 1 where z >= logit_threshold(thr), compared in fp32."""
    z = np.asarray(lg, dtype=np.float32)
    return (z >= logit_threshold(thr)).astype(np.uint8)


def stats(lg, t, thr=0.5):
    """int64 [B, C, 4] = tp, fp, fn, tn over the valid elements of each plane."""
    z = np.asarray(lg)
    B, C = z.shape[:2]
    pred = labels(z, thr).reshape(B, C, -1).astype(bool)
    ti = np.asarray(t).reshape(B, C, -1).astype(np.int64)
    valid, lab = (ti == 0) | (ti == 1), ti == 1
    tp = (pred & lab).sum(2)
    fp = (pred & valid).sum(2) - tp
    fn = lab.sum(2) - tp
    tn = valid.sum(2) - tp - fp - fn
    return np.stack([tp, fp, fn, tn], -1).astype(np.int64)

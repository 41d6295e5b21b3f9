"""tests/golden/sigmoid_loss_stats.npz from the REAL reference code (build container only, where the reference tree exists), float64:

  * the loss cases of tests/sigmoid_ref.py::loss_case ("b1": one logit, pos_weight 4; "m3": three overlapping planes, all weight
    vectors drawn; "f5": five planes, all three terms on with unequal scales), each with 20 % void elements, composed from
      - F.binary_cross_entropy_with_logits(weight, pos_weight, reduction="sum") over the valid elements, divided by their count,
      - utils/loss.py::DiceLoss._dice_loss(sigmoid(z[:, c]), t[:, c], ignore_c) per class, weighted and averaged as DiceLoss.forward,
      - the per-class mean of sigmoid_focal_loss over the class's valid elements, summed as utils/loss.py::FocalLoss.forward does
        (torchvision is not installed here: tests/void_ref.py::sigmoid_focal_loss stands in, written from its documented formula);
    stored: the four terms, a digest [sum, sum |.|, sum of squares, max |.|] and every 97th element of d total / d logits;
  * utils/functional.py::get_stats(mode="multilabel", or "binary" at C = 1, threshold) on sigmoid(logits) at C in {1, 2, 5, 64} and
    thr in {0.5, 0.3}, without void elements and with 20 % of them (get_stats has no void: prediction and target are zeroed there and
    the void count is taken off tn), and every metric function of that file under every reduction on float64 copies of the statistics.

Inputs are tools/detweights recipes built by tests/sigmoid_ref.py, so only the expected numbers are stored."""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sigmoid_ref as S  # noqa: E402
import void_ref as V  # noqa: E402


def reference_loss(ref_loss, z, t, w_bce, pos_weight, w_dice, bce_scale=1.0, dice_scale=1.0, focal_scale=0.0, gamma=2.0, alpha=0.25):
    B, C = z.shape[:2]
    valid = (t == 0) | (t == 1)
    tt = (t == 1).double()
    shape = (1, C) + (1,) * (z.dim() - 2)
    elem = torch.nn.functional.binary_cross_entropy_with_logits(z, tt, weight=w_bce.double().view(shape).expand_as(z),
                                                                pos_weight=pos_weight.double().view(shape), reduction="none")
    bce = bce_scale * elem[valid].sum() / valid.sum()
    dice_mod = ref_loss.DiceLoss(C)
    dice = sum(dice_mod._dice_loss(torch.sigmoid(z[:, c]), tt[:, c], (~valid[:, c]).long()) * float(w_dice[c]) for c in range(C)) / C
    focal = z.sum() * 0
    if focal_scale:
        focal = focal_scale * sum(V.sigmoid_focal_loss(z[:, c][valid[:, c]], tt[:, c][valid[:, c]], alpha=alpha, gamma=gamma, reduction="mean")
                                  for c in range(C))
    dice = dice_scale * dice
    return bce + dice + focal, bce, dice, focal


def reference_stats(ref_fn, lg, t, thr):
    C = lg.shape[1]
    valid = (t == 0) | (t == 1)
    prob = torch.sigmoid(lg) * valid                  # (thr > 0: a zeroed element is predicted off)
    tp, fp, fn, tn = ref_fn.get_stats(prob, torch.where(valid, t, torch.zeros_like(t)), mode="binary" if C == 1 else "multilabel",
                                      threshold=thr)
    tn = tn - (~valid).flatten(2).sum(2)
    return torch.stack([tp, fp, fn, tn], -1)


def main():
    ref_loss, ref_fn = V.reference_modules()
    out = {}
    for tag in S.LOSS_TAGS:
        lg, t, w_bce, pw, w_dice, kw = S.loss_case(tag)
        l64 = lg.double().requires_grad_(True)
        terms = reference_loss(ref_loss, l64, t, w_bce, pw, w_dice, **kw)
        terms[0].backward()
        out["%s/loss4" % tag] = np.array([float(v.detach()) for v in terms])
        out["%s/grad_digest" % tag] = S.grad_digest(l64.grad.numpy())
        out["%s/grad_sample" % tag] = S.grad_sample(l64.grad.numpy())
    for C in S.STATS_C:
        cw = S.stats_class_weights(C)
        for void in (False, True):
            lg, t = S.stats_case(C, void)
            for thr in S.STATS_THR:
                key = "%d/%s/%g" % (C, "void" if void else "full", thr)
                st = reference_stats(ref_fn, lg, t, thr)
                out["stats/" + key] = st.numpy().astype(np.int64)
                tp, fp, fn, tn = (st[..., i].double() for i in range(4))
                vals = []
                for m in V.METRICS:
                    name, kw = V.REFERENCE_NAMES.get(m, (m, {}))
                    for r in V.REDUCTIONS:
                        with warnings.catch_warnings():
                            warnings.simplefilter("ignore")
                            v = getattr(ref_fn, name)(tp, fp, fn, tn, reduction=r, class_weights=cw if "weighted" in r else None, **kw)
                        vals.append(float(v))
                out["s64/" + key] = np.array(vals, dtype=np.float64).reshape(len(V.METRICS), len(V.REDUCTIONS))
    path = os.path.join(ROOT, "tests", "golden", "sigmoid_loss_stats.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), {k: v.tolist() for k, v in out.items() if v.size <= 4})


if __name__ == "__main__":
    main()

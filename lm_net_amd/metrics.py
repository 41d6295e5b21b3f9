"""On-device segmentation metrics.

The reference moves every batch to the CPU and updates a torchmetrics collection (``utils/train_eval_utils.py:150-156``,
``train.py:165-174``).  ``ConfusionMeter`` keeps the confusion matrix of ``argmax(logits, 1)`` against the labels on the
GPU (one kernel per batch, no sync) and derives Dice ``2TP/(2TP+FP+FN)`` and IoU ``TP/(TP+FP+FN)`` per class
(``train_eval_utils.py:78-95``) when ``compute()`` is called, plus the reference ``Evaluator``'s other metrics
(``train_eval_utils.py:55-118``) under its method names.  Any class count 2..64 (labels outside [0, C) are not counted).
"""
import numpy as np
import torch

from . import hip


class ConfusionMeter:
    def __init__(self, n_classes=2, device="cuda"):
        if not 2 <= n_classes <= 64:
            raise ValueError("ConfusionMeter: n_classes = %d outside [2, 64]" % n_classes)
        self.n = n_classes
        self.total = torch.zeros(n_classes, n_classes, device=device, dtype=torch.float64)

    def reset(self):
        self.total.zero_()

    @torch.no_grad()
    def update(self, logits, target):
        if not logits.is_cuda:
            raise RuntimeError("lm_net_amd.ConfusionMeter: device tensors required (the HIP path has no CPU fallback)")
        counts = torch.zeros(self.n, self.n, device=logits.device)      # exact: < 2^24 per cell and launch
        hip.confusion(logits.contiguous().float(), target.contiguous().long(), counts)
        self.total += counts.double()

    def compute(self):
        """{'dice': [per class], 'iou': [per class], 'accuracy': float, 'confusion': [[...]]} -- rows = label -- and the
        Evaluator metrics of evaluator_metrics() (Mean_Dice, Mean_Intersection_over_Union, ...)."""
        m = self.total.cpu()
        tp = m.diag()
        fp, fn = m.sum(0) - tp, m.sum(1) - tp
        dice = (2 * tp / (2 * tp + fp + fn).clamp_min(1)).tolist()
        iou = (tp / (tp + fp + fn).clamp_min(1)).tolist()
        out = dict(dice=dice, iou=iou, accuracy=float(tp.sum() / m.sum().clamp_min(1)), confusion=m.long().tolist())
        out.update(evaluator_metrics(m.numpy()))
        return out


def evaluator_metrics(cm):
    """The reference Evaluator's metrics of a confusion matrix (rows = label), with its formulas and NaN handling (np.nanmean over
    classes; a 0/0 of a scalar metric is NaN).  Recall, Precision, Specificity are those of class 1 against class 0, as there."""
    cm = np.asarray(cm, dtype=np.float64)
    d, rows, cols, tot = np.diag(cm), cm.sum(1), cm.sum(0), cm.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        iu = d / (rows + cols - d)
        freq = rows / tot
        out = {"Mean_Accuracy": np.nanmean(d / tot),
               "Mean_Recall": np.nanmean(d / rows),
               "Precision": cm[1][1] / (cm[1][1] + cm[0][1]),
               "Recall": cm[1][1] / (cm[1][1] + cm[1][0]),
               "Specificity": cm[0][0] / (cm[0][0] + cm[0][1]),
               "Mean_Dice": np.nanmean(2 * d / (rows + cols)),
               "Mean_Intersection_over_Union": np.nanmean(iu),
               "Frequency_Weighted_Intersection_over_Union": (freq[freq > 0] * iu[freq > 0]).sum()}
    return {k: float(v) for k, v in out.items()}

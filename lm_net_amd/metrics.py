"""On-device segmentation metrics.

The reference moves every batch to the CPU and updates a torchmetrics collection (``utils/train_eval_utils.py:150-156``,
``train.py:165-174``).  ``ConfusionMeter`` keeps the confusion matrix of ``argmax(logits, 1)`` against the labels on the
GPU (one kernel per batch, no sync) and derives Dice ``2TP/(2TP+FP+FN)`` and IoU ``TP/(TP+FP+FN)`` per class
(``train_eval_utils.py:78-95``) when ``compute()`` is called, plus the reference ``Evaluator``'s other metrics
(``train_eval_utils.py:55-118``) under its method names.  Any class count 2..64 (labels outside [0, C) are not counted).

``SurfaceDistanceMeter`` adds the boundary metrics that go with them in a results table -- HD, HD95, ASSD and RVD in the
``medpy.metric.binary`` conventions -- which the reference's ``evaluate()`` prepares for (``train_eval_utils.py:7`` imports
``hausdorff_distance``, ``:178-179`` set up ``hausdorff_distance_list`` / ``rvd_list``, ``:14-52`` ``ravd`` / ``RVDEvaluator``) and
never computes.  The device produces ten exact raw statistics per (sample, class) pair (``lmn_surface_dist``); ``compute()`` turns
them into the metrics in float64 on the host.

``ImageStatsMeter`` keeps tp / fp / fn / tn per IMAGE and class (``get_stats`` of ``utils/functional.py:61-201`` in mode
"multiclass", with ``ignore_index``) and scores them with the metric set and the reductions of that file (``:237-358``), among them
the ``*-imagewise`` ones; ``per_image`` gives the per-case scores behind a "mean +/- std over cases" column, which a pooled
confusion matrix cannot.

``CurveMeter`` sweeps the threshold the other meters fix: per (image, class) histograms of the scores of positives and negatives over
a threshold table (``lmn_curve_hist``, integer counting on the device), from which ROC, precision-recall, AUROC (the ``AUROC`` of the
reference's torchmetrics collection, ``train.py:29``), average precision and the best threshold of any thresholded metric follow in
float64 on the host.

``VolumeSurfaceMeter`` scores a whole 3D case: Dice, Jaccard, HD, HD95, ASSD and RVD of the ``[D, H, W]`` label volume with integer
voxel pitches (``medpy.metric.binary`` ``dc`` / ``jc`` / ``hd`` / ``hd95`` / ``assd`` / ``ravd`` per case), from the eleven exact raw
statistics per (case, class) of ``lmn_volume_dist``; slices arrive batch by batch from a 2D validation loop (``push`` / ``close_case``).

``LesionMeter`` scores a case per LESION: the 3D components of prediction and target (``lmn_cc3d_label``) and the join between them, a
device hash table of component pairs with their shared voxel counts (``lmn_lesion_match``); detection by overlap, lesion-wise F1,
panoptic quality and a lesion-wise Dice follow from those integers in float64 on the host (``lesion_metrics``).
"""
import warnings

import numpy as np
import torch

from . import hip


def _prediction(pred, n_classes, what, label_dtype):
    """The one input contract of the meters' predictions (pure: no device check).  Floating-point logits [B, C, H, W] with
    C = n_classes come back contiguous fp32; an integer or bool label map [B, H, W] comes back contiguous as ``label_dtype``:
    torch.uint8 (-1 and everything >= 255 become 255, "no class") or torch.int64."""
    if pred.dim() == 4 and pred.is_floating_point():
        if pred.shape[1] != n_classes:
            raise ValueError("%s: logits with %d channels, n_classes = %d" % (what, pred.shape[1], n_classes))
        return pred.contiguous().float()
    if pred.dim() != 3 or pred.is_floating_point():
        raise ValueError("%s: pred must be logits [B, C, H, W] or an INTEGER label map [B, H, W], got a %d-D %s tensor"
                         % (what, pred.dim(), pred.dtype))
    if label_dtype == torch.int64:
        return pred.contiguous().long()
    if pred.dtype not in (torch.uint8, torch.bool):
        pred = pred.clamp(-1, 255)                               # (-1 -> 255: no class)
    return pred.to(torch.uint8).contiguous()


def _target(target, pred, what):
    """The labels of a prediction as _prediction returns it: contiguous int64 [B, H, W] of the prediction's batch and image size."""
    target = target.contiguous().long()
    if target.dim() != 3 or target.shape[0] != pred.shape[0] or target.shape[-2:] != pred.shape[-2:]:
        raise ValueError("%s: target %s does not match pred %s" % (what, tuple(target.shape), tuple(pred.shape)))
    return target


CONFUSION_MAX_PIXELS = (1 << 24) - 1    # lmn_confusion / lmn_confusion_labels count in float cells and refuse B * HW >= 2^24 per call


def _confusion_calls(pred, target, limit=CONFUSION_MAX_PIXELS):
    """(pred, target) pieces of at most ``limit`` pixels each that together cover every pixel once (pure: no device check): whole images
    while one image fits, else contiguous pixel ranges of one image ([1, C, 1, n] logits -- a copy of the slice -- or a [1, 1, n] map)."""
    B, hw = int(target.shape[0]), int(target.shape[1] * target.shape[2])
    if B * hw <= limit:
        yield pred, target
    elif hw <= limit:
        nb = limit // hw
        for b in range(0, B, nb):
            yield pred[b:b + nb], target[b:b + nb]
    else:
        for b in range(B):                                           # (pieces keep the rank the entries' wrappers go by)
            p = pred[b:b + 1].reshape(1, -1, 1, hw) if pred.dim() == 4 else pred[b:b + 1].reshape(1, 1, hw)
            t = target[b:b + 1].reshape(1, 1, hw)
            for i in range(0, hw, limit):
                yield p[..., i:i + limit].contiguous(), t[..., i:i + limit]


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
        """logits [B, C, H, W] (arg-max, first maximum wins) or an integer label map [B, H, W] (e.g. DevicePostprocess's labels_net;
        predictions outside [0, C) are not counted)."""
        if not logits.is_cuda:
            raise RuntimeError("lm_net_amd.ConfusionMeter: device tensors required (the HIP path has no CPU fallback)")
        pred = _prediction(logits, self.n, "ConfusionMeter", torch.uint8)
        target = _target(target, pred, "ConfusionMeter")
        for p, t in _confusion_calls(pred, target):
            counts = torch.zeros(self.n, self.n, device=pred.device)    # float cells, exact: every call sees < 2^24 pixels
            (hip.confusion if p.dim() == 4 else hip.confusion_labels)(p, t, counts)
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


def _m_fbeta(tp, fp, fn, tn, beta=1.0):
    return (1 + beta ** 2) * tp / ((1 + beta ** 2) * tp + beta ** 2 * fn + fp)


def _m_sens(tp, fp, fn, tn):
    return tp / (tp + fn)


def _m_spec(tp, fp, fn, tn):
    return tn / (tn + fp)


def _m_fnr(tp, fp, fn, tn):
    return fn / (fn + tp)


def _m_fpr(tp, fp, fn, tn):
    return fp / (fp + tn)


# the metric functions of utils/functional.py:302-358 under its public names (and the short forms of a results table)
STATS_METRICS = {
    "fbeta": _m_fbeta, "f1": _m_fbeta, "iou": lambda tp, fp, fn, tn: tp / (tp + fp + fn),
    "accuracy": lambda tp, fp, fn, tn: (tp + tn) / (tp + fp + fn + tn),
    "precision": lambda tp, fp, fn, tn: tp / (tp + fp), "recall": _m_sens, "sensitivity": _m_sens, "specificity": _m_spec,
    "balanced_accuracy": lambda tp, fp, fn, tn: (_m_sens(tp, fp, fn, tn) + _m_spec(tp, fp, fn, tn)) / 2,
    "npv": lambda tp, fp, fn, tn: tn / (tn + fn), "fnr": _m_fnr, "fpr": _m_fpr,
    "fdr": lambda tp, fp, fn, tn: 1 - tp / (tp + fp), "for": lambda tp, fp, fn, tn: 1 - tn / (tn + fn),
    "positive_likelihood_ratio": lambda tp, fp, fn, tn: _m_sens(tp, fp, fn, tn) / _m_fpr(tp, fp, fn, tn),
    "negative_likelihood_ratio": lambda tp, fp, fn, tn: _m_fnr(tp, fp, fn, tn) / _m_spec(tp, fp, fn, tn),
}
_ALIASES = {"f1_score": "f1", "fbeta_score": "fbeta", "iou_score": "iou", "positive_predictive_value": "precision",
            "negative_predictive_value": "npv", "false_negative_rate": "fnr", "false_positive_rate": "fpr",
            "false_discovery_rate": "fdr", "false_omission_rate": "for"}
STATS_REDUCTIONS = ("micro", "macro", "weighted", "micro-imagewise", "macro-imagewise", "weighted-imagewise", "none")


def _metric_fn(metric, beta):
    name = _ALIASES.get(metric, metric)
    if name not in STATS_METRICS:
        raise ValueError("unknown metric %r (known: %s)" % (metric, ", ".join(sorted(STATS_METRICS))))
    fn = STATS_METRICS[name]
    return (lambda *a: fn(*a, beta=float(beta))) if name == "fbeta" else fn


def _zero_div(x, zero_division):
    nans = np.isnan(x)
    if nans.any() and zero_division == "warn":
        warnings.warn("Zero division in metric calculation!")
    return np.where(nans, 0.0 if zero_division == "warn" else float(zero_division), x)


def stats_score(tp, fp, fn, tn, metric, reduction="micro", class_weights=None, zero_division=1.0, beta=1.0):
    """One metric of per-image statistics ([N, C] each) under one reduction, in float64: ``_compute_metric`` of
    ``utils/functional.py:237-296`` as it stands there -- "micro" leaves a 0/0 as NaN, the class weights are normalised to sum 1 and
    the weighted class scores are then AVERAGED (so "weighted" is 1/C of a weighted mean), and "none" returns the sum over images of
    the class-mean score.  Only a 0/0 is replaced by ``zero_division``; x/0 stays inf."""
    fnc = _metric_fn(metric, beta)
    tp, fp, fn, tn = (np.asarray(a, dtype=np.float64) for a in (tp, fp, fn, tn))
    if reduction not in STATS_REDUCTIONS and reduction is not None:
        raise ValueError("reduction %r not in %s" % (reduction, STATS_REDUCTIONS))
    if class_weights is None and reduction is not None and "weighted" in reduction:
        raise ValueError("Class weights should be provided for `%s` reduction" % reduction)
    cw = np.asarray(1.0 if class_weights is None else class_weights, dtype=np.float64)
    cw = cw / cw.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        if reduction == "micro":
            return float(fnc(tp.sum(), fp.sum(), fn.sum(), tn.sum()))
        if reduction in ("macro", "weighted"):
            return float((_zero_div(fnc(tp.sum(0), fp.sum(0), fn.sum(0), tn.sum(0)), zero_division) * cw).mean())
        if reduction == "micro-imagewise":
            return float(_zero_div(fnc(tp.sum(1), fp.sum(1), fn.sum(1), tn.sum(1)), zero_division).mean())
        score = _zero_div(fnc(tp, fp, fn, tn), zero_division)
        if reduction in ("macro-imagewise", "weighted-imagewise"):
            return float((score.mean(0) * cw).mean())
        return float(score.mean(1).sum())


class _RawStatsMeter:
    """What the statistics meters share: a list of raw [N, C, 4] int64 device tensors (tp, fp, fn, tn per image and class) and their
    scores.  A subclass sets ``n`` and ``device`` and appends to ``_stats`` in its update()."""

    def reset(self):
        self._stats = []

    def add_raw(self, stats):
        """Append raw statistics [N, C, 4] int64 (tp, fp, fn, tn), e.g. another rank's raw()."""
        if stats.dim() != 3 or tuple(stats.shape[1:]) != (self.n, 4):
            raise ValueError("%s.add_raw: shape %s" % (type(self).__name__, tuple(stats.shape)))
        self._stats.append(stats.to(self.device, torch.int64))

    def raw(self):
        """The statistics so far, in update order: int64 [N, C, 4] on the device."""
        return torch.cat(self._stats) if self._stats else torch.zeros(0, self.n, 4, device=self.device, dtype=torch.int64)

    def stats(self):
        """tp, fp, fn, tn as four [N, C] int64 host tensors (synchronises)."""
        r = self.raw().cpu()
        return r[..., 0], r[..., 1], r[..., 2], r[..., 3]

    def score(self, metric, reduction="micro", class_weights=None, zero_division=1.0, beta=1.0):
        """stats_score of everything seen so far: float64 on the host."""
        tp, fp, fn, tn = (a.numpy() for a in self.stats())
        return stats_score(tp, fp, fn, tn, metric, reduction, class_weights, zero_division, beta)

    def per_image(self, metric, zero_division=1.0, beta=1.0):
        """The [N, C] float64 scores of one metric per image and class (0/0 -> zero_division): mean +/- std over cases from these."""
        tp, fp, fn, tn = (a.numpy().astype(np.float64) for a in self.stats())
        with np.errstate(divide="ignore", invalid="ignore"):
            return _zero_div(_metric_fn(metric, beta)(tp, fp, fn, tn), zero_division)


class ImageStatsMeter(_RawStatsMeter):
    """tp, fp, fn, tn per image and class, accumulated on the device (``lmn_image_stats``: integer arithmetic, exact).

    A pixel whose label lies outside [0, C) is void -- ``ignore_index`` (which must lie outside [0, C)) and any other out-of-range
    value alike, as ``ConfusionMeter`` drops them (the reference's ``get_stats`` counts a stray label that is not ``ignore_index`` as a
    false positive of the predicted class) -- and adds to none of the four, so tp + fp + fn + tn is the image's valid-pixel count for
    every class.  update(pred, target): pred = fp32 logits [B, C, H, W] (arg-max, first maximum wins) or an integer label map
    [B, H, W] (e.g. DevicePostprocess's labels_net; values outside [0, C) mean "no class"); the [B, C, 4] int64 result stays on the
    device and nothing synchronises."""

    def __init__(self, n_classes, ignore_index=None, device="cuda"):
        if not 2 <= n_classes <= 64:
            raise ValueError("ImageStatsMeter: n_classes = %d outside [2, 64]" % n_classes)
        if ignore_index is not None and 0 <= int(ignore_index) < n_classes:
            raise ValueError("ImageStatsMeter: ignore_index = %d lies inside [0, %d)" % (ignore_index, n_classes))
        self.n, self.ignore_index, self.device = n_classes, None if ignore_index is None else int(ignore_index), torch.device(device)
        self._stats = []

    @torch.no_grad()
    def update(self, pred, target):
        if not pred.is_cuda or not target.is_cuda:
            raise RuntimeError("lm_net_amd.ImageStatsMeter: device tensors required (the HIP path has no CPU fallback)")
        pred = _prediction(pred, self.n, "ImageStatsMeter", torch.uint8)
        target = _target(target, pred, "ImageStatsMeter")
        stats = torch.empty(target.shape[0], self.n, 4, device=pred.device, dtype=torch.int64)
        hip.image_stats(pred, target, self.n, self.ignore_index, stats)
        self._stats.append(stats)


def _sigmoid_inputs(logits, target, n_classes, what):
    """logits fp32 contiguous [B, C, H, W]; target uint8 / int64 contiguous of the same size (bool -> uint8; [B, H, W] when C = 1)."""
    if logits.dim() != 4 or not logits.is_floating_point():
        raise ValueError("%s: logits must be floating-point [B, C, H, W], got %s %s" % (what, logits.dtype, tuple(logits.shape)))
    B, Cn, H, W = logits.shape
    if not 1 <= Cn <= 64 or (n_classes is not None and Cn != n_classes):
        raise ValueError("%s: logits with %d channels, n_classes = %s (1..64)" % (what, Cn, n_classes))
    if B * Cn > 65535 or B * H * W >= 1 << 31:
        raise ValueError("%s: B * C = %d, B * H * W = %d beyond the limits B * C <= 65535, B * H * W < 2^31" % (what, B * Cn, B * H * W))
    if not logits.is_cuda or (target is not None and not target.is_cuda):
        raise RuntimeError("lm_net_amd.%s: device tensors required (the HIP path has no CPU fallback)" % what)
    if target is not None:
        if target.is_floating_point():
            raise ValueError("%s: the target must be uint8, bool or int64, got %s" % (what, target.dtype))
        if target.dtype == torch.bool:
            target = target.to(torch.uint8)
        elif target.dtype not in (torch.uint8, torch.int64):
            target = target.long()
        if tuple(target.shape) != (B, Cn, H, W) and not (Cn == 1 and tuple(target.shape) == (B, H, W)):
            raise ValueError("%s: target %s does not match logits %s" % (what, tuple(target.shape), tuple(logits.shape)))
        target = target.contiguous()
    return logits.float().contiguous(), target


@torch.no_grad()
def sigmoid_labels(logits, threshold=0.5):
    """uint8 [B, C, H, W]: 1 where sigmoid(logits) >= threshold -- compared as logits >= log(thr / (1 - thr)) in fp32 -- else 0
    (``lmn_sigmoid_stats``, no synchronisation).  Viewed as [B * C, H, W] these are ordinary two-class label maps for
    ``ConfusionMeter(2)``, ``SurfaceDistanceMeter(2)`` and ``DevicePostprocess(2)``."""
    lt = hip.sig_logit_threshold(threshold)
    logits, _ = _sigmoid_inputs(logits, None, None, "sigmoid_labels")
    out = torch.empty(logits.shape, device=logits.device, dtype=torch.uint8)
    hip.sigmoid_stats(logits, None, lt, None, out)
    return out


class SigmoidStatsMeter(_RawStatsMeter):
    """tp, fp, fn, tn per image and class of a sigmoid head -- a one-logit binary model or a multi-label one -- accumulated on the
    device (``lmn_sigmoid_stats``: integer arithmetic, exact): ``get_stats`` of ``utils/functional.py:61-219`` in the modes "binary"
    and "multilabel" on ``sigmoid(logits)`` with ``threshold``, away from rounding ties.

    An element is predicted on when ``logits >= log(threshold / (1 - threshold))`` (fp32; exactly 0 at 0.5).  An element whose target
    is neither 0 nor 1 is void and adds to none of the four, so tp + fp + fn + tn is the valid count of its (image, class) plane.
    update(logits, target): logits [B, C, H, W]; target of the same shape ([B, H, W] when C = 1), uint8, bool or int64; the [B, C, 4]
    int64 result stays on the device and nothing synchronises.  Scores are those of ``ImageStatsMeter``."""

    def __init__(self, n_classes, threshold=0.5, device="cuda"):
        if not 1 <= n_classes <= 64:
            raise ValueError("SigmoidStatsMeter: n_classes = %d outside [1, 64]" % n_classes)
        if not 0.0 < float(threshold) < 1.0:
            raise ValueError("SigmoidStatsMeter: threshold = %g outside (0, 1)" % threshold)
        self.n, self.threshold, self.device = n_classes, float(threshold), torch.device(device)
        self.logit_threshold = hip.sig_logit_threshold(threshold)
        self._stats = []

    @torch.no_grad()
    def update(self, logits, target):
        logits, target = _sigmoid_inputs(logits, target, self.n, "SigmoidStatsMeter")
        stats = torch.empty(logits.shape[0], self.n, 4, device=logits.device, dtype=torch.int64)
        hip.sigmoid_stats(logits, target, self.logit_threshold, stats, None)
        self._stats.append(stats)

    @torch.no_grad()
    def labels(self, logits):
        """The thresholded uint8 [B, C, H, W] maps of the logits (sigmoid_labels at the meter's threshold)."""
        logits, _ = _sigmoid_inputs(logits, None, self.n, "SigmoidStatsMeter")
        out = torch.empty(logits.shape, device=logits.device, dtype=torch.uint8)
        hip.sigmoid_stats(logits, None, self.logit_threshold, None, out)
        return out


def curve_counts(hist):
    """tp, fp, fn, tn (int64 numpy, [..., N]) at every threshold from score histograms [..., 2, N + 1] (negatives, positives): an
    element of bin b is predicted on at threshold k when b >= k + 1, so tp and fp are suffix sums."""
    hist = np.asarray(hist, dtype=np.int64)
    above = np.flip(np.cumsum(np.flip(hist, -1), -1), -1)           # above[..., b] = elements of bins >= b
    fp, tp = above[..., 0, 1:], above[..., 1, 1:]
    return tp, fp, above[..., 1, :1] - tp, above[..., 0, :1] - fp


def _nan_div(a, b):
    """a / b in float64, NaN where b == 0 (no warning)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.where(b > 0, a / np.where(b > 0, b, 1.0), np.nan)


def _nanmean_last(a):
    """nanmean over the last axis; NaN (and no warning) where every entry is NaN."""
    ok = ~np.isnan(a)
    return _nan_div(np.where(ok, a, 0.0).sum(-1), ok.sum(-1))


class CurveMeter:
    """ROC and precision-recall curves, AUROC, average precision and the best threshold of any thresholded metric, per class, from
    score histograms accumulated on the device (``lmn_curve_hist``: integer counting, exact, no synchronisation).  It stands in for
    the ``AUROC`` of the reference's torchmetrics collection (``train.py:29``) with binned thresholds, and for one
    ``SigmoidStatsMeter`` per threshold.

    ``thresholds``: an integer N (t_k = k / (N - 1), torchmetrics' binned thresholds) or a non-decreasing sequence inside [0, 1], at
    most 1024 either way.  An element is predicted on at threshold t_k when its score >= t_k, compared in fp32:
      scores="sigmoid"      values are logits; compared as logit >= fp32(log(t / (1 - t))), the comparison of ``SigmoidStatsMeter``
                            (0 -> -inf: always on unless NaN; 1 -> +inf)
      scores="probability"  values are probabilities (``TiledPredictor(average="softmax" | "sigmoid").map``); compared as they are
      scores="softmax"      values are logits of 2..64 classes; the score is expf(z_c - logsumexp(z)) in fp32
    A NaN score is predicted off at every threshold.

    update(values, target): values floating [B, C, H, W]; target [B, C, H, W] planes ([B, H, W] when C = 1; 1 positive, 0 negative,
    anything else void: the contract of ``SigmoidStatsMeter``) or, for C >= 2, an integer label map [B, H, W] scored one-vs-rest (a
    label outside [0, C) is void).  The [B, C, 2, N + 1] int64 histograms stay on the device.  All scores are float64 host arithmetic
    on the integer counts."""

    def __init__(self, n_classes, scores="sigmoid", thresholds=101, device="cuda"):
        if scores not in ("sigmoid", "softmax", "probability"):
            raise ValueError("CurveMeter: scores=%r, expected 'sigmoid', 'softmax' or 'probability'" % (scores,))
        if not (2 if scores == "softmax" else 1) <= n_classes <= 64:
            raise ValueError("CurveMeter: n_classes = %d outside [%d, 64]" % (n_classes, 2 if scores == "softmax" else 1))
        self.n, self.scores, self.device = int(n_classes), scores, torch.device(device)
        self.thresholds = hip.curve_thresholds(thresholds)
        self.edges = hip.curve_edges(thresholds, "logit" if scores == "sigmoid" else "probability")
        self.score_kind = hip.CURVE_SOFTMAX if scores == "softmax" else hip.CURVE_RAW
        self._edges_dev, self._ws, self._hist = {}, {}, []

    def reset(self):
        self._hist = []

    @torch.no_grad()
    def update(self, values, target):
        what = "CurveMeter"
        labels = values.dim() == 4 and values.shape[1] >= 2 and target.dim() == 3 and not target.is_floating_point()
        if labels:
            values, _ = _sigmoid_inputs(values, None, self.n, what)
            if not target.is_cuda:
                raise RuntimeError("lm_net_amd.%s: device tensors required (the HIP path has no CPU fallback)" % what)
            if target.shape[0] != values.shape[0] or target.shape[-2:] != values.shape[-2:]:
                raise ValueError("%s: label map %s does not match values %s" % (what, tuple(target.shape), tuple(values.shape)))
            target = (target if target.dtype in (torch.uint8, torch.int64) else target.long()).contiguous()
        else:
            values, target = _sigmoid_inputs(values, target, self.n, what)
            if target is None:
                raise ValueError("%s: a target is required" % what)
        B, Cn, H, W = values.shape
        dev = values.device
        if dev not in self._edges_dev:
            self._edges_dev[dev] = torch.from_numpy(self.edges).to(dev)
        ws = None
        if self.score_kind == hip.CURVE_SOFTMAX:
            key = (dev, B, H * W)
            if key not in self._ws:                              # (one scratch per shape: a later launch on the stream reuses it)
                self._ws[key] = torch.empty(hip.curve_workspace(self.score_kind, B, H * W), device=dev, dtype=torch.uint8)
            ws = self._ws[key]
        hist = torch.empty(B, Cn, 2, self.edges.size + 1, device=dev, dtype=torch.int64)
        hip.curve_hist(values, target, hip.CURVE_LABELS if labels else hip.CURVE_PLANES, self.score_kind, self._edges_dev[dev], hist, ws)
        self._hist.append(hist)

    def add_raw(self, hist):
        """Append raw histograms [N_images, C, 2, N + 1] int64, e.g. another rank's raw()."""
        if hist.dim() != 4 or tuple(hist.shape[1:]) != (self.n, 2, self.edges.size + 1):
            raise ValueError("CurveMeter.add_raw: shape %s" % (tuple(hist.shape),))
        self._hist.append(hist.to(self.device, torch.int64))

    def raw(self):
        """The histograms so far, in update order: int64 [N_images, C, 2, N + 1] on the device."""
        if not self._hist:
            return torch.zeros(0, self.n, 2, self.edges.size + 1, device=self.device, dtype=torch.int64)
        return torch.cat(self._hist)

    def counts(self, per_image=False):
        """tp, fp, fn, tn at every threshold: int64 numpy [C, N] pooled over the images, or [N_images, C, N] (synchronises)."""
        h = self.raw().cpu().numpy()
        return curve_counts(h if per_image else h.sum(0))

    def roc(self):
        """fpr, tpr ([C, N] float64, NaN for a class without negatives / positives) and the thresholds [N]."""
        tp, fp, fn, tn = self.counts()
        return _nan_div(fp, fp + tn), _nan_div(tp, tp + fn), self.thresholds.copy()

    def pr(self):
        """precision (1 where nothing is predicted on), recall ([C, N] float64, NaN for a class without positives), thresholds [N]."""
        tp, fp, fn, tn = self.counts()
        return np.where(tp + fp > 0, _nan_div(tp, tp + fp), 1.0), _nan_div(tp, tp + fn), self.thresholds.copy()

    @staticmethod
    def _average(v, average):
        if average not in ("none", "macro"):
            raise ValueError("CurveMeter: average=%r, expected 'none' or 'macro'" % (average,))
        return v if average == "none" else _nanmean_last(v)

    def auroc(self, average="none", per_image=False):
        """The area under the binned ROC by the trapezoid rule, the end points (0, 0) and (1, 1) always added: float64 [C] (or
        [N_images, C]); NaN without a positive or without a negative; "macro": the nanmean over the classes."""
        tp, fp, fn, tn = self.counts(per_image)
        fpr, tpr = _nan_div(fp, fp + tn), _nan_div(tp, tp + fn)
        one, zero = np.ones(fpr.shape[:-1] + (1,)), np.zeros(fpr.shape[:-1] + (1,))
        x, y = np.concatenate([one, fpr, zero], -1), np.concatenate([one, tpr, zero], -1)       # (thresholds ascend: x descends)
        return self._average(((x[..., :-1] - x[..., 1:]) * (y[..., :-1] + y[..., 1:]) / 2).sum(-1), average)

    def average_precision(self, average="none", per_image=False):
        """sum_k (R_k - R_{k+1}) P_k with R_N = 0 (torchmetrics' binned average precision): float64 [C] (or [N_images, C]); NaN
        without a positive."""
        tp, fp, fn, tn = self.counts(per_image)
        prec, rec = np.where(tp + fp > 0, _nan_div(tp, tp + fp), 1.0), _nan_div(tp, tp + fn)
        nxt = np.concatenate([rec[..., 1:], np.zeros(rec.shape[:-1] + (1,))], -1)
        return self._average(((rec - nxt) * prec).sum(-1), average)

    def score(self, metric, zero_division=1.0, beta=1.0):
        """Any entry of STATS_METRICS at every threshold, from the pooled counts: float64 [C, N] (0/0 -> zero_division)."""
        tp, fp, fn, tn = (a.astype(np.float64) for a in self.counts())
        with np.errstate(divide="ignore", invalid="ignore"):
            return _zero_div(_metric_fn(metric, beta)(tp, fp, fn, tn), zero_division)

    def best_threshold(self, metric="f1", zero_division=1.0, beta=1.0):
        """Per class, the threshold of the highest score (the lowest such threshold on a tie) and that score: two float64 [C] arrays.
        The first is the number to hand to ``SigmoidStatsMeter(threshold=...)``."""
        s = self.score(metric, zero_division, beta)
        k = np.argmax(s, -1)                                     # (the first maximum)
        return self.thresholds[k], s[np.arange(s.shape[0]), k]


class SurfaceDistanceMeter:
    """HD, HD95, ASSD and RVD per class, accumulated on the device.

    For one sample and class k, P = (pred == k), T = (target == k).  The border of a mask is its pixels with a 4-neighbour outside
    it (outside the image counts as outside); D2(A -> B) is the squared pixel distance of every border pixel of A to the nearest
    border pixel of B.  HD = sqrt(max D2), HD95 = numpy's 95th percentile (linear) of the pooled sqrt(D2(P -> T)) U sqrt(D2(T -> P)),
    ASSD = the mean of the two directed means, RVD = (|P| - |T|) / |T| (0 when |T| = 0).  A pair is valid for HD / HD95 / ASSD when
    P and T are both non-empty; the others are counted as empty_pred / empty_target / empty_both and not scored.  ``spacing``: one
    isotropic pixel size that scales HD, HD95 and ASSD.

    update(pred, target): pred = fp32 logits [B, C, H, W] (arg-max, first maximum wins) or an integer label map [B, H, W]; target
    [B, H, W] integer; 2 <= H, W <= 1024; no host synchronisation.  Batches whose pairs need more than ``workspace_mb`` of scratch
    run in chunks of samples (and of classes, if one sample is too much); the statistics do not depend on the chunking."""

    RAW_I = ("n_pred", "n_target", "border_pred", "border_target", "max_d2_pt", "max_d2_tp", "d2_lo", "d2_hi")

    def __init__(self, n_classes, classes=None, spacing=1.0, device="cuda", workspace_mb=256):
        if not 2 <= n_classes <= 64:
            raise ValueError("SurfaceDistanceMeter: n_classes = %d outside [2, 64]" % n_classes)
        classes = list(range(1, n_classes)) if classes is None else [int(k) for k in classes]
        if not classes or len(set(classes)) != len(classes) or min(classes) < 0 or max(classes) >= n_classes:
            raise ValueError("SurfaceDistanceMeter: classes %r must be distinct ids in [0, %d)" % (classes, n_classes))
        if not spacing > 0 or not workspace_mb > 0:
            raise ValueError("SurfaceDistanceMeter: spacing and workspace_mb must be positive")
        self.n, self.classes, self.spacing, self.device = n_classes, classes, float(spacing), torch.device(device)
        self.workspace_bytes = int(workspace_mb * (1 << 20))
        self._si, self._sf = [], []

    def reset(self):
        self._si, self._sf = [], []

    def chunking(self, B, H, W):
        """(samples, classes) per lmn_surface_dist call: the largest chunk whose scratch fits workspace_mb."""
        nk = len(self.classes)
        need = lambda b, k: hip.surface_workspace(b, k, H, W)
        if need(1, 1) > self.workspace_bytes:
            raise ValueError("SurfaceDistanceMeter: one %dx%d pair needs %d bytes of scratch, workspace_mb allows %d"
                             % (H, W, need(1, 1), self.workspace_bytes))
        if need(1, nk) > self.workspace_bytes:
            return 1, max(k for k in range(1, nk) if need(1, k) <= self.workspace_bytes)
        cap = min(B, 65535 // nk)
        return max(b for b in range(1, cap + 1) if need(b, nk) <= self.workspace_bytes), nk

    @torch.no_grad()
    def update(self, pred, target):
        if not pred.is_cuda or not target.is_cuda:
            raise RuntimeError("lm_net_amd.SurfaceDistanceMeter: device tensors required (the HIP path has no CPU fallback)")
        pred = _prediction(pred, self.n, "SurfaceDistanceMeter", torch.int64)
        target = _target(target, pred, "SurfaceDistanceMeter")
        B, H, W = target.shape
        nk = len(self.classes)
        bs, ks = self.chunking(B, H, W)
        ws = torch.empty(hip.surface_workspace(bs, ks, H, W), device=pred.device, dtype=torch.uint8)
        si = torch.empty(B, nk, 8, device=pred.device, dtype=torch.int64)
        sf = torch.empty(B, nk, 2, device=pred.device, dtype=torch.float64)
        for b0 in range(0, B, bs):
            b1 = min(b0 + bs, B)
            for k0 in range(0, nk, ks):
                k1 = min(k0 + ks, nk)
                whole = k0 == 0 and k1 == nk                     # (a chunk of whole samples is a contiguous slice: written in place)
                ci = si[b0:b1] if whole else torch.empty(b1 - b0, k1 - k0, 8, device=pred.device, dtype=torch.int64)
                cf = sf[b0:b1] if whole else torch.empty(b1 - b0, k1 - k0, 2, device=pred.device, dtype=torch.float64)
                hip.surface_dist(pred[b0:b1], target[b0:b1], self.n, self.classes[k0:k1], ws, ci, cf)
                if not whole:
                    si[b0:b1, k0:k1], sf[b0:b1, k0:k1] = ci, cf
        self._si.append(si)
        self._sf.append(sf)

    def add_raw(self, stats_i, stats_f):
        """Append raw statistics ([N, len(classes), 8] int64, [N, len(classes), 2] float64), e.g. another rank's raw()."""
        nk = len(self.classes)
        if tuple(stats_i.shape[1:]) != (nk, 8) or tuple(stats_f.shape[1:]) != (nk, 2) or stats_i.shape[0] != stats_f.shape[0]:
            raise ValueError("SurfaceDistanceMeter.add_raw: shapes %s, %s" % (tuple(stats_i.shape), tuple(stats_f.shape)))
        self._si.append(stats_i.to(self.device, torch.int64))
        self._sf.append(stats_f.to(self.device, torch.float64))

    def raw(self):
        """The raw statistics so far, in update order: int64 [N, len(classes), 8] (fields RAW_I) and float64 [N, len(classes), 2]
        (the sums of sqrt(D2(P -> T)) and sqrt(D2(T -> P))), on the meter's device."""
        nk = len(self.classes)
        if not self._si:
            return (torch.zeros(0, nk, 8, device=self.device, dtype=torch.int64),
                    torch.zeros(0, nk, 2, device=self.device, dtype=torch.float64))
        return torch.cat(self._si), torch.cat(self._sf)

    def compute(self):
        """{'classes', 'hd', 'hd95', 'assd', 'rvd', 'rvd_total', 'valid', 'empty_pred', 'empty_target', 'empty_both': per class;
        'mean_hd', 'mean_hd95', 'mean_assd': nanmean over classes; 'per_sample': {'hd', 'hd95', 'assd', 'rvd'} as float64
        [N, len(classes)] arrays, nan on pairs that are not scored}."""
        si, sf = self.raw()
        return surface_metrics(si.cpu().numpy(), sf.cpu().numpy(), self.classes, self.spacing)


def surface_metrics(si, sf, classes, spacing=1.0):
    """SurfaceDistanceMeter.compute() of raw statistics si [N, nk, 8] int64, sf [N, nk, 2] float64 (numpy, float64 throughout)."""
    si, sf = np.asarray(si, dtype=np.int64), np.asarray(sf, dtype=np.float64)
    n_p, n_t, b_p, b_t, m_pt, m_tp, d_lo, d_hi = (si[..., i] for i in range(8))
    valid = (n_p > 0) & (n_t > 0)
    nan = np.full(valid.shape, np.nan)
    n = np.where(valid, b_p + b_t, 1)
    rem = (95 * (n - 1)) % 100                                   # the rank arithmetic is integer: lo = 95 (n - 1) // 100
    v_lo, v_hi = np.sqrt(d_lo.astype(np.float64)), np.sqrt(d_hi.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        hd = np.where(valid, np.sqrt(np.maximum(m_pt, m_tp).astype(np.float64)), nan) * spacing
        hd95 = np.where(valid, v_lo + (v_hi - v_lo) * rem / 100, nan) * spacing
        assd = np.where(valid, (sf[..., 0] / b_p + sf[..., 1] / b_t) / 2, nan) * spacing
        rvd = np.where(n_t > 0, (n_p - n_t) / n_t.astype(np.float64), 0.0)
        sp, st = n_p.sum(0), n_t.sum(0)
        rvd_total = np.where(st > 0, (sp - st) / st.astype(np.float64), 0.0)

    def mean0(a):                                                # nanmean over samples, nan (and no warning) for an empty column
        ok = ~np.isnan(a)
        cnt = ok.sum(0)
        return np.where(cnt > 0, np.where(ok, a, 0.0).sum(0) / np.maximum(cnt, 1), np.nan)

    def mean_all(v):
        v = np.asarray(v, dtype=np.float64)
        return float(v[~np.isnan(v)].mean()) if (~np.isnan(v)).any() else float("nan")

    out = {"classes": list(classes), "hd": mean0(hd).tolist(), "hd95": mean0(hd95).tolist(), "assd": mean0(assd).tolist(),
           "rvd": mean0(rvd).tolist(), "rvd_total": rvd_total.tolist(), "valid": valid.sum(0).tolist(),
           "empty_pred": ((n_p == 0) & (n_t > 0)).sum(0).tolist(), "empty_target": ((n_p > 0) & (n_t == 0)).sum(0).tolist(),
           "empty_both": ((n_p == 0) & (n_t == 0)).sum(0).tolist(),
           "per_sample": {"hd": hd, "hd95": hd95, "assd": assd, "rvd": rvd}}
    for k in ("hd", "hd95", "assd"):
        out["mean_" + k] = mean_all(out[k])
    return out


@torch.no_grad()
def _push_slices(meter, what, pred, target):
    """push() of the per-case meters (``what`` names the class in the messages): narrow n consecutive slices of the open case to uint8
    on the device (lmn_volume_labels; 255 = no class) behind the ``meter._depth`` slices that ``meter._case`` = (lab_pred, lab_target),
    uint8 [capacity, H, W], holds already.  The buffers grow by device copies; nothing synchronises."""
    if not pred.is_cuda or not target.is_cuda:
        raise RuntimeError("lm_net_amd.%s: device tensors required (the HIP path has no CPU fallback)" % what)
    pred = _prediction(pred, meter.n, what, torch.int64)
    target = _target(target, pred, what)
    n, H, W = target.shape
    if n < 1:
        raise ValueError("%s.push: no slices" % what)
    if meter._case is not None and tuple(meter._case[0].shape[1:]) != (H, W):
        raise ValueError("%s.push: slices of %dx%d into an open case of %dx%d" % ((what, H, W) + tuple(meter._case[0].shape[1:])))
    if not (2 <= H <= hip.VOLUME_MAX_SIDE and 2 <= W <= hip.VOLUME_MAX_SIDE) or meter._depth + n > hip.VOLUME_MAX_SIDE:
        raise ValueError("%s.push: a case of %d slices of %dx%d is outside 1 <= D <= %d, 2 <= H, W <= %d"
                         % (what, meter._depth + n, H, W, hip.VOLUME_MAX_SIDE, hip.VOLUME_MAX_SIDE))
    cap = 0 if meter._case is None else meter._case[0].shape[0]
    if meter._depth + n > cap:                                   # grow the case buffers (device copy, no sync)
        cap = min(max(meter._depth + n, 2 * cap), hip.VOLUME_MAX_SIDE)
        grown = tuple(torch.empty(cap, H, W, device=pred.device, dtype=torch.uint8) for _ in range(2))
        for new, old in zip(grown, meter._case or ()):
            new[:meter._depth].copy_(old[:meter._depth])
        meter._case = grown
    hip.volume_labels(pred, target, meter.n, meter._case[0], meter._case[1], meter._depth)
    meter._depth += n


class VolumeSurfaceMeter:
    """Per-case 3D Dice, Jaccard, HD, HD95, ASSD and RVD per class of a label VOLUME, accumulated on the device: medpy.metric.binary
    dc, jc, hd, hd95, assd and ravd of the whole [D, H, W] case, the numbers of a CT results table.  (SurfaceDistanceMeter scores every
    slice as its own 2D sample; the mean of per-slice HD95 is not the HD95 of the case.)

    For one case and class k, P = (pred == k), T = (target == k).  The border of a mask is its voxels with a 6-neighbour outside it
    (outside the volume counts as outside: scipy's binary_erosion with generate_binary_structure(3, 1) and border_value=0, which medpy
    uses; in a one-slice volume every mask voxel is a border voxel).  D2(A -> B) is the squared distance of every border voxel of A to
    the nearest border voxel of B.  ``spacing = (kz, ky, kx)``: positive INTEGERS, the voxel pitch along each axis in steps of ``unit``
    (a positive float, e.g. millimetres): 3.0 x 0.78 x 0.78 mm is ``spacing=(50, 13, 13), unit=0.06``.  Integer pitches keep every
    squared distance d2 = (kz dz)^2 + (ky dy)^2 + (kx dx)^2 an exact integer, so the statistics are bit-reproducible; a float pitch
    is out of scope.  HD = sqrt(max D2), HD95 = numpy's 95th percentile (linear) of the pooled sqrt(D2(P -> T)) U sqrt(D2(T -> P)),
    ASSD = the mean of the two directed means, all three scaled by ``unit``; RVD = (|P| - |T|) / |T| (0 when |T| = 0); Dice =
    2 |P n T| / (|P| + |T|) and Jaccard = |P n T| / |P u T| (nan when both masks are empty).  A pair is valid for the distances when P
    and T are both non-empty; the others are counted as empty_pred / empty_target / empty_both and not scored.

    update(pred, target) scores ONE case: pred = fp32 logits [D, C, H, W] (arg-max, first maximum wins) or an integer label volume
    [D, H, W]; target [D, H, W] integer; labels outside [0, C) belong to no class.  push(pred, target) appends a batch of consecutive
    slices of the current case (the call of a 2D validation loop: it narrows the slices to uint8 on the device and nothing else),
    close_case() scores what was pushed.  Limits, checked when a case is closed: 1 <= D <= 1024, 2 <= H, W <= 1024 and
    (kz (D-1))^2 + (ky (H-1))^2 + (kx (W-1))^2 < 2^31.  No call synchronises with the host.  A case whose classes need more than
    ``workspace_mb`` of scratch (about 20 bytes per voxel and class) runs in chunks of classes; the statistics do not depend on the
    chunking."""

    RAW_I = SurfaceDistanceMeter.RAW_I + ("n_both",)

    def __init__(self, n_classes, classes=None, spacing=(1, 1, 1), unit=1.0, device="cuda", workspace_mb=1024):
        if not 2 <= n_classes <= 64:
            raise ValueError("VolumeSurfaceMeter: n_classes = %d outside [2, 64]" % n_classes)
        classes = list(range(1, n_classes)) if classes is None else [int(k) for k in classes]
        if not classes or len(set(classes)) != len(classes) or min(classes) < 0 or max(classes) >= n_classes:
            raise ValueError("VolumeSurfaceMeter: classes %r must be distinct ids in [0, %d)" % (classes, n_classes))
        try:
            ok = len(spacing) == 3 and all(int(k) == k and 1 <= k < 2 ** 31 for k in spacing)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("VolumeSurfaceMeter: spacing %r must be three positive integers (kz, ky, kx): the pitches in steps of "
                             "`unit` (a float pitch is out of scope)" % (spacing,))
        if not unit > 0 or not workspace_mb > 0:
            raise ValueError("VolumeSurfaceMeter: unit and workspace_mb must be positive")
        self.n, self.classes, self.device = n_classes, classes, torch.device(device)
        self.spacing, self.unit = tuple(int(k) for k in spacing), float(unit)
        self.workspace_bytes = int(workspace_mb * (1 << 20))
        self._si, self._sf = [], []
        self._case, self._depth = None, 0                        # (lab_pred, lab_target) uint8 [capacity, H, W]; slices pushed

    def reset(self):
        self._si, self._sf = [], []
        self._case, self._depth = None, 0

    def chunking(self, D, H, W):
        """Classes per lmn_volume_dist call: the most whose scratch fits workspace_mb."""
        nk = len(self.classes)
        need = lambda k: hip.volume_workspace(D, H, W, k)
        if need(1) > self.workspace_bytes:
            raise ValueError("VolumeSurfaceMeter: one class of a %dx%dx%d case needs %d bytes of scratch, workspace_mb allows %d"
                             % (D, H, W, need(1), self.workspace_bytes))
        return max(k for k in range(1, nk + 1) if need(k) <= self.workspace_bytes)

    def push(self, pred, target):
        """Append n consecutive slices of the current case: pred fp32 logits [n, C, H, W] or integer labels [n, H, W], target
        [n, H, W]."""
        _push_slices(self, "VolumeSurfaceMeter", pred, target)

    @torch.no_grad()
    def close_case(self):
        """Score the slices pushed since the last case and append its raw statistics."""
        if self._case is None or self._depth == 0:
            raise ValueError("VolumeSurfaceMeter.close_case: no slices were pushed")
        (lab_p, lab_t), D = self._case, self._depth
        H, W = lab_p.shape[1:]
        self._case, self._depth = None, 0
        span = hip.volume_span((D, H, W), self.spacing)
        if span >= 2 ** 31:
            raise ValueError("VolumeSurfaceMeter: (kz (D-1))^2 + (ky (H-1))^2 + (kx (W-1))^2 = %d for spacing %r and a %dx%dx%d case; the "
                             "bound is < 2^31 = %d" % (span, self.spacing, D, H, W, 2 ** 31))
        nk = len(self.classes)
        ks = self.chunking(D, H, W)
        dev = lab_p.device
        ws = torch.empty(hip.volume_workspace(D, H, W, ks), device=dev, dtype=torch.uint8)
        si = torch.empty(nk, hip.VOLUME_NSTAT_I, device=dev, dtype=torch.int64)
        sf = torch.empty(nk, hip.VOLUME_NSTAT_F, device=dev, dtype=torch.float64)
        for k0 in range(0, nk, ks):                              # (a chunk of classes is a contiguous slice: written in place)
            k1 = min(k0 + ks, nk)
            hip.volume_dist(lab_p[:D], lab_t[:D], self.n, self.classes[k0:k1], self.spacing, ws, si[k0:k1], sf[k0:k1])
        self._si.append(si[None])
        self._sf.append(sf[None])

    def update(self, pred, target):
        """Score one whole case: push + close_case."""
        if self._depth:
            raise ValueError("VolumeSurfaceMeter.update: a case with %d pushed slices is open; close_case() first" % self._depth)
        self.push(pred, target)
        self.close_case()

    def add_raw(self, stats_i, stats_f):
        """Append raw statistics ([N, len(classes), 9] int64, [N, len(classes), 2] float64), e.g. another rank's raw()."""
        nk = len(self.classes)
        if tuple(stats_i.shape[1:]) != (nk, 9) or tuple(stats_f.shape[1:]) != (nk, 2) or stats_i.shape[0] != stats_f.shape[0]:
            raise ValueError("VolumeSurfaceMeter.add_raw: shapes %s, %s" % (tuple(stats_i.shape), tuple(stats_f.shape)))
        self._si.append(stats_i.to(self.device, torch.int64))
        self._sf.append(stats_f.to(self.device, torch.float64))

    def raw(self):
        """The raw statistics of the closed cases, in order: int64 [N, len(classes), 9] (fields RAW_I) and float64 [N, len(classes), 2]
        (the sums of sqrt(D2(P -> T)) and sqrt(D2(T -> P)), in steps of ``unit``), on the meter's device."""
        nk = len(self.classes)
        if not self._si:
            return (torch.zeros(0, nk, 9, device=self.device, dtype=torch.int64),
                    torch.zeros(0, nk, 2, device=self.device, dtype=torch.float64))
        return torch.cat(self._si), torch.cat(self._sf)

    def compute(self):
        """The keys of SurfaceDistanceMeter.compute() -- the distances scaled by ``unit`` -- plus 'dice', 'jaccard' (per class: nanmean
        over cases), 'mean_dice' (nanmean over classes) and 'per_case': {'hd', 'hd95', 'assd', 'rvd', 'dice', 'jaccard'} as float64
        [N, len(classes)] arrays, nan where a pair is not scored ('per_sample' names the same dictionary)."""
        si, sf = self.raw()
        return volume_metrics(si.cpu().numpy(), sf.cpu().numpy(), self.classes, self.unit)


def volume_metrics(si, sf, classes, unit=1.0):
    """VolumeSurfaceMeter.compute() of raw statistics si [N, nk, 9] int64, sf [N, nk, 2] float64 (numpy, float64 throughout)."""
    si = np.asarray(si, dtype=np.int64)
    out = surface_metrics(si[..., :8], sf, classes, unit)
    n_p, n_t, n_b = si[..., 0], si[..., 1], si[..., 8]
    with np.errstate(divide="ignore", invalid="ignore"):
        dice = np.where(n_p + n_t > 0, 2 * n_b / (n_p + n_t).astype(np.float64), np.nan)        # medpy dc; nan, not 0, on 0 / 0
        jacc = np.where(n_p + n_t - n_b > 0, n_b / (n_p + n_t - n_b).astype(np.float64), np.nan)   # medpy jc
    per = dict(out["per_sample"], dice=dice, jaccard=jacc)
    out["per_case"] = out["per_sample"] = per
    for key, a in (("dice", dice), ("jaccard", jacc)):
        ok = ~np.isnan(a)
        cnt = ok.sum(0)
        out[key] = np.where(cnt > 0, np.where(ok, a, 0.0).sum(0) / np.maximum(cnt, 1), np.nan).tolist()
    d = np.asarray(out["dice"], dtype=np.float64)
    out["mean_dice"] = float(d[~np.isnan(d)].mean()) if (~np.isnan(d)).any() else float("nan")
    return out


class LesionMeter:
    """Per-LESION detection and panoptic quality per class of a label volume, accumulated on the device: how many target lesions were
    found, how many predicted lesions are false alarms, lesion-wise F1 and panoptic quality -- the lesion column of a results table,
    which otherwise goes through .cpu() and scipy.ndimage.label for every case.  (The pooled meters cannot give it: a voxel-wise Dice
    of 0.9 says nothing about a missed 30-voxel metastasis.)

    For one case, Lp and Lt are the uint8 label volumes [D, H, W] of prediction and target; a 2D image is a one-slice case.  A value
    >= C is read as 0 on both sides, so VOID TARGET VOXELS ARE BACKGROUND for this meter.
      Lesions: for each scored class k (``classes``, default 1 .. C-1) the components of Lp == k (side 0, sizes n_p) and of Lt == k
        (side 1, sizes n_g) under ``connectivity`` 6, 18 or 26 -- the components of lmn_cc3d_label.  The root of a lesion is its
        smallest linear voxel index; it identifies the lesion and its class.
      Pairs: for every pair (p, g) of the same class that shares a voxel, n_pg is the number of shared voxels.
      Detection by overlap (``overlap`` = tau in [0, 1], default 0; ``min_size``, default 0): components with fewer than min_size
        voxels are dropped from both sides, and their pairs go with them.  o_g = sum_p n_pg, o_p = sum_g n_pg.  g is detected iff
        o_g >= 1 and o_g >= tau n_g; p is a hit iff o_p >= 1 and o_p >= tau n_p (both comparisons in float64).  det_tp, det_fn =
        |G| - det_tp, det_fp = the p that are no hit; sensitivity = det_tp / |G|, precision = (|P| - det_fp) / |P|, f1 = 2sp / (s + p)
        and 0 when s + p = 0; a ratio is nan where its denominator is 0.
      Matching by IoU (``iou`` = theta in [0.5, 1), default 0.5): (p, g) is matched iff n_pg / (n_p + n_g - n_pg) > theta, which is
        unique because theta >= 0.5.  tp, fp = |P| - tp, fn = |G| - tp; sq = sum IoU / tp, rq = tp / (tp + fp/2 + fn/2), pq = sq rq:
        0 when tp = 0 and the denominator is positive, nan when there are no lesions on either side.  lesion_dice = the sum over the
        matched pairs of 2 n_pg / (n_p + n_g), divided by tp + fp + fn: in the spirit of the BraTS lesion-wise Dice, without its
        dilation; it is not that challenge's code.
      Reductions: 'pooled' sums the counts over the cases and applies the formulas; 'per_case' holds arrays [N, len(classes)]; 'mean'
        is the nanmean of per_case over the cases; sensitivity_by_size(bins) is the pooled sensitivity per stratum of n_g.

    push(pred, target), close_case() and update(pred, target) work as in VolumeSurfaceMeter; update_images(pred, target) scores each
    image of a [B, H, W] batch as a one-slice case.  A case may hold ``max_components`` lesions (both sides, all scored classes) and
    ``max_pairs`` pairs (the table has the power of two >= 2 max_pairs slots); compute() raises when a case had more.  close_case()
    needs 16 bytes of scratch per voxel, checked against ``workspace_mb`` there.  Only compute() and sensitivity_by_size() synchronise
    with the host."""

    def __init__(self, n_classes, classes=None, connectivity=26, max_components=8192, max_pairs=8192, workspace_mb=2048, device="cuda"):
        if not 2 <= n_classes <= 64:
            raise ValueError("LesionMeter: n_classes = %d outside [2, 64]" % n_classes)
        classes = list(range(1, n_classes)) if classes is None else [int(k) for k in classes]
        if not classes or len(set(classes)) != len(classes) or min(classes) < 1 or max(classes) >= n_classes:
            raise ValueError("LesionMeter: classes %r must be distinct ids in [1, %d)" % (classes, n_classes))
        if connectivity not in (6, 18, 26):
            raise ValueError("LesionMeter: connectivity %r is none of 6, 18, 26" % (connectivity,))
        if int(max_components) != max_components or not 1 <= max_components < 2 ** 31:
            raise ValueError("LesionMeter: max_components %r must be an integer in [1, 2^31)" % (max_components,))
        if int(max_pairs) != max_pairs or not 1 <= 2 * max_pairs <= hip.LESION_MAX_SLOTS:
            raise ValueError("LesionMeter: max_pairs %r must be an integer in [1, %d]" % (max_pairs, hip.LESION_MAX_SLOTS // 2))
        if not workspace_mb > 0:
            raise ValueError("LesionMeter: workspace_mb must be positive")
        self.n, self.classes, self.device, self.connectivity = n_classes, classes, torch.device(device), int(connectivity)
        self.class_mask = sum(1 << k for k in classes)
        self.max_components, self.max_pairs = int(max_components), int(max_pairs)
        self.pair_slots = hip.LESION_MIN_SLOTS
        while self.pair_slots < 2 * self.max_pairs:
            self.pair_slots *= 2
        self.workspace_bytes = int(workspace_mb * (1 << 20))
        self.reset()

    def reset(self):
        self._rec = []                                           # per closed case (or add_raw): the five record tensors, [n, ...]
        self._case, self._depth = None, 0                        # (lab_pred, lab_target) uint8 [capacity, H, W]; slices pushed

    def scratch_bytes(self, D, H, W):
        """Bytes of scratch close_case() takes for a D x H x W case; raises where workspace_mb does not allow them."""
        need = hip.lesion_workspace(D, H, W)
        if need > self.workspace_bytes:
            raise ValueError("LesionMeter: a %dx%dx%d case needs %d bytes of scratch, workspace_mb allows %d"
                             % (D, H, W, need, self.workspace_bytes))
        return need

    def push(self, pred, target):
        """Append n consecutive slices of the current case: pred fp32 logits [n, C, H, W] or integer labels [n, H, W], target
        [n, H, W]."""
        _push_slices(self, "LesionMeter", pred, target)

    @torch.no_grad()
    def close_case(self):
        """Match the lesions of the slices pushed since the last case and append its records in canonical order: sorted by key, the
        empty slots last (a device sort, no sync)."""
        if self._case is None or self._depth == 0:
            raise ValueError("LesionMeter.close_case: no slices were pushed")
        (lab_p, lab_t), D = self._case, self._depth
        H, W = lab_p.shape[1:]
        self._case, self._depth = None, 0
        dev = lab_p.device
        ws = torch.empty(self.scratch_bytes(D, H, W), device=dev, dtype=torch.uint8)
        ck = torch.empty(self.max_components, device=dev, dtype=torch.int64)
        cs = torch.empty(self.max_components, device=dev, dtype=torch.int32)
        pk = torch.empty(self.pair_slots, device=dev, dtype=torch.int64)
        pc = torch.empty(self.pair_slots, device=dev, dtype=torch.int32)
        ctrl = torch.empty(hip.LESION_NCTRL, device=dev, dtype=torch.int32)
        hip.lesion_match(lab_p[:D], lab_t[:D], self.n, self.connectivity, self.class_mask, ws, ck, cs, pk, pc, ctrl)
        ck, cs = _canonical_records(ck, cs)
        pk, pc = _canonical_records(pk, pc)
        self._rec.append((ck[None], cs[None], pk[None], pc[None], ctrl[None]))

    def update(self, pred, target):
        """Score one whole case: push + close_case."""
        if self._depth:
            raise ValueError("LesionMeter.update: a case with %d pushed slices is open; close_case() first" % self._depth)
        self.push(pred, target)
        self.close_case()

    def update_images(self, pred, target):
        """Score every image of a batch as a one-slice case: pred fp32 logits [B, C, H, W] or integer labels [B, H, W], target
        [B, H, W]."""
        if self._depth:
            raise ValueError("LesionMeter.update_images: a case with %d pushed slices is open; close_case() first" % self._depth)
        if target.dim() != 3 or pred.shape[0] != target.shape[0]:
            raise ValueError("LesionMeter.update_images: pred %s, target %s: a batch [B, H, W] required"
                             % (tuple(pred.shape), tuple(target.shape)))
        for b in range(target.shape[0]):
            self.update(pred[b:b + 1], target[b:b + 1])

    def _shapes(self):
        return ((self.max_components,), (self.max_components,), (self.pair_slots,), (self.pair_slots,), (hip.LESION_NCTRL,))

    RAW_DTYPES = (torch.int64, torch.int32, torch.int64, torch.int32, torch.int32)

    def add_raw(self, comp_keys, comp_sizes, pair_keys, pair_counts, ctrl):
        """Append records ([N, max_components] int64 / int32, [N, pair_slots] int64 / int32, [N, 4] int32), e.g. another rank's
        raw()."""
        rec = (comp_keys, comp_sizes, pair_keys, pair_counts, ctrl)
        if any(t.dim() != 2 or tuple(t.shape[1:]) != s or t.shape[0] != ctrl.shape[0] for t, s in zip(rec, self._shapes())):
            raise ValueError("LesionMeter.add_raw: shapes %s; [N, ...] of %s required" % ([tuple(t.shape) for t in rec], list(self._shapes())))
        self._rec.append(tuple(t.to(self.device, dt) for t, dt in zip(rec, self.RAW_DTYPES)))

    def raw(self):
        """The records of the closed cases, in order, on the meter's device: comp_keys int64 [N, max_components] (side << 40 | class << 32
        | root) and comp_sizes int32; pair_keys int64 [N, pair_slots] (root_p << 32 | root_g) and pair_counts int32; ctrl int32 [N, 4]
        (lesions found, pairs stored, pair insertions dropped, 0).  Each case sorted by key, unused slots (-1 / 0) last: two runs on
        one input are bit-identical."""
        if not self._rec:
            return tuple(torch.zeros((0,) + s, device=self.device, dtype=dt) for s, dt in zip(self._shapes(), self.RAW_DTYPES))
        return tuple(torch.cat(ts) for ts in zip(*self._rec))

    def compute(self, overlap=0.0, iou=0.5, min_size=0):
        """lesion_metrics of the records (the one synchronising call): {'classes', 'pooled', 'per_case', 'mean'}.  Raises ValueError
        for a case that found more lesions than max_components or dropped a pair insertion."""
        return lesion_metrics(tuple(t.cpu().numpy() for t in self.raw()), self.classes, overlap=overlap, iou=iou, min_size=min_size)

    def sensitivity_by_size(self, bins, overlap=0.0, min_size=0):
        """Pooled sensitivity per stratum [bins[i], bins[i + 1]) of the target lesion size n_g: {'bins', 'n_target', 'det_tp',
        'sensitivity'}, the last three [len(bins) - 1, len(classes)]."""
        return lesion_metrics(tuple(t.cpu().numpy() for t in self.raw()), self.classes, overlap=overlap, min_size=min_size,
                              size_bins=bins)["by_size"]


def _canonical_records(keys, values):
    """Records of one case sorted by key with the empty slots (key -1, value 0) last, on the device.  (A key is below 2^62, so
    clearing the sign bit leaves it alone and turns -1 into the largest int64.)"""
    top = torch.iinfo(torch.int64).max
    k, order = torch.sort(keys & top)
    return torch.where(k == top, torch.full_like(k, -1), k), values[order]


LESION_COUNTS = ("n_pred", "n_target", "det_tp", "det_fn", "det_fp", "tp", "fp", "fn")
LESION_SCORES = ("sensitivity", "precision", "f1", "sq", "rq", "pq", "lesion_dice")


def _lesion_scores(c, sum_iou, sum_dice):
    """The formulas of LesionMeter on count arrays (a dictionary of LESION_COUNTS) and the sums over the matched pairs, float64."""
    f = {k: np.asarray(v, dtype=np.float64) for k, v in c.items()}
    sum_iou, sum_dice = np.asarray(sum_iou, dtype=np.float64), np.asarray(sum_dice, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = _nan_div(f["det_tp"], f["n_target"])
        p = _nan_div(f["n_pred"] - f["det_fp"], f["n_pred"])
        f1 = np.where(s + p == 0, 0.0, 2 * s * p / (s + p))           # (nan where s or p is)
        den = f["tp"] + 0.5 * f["fp"] + 0.5 * f["fn"]
        sq = _nan_div(sum_iou, f["tp"])
        rq = _nan_div(f["tp"], den)
        pq = np.where(den > 0, np.where(f["tp"] > 0, sq * rq, 0.0), np.nan)
        ld = _nan_div(sum_dice, f["tp"] + f["fp"] + f["fn"])
    return dict(sensitivity=s, precision=p, f1=f1, sq=sq, rq=rq, pq=pq, lesion_dice=ld)


def lesion_metrics(records, classes, overlap=0.0, iou=0.5, min_size=0, size_bins=None):
    """LesionMeter.compute() of records = (comp_keys [N, M], comp_sizes [N, M], pair_keys [N, S], pair_counts [N, S], ctrl [N, 4]) as
    LesionMeter.raw() returns them (numpy; the order of the records of a case does not matter here).  Integers and float64 throughout.
    Returns {'classes', 'pooled': counts (LESION_COUNTS) and scores (LESION_SCORES) per class, 'per_case': the same as [N, nk] arrays,
    'mean': the nanmean of the per-case scores over the cases}, plus 'by_size' when size_bins is given."""
    ck, cs, pk, pc, ctrl = (np.asarray(a) for a in records)
    if not 0.0 <= overlap <= 1.0:
        raise ValueError("lesion_metrics: overlap %r outside [0, 1]" % (overlap,))
    if not 0.5 <= iou < 1.0:
        raise ValueError("lesion_metrics: iou %r outside [0.5, 1): below 0.5 a match is not unique" % (iou,))
    if int(min_size) != min_size or min_size < 0:
        raise ValueError("lesion_metrics: min_size %r must be an integer >= 0" % (min_size,))
    N, nk = ck.shape[0], len(classes)
    for n in range(N):
        if ctrl[n, 0] > ck.shape[1]:
            raise ValueError("lesion_metrics: case %d has %d lesions, max_components allows %d" % (n, ctrl[n, 0], ck.shape[1]))
        if ctrl[n, 2] > 0:
            raise ValueError("lesion_metrics: case %d dropped %d pair insertions: its table of %d slots (2 max_pairs, rounded up) is "
                             "full" % (n, ctrl[n, 2], pk.shape[1]))
    col = np.full(256, -1, np.int64)                                  # class id -> column of `classes`
    col[[int(k) for k in classes]] = np.arange(nk)
    counts = {k: np.zeros((N, nk), np.int64) for k in LESION_COUNTS}
    sum_iou, sum_dice = np.zeros((N, nk)), np.zeros((N, nk))
    edges = None
    if size_bins is not None:
        edges = np.asarray(size_bins, dtype=np.float64)
        if edges.ndim != 1 or edges.size < 2 or not (np.diff(edges) > 0).all():
            raise ValueError("lesion_metrics: size_bins %r must be at least two ascending edges" % (size_bins,))
        bin_n, bin_tp = np.zeros((edges.size - 1, nk), np.int64), np.zeros((edges.size - 1, nk), np.int64)
    for n in range(N):
        ok = ck[n] >= 0
        key, size = ck[n][ok].astype(np.int64), cs[n][ok].astype(np.int64)
        keep = size >= min_size
        key, size = key[keep], size[keep]
        side, root = key >> 40, key & 0xFFFFFFFF
        cj = col[(key >> 32) & 0xFF]
        on = cj >= 0                                                  # (records of a class this call does not score)
        P, G = np.flatnonzero((side == 0) & on), np.flatnonzero((side == 1) & on)
        P, G = P[np.argsort(root[P], kind="stable")], G[np.argsort(root[G], kind="stable")]
        ok = pk[n] >= 0
        pkey, npg = pk[n][ok].astype(np.int64), pc[n][ok].astype(np.int64)
        ip, ig = np.searchsorted(root[P], pkey >> 32), np.searchsorted(root[G], pkey & 0xFFFFFFFF)
        # a pair whose lesion was dropped by min_size, or is of a class outside `classes`, goes with it
        live = (ip < P.size) & (ig < G.size)
        live[live] = (root[P][ip[live]] == pkey[live] >> 32) & (root[G][ig[live]] == pkey[live] & 0xFFFFFFFF)
        ip, ig, npg = ip[live], ig[live], npg[live]
        n_p, n_g = size[P], size[G]
        o_p, o_g = np.bincount(ip, npg, P.size), np.bincount(ig, npg, G.size)          # float64 sums of integers < 2^53: exact
        hit = (o_p >= 1) & (o_p >= overlap * n_p.astype(np.float64))
        det = (o_g >= 1) & (o_g >= overlap * n_g.astype(np.float64))
        union = (n_p[ip] + n_g[ig] - npg).astype(np.float64)
        v_iou = npg / union
        match = v_iou > iou
        v_dice = 2 * npg / (n_p[ip] + n_g[ig]).astype(np.float64)
        cP, cG = cj[P], cj[G]
        counts["n_pred"][n] = np.bincount(cP, minlength=nk)
        counts["n_target"][n] = np.bincount(cG, minlength=nk)
        counts["det_tp"][n] = np.bincount(cG[det], minlength=nk)
        counts["det_fp"][n] = np.bincount(cP[~hit], minlength=nk)
        counts["tp"][n] = np.bincount(cP[ip[match]], minlength=nk)
        sum_iou[n] = np.bincount(cP[ip[match]], v_iou[match], nk)
        sum_dice[n] = np.bincount(cP[ip[match]], v_dice[match], nk)
        if edges is not None:
            b = np.searchsorted(edges, n_g, side="right") - 1
            inb = (b >= 0) & (b < edges.size - 1)
            np.add.at(bin_n, (b[inb], cG[inb]), 1)
            np.add.at(bin_tp, (b[inb & det], cG[inb & det]), 1)
    counts["det_fn"] = counts["n_target"] - counts["det_tp"]
    counts["fp"] = counts["n_pred"] - counts["tp"]
    counts["fn"] = counts["n_target"] - counts["tp"]
    per_case = dict(counts, **_lesion_scores(counts, sum_iou, sum_dice))
    pooled_counts = {k: v.sum(0) for k, v in counts.items()}
    pooled = dict(pooled_counts, **_lesion_scores(pooled_counts, sum_iou.sum(0), sum_dice.sum(0)))
    mean = {}
    for k in LESION_SCORES:
        mean[k] = _nanmean_last(per_case[k].T)
    out = {"classes": list(classes), "pooled": pooled, "per_case": per_case, "mean": mean}
    if edges is not None:
        out["by_size"] = {"bins": edges.tolist(), "n_target": bin_n, "det_tp": bin_tp,
                          "sensitivity": _nan_div(bin_tp, bin_n)}
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

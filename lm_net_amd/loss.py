"""The reference's training loss as ONE fused HIP pass per direction.

``utils/train_eval_utils.py:141``::

    loss = criterion(output, labels) + criterion_dice(output, labels.unsqueeze(1).float(), weight=[1.0, 4.0])

with ``criterion = CrossEntropyLoss(weight=[1, 4], label_smoothing=args.smoothing)`` (``train.py:157``) and
``criterion_dice = DiceLoss(num_classes)`` (``utils/loss.py:170-206``).  ``SegLoss`` computes the same scalar from the
``[B, C, H, W]`` logits with two kernels (batch sums, then a one-block finish) and the gradient with one more; the
loss value stays on the device, so nothing synchronises the step.

Void labels and the focal term.  ``SegLoss(..., ignore_index=255)`` is ``F.cross_entropy(..., ignore_index=255)`` plus the reference
``DiceLoss(...)(..., ignore=(labels == 255))`` (``utils/loss.py:183-206``): a void pixel adds to no sum and receives a zero gradient.
``focal_scale`` adds the reference's ``FocalLoss`` (``utils/loss.py:126-148``: a per-class sigmoid focal loss, mean over the valid
pixels, summed over classes); ``FocalLoss`` is that term alone.  A label outside ``[0, C)`` is void even when it is not
``ignore_index`` -- as ``ConfusionMeter`` drops it -- where torch would raise.  Deliberate difference from torch: a batch without
a valid pixel gives ``0`` for the cross-entropy and focal terms (torch: NaN) and a zero gradient, so that one empty batch cannot
destroy the parameters of a loop that never synchronises.  Parity with torchvision's own ``sigmoid_focal_loss`` is not pinned by the
tests (torchvision is not a dependency); its documented formula is.
"""
import collections

import torch

from . import hip


class _SegLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, w_ce, w_dice, label_smoothing, smooth):
        if not logits.is_cuda:
            raise RuntimeError("lm_net_amd.SegLoss: device tensors required (the HIP path has no CPU fallback)")
        logits = logits.contiguous()
        target = target.contiguous()
        Cn = logits.shape[1]
        sums = torch.empty(3 + 3 * Cn, device=logits.device)
        coef = torch.empty(3 + 2 * Cn, device=logits.device)
        loss = torch.empty(1, device=logits.device)
        hip.segloss_fwd(logits, target, w_ce, w_dice, label_smoothing, smooth, sums, coef, loss)
        ctx.save_for_backward(logits, target, w_ce, coef)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        logits, target, w_ce, coef = ctx.saved_tensors
        d = torch.empty_like(logits)
        hip.segloss_bwd(logits, target, w_ce, coef, g.reshape(1).contiguous().float(), d)
        return d, None, None, None, None, None


class _SegLossExFn(torch.autograd.Function):
    """The entries of include/lmnet_loss.h: void labels, per-term scales, the focal term.  `holder.terms` receives the device tensor
    [total, ce, dice, focal]."""

    @staticmethod
    def forward(ctx, logits, target, w_ce, w_dice, param, holder):
        if not logits.is_cuda:
            raise RuntimeError("lm_net_amd.SegLoss: device tensors required (the HIP path has no CPU fallback)")
        logits = logits.contiguous()
        target = target.contiguous()
        Cn = logits.shape[1]
        sums = torch.empty(hip.loss_sums_floats(Cn), device=logits.device)
        coef = torch.empty(hip.loss_coef_floats(Cn), device=logits.device)
        loss4 = torch.empty(4, device=logits.device)
        hip.segloss_ex_fwd(logits, target, w_ce, w_dice, param, sums, coef, loss4)
        ctx.save_for_backward(logits, target, w_ce, coef)
        ctx.param = param
        holder.terms = loss4
        return loss4[0]

    @staticmethod
    def backward(ctx, g):
        logits, target, w_ce, coef = ctx.saved_tensors
        d = torch.empty_like(logits)
        hip.segloss_ex_bwd(logits, target, w_ce, coef, g.reshape(1).contiguous().float(), ctx.param, d)
        return d, None, None, None, None, None


class SegLoss(torch.nn.Module):
    """``CrossEntropyLoss(weight=ce_weight, label_smoothing) + DiceLoss(n_classes)(…, weight=dice_weight)``.

    Any class count 2..64; labels must lie in [0, C).  ``ce_weight=None`` / ``dice_weight=None`` mean all ones, sized from the
    logits (the reference's own defaults: ``nn.CrossEntropyLoss()``, ``DiceLoss`` with ``weight=None``).

    With every argument after ``smooth`` at its default this launches the kernels it always did.  Any other value routes to the
    entries of ``include/lmnet_loss.h``: ``ignore_index`` (outside [0, C); labels outside [0, C) are void in any case on this route),
    ``ce_scale`` / ``dice_scale`` / ``focal_scale`` (factors of the three terms, >= 0), ``focal_gamma`` (>= 0) and ``focal_alpha``
    (<= 1; negative: no alpha weighting).  ``terms`` then holds the device tensor ``[total, ce, dice, focal]`` of the last call
    (no synchronisation); on the default route it is None."""

    MAX_CLASSES = 64

    def __init__(self, ce_weight=(1.0, 4.0), dice_weight=(1.0, 4.0), label_smoothing=0.0, smooth=1e-5, ignore_index=None,
                 ce_scale=1.0, dice_scale=1.0, focal_scale=0.0, focal_gamma=2.0, focal_alpha=0.25):
        super().__init__()
        if min(ce_scale, dice_scale, focal_scale) < 0:
            raise ValueError("SegLoss: negative scale (ce %g, dice %g, focal %g)" % (ce_scale, dice_scale, focal_scale))
        if focal_gamma < 0 or focal_alpha > 1:
            raise ValueError("SegLoss: focal_gamma = %g must be >= 0 and focal_alpha = %g <= 1" % (focal_gamma, focal_alpha))
        n_known = max((len(w) for w in (ce_weight, dice_weight) if w is not None), default=0)
        if ignore_index is not None and 0 <= int(ignore_index) < max(n_known, 2):
            raise ValueError("SegLoss: ignore_index = %d lies inside the class range" % ignore_index)
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        self.extended = (ignore_index is not None or (ce_scale, dice_scale, focal_scale) != (1.0, 1.0, 0.0)
                         or (focal_gamma, focal_alpha) != (2.0, 0.25))
        self.param = hip.loss_param(ignore_index, label_smoothing, smooth, ce_scale, dice_scale, focal_scale, focal_gamma, focal_alpha)
        self.terms = None
        self.register_buffer("ce_weight", None if ce_weight is None else torch.tensor(ce_weight, dtype=torch.float32))
        self.register_buffer("dice_weight", None if dice_weight is None else torch.tensor(dice_weight, dtype=torch.float32))
        self.label_smoothing, self.smooth = float(label_smoothing), float(smooth)

    def _weight(self, w, Cn, dev, what):
        if w is None:
            return torch.ones(Cn, device=dev, dtype=torch.float32)
        if w.numel() != Cn:
            raise ValueError("SegLoss: %d classes in the logits, %d %s weights" % (Cn, w.numel(), what))
        return w

    def forward(self, logits, target):
        Cn = logits.shape[1]
        if not 2 <= Cn <= self.MAX_CLASSES:
            raise ValueError("SegLoss: %d classes in the logits; the fused loss takes 2..%d" % (Cn, self.MAX_CLASSES))
        w_ce = self._weight(self.ce_weight, Cn, logits.device, "ce")
        w_dice = self._weight(self.dice_weight, Cn, logits.device, "dice")
        if target.dim() == logits.dim():          # the reference passes labels.unsqueeze(1) to the Dice term
            target = target[:, 0]
        if not self.extended:
            return _SegLossFn.apply(logits, target.long(), w_ce, w_dice, self.label_smoothing, self.smooth)
        if self.ignore_index is not None and 0 <= self.ignore_index < Cn:
            raise ValueError("SegLoss: ignore_index = %d lies inside [0, %d)" % (self.ignore_index, Cn))
        if not logits.is_cuda:
            raise RuntimeError("lm_net_amd.SegLoss: device tensors required (the HIP path has no CPU fallback)")
        return _SegLossExFn.apply(logits.float(), target.long(), w_ce, w_dice, self.param, self)


class FocalLoss(SegLoss):
    """The reference's ``FocalLoss`` (``utils/loss.py:126-148``): for every class the sigmoid focal loss of its logit against the
    one-hot label, mean over the valid pixels, summed over classes.  ``SegLoss`` with the other two terms scaled to 0."""

    def __init__(self, num_classes=2, gamma=2.0, alpha=0.25, ignore_index=None):
        if not 2 <= num_classes <= self.MAX_CLASSES:
            raise ValueError("FocalLoss: num_classes = %d outside [2, %d]" % (num_classes, self.MAX_CLASSES))
        super().__init__(ce_weight=None, dice_weight=None, ignore_index=ignore_index, ce_scale=0.0, dice_scale=0.0, focal_scale=1.0,
                         focal_gamma=gamma, focal_alpha=alpha)
        self.num_classes = num_classes
        if ignore_index is not None and 0 <= int(ignore_index) < num_classes:
            raise ValueError("FocalLoss: ignore_index = %d lies inside [0, %d)" % (ignore_index, num_classes))

    def forward(self, logits, target):
        if logits.shape[1] != self.num_classes:
            raise ValueError("FocalLoss: %d classes in the logits, num_classes = %d" % (logits.shape[1], self.num_classes))
        return super().forward(logits, target)


class _SigmoidSegLossFn(torch.autograd.Function):
    """The loss entries of include/lmnet_sigmoid.h.  `holder.terms` receives the device tensor [total, bce, dice, focal]."""

    @staticmethod
    def forward(ctx, logits, target, w_bce, pos_weight, w_dice, param, holder):
        Cn = logits.shape[1]
        sums = torch.empty(hip.sig_sums_words(Cn), device=logits.device, dtype=torch.int32)
        coef = torch.empty(hip.sig_coef_floats(Cn), device=logits.device)
        loss4 = torch.empty(4, device=logits.device)
        hip.sigloss_fwd(logits, target, w_bce, pos_weight, w_dice, param, sums, coef, loss4)
        ctx.save_for_backward(logits, target, pos_weight, coef)
        ctx.param = param
        holder.terms = loss4
        return loss4[0]

    @staticmethod
    def backward(ctx, g):
        logits, target, pos_weight, coef = ctx.saved_tensors
        d = torch.empty_like(logits)
        hip.sigloss_bwd(logits, target, pos_weight, coef, g.reshape(1).contiguous().float(), ctx.param, d)
        return d, None, None, None, None, None, None


class SigmoidSegLoss(torch.nn.Module):
    """BCE + Dice (+ focal) for sigmoid heads: one-logit binary models and multi-label models, every class a binary problem of its own.

    ``bce_scale * F.binary_cross_entropy_with_logits(z, t, weight=bce_weight, pos_weight=pos_weight)`` (weights per class, mean over the
    valid elements) ``+ dice_scale *`` the reference's ``DiceLoss._dice_loss(sigmoid(z[:, c]), t[:, c], ignore_c)`` weighted by
    ``dice_weight`` and averaged over classes as ``DiceLoss.forward`` does (``utils/loss.py:183-206``) ``+ focal_scale *`` the
    reference's ``FocalLoss`` (``utils/loss.py:126-148``), each class's mean taken over its valid elements.

    logits ``[B, C, H, W]`` with 1 <= C <= 64; target ``[B, C, H, W]`` -- or ``[B, H, W]`` / ``[B, 1, H, W]`` when C = 1 -- of dtype
    uint8, bool (taken as uint8) or int64, e.g. the int64 {0, 1} masks of ``DevicePreprocess`` / ``DeviceAugment(mask_mode="binary")``
    as they are.  An element is valid when its target is 0 or 1; every other value (255, -100, ...) is void for that element alone: it
    adds to no sum and receives a zero gradient, which also covers a class that is not annotated in some image.  Soft (floating-point)
    targets are out of scope.  ``None`` weights mean all ones, sized from the logits.  ``terms`` holds the device tensor
    ``[total, bce, dice, focal]`` of the last call; nothing synchronises.  Deliberate difference from torch: without a valid element
    the BCE term and its gradient are 0, and a class without a valid element adds 0 to the focal term (torch: NaN)."""

    MAX_CLASSES = 64

    def __init__(self, bce_weight=None, pos_weight=None, dice_weight=None, smooth=1e-5, bce_scale=1.0, dice_scale=1.0, focal_scale=0.0,
                 focal_gamma=2.0, focal_alpha=0.25):
        super().__init__()
        if min(bce_scale, dice_scale, focal_scale) < 0:
            raise ValueError("SigmoidSegLoss: negative scale (bce %g, dice %g, focal %g)" % (bce_scale, dice_scale, focal_scale))
        if focal_gamma < 0 or focal_alpha > 1:
            raise ValueError("SigmoidSegLoss: focal_gamma = %g must be >= 0 and focal_alpha = %g <= 1" % (focal_gamma, focal_alpha))
        if smooth < 0:
            raise ValueError("SigmoidSegLoss: smooth = %g is negative" % smooth)
        self.args = (float(smooth), float(bce_scale), float(dice_scale), float(focal_scale), float(focal_gamma), float(focal_alpha))
        self.terms = None
        for name, w in (("bce_weight", bce_weight), ("pos_weight", pos_weight), ("dice_weight", dice_weight)):
            w = None if w is None else torch.as_tensor(w, dtype=torch.float32).reshape(-1).clone()
            if w is not None and not 1 <= w.numel() <= self.MAX_CLASSES:
                raise ValueError("SigmoidSegLoss: %d %s entries; the loss takes 1..%d classes" % (w.numel(), name, self.MAX_CLASSES))
            self.register_buffer(name, w)

    def _weight(self, w, Cn, dev, what):
        if w is None:
            return torch.ones(Cn, device=dev, dtype=torch.float32)
        if w.numel() != Cn:
            raise ValueError("SigmoidSegLoss: %d classes in the logits, %d %s weights" % (Cn, w.numel(), what))
        return w.to(dev)

    def forward(self, logits, target):
        if logits.dim() != 4:
            raise ValueError("SigmoidSegLoss: logits must be [B, C, H, W], got %s" % (tuple(logits.shape),))
        B, Cn, H, W = logits.shape
        if not 1 <= Cn <= self.MAX_CLASSES:
            raise ValueError("SigmoidSegLoss: %d classes in the logits; the loss takes 1..%d" % (Cn, self.MAX_CLASSES))
        if target.is_floating_point():
            raise ValueError("SigmoidSegLoss: floating-point (soft) targets are not supported; pass uint8, bool or int64, got %s" % target.dtype)
        if target.dtype == torch.bool:
            target = target.to(torch.uint8)
        if target.dtype not in (torch.uint8, torch.int64):
            raise ValueError("SigmoidSegLoss: target must be uint8, bool or int64, got %s" % target.dtype)
        ok = tuple(target.shape) == (B, Cn, H, W) or (Cn == 1 and tuple(target.shape) == (B, H, W))
        if not ok:
            raise ValueError("SigmoidSegLoss: target %s does not match logits %s ([B, C, H, W], or [B, H, W] when C = 1)"
                             % (tuple(target.shape), tuple(logits.shape)))
        if B * Cn > 65535 or H * W >= 1 << 31 or B * H * W >= 1 << 31:
            raise ValueError("SigmoidSegLoss: B * C = %d, H * W = %d beyond the limits B * C <= 65535, H * W < 2^31, B * H * W < 2^31"
                             % (B * Cn, H * W))
        w_bce = self._weight(self.bce_weight, Cn, logits.device, "bce")
        pos_w = self._weight(self.pos_weight, Cn, logits.device, "pos")
        w_dice = self._weight(self.dice_weight, Cn, logits.device, "dice")
        if not logits.is_cuda or not target.is_cuda:
            raise RuntimeError("lm_net_amd.SigmoidSegLoss: device tensors required (the HIP path has no CPU fallback)")
        param = hip.sig_param(*self.args, target_kind=hip.sig_target_kind(target))
        return _SigmoidSegLossFn.apply(logits.float().contiguous(), target.contiguous(), w_bce, pos_w, w_dice, param, self)


# ---------------------------------------------------------------------------------------------------------------- criteria front end
# What BoundaryLoss / HausdorffDTLoss, LovaszLoss and RegionLoss (and distance_maps, lovasz_ranks, region_sums) share on the host: the
# class count and class list, the head, the logits and target check, the scale test and the per-geometry scratch.  Each family keeps
# what `classes=None` or a string means, its own limits and its kernels.
_MAX_CLASSES = 64
_HEADS = ("softmax", "sigmoid")


def _check_n_classes(what, n_classes):
    if int(n_classes) != n_classes or not 1 <= n_classes <= _MAX_CLASSES:
        raise ValueError("%s: n_classes = %r outside [1, %d]" % (what, n_classes, _MAX_CLASSES))


def _check_head(what, head, n_classes):
    if head not in _HEADS:
        raise ValueError("%s: head = %r, expected 'softmax' or 'sigmoid'" % (what, head))
    _check_n_classes(what, n_classes)
    if head == "softmax" and n_classes < 2:
        raise ValueError("%s: a softmax head needs n_classes >= 2 (one logit: head='sigmoid')" % what)


def _parse_classes(what, n_classes, classes, none=None):
    """(sorted class ids, class_mask) of distinct integers in [0, n_classes).  `none(n_classes)`: the ids that classes=None stands for."""
    _check_n_classes(what, n_classes)
    if classes is None and none is not None:
        classes = none(int(n_classes))
    ids = [int(k) for k in classes]
    if not ids or len(set(ids)) != len(ids) or any(k != c for k, c in zip(ids, classes)) or min(ids) < 0 or max(ids) >= n_classes:
        raise ValueError("%s: classes %r must be distinct integers in [0, %d)" % (what, list(classes), n_classes))
    ids.sort()
    return ids, sum(1 << k for k in ids)


def _check_scale(what, scale):
    if not (scale - scale == 0.0):
        raise ValueError("%s: scale = %r is not finite" % (what, scale))


def _check_pair(what, n_classes, head, logits, target, float_logits, limits):
    """-> (fp32 contiguous logits, contiguous target of the head's shape).  limits(B, C, H, W) raises the family's own limits: after the
    logits' shape is known, before the target is looked at."""
    if logits.dim() != 4 or logits.shape[1] != n_classes or (float_logits and not logits.is_floating_point()):
        if float_logits:
            raise ValueError("%s: logits must be floating point [B, %d, H, W], got %s %s" % (what, n_classes, logits.dtype, tuple(logits.shape)))
        raise ValueError("%s: logits must be [B, %d, H, W], got %s" % (what, n_classes, tuple(logits.shape)))
    B, Cn, H, W = logits.shape
    limits(B, Cn, H, W)
    if target.dtype == torch.bool:
        target = target.to(torch.uint8)
    if target.dtype not in (torch.uint8, torch.int64):
        raise ValueError("%s: target must be uint8, bool or int64, got %s" % (what, target.dtype))
    if head == "softmax":
        if target.dim() == 4 and target.shape[1] == 1:
            target = target[:, 0]
        ok = tuple(target.shape) == (B, H, W)
    else:
        if Cn == 1 and tuple(target.shape) == (B, H, W):
            target = target[:, None]
        ok = tuple(target.shape) == (B, Cn, H, W)
    if not ok:
        raise ValueError("%s: target %s does not match logits %s under a %s head" % (what, tuple(target.shape), tuple(logits.shape), head))
    if not logits.is_cuda or not target.is_cuda:
        raise RuntimeError("lm_net_amd.%s: device tensors required (the HIP path has no CPU fallback)" % what)
    return logits.float().contiguous(), target.contiguous()


def _check_elements(what, B, Cn, H, W):
    if min(B, H, W) < 1 or B * Cn * H * W >= 1 << 31:
        raise ValueError("%s: B * C * H * W = %d outside the limit [1, 2^31)" % (what, B * Cn * H * W))


def _scratch(crit, logits, make):
    """The scratch of the logits' geometry, made once by make() and kept in crit._scratch: a plain dict under a name that is none of
    torch.nn.Module's registries (_parameters, _buffers, _modules), so state_dict() and .to() never see it."""
    key = (logits.device, logits.shape[0]) + tuple(logits.shape[2:])
    if key not in crit._scratch:
        crit._scratch[key] = make()
    return crit._scratch[key]


# ---------------------------------------------------------------------------------------------------------------- distance maps
# Boundary and Hausdorff losses on dense signed distance maps (include/distmap/lmnet_distmap.h).  The map is stored as the signed
# SQUARED distance, an exact int32; a plane whose mask is empty or the whole image is all 0 and flagged.
_DIST_MODES = {"labels": None, "softmax": hip.DISTMAP_SOFTMAX, "sigmoid": hip.DISTMAP_SIGMOID}


def _dist_none(n_classes):
    """classes=None: 1 .. n_classes - 1, or class 0 when there is one class only."""
    return list(range(1, n_classes)) if n_classes > 1 else [0]


def _dist_check_size(what, B, nk, H, W):
    if not (2 <= H <= hip.DISTMAP_MAX_SIDE and 2 <= W <= hip.DISTMAP_MAX_SIDE):
        raise ValueError("%s: size %d x %d outside the limit 2 <= H, W <= %d" % (what, H, W, hip.DISTMAP_MAX_SIDE))
    if B < 1 or B * nk * H * W >= 1 << 31:
        raise ValueError("%s: B * nk * H * W = %d outside the limit [1, 2^31)" % (what, B * nk * H * W))


def _dist_run(src, n_classes, class_mask, nk, mode, threshold):
    """(sd2, flags) of a checked source: the scratch comes from the caching allocator, nothing synchronises."""
    B, H, W = src.shape[0], src.shape[-2], src.shape[-1]
    ws = torch.empty(hip.dist_workspace(B, nk, H, W), device=src.device, dtype=torch.uint8)
    sd2 = torch.empty((B, nk, H, W), device=src.device, dtype=torch.int32)
    flags = torch.empty((B, nk), device=src.device, dtype=torch.int32)
    hip.dist_map(src, n_classes, class_mask, ws, sd2, flags, mode=mode, threshold=threshold)
    return sd2, flags


def distance_maps(labels_or_logits, n_classes, classes=None, mode="labels", threshold=0.5):
    """The dense signed Euclidean distance transform of the class masks, exact, on the device: ``(sd2, flags)`` with ``sd2`` int32
    ``[B, nk, H, W]`` the signed SQUARED distance between pixel centres (``+min |x - q|^2`` over the mask for a pixel outside it,
    ``-min |x - q|^2`` over the complement for a pixel inside) and ``flags`` int32 ``[B, nk]``: 0, 1 for an empty mask, 2 for a mask
    that is the whole image.  ``sd2.abs().float().sqrt()`` is ``edt(M) + edt(~M)`` of ``scipy.ndimage.distance_transform_edt``.
    Deliberate difference from scipy: a flagged plane is all 0 (scipy returns arbitrary numbers for an input without a zero).

    ``mode="labels"``: an int64 or uint8 label map ``[B, H, W]`` (``[B, 1, H, W]`` is accepted); the mask of class k is ``label == k``
    and a label outside ``[0, n_classes)`` belongs to no class.  ``mode="softmax"``: fp32 logits ``[B, C, H, W]``, mask
    ``softmax(z)_k > threshold``.  ``mode="sigmoid"``: mask ``sigmoid(z_k) > threshold`` (compared as ``z_k > logit(threshold)``).
    ``classes=None`` means ``1 .. n_classes - 1`` (class 0 when there is only one); the planes come in ascending class order.
    Limits: 1 .. 64 classes, 2 <= H, W <= 1024, B * nk * H * W < 2^31.  Device tensors only; nothing synchronises."""
    what = "distance_maps"
    if mode not in _DIST_MODES:
        raise ValueError("%s: mode = %r, expected 'labels', 'softmax' or 'sigmoid'" % (what, mode))
    ids, mask = _parse_classes(what, n_classes, classes, _dist_none)
    x = labels_or_logits
    if not 0.0 < float(threshold) < 1.0:
        raise ValueError("%s: threshold = %g outside (0, 1)" % (what, threshold))
    if mode == "labels":
        if x.dim() == 4 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 3 or x.dtype not in (torch.int64, torch.uint8):
            raise ValueError("%s: a uint8 or int64 label map [B, H, W] required, got %s %s" % (what, x.dtype, tuple(x.shape)))
        thr = 0.0
    else:
        if x.dim() != 4 or x.shape[1] != n_classes or not x.is_floating_point():
            raise ValueError("%s: logits [B, %d, H, W] required, got %s %s" % (what, n_classes, x.dtype, tuple(x.shape)))
        if mode == "softmax" and n_classes < 2:
            raise ValueError("%s: a softmax needs n_classes >= 2" % what)
        thr = float(threshold) if mode == "softmax" else hip.sig_logit_threshold(threshold)
        x = x.detach().float()
    _dist_check_size(what, x.shape[0], len(ids), x.shape[-2], x.shape[-1])
    if not x.is_cuda:
        raise RuntimeError("lm_net_amd.distance_maps: device tensors required (the HIP path has no CPU fallback)")
    return _dist_run(x.contiguous(), int(n_classes), mask, len(ids), _DIST_MODES[mode], thr)


class _DistLossFn(torch.autograd.Function):
    """The loss entries of include/distmap/lmnet_distmap.h.  cfg = (head, term, alpha, scale, class_mask)."""

    @staticmethod
    def forward(ctx, logits, target, sd2_g, sd2_p, cfg):
        head, term, alpha, scale, class_mask = cfg
        sums = torch.empty(hip.DISTMAP_SUMS_WORDS, device=logits.device, dtype=torch.int32)
        loss = torch.empty(1, device=logits.device)
        hip.dist_loss_fwd(logits, target, head, term, alpha, scale, class_mask, sd2_g, sd2_p, sums, loss)
        ctx.save_for_backward(logits, target, sd2_g, sums, *(() if sd2_p is None else (sd2_p,)))
        ctx.cfg = cfg
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        logits, target, sd2_g, sums = ctx.saved_tensors[:4]
        sd2_p = ctx.saved_tensors[4] if len(ctx.saved_tensors) > 4 else None
        head, term, alpha, scale, class_mask = ctx.cfg
        d = torch.empty_like(logits)
        hip.dist_loss_bwd(logits, target, head, term, alpha, class_mask, sd2_g, sd2_p, sums, g.reshape(1).contiguous().float(), d)
        return d, None, None, None, None


class _DistLoss(torch.nn.Module):
    """What BoundaryLoss and HausdorffDTLoss share: the classes, the head, the checks and the target's distance map."""

    MAX_CLASSES = _MAX_CLASSES
    TERM = None

    def __init__(self, n_classes, classes=None, head="softmax", scale=1.0):
        super().__init__()
        self.what = type(self).__name__
        _check_head(self.what, head, n_classes)
        self.classes, self.class_mask = _parse_classes(self.what, n_classes, classes, _dist_none)
        self.n_classes, self.head = int(n_classes), head
        self.scale = float(scale)
        self.maps = None

    def _limits(self, B, Cn, H, W):
        _dist_check_size(self.what, B, len(self.classes), H, W)
        if B * Cn * H * W >= 1 << 31:
            raise ValueError("%s: B * C * H * W = %d beyond the limit 2^31" % (self.what, B * Cn * H * W))

    def target_maps(self, target):
        """(sd2, flags) of the target's masks for this loss's classes and head: what ``forward(..., maps=)`` takes, so that a caller who
        trains both terms computes it once.  Softmax head: ``distance_maps(target, n_classes, classes)``.  Sigmoid head: plane k's mask
        is ``target[:, k] == 1`` (a void element belongs to no mask)."""
        if self.head == "softmax":
            return distance_maps(target, self.n_classes, self.classes)
        if target.dtype == torch.bool:
            target = target.to(torch.uint8)
        if target.dim() == 3:
            target = target[:, None]
        if target.dim() != 4 or target.shape[1] != self.n_classes or target.dtype not in (torch.uint8, torch.int64):
            raise ValueError("%s: target planes [B, %d, H, W] of uint8, bool or int64 required, got %s %s"
                             % (self.what, self.n_classes, target.dtype, tuple(target.shape)))
        B, _, H, W = target.shape
        nk = len(self.classes)
        planes = target if nk == self.n_classes else torch.stack([target[:, k] for k in self.classes], 1)    # (no index tensor: no copy)
        sd2, flags = distance_maps(planes.reshape(B * nk, H, W), 2, [1])             # every plane a two-class label map
        return sd2.view(B, nk, H, W), flags.view(B, nk)

    def _prediction_maps(self, logits):
        return None

    def _alpha(self):
        return 2.0

    def forward(self, logits, target, maps=None):
        _check_scale(self.what, self.scale)
        logits, target = _check_pair(self.what, self.n_classes, self.head, logits, target, False, self._limits)
        if maps is None:
            maps = self.target_maps(target)
        sd2 = maps[0]
        want = (logits.shape[0], len(self.classes)) + tuple(logits.shape[2:])
        if tuple(sd2.shape) != want or sd2.dtype != torch.int32 or not sd2.is_cuda:
            raise ValueError("%s: maps[0] must be an int32 device tensor %s, got %s %s" % (self.what, want, sd2.dtype, tuple(sd2.shape)))
        self.maps = sd2
        head = hip.DISTMAP_SOFTMAX if self.head == "softmax" else hip.DISTMAP_SIGMOID
        cfg = (head, self.TERM, self._alpha(), self.scale, self.class_mask)
        return _DistLossFn.apply(logits, target, sd2.contiguous(), self._prediction_maps(logits), cfg)


class BoundaryLoss(_DistLoss):
    """The boundary loss of Kervadec et al. (MIDL 2019): ``scale * mean(p * phi)`` over the valid pixels and the scored classes, with
    ``phi`` the signed distance map of the target (``one_hot2dist``: ``edt(neg) * neg - (edt(pos) - 1) * pos``; 0 on a plane whose
    mask is empty or the whole image: Kervadec's ``if posmask.any()``) computed on the device at every step by ``distance_maps``.

    ``classes=None`` means ``1 .. n_classes - 1`` (Kervadec's ``idc=[1]`` at two classes); for a one-logit sigmoid head it is class 0,
    the only plane.  ``scale`` is a plain attribute read at every call, so ``seg(l, y) + bl(l, y)`` with a rising ``bl.scale`` is the
    paper's schedule.  ``head="softmax"``: fp32 logits ``[B, C, H, W]`` and an int64 / uint8 label map ``[B, H, W]`` (``[B, 1, H, W]``
    accepted), valid pixels are those with a label in ``[0, C)``.  ``head="sigmoid"``: target planes ``[B, C, H, W]`` (or
    ``[B, H, W]`` at C = 1), a valid element is one whose target is 0 or 1.  ``maps`` holds the last target ``sd2``;
    ``forward(logits, target, maps=crit.target_maps(target))`` takes a precomputed ``(sd2, flags)``.  Nothing synchronises.
    Deliberate difference from torch: without a valid pixel the loss is 0 and the gradient all zero, never NaN.  Parity with
    Kervadec's or MONAI's code is not pinned by the tests (neither is a dependency); the formulas of
    ``include/distmap/lmnet_distmap.h`` are.  Limits: 1 .. 64 classes, 2 <= H, W <= 1024, B * nk * H * W < 2^31."""

    TERM = hip.DISTMAP_BOUNDARY


class HausdorffDTLoss(_DistLoss):
    """The distance-transform Hausdorff loss of Karimi and Salcudean (TMI 2019): ``scale * mean((p - g)^2 (d_p^alpha + d_g^alpha))``
    over the valid pixels and the scored classes, with ``d_g = sqrt(|sd2|)`` of the target's mask and ``d_p`` the same of the
    prediction thresholded at 0.5 (``softmax(z)_k > 0.5`` or ``z_k > 0``), both computed on the device at every step; ``d_p`` is a
    constant of the step (no gradient flows through it).  ``alpha`` in (0, 8]; ``alpha == 2`` uses the integer squares as they are.
    Classes, heads, targets, ``scale``, ``maps`` and the limits are those of ``BoundaryLoss``; ``pred_maps`` holds the last ``d_p^2``."""

    TERM = hip.DISTMAP_HAUSDORFF

    def __init__(self, n_classes, classes=None, head="softmax", alpha=2.0, scale=1.0):
        super().__init__(n_classes, classes, head, scale)
        if not 0.0 < float(alpha) <= 8.0:
            raise ValueError("HausdorffDTLoss: alpha = %r outside the limit (0, 8]" % (alpha,))
        self.alpha = float(alpha)
        self.pred_maps = None

    def _alpha(self):
        return self.alpha

    def _prediction_maps(self, logits):
        self.pred_maps = distance_maps(logits, self.n_classes, self.classes, mode=self.head)[0]
        return self.pred_maps


# ------------------------------------------------------------------------------------------------------------------------ Lovasz
# The Lovasz-Softmax loss and the Lovasz hinge (include/lovasz/lmnet_lovasz.h): a stable segmented sort of the errors on the device,
# an integer scan of the foreground over the sorted order and the closed form of Berman's lovasz_grad.
_LOVASZ_HEADS = {"softmax": hip.LOVASZ_SOFTMAX, "sigmoid": hip.LOVASZ_SIGMOID}


def _lovasz_config(what, n_classes, head, classes):
    """(sorted class ids, class_mask, present) of the constructor arguments."""
    _check_head(what, head, n_classes)
    if not isinstance(classes, str):
        return _parse_classes(what, n_classes, classes) + (False,)
    if classes not in ("present", "all"):
        raise ValueError("%s: classes = %r, expected 'present', 'all' or a list of class ids" % (what, classes))
    present = classes == "present" and head == "softmax"          # Berman's hinge skips no plane
    return _parse_classes(what, n_classes, None, range) + (present,)


def _lovasz_check(what, n_classes, head, nk, per_image, logits, target):
    def limits(B, Cn, H, W):
        _check_elements(what, B, Cn, H, W)
        if per_image and B * nk > hip.LOVASZ_MAX_SEGMENTS:
            raise ValueError("%s: per_image: B * classes = %d segments above the limit %d" % (what, B * nk, hip.LOVASZ_MAX_SEGMENTS))
    return _check_pair(what, n_classes, head, logits, target, True, limits)


def _lovasz_buffers(device, B, nk, H, W, per_image):
    """The scratch of one geometry: workspace, errors, perm, counts."""
    S, P = hip.lovasz_segments(B, nk, H, W, per_image)
    return (torch.empty(hip.lovasz_workspace(S, P), device=device, dtype=torch.uint8), torch.empty((S, P), device=device),
            torch.empty((S, P), device=device, dtype=torch.int32), torch.empty((S, 2), device=device, dtype=torch.int32))


class _LovaszFn(torch.autograd.Function):
    """The loss entries of include/lovasz/lmnet_lovasz.h.  cfg = (head, per_image, present, class_mask, scale, buffers)."""

    @staticmethod
    def forward(ctx, logits, target, cfg):
        head, per_image, present, class_mask, scale, (ws, errors, perm, counts) = cfg
        B, _, H, W = logits.shape
        coef = torch.empty((B, errors.shape[0] * errors.shape[1] // (B * H * W), H, W), device=logits.device)
        sums = torch.empty(hip.LOVASZ_SUMS_WORDS, device=logits.device, dtype=torch.int32)
        loss = torch.empty(1, device=logits.device)
        hip.lovasz_fwd(logits, target, head, per_image, present, class_mask, scale, ws, errors, perm, counts, coef, sums, loss)
        ctx.save_for_backward(logits, target, coef, sums)
        ctx.cfg = (head, class_mask)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        logits, target, coef, sums = ctx.saved_tensors
        head, class_mask = ctx.cfg
        d = torch.empty_like(logits)
        hip.lovasz_bwd(logits, target, head, class_mask, coef, sums, g.reshape(1).contiguous().float(), d)
        return d, None, None


class LovaszLoss(torch.nn.Module):
    """The Lovasz-Softmax loss and, with ``head="sigmoid"``, the Lovasz hinge of Berman, Triki and Blaschko (CVPR 2018): the convex
    Lovasz extension of the Jaccard loss, the one criterion of the package that trains against the mIoU column itself.  Per scored
    class the errors ``|fg - softmax(z)_k|`` (hinge: ``1 - z (2 t - 1)``, entering as ``relu``) are sorted descending on the device
    -- a stable segmented radix sort, ties by pixel index -- and weighted by the gradient of the Jaccard index along that order, taken
    in closed form from an integer scan; ``scale`` times the class mean is returned.

    ``classes="present"`` (Berman's default) averages over the classes that occur in the batch (in the image with ``per_image``),
    ``"all"`` or a list of class ids over all of the scored ones; the hinge skips no plane.  ``per_image=True`` takes the extension
    per image and averages over the images.  ``scale`` is a plain attribute read at every call, so ``seg(l, y) + lov(l, y)`` works as
    it stands.  ``head="softmax"``: fp32 logits ``[B, C, H, W]`` and an int64 / uint8 label map ``[B, H, W]`` (``[B, 1, H, W]``
    accepted), a pixel is valid when its label is in ``[0, C)`` and void otherwise, ``ignore_index`` or not.  ``head="sigmoid"``:
    1 .. 64 planes, target planes ``[B, C, H, W]`` (or ``[B, H, W]`` at C = 1) of uint8 / bool / int64, an element is valid when its
    target is 0 or 1.  Device tensors only; nothing synchronises; the scratch of a geometry (workspace, errors, order, counts) is kept
    and the per-call tensors (coefficients, sums, loss, gradient) come from torch's caching allocator, so nothing is allocated on the
    device after the first call of a geometry (``ranks`` holds the last ``(errors, perm, counts)``: they are overwritten by the next
    call).  The scratch is per geometry, not per stream: use from two streams at once needs one LovaszLoss object per stream.
    No float atomics: loss and gradient are bit-identical from call to call in either deterministic mode.
    Deliberate difference from torch: a segment without a valid element contributes 0 and an average over no segment is 0 with an
    all-zero gradient, never NaN; every void position has gradient +0.  Limits: B * C * H * W < 2^31, at most 65535 segments."""

    def __init__(self, n_classes, head="softmax", classes="present", per_image=False, scale=1.0):
        super().__init__()
        self.classes, self.class_mask, self.present = _lovasz_config("LovaszLoss", n_classes, head, classes)
        self.n_classes, self.head, self.per_image = int(n_classes), head, bool(per_image)
        self.scale = float(scale)
        self.ranks = None
        self._scratch = {}

    def forward(self, logits, target):
        _check_scale("LovaszLoss", self.scale)
        nk = len(self.classes)
        logits, target = _lovasz_check("LovaszLoss", self.n_classes, self.head, nk, self.per_image, logits, target)
        B, _, H, W = logits.shape
        buf = _scratch(self, logits, lambda: _lovasz_buffers(logits.device, B, nk, H, W, self.per_image))
        self.ranks = buf[1:]
        cfg = (_LOVASZ_HEADS[self.head], self.per_image, self.present, self.class_mask, self.scale, buf)
        return _LovaszFn.apply(logits, target, cfg)


def lovasz_ranks(logits, target, n_classes, head="softmax", classes="present", per_image=False):
    """``(errors, perm, counts)`` of the Lovasz losses: with one segment per scored class over the ``P = B*H*W`` pixels of the batch
    (``per_image``: per (image, class), ``s = b * nk + kk``, ``P = H*W``), ``errors`` fp32 ``[S, P]`` (0 at a void element), ``perm``
    int32 ``[S, P]`` the stable order -- the valid elements by error descending, ties by element index ascending, the void elements
    after them -- and ``counts`` int32 ``[S, 2]`` the valid and the valid foreground elements of every segment.  The arguments are
    those of ``LovaszLoss``; fresh tensors are returned.  Device tensors only; nothing synchronises."""
    ids, mask, present = _lovasz_config("lovasz_ranks", n_classes, head, classes)
    logits, target = _lovasz_check("lovasz_ranks", int(n_classes), head, len(ids), per_image, logits.detach(), target)
    B, _, H, W = logits.shape
    ws, errors, perm, counts = _lovasz_buffers(logits.device, B, len(ids), H, W, bool(per_image))
    coef = torch.empty((B, len(ids), H, W), device=logits.device)
    sums = torch.empty(hip.LOVASZ_SUMS_WORDS, device=logits.device, dtype=torch.int32)
    loss = torch.empty(1, device=logits.device)
    hip.lovasz_fwd(logits, target, _LOVASZ_HEADS[head], bool(per_image), present, mask, 1.0, ws, errors, perm, counts, coef, sums, loss)
    return errors, perm, counts


# ------------------------------------------------------------------------------------------------------------------------ region overlap
# Dice, Jaccard, Tversky / focal Tversky and generalized Dice, per batch or per image (include/region/lmnet_region.h): one sums pass
# over logits and labels, a one-block finish in fp64, one pointwise backward.
_REGION_HEADS = {"softmax": hip.REGION_SOFTMAX, "sigmoid": hip.REGION_SIGMOID}
_REGION_KINDS = {"dice": hip.REGION_DICE, "jaccard": hip.REGION_JACCARD, "tversky": hip.REGION_TVERSKY, "generalized_dice": hip.REGION_GDICE}
_REGION_DENOMINATORS = {"linear": hip.REGION_LINEAR, "squared": hip.REGION_SQUARED}


def _region_config(what, n_classes, head, classes):
    """(sorted class ids, class_mask) of the constructor arguments."""
    _check_head(what, head, n_classes)
    if isinstance(classes, str):
        raise ValueError("%s: classes = %r, expected None or a list of class ids" % (what, classes))
    return _parse_classes(what, n_classes, classes, range)


def _region_check(what, n_classes, head, logits, target):
    def limits(B, Cn, H, W):
        _check_elements(what, B, Cn, H, W)
        if B > hip.REGION_MAX_BATCH:
            raise ValueError("%s: B = %d above the limit %d" % (what, B, hip.REGION_MAX_BATCH))
    return _check_pair(what, n_classes, head, logits, target, True, limits)


def _region_buffers(device, head, B, Cn, H, W, class_mask, nk, per_image):
    """The scratch of one geometry: workspace (the deterministic-mode slots), sums, counts, per_class."""
    G = B if per_image else 1
    return (torch.empty(hip.region_workspace(_REGION_HEADS[head], B, Cn, H, W, class_mask), device=device, dtype=torch.uint8),
            torch.empty((G, nk, 3), device=device), torch.empty((G, nk, 2), device=device, dtype=torch.int32), torch.empty((G, nk), device=device))


class _RegionFn(torch.autograd.Function):
    """The loss entries of include/region/lmnet_region.h.  cfg = (head, kind, denominator, per_image, alpha, beta, smooth, exponent,
    scale, class_mask, weight, buffers)."""

    @staticmethod
    def forward(ctx, logits, target, cfg):
        head, kind, den, per_image, alpha, beta, smooth, exponent, scale, class_mask, weight, (ws, sums, counts, per_class) = cfg
        coef = torch.empty_like(sums)
        loss = torch.empty(1, device=logits.device)
        hip.region_fwd(logits, target, head, kind, den, per_image, alpha, beta, smooth, exponent, scale, class_mask, weight, ws, sums, counts,
                       coef, per_class, loss)
        ctx.save_for_backward(logits, target, coef)
        ctx.cfg = (head, per_image, class_mask)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        logits, target, coef = ctx.saved_tensors
        head, per_image, class_mask = ctx.cfg
        d = torch.empty_like(logits)
        hip.region_bwd(logits, target, head, per_image, class_mask, coef, g.reshape(1).contiguous().float(), d)
        return d, None, None


class RegionLoss(torch.nn.Module):
    """The region-overlap losses: soft Dice, soft Jaccard, Tversky / focal Tversky (Salehi et al. 2017; Abraham and Khan 2019) and the
    generalized Dice loss (Sudre et al. 2017), per batch or per image (nnU-Net's ``batch_dice=False``), under a softmax or a sigmoid
    head.  With the sums of a group (one image with ``per_image``, else the batch) and a scored class, ``I = sum p t``, ``P1 = sum p``,
    ``P2 = sum p^2``, ``T = sum t`` over the valid elements, ``D = P2 + T`` (``denominator="squared"``) or ``P1 + T`` (``"linear"``),
    ``s = smooth``:

      ``dice``              ``R = (2 I + s) / (D + s)``
      ``jaccard``           ``R = (I + s) / (D - I + s)``
      ``tversky``           ``R = (I + s) / (I + alpha (P1 - I) + beta (T - I) + s)``; linear only
      ``generalized_dice``  ``R_g = (2 sum_k v_k I_k + s) / (sum_k v_k (P1_k + T_k) + s)``, ``v_k = 1 / T_k^2``, a class absent from the
                            group takes the group's largest finite ``v`` (MONAI's rule); linear only, no ``weight``

    ``L = (1 - R) ** exponent`` (``exponent=0.75`` is the focal Tversky loss at gamma = 4/3) and the result is
    ``scale / (G nk) * sum_g sum_k weight_k L_gk``.  ``classes=None`` scores all classes, the background included (the reference's
    ``DiceLoss``); a list of ids scores those (nnU-Net's ``do_bg=False``).  ``denominator=None`` means ``"squared"`` for dice and jaccard,
    the reference's form, and ``"linear"`` for the other two kinds.  ``scale`` is a plain attribute read at every call, so
    ``seg(l, y) + reg(l, y)`` works as it stands.  ``per_class`` holds the device tensor ``[G, nk]`` of ``L_gk`` (unweighted, unscaled)
    of the last call, ``sums`` / ``counts`` its ``[G, nk, 3]`` / ``[G, nk, 2]`` overlaps (I, P1, P2 / T, N); they are overwritten by the
    next call of the same geometry.

    ``head="softmax"``: fp32 logits ``[B, C, H, W]`` and an int64 / uint8 label map ``[B, H, W]`` (``[B, 1, H, W]`` accepted), a pixel is
    valid when its label is in ``[0, C)`` and void otherwise, ``ignore_index`` or not.  ``head="sigmoid"``: 1 .. 64 planes, target planes
    ``[B, C, H, W]`` (or ``[B, H, W]`` at C = 1) of uint8 / bool / int64, an element is valid when its target is 0 or 1.  Device tensors
    only; nothing synchronises; the scratch of a geometry is kept and the per-call tensors come from torch's caching allocator, so
    nothing is allocated on the device after the first call of a geometry.  The scratch is per geometry, not per stream: use from two
    streams at once needs one RegionLoss object per stream.
    Deliberate difference from torch: a denominator that is exactly 0 gives R = 1, a group without a valid element contributes 0, the
    loss is never NaN, ``u = 1 - R <= 0`` under ``exponent != 1`` gives 0 with a zero gradient, and every void position has gradient
    +0.  Limits: B <= 65535, B * C * H * W < 2^31."""

    def __init__(self, n_classes, kind="dice", head="softmax", classes=None, weight=None, per_image=False, denominator=None, smooth=1e-5,
                 alpha=0.5, beta=0.5, exponent=1.0, scale=1.0):
        super().__init__()
        self.classes, self.class_mask = _region_config("RegionLoss", n_classes, head, classes)
        if kind not in _REGION_KINDS:
            raise ValueError("RegionLoss: kind = %r, expected one of %s" % (kind, sorted(_REGION_KINDS)))
        if denominator is None:
            denominator = "squared" if kind in ("dice", "jaccard") else "linear"
        if denominator not in _REGION_DENOMINATORS:
            raise ValueError("RegionLoss: denominator = %r, expected 'linear' or 'squared'" % (denominator,))
        if denominator == "squared" and kind not in ("dice", "jaccard"):
            raise ValueError("RegionLoss: the squared denominator exists for dice and jaccard only, not for %s" % kind)
        if not (0.0 <= alpha < float("inf") and 0.0 <= beta < float("inf")):
            raise ValueError("RegionLoss: alpha = %r, beta = %r must be finite and >= 0" % (alpha, beta))
        if not 0.0 <= smooth < float("inf"):
            raise ValueError("RegionLoss: smooth = %r must be finite and >= 0" % (smooth,))
        if not 0.0 < exponent <= 8.0:
            raise ValueError("RegionLoss: exponent = %r outside (0, 8]" % (exponent,))
        if weight is not None:
            if kind == "generalized_dice":
                raise ValueError("RegionLoss: generalized_dice takes no class weight (its weights are 1 / T_k^2)")
            weight = torch.as_tensor(weight, dtype=torch.float32).reshape(-1)
            if weight.numel() != len(self.classes) or not bool(torch.isfinite(weight).all()):
                raise ValueError("RegionLoss: weight needs %d finite values, one per scored class" % len(self.classes))
        self.register_buffer("weight", weight)
        self.n_classes, self.kind, self.head, self.per_image, self.denominator = int(n_classes), kind, head, bool(per_image), denominator
        self.smooth, self.alpha, self.beta, self.exponent = float(smooth), float(alpha), float(beta), float(exponent)
        self.scale = float(scale)
        self.per_class = self.sums = self.counts = None
        self._scratch = {}

    def forward(self, logits, target):
        _check_scale("RegionLoss", self.scale)
        logits, target = _region_check("RegionLoss", self.n_classes, self.head, logits, target)
        B, Cn, H, W = logits.shape
        buf = _scratch(self, logits, lambda: _region_buffers(logits.device, self.head, B, Cn, H, W, self.class_mask, len(self.classes),
                                                             self.per_image))
        if self.weight is not None and self.weight.device != logits.device:
            self.weight = self.weight.to(logits.device)
        self.sums, self.counts, self.per_class = buf[1:]
        cfg = (_REGION_HEADS[self.head], _REGION_KINDS[self.kind], _REGION_DENOMINATORS[self.denominator], self.per_image, self.alpha, self.beta,
               self.smooth, self.exponent, self.scale, self.class_mask, self.weight, buf)
        return _RegionFn.apply(logits, target, cfg)


def region_sums(logits, target, n_classes, head="softmax", classes=None, per_image=False):
    """``(sums, counts)``: the soft overlaps of every (group, scored class) -- ``sums`` fp32 ``[G, nk, 3]`` = ``sum p t``, ``sum p``,
    ``sum p^2`` and ``counts`` int32 ``[G, nk, 2]`` = ``sum t`` and the number of valid elements, ``G = B`` with ``per_image``, else 1
    -- for monitoring a soft Dice without a synchronisation.  The arguments are those of ``RegionLoss``; fresh tensors are returned.
    Device tensors only; nothing synchronises."""
    ids, mask = _region_config("region_sums", n_classes, head, classes)
    logits, target = _region_check("region_sums", int(n_classes), head, logits.detach(), target)
    B, Cn, H, W = logits.shape
    ws, sums, counts, per_class = _region_buffers(logits.device, head, B, Cn, H, W, mask, len(ids), bool(per_image))
    coef = torch.empty_like(sums)
    loss = torch.empty(1, device=logits.device)
    hip.region_fwd(logits, target, _REGION_HEADS[head], hip.REGION_DICE, hip.REGION_SQUARED, bool(per_image), 0.5, 0.5, 1e-5, 1.0, 1.0, mask,
                   None, ws, sums, counts, coef, per_class, loss)
    return sums, counts


# ------------------------------------------------------------------------------------------------------------------------ soft targets
# Criteria that read a distribution per pixel (include/soft/lmnet_soft.h): cross entropy + Dice against probabilities or against the
# two-hot target of a Mixup batch, and the distillation term against a teacher's logits.  One sums pass over logits and target, a
# one-block finish in fp64, one pointwise backward.
_SOFT_HEADS = {"softmax": hip.SOFT_SOFTMAX, "sigmoid": hip.SOFT_SIGMOID}


class MixedTarget(collections.namedtuple("MixedTarget", ("ya", "yb", "lam"))):
    """The target of a ``DeviceMix`` batch: two label maps ``[B, H, W]`` of one type and ``lam`` fp32 ``[B]`` on the device, standing
    for ``q = lam onehot(ya) + (1 - lam) onehot(yb)``.  ``SoftSegLoss`` takes it as it is.  ``labels`` is the hard label map ``ya`` for
    the criteria that read integer labels -- it exists only when the ``DeviceMix`` that made the target cannot draw Mixup
    (``mixup_alpha == 0``: CutMix pastes labels with the pixels, so ``ya == yb`` and ``lam == 1``); otherwise it raises."""

    hard = False        # set by DeviceMix on the targets of a mixer that cannot draw Mixup

    @property
    def labels(self):
        if not self.hard:
            raise ValueError("MixedTarget.labels: the DeviceMix that made this target can draw Mixup (mixup_alpha > 0), so there is no "
                             "hard label map; pass the target to SoftSegLoss")
        return self.ya


def _soft_limits(what):
    def limits(B, Cn, H, W):
        _check_elements(what, B, Cn, H, W)
        if B > hip.SOFT_MAX_BATCH:
            raise ValueError("%s: B = %d above the limit %d" % (what, B, hip.SOFT_MAX_BATCH))
    return limits


def _soft_logits(what, n_classes, logits):
    """The checks of _check_pair on the logits alone, in its words -> (B, C, H, W)."""
    if logits.dim() != 4 or logits.shape[1] != n_classes or not logits.is_floating_point():
        raise ValueError("%s: logits must be floating point [B, %d, H, W], got %s %s" % (what, n_classes, logits.dtype, tuple(logits.shape)))
    _soft_limits(what)(*logits.shape)
    return tuple(logits.shape)


def _soft_label_map(what, logits, target):
    """The checks of _check_pair on a label map under a softmax head, in its words, without the device test."""
    if not torch.is_tensor(target) or target.dtype not in (torch.uint8, torch.int64, torch.bool):
        raise ValueError("%s: target must be uint8, bool or int64, got %s" % (what, getattr(target, "dtype", type(target).__name__)))
    shape = tuple(target.shape[:1] + target.shape[2:]) if target.dim() == 4 and target.shape[1] == 1 else tuple(target.shape)
    if shape != (logits.shape[0],) + tuple(logits.shape[2:]):
        raise ValueError("%s: target %s does not match logits %s under a softmax head" % (what, tuple(target.shape), tuple(logits.shape)))


def _soft_float_target(what, head, logits, target, name):
    if tuple(target.shape) != tuple(logits.shape):
        raise ValueError("%s: %s %s does not match logits %s under a %s head" % (what, name, tuple(target.shape), tuple(logits.shape), head))
    if not logits.is_cuda or not target.is_cuda:
        raise RuntimeError("lm_net_amd.%s: device tensors required (the HIP path has no CPU fallback)" % what)


class _SoftFn(torch.autograd.Function):
    """The loss entries of include/soft/lmnet_soft.h.  cfg = (reader, head, target, ya, yb, lam, temperature, eps, smooth, ce_scale,
    dice_scale, w_ce, w_dice, (workspace, sums, counts), holder); `holder.terms` receives the device tensor of the three terms."""

    @staticmethod
    def forward(ctx, logits, cfg):
        reader, head, target, ya, yb, lam, T, eps, smooth, ce_scale, dice_scale, w_ce, w_dice, (ws, sums, counts), holder = cfg
        coef = torch.empty(1 + 2 * logits.shape[1], device=logits.device)
        terms = torch.empty(3, device=logits.device)
        hip.soft_fwd(logits, reader, head, target, ya, yb, lam, T, eps, smooth, ce_scale, dice_scale, w_ce, w_dice, ws, sums, counts, coef, terms)
        ctx.save_for_backward(logits, coef)
        ctx.cfg = (reader, head, target, ya, yb, lam, T, eps, w_ce)
        holder.terms = terms
        return terms[0]

    @staticmethod
    def backward(ctx, g):
        logits, coef = ctx.saved_tensors
        reader, head, target, ya, yb, lam, T, eps, w_ce = ctx.cfg
        d = torch.empty_like(logits)
        hip.soft_bwd(logits, reader, head, target, ya, yb, lam, T, eps, w_ce, coef, g.reshape(1).contiguous().float(), d)
        return d, None


def _soft_buffers(device, readers, head, B, Cn, H, W):
    """The scratch of one geometry: workspace (the deterministic-mode slots, sized for every reader of the criterion), sums, counts."""
    ws = max(hip.soft_workspace(r, _SOFT_HEADS[head], B, Cn, H, W) for r in readers)
    return (torch.empty(ws, device=device, dtype=torch.uint8), torch.empty(1 + 3 * Cn, device=device),
            torch.empty(1, device=device, dtype=torch.int32))


class SoftSegLoss(torch.nn.Module):
    """``SegLoss`` against a distribution per pixel: ``ce_scale * F.cross_entropy(logits, q, weight=ce_weight, label_smoothing) +
    dice_scale *`` the reference's ``DiceLoss`` on the float target ``q`` (``utils/loss.py:183-206``: ``1 - (2 sum p q + s) /
    (sum p^2 + sum q^2 + s)`` per class, weighted by ``dice_weight`` and averaged over the classes; ``q`` enters the Dice term unsmoothed).

    ``target`` is a float tensor ``q`` ``[B, C, H, W]``, used as given (not renormalised, as torch), or a ``MixedTarget`` of
    ``DeviceMix``, the two-hot ``q = lam onehot(ya) + (1 - lam) onehot(yb)`` that is never materialised.  A pixel is void when any
    ``q_c`` is negative or not finite (fill a void pixel with NaN or -1), or when one of the two labels lies outside ``[0, C)``.  Torch's
    probability-target cross entropy divides by the pixel count, not by the weight sum, so with non-unit weights the cross-entropy term
    differs from the index-target ``SegLoss`` by that normalisation, on purpose; with unit weights and a one-hot ``q`` the two agree.
    ``None`` weights mean all ones.  ``ce_scale`` / ``dice_scale`` are plain attributes read at every call.  ``terms`` holds the
    device tensor ``[total, ce, dice]`` of the last call and ``counts`` the int32 device tensor ``[N]`` of its valid pixels (overwritten
    by the next call of the geometry); nothing synchronises.  Softmax heads only, 2 .. 64 classes, fp32 logits.
    Device tensors only; the scratch of a geometry is kept and the per-call tensors come from torch's caching allocator, so nothing
    is allocated on the device after the first call of a geometry; the scratch is per geometry, not per stream.
    Deliberate difference from torch: without a valid pixel every term is 0 with a zero gradient, never NaN; every void position has
    gradient +0; a Dice denominator that is exactly 0 gives a ratio of 1.  Limits: B <= 65535, B * C * H * W < 2^31.
    Out of scope: a soft BCE under sigmoid heads (``SigmoidSegLoss`` keeps refusing float targets: mix the planes in torch),
    per-image Dice, bf16 probability targets."""

    def __init__(self, n_classes, ce_weight=None, dice_weight=None, label_smoothing=0.0, smooth=1e-5, ce_scale=1.0, dice_scale=1.0):
        super().__init__()
        _check_head("SoftSegLoss", "softmax", n_classes)
        if not 0.0 <= label_smoothing <= 1.0:
            raise ValueError("SoftSegLoss: label_smoothing = %r outside [0, 1]" % (label_smoothing,))
        if not 0.0 <= smooth < float("inf"):
            raise ValueError("SoftSegLoss: smooth = %r must be finite and >= 0" % (smooth,))
        for name, w in (("ce_weight", ce_weight), ("dice_weight", dice_weight)):
            if w is not None:
                w = torch.as_tensor(w, dtype=torch.float32).reshape(-1).clone()
                if w.numel() != n_classes or not bool(torch.isfinite(w).all()):
                    raise ValueError("SoftSegLoss: %s needs %d finite values, one per class" % (name, n_classes))
            self.register_buffer(name, w)
        self.n_classes, self.label_smoothing, self.smooth = int(n_classes), float(label_smoothing), float(smooth)
        self.ce_scale, self.dice_scale = float(ce_scale), float(dice_scale)
        self.terms = self.counts = None
        self._scratch = {}

    def forward(self, logits, target):
        what = "SoftSegLoss"
        _check_scale(what, self.ce_scale)
        _check_scale(what, self.dice_scale)
        ya = yb = lam = q = None
        if isinstance(target, MixedTarget):
            _soft_logits(what, self.n_classes, logits)
            for t in (target.ya, target.yb):               # both maps, before the device of either is looked at
                _soft_label_map(what, logits, t)
            logits, ya = _check_pair(what, self.n_classes, "softmax", logits, target.ya, True, _soft_limits(what))
            _, yb = _check_pair(what, self.n_classes, "softmax", logits, target.yb, True, _soft_limits(what))
            lam = target.lam
            if ya.dtype != yb.dtype:
                raise ValueError("%s: the two label maps of a MixedTarget must share a type, got %s and %s" % (what, ya.dtype, yb.dtype))
            if not torch.is_tensor(lam) or lam.dtype != torch.float32 or tuple(lam.shape) != (logits.shape[0],) or not lam.is_cuda:
                raise ValueError("%s: lam of a MixedTarget must be an fp32 device tensor [%d]" % (what, logits.shape[0]))
            reader, lam = hip.SOFT_PAIR, lam.contiguous()
        else:
            _soft_logits(what, self.n_classes, logits)
            if not torch.is_tensor(target) or not target.is_floating_point():
                raise ValueError("%s: target must be a floating-point tensor [B, C, H, W] or a MixedTarget, got %s"
                                 % (what, target.dtype if torch.is_tensor(target) else type(target).__name__))
            if target.dtype != torch.float32:
                raise ValueError("%s: the probability target must be fp32, got %s (bf16 probability targets are out of scope)" % (what, target.dtype))
            _soft_float_target(what, "softmax", logits, target, "target")
            reader, logits, q = hip.SOFT_PROBS, logits.float().contiguous(), target.detach().contiguous()
        B, Cn, H, W = logits.shape
        buf = _scratch(self, logits, lambda: _soft_buffers(logits.device, (hip.SOFT_PROBS, hip.SOFT_PAIR), "softmax", B, Cn, H, W))
        for name in ("ce_weight", "dice_weight"):
            w = getattr(self, name)
            if w is not None and w.device != logits.device:
                setattr(self, name, w.to(logits.device))
        self.counts = buf[2]
        cfg = (reader, hip.SOFT_SOFTMAX, q, ya, yb, lam, 1.0, self.label_smoothing, self.smooth, self.ce_scale, self.dice_scale, self.ce_weight,
               self.dice_weight, buf, self)
        return _SoftFn.apply(logits, cfg)


class DistillLoss(torch.nn.Module):
    """The distillation term of Hinton et al. (2015): ``scale * T^2 / N * sum KL(q || p)`` with ``q = softmax(teacher / T)``,
    ``p = softmax(logits / T)`` over the N valid pixels, or, with ``head="sigmoid"``, the Bernoulli divergence of
    ``q = sigmoid(teacher / T)`` from ``p = sigmoid(logits / T)`` over the N valid elements.  A per-pixel mean, so the scale does not
    depend on the image size; torch's ``batchmean`` is not reproduced.

    ``forward(logits, teacher_logits, valid=None)``: the teacher is fp32 or bf16 ``[B, C, H, W]`` (read as it is stored), detached, and
    gets no gradient.  ``valid`` is the batch's own target: a uint8 / int64 label map ``[B, H, W]`` under a softmax head (a pixel counts
    when its label lies in ``[0, C)``), target planes ``[B, C, H, W]`` under a sigmoid head (an element counts when its value is 0 or
    1); ``None`` counts everything.  ``scale`` is a plain attribute read at every call, so ``seg(l, y) + kd(l, teacher(x), y)`` is
    Hinton's recipe with the void pixels excluded.  ``log q`` and ``log p`` come from one device routine: a teacher whose logits equal
    the student's bit for bit gives exactly 0 and an all-zero gradient, and logits of +-100 stay finite.  ``terms`` holds the device
    tensor ``[scale * kd, kd, 0]`` of the last call and ``counts`` the int32 device tensor ``[N]``; nothing synchronises.  Device tensors only; the scratch of a geometry is kept and
    the per-call tensors come from torch's caching allocator; the scratch is per geometry, not per stream.
    Deliberate difference from torch: without a valid pixel the term is 0 with a zero gradient, never NaN, and every void position has
    gradient +0.  Limits: 1 .. 64 classes (softmax: from 2), B <= 65535, B * C * H * W < 2^31.  Out of scope: Dice against the teacher."""

    def __init__(self, n_classes, temperature=1.0, head="softmax", scale=1.0):
        super().__init__()
        _check_head("DistillLoss", head, n_classes)
        if not 0.0 < float(temperature) < float("inf"):
            raise ValueError("DistillLoss: temperature = %r must be finite and > 0" % (temperature,))
        self.n_classes, self.head, self.temperature = int(n_classes), head, float(temperature)
        self.scale = float(scale)
        self.terms = self.counts = None
        self._scratch = {}

    def forward(self, logits, teacher_logits, valid=None):
        what = "DistillLoss"
        _check_scale(what, self.scale)
        if valid is not None:
            logits, valid = _check_pair(what, self.n_classes, self.head, logits, valid, True, _soft_limits(what))
        else:
            _soft_logits(what, self.n_classes, logits)
        if not torch.is_tensor(teacher_logits) or not teacher_logits.is_floating_point():
            raise ValueError("%s: teacher_logits must be a floating-point tensor [B, C, H, W]" % what)
        _soft_float_target(what, self.head, logits, teacher_logits, "teacher_logits")
        logits = logits.float().contiguous()
        teacher = teacher_logits.detach()
        teacher = (teacher if teacher.dtype == torch.bfloat16 else teacher.float()).contiguous()
        reader = hip.SOFT_TEACHER_BF16 if teacher.dtype == torch.bfloat16 else hip.SOFT_TEACHER_F32
        B, Cn, H, W = logits.shape
        buf = _scratch(self, logits, lambda: _soft_buffers(logits.device, (hip.SOFT_TEACHER_F32, hip.SOFT_TEACHER_BF16), self.head, B, Cn, H, W))
        self.counts = buf[2]
        cfg = (reader, _SOFT_HEADS[self.head], teacher, valid, None, None, self.temperature, 0.0, 0.0, self.scale, 0.0, None, None, buf, self)
        return _SoftFn.apply(logits, cfg)


# ------------------------------------------------------------------------------------------------------------------------ hard pixels
# Top-k and OHEM cross entropy (include/hard/lmnet_hard.h): a values pass over logits and target, an exact three-level radix select of
# the K-th largest value with K formed on the device, a sum pass, a one-block finish in fp64, one pointwise backward.
_HARD_HEADS = {"softmax": hip.HARD_SOFTMAX, "sigmoid": hip.HARD_SIGMOID}


def _hard_config(what, n_classes, head, keep, min_kept, thresh, weight):
    """(keep or 0.0, min_kept, thresh, weight tensor or None) of the constructor arguments."""
    _check_head(what, head, n_classes)
    if keep is not None and not 0.0 < float(keep) <= 1.0:
        raise ValueError("%s: keep = %r outside (0, 1]" % (what, keep))
    if isinstance(min_kept, bool) or int(min_kept) != min_kept or not 0 <= min_kept < 1 << 62:
        raise ValueError("%s: min_kept = %r must be an integer >= 0" % (what, min_kept))
    if thresh is not None and not 0.0 < float(thresh) <= 1.0:
        raise ValueError("%s: thresh = %r outside (0, 1]" % (what, thresh))
    if keep is None and thresh is None and min_kept == 0:
        raise ValueError("%s: one of keep, min_kept > 0 and thresh must be given" % what)
    if weight is not None:
        weight = torch.as_tensor(weight, dtype=torch.float32).reshape(-1).clone()
        if weight.numel() != n_classes or not bool(torch.isfinite(weight).all()) or bool((weight < 0).any()):
            raise ValueError("%s: weight needs %d finite values >= 0, one per class" % (what, n_classes))
    return (0.0 if keep is None else float(keep)), int(min_kept), (None if thresh is None else float(thresh)), weight


def _hard_check(what, n_classes, head, per_image, logits, target):
    def limits(B, Cn, H, W):
        _check_elements(what, B, Cn, H, W)
        if B > hip.HARD_MAX_BATCH:
            raise ValueError("%s: B = %d above the limit %d" % (what, B, hip.HARD_MAX_BATCH))
        if per_image and B > hip.HARD_MAX_GROUPS:
            raise ValueError("%s: per_image: B = %d groups above the limit %d" % (what, B, hip.HARD_MAX_GROUPS))
    return _check_pair(what, n_classes, head, logits, target, True, limits)


def _hard_workspace(device, head, per_image, B, Cn, H, W):
    """The scratch of one geometry: the histograms, counts and slots."""
    return torch.empty(hip.hard_workspace(_HARD_HEADS[head], per_image, B, Cn, H, W), device=device, dtype=torch.uint8)


def _hard_outputs(logits, head, per_image):
    """The per-call tensors: values, selection, terms, loss."""
    B, Cn, H, W = logits.shape
    G = B if per_image else 1
    return (torch.empty((B, H, W) if head == "softmax" else (B, Cn, H, W), device=logits.device),
            torch.empty((G, hip.HARD_RECORD_WORDS), device=logits.device, dtype=torch.int32), torch.empty(G, device=logits.device),
            torch.empty(1, device=logits.device))


class _HardFn(torch.autograd.Function):
    """The loss entries of include/hard/lmnet_hard.h.  cfg = (head, per_image, keep, min_kept, cut, scale, weight, workspace, holder);
    `holder.selection`, `.values` and `.terms` receive the device tensors of the call."""

    @staticmethod
    def forward(ctx, logits, target, cfg):
        head, per_image, keep, min_kept, cut, scale, weight, ws, holder = cfg
        values, selection, terms, loss = _hard_outputs(logits, "softmax" if head == hip.HARD_SOFTMAX else "sigmoid", per_image)
        hip.hard_fwd(logits, target, head, per_image, keep, min_kept, cut, scale, weight, ws, values, selection, terms, loss)
        ctx.save_for_backward(logits, target, values, selection)
        ctx.cfg = (head, per_image, scale, weight)
        holder.selection, holder.values, holder.terms = selection, values, terms
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        logits, target, values, selection = ctx.saved_tensors
        head, per_image, scale, weight = ctx.cfg
        d = torch.empty_like(logits)
        hip.hard_bwd(logits, target, head, per_image, scale, weight, values, selection, g.reshape(1).contiguous().float(), d)
        return d, None, None


class HardPixelLoss(torch.nn.Module):
    """The cross entropy of the hard pixels only: nnU-Net's ``TopKLoss`` (``keep``: the mean of the worst ``keep * N`` per-pixel
    cross entropies) and OHEM, online hard example mining (``thresh``, ``min_kept``: every pixel whose true-class probability is
    below ``thresh``, and at least ``min_kept`` pixels), with the count formed and the cutoff selected on the device.

    An ELEMENT is a pixel under ``head="softmax"`` (2 .. 64 classes, an int64 / uint8 label map ``[B, H, W]``, ``[B, 1, H, W]``
    accepted), with value ``l = weight[y] * (logsumexp(z) - z[y])`` and void when its label lies outside ``[0, C)``; under
    ``head="sigmoid"`` (1 .. 64 planes, target planes ``[B, C, H, W]``, ``[B, H, W]`` at C = 1, of uint8 / bool / int64) it is a
    (pixel, class) entry with ``l = weight[c] * BCE_with_logits(z, t)``, void when its target is neither 0 nor 1.  A GROUP is the
    batch, or one image with ``per_image=True``; under a sigmoid head the classes of a group are pooled.  For a group with N valid
    elements

      ``K = min(N, max(1, floor(float32(keep) * N), min_kept, #{l > float32(-log(thresh))}))``

    (an argument that is not given counts 0; ``floor(keep * N)`` is nnU-Net's ``int(n * k / 100)``), the group's term is the mean of
    its K largest values -- exactly ``torch.topk(l, K).values.mean()`` -- and the loss is ``scale / G`` times the sum of the terms.
    Ties: with ``tau`` the K-th largest value, ``n_gt`` the values above it and ``n_eq`` the values equal to it, an element above
    ``tau`` has gradient weight ``1 / K`` and the tied elements at the cutoff share the rest, ``(K - n_gt) / (n_eq K)`` each, so the
    result is a function of the inputs alone and equals torch whenever the cutoff is not tied.  Selection and sum both use the
    WEIGHTED value: with class weights other than 1, ``thresh`` is no longer a pure probability threshold (it compares
    ``weight * -log p`` with ``-log(thresh)``).  At least one of ``keep``, ``min_kept > 0`` and ``thresh`` must be given;
    ``weight`` is ``None`` (all ones) or C finite values ``>= 0``.  ``scale`` is a plain attribute read at every call, so
    ``RegionLoss(C, classes=range(1, C))(l, y) + HardPixelLoss(C, keep=0.1)(l, y)`` is nnU-Net's ``DC_and_topk_loss`` as it stands,
    and ``HardPixelLoss(C, thresh=0.7, min_kept=100000)`` is the usual OHEM rule.

    ``selection`` holds the device int32 tensor ``[G, 5]`` of the last call -- N, K, n_gt, n_eq and the bits of ``tau`` -- so the
    kept fraction K / N can be logged without a synchronisation; ``values`` its per-element values (-1 at a void element) and
    ``terms`` its per-group terms.  Device tensors only; nothing synchronises; the scratch of a geometry (histograms, counts, slots)
    is kept and the per-call tensors (values, selection, terms, loss, gradient) come from torch's caching allocator, so nothing is
    allocated on the device after the first call of a geometry.  The scratch is per geometry, not per stream: use from two streams
    at once needs one HardPixelLoss object per stream.  No float atomics: loss, selection and gradient are bit-identical from call
    to call in either deterministic mode.
    Deliberate difference from torch: a group without a valid element contributes 0, the loss is never NaN for finite logits, and
    every void position and every unselected element has gradient +0.  Parity with nnU-Net's or mmsegmentation's code is not pinned
    by the tests (neither is a dependency); the formulas of ``include/hard/lmnet_hard.h`` are.
    Limits: B <= 65535, B * C * H * W < 2^31, and with ``per_image`` at most 1024 images (every group owns three histograms of the
    scratch)."""

    def __init__(self, n_classes, head="softmax", keep=None, min_kept=0, thresh=None, weight=None, per_image=False, scale=1.0):
        super().__init__()
        self.keep, self.min_kept, self.thresh, weight = _hard_config("HardPixelLoss", n_classes, head, keep, min_kept, thresh, weight)
        self.register_buffer("weight", weight)
        self.n_classes, self.head, self.per_image = int(n_classes), head, bool(per_image)
        self.scale = float(scale)
        self.selection = self.values = self.terms = None
        self._scratch = {}

    def forward(self, logits, target):
        _check_scale("HardPixelLoss", self.scale)
        logits, target = _hard_check("HardPixelLoss", self.n_classes, self.head, self.per_image, logits, target)
        B, Cn, H, W = logits.shape
        ws = _scratch(self, logits, lambda: _hard_workspace(logits.device, self.head, self.per_image, B, Cn, H, W))
        if self.weight is not None and self.weight.device != logits.device:
            self.weight = self.weight.to(logits.device)
        cfg = (_HARD_HEADS[self.head], self.per_image, self.keep, self.min_kept, hip.hard_cut(self.thresh), self.scale, self.weight, ws, self)
        return _HardFn.apply(logits, target, cfg)


def hard_pixel_values(logits, target, n_classes, head="softmax", weight=None, per_image=False, keep=None, min_kept=0, thresh=None):
    """``(values, selection)`` of ``HardPixelLoss``: ``values`` fp32, the per-element value in the layout of the logits' elements
    (``[B, H, W]`` under a softmax head), -1 at a void element, and ``selection`` int32 ``[G, 5]`` -- N, K, n_gt, n_eq and the bits
    of the K-th largest value ``tau`` of every group -- for monitoring the kept fraction or the cutoff without a synchronisation.
    The arguments are those of ``HardPixelLoss``; fresh tensors are returned.  Device tensors only; nothing synchronises."""
    what = "hard_pixel_values"
    keep, min_kept, thresh, weight = _hard_config(what, n_classes, head, keep, min_kept, thresh, weight)
    logits, target = _hard_check(what, int(n_classes), head, bool(per_image), logits.detach(), target)
    B, Cn, H, W = logits.shape
    ws = _hard_workspace(logits.device, head, bool(per_image), B, Cn, H, W)
    values, selection, terms, loss = _hard_outputs(logits, head, bool(per_image))
    hip.hard_fwd(logits, target, _HARD_HEADS[head], bool(per_image), keep, min_kept, hip.hard_cut(thresh), 1.0,
                 None if weight is None else weight.to(logits.device), ws, values, selection, terms, loss)
    return values, selection

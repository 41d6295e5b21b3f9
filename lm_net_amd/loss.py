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

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

"""lm_net_amd -- MI355X-native (gfx950) implementation of the LM-Net forward/backward hot path.

    from lm_net_amd import LM_Net          # drop-in for ``from core.LM_Net import LM_Net``

Around the path (SURVEY.md section 8f "next" rows): ``lm_net_amd.loss.SegLoss`` (fused CE + Dice, void labels, focal term;
``FocalLoss``), ``lm_net_amd.metrics.ImageStatsMeter`` (per-image tp / fp / fn / tn and the metric set built on them),
``lm_net_amd.loss.SigmoidSegLoss`` and ``lm_net_amd.metrics.SigmoidStatsMeter`` (BCE + Dice + focal and the thresholded statistics of
one-logit and multi-label sigmoid heads), ``lm_net_amd.metrics.CurveMeter`` (ROC, precision-recall, AUROC, average precision and the
best threshold of any thresholded metric from on-device score histograms),
``lm_net_amd.loss.BoundaryLoss`` / ``HausdorffDTLoss`` (boundary and distance-transform Hausdorff losses on exact signed distance
maps made on the device at every step; ``lm_net_amd.loss.distance_maps``),
``lm_net_amd.loss.LovaszLoss`` (the Lovasz-Softmax loss and the Lovasz hinge, the convex surrogate of the Jaccard index, on a stable
segmented device sort; ``lm_net_amd.loss.lovasz_ranks``),
``lm_net_amd.loss.RegionLoss`` (Dice, Jaccard, Tversky / focal Tversky and generalized Dice, per batch or per image, from one sums
pass; ``lm_net_amd.loss.region_sums``),
``lm_net_amd.loss.SoftSegLoss`` / ``DistillLoss`` (cross entropy + Dice against a distribution per pixel and the distillation term
against a teacher's logits) with ``lm_net_amd.data.DeviceMix`` (Mixup / CutMix of a device batch; ``MixedTarget``),
``lm_net_amd.loss.HardPixelLoss`` (top-k and OHEM cross entropy: the hardest pixels only, selected by an exact device radix select
with the count formed on the device; ``lm_net_amd.loss.hard_pixel_values``),
``lm_net_amd.optim.FusedAdamW`` (one-launch AdamW; parameter groups, gradient clipping, the GradScaler skip and an EMA of the weights
without a host decision; ``lm_net_amd.optim.decay_groups``), ``lm_net_amd.metrics.ConfusionMeter`` (on-device Dice / IoU),
``lm_net_amd.metrics.SurfaceDistanceMeter`` (on-device HD / HD95 / ASSD / RVD),
``lm_net_amd.metrics.VolumeSurfaceMeter`` (per-case 3D Dice / HD / HD95 / ASSD / RVD of a label volume with integer voxel pitches),
``lm_net_amd.metrics.LesionMeter`` (per-lesion detection, lesion-wise F1 and panoptic quality: the join of the 3D components of prediction
and target in a device hash table),
``lm_net_amd.post.DevicePostprocess`` (on-device arg-max, connected-component cleaning, resize back to the frame, overlay),
``lm_net_amd.post.VolumePostprocess`` (3D connected-component cleaning of a whole case: the n largest components of an organ, a minimal
volume, cavity filling, between the prediction and ``VolumeSurfaceMeter``),
``lm_net_amd.data.VolumeSlicer`` (the input side of a CT / MR case: int16 volumes to windowed, z-scored 2.5D fp32 batches on the device),
``lm_net_amd.infer.TiledPredictor`` (frames of any size: overlapping tiles, mirrored copies and one blend launch),
``lm_net_amd.ddp.DistributedLMNet`` (bucketed RCCL gradient all-reduce).
"""
from .LM_Net import LM_Net  # noqa: F401
from .data import DeviceMix, VolumeSlicer  # noqa: F401
from .loss import (BoundaryLoss, DistillLoss, FocalLoss, HardPixelLoss, HausdorffDTLoss, LovaszLoss, MixedTarget, RegionLoss,  # noqa: F401
                   SegLoss, SigmoidSegLoss, SoftSegLoss, distance_maps, hard_pixel_values, lovasz_ranks, region_sums)
from .metrics import CurveMeter, ImageStatsMeter, LesionMeter, SigmoidStatsMeter, VolumeSurfaceMeter  # noqa: F401
from .post import VolumePostprocess  # noqa: F401

__all__ = ["LM_Net", "SegLoss", "FocalLoss", "ImageStatsMeter", "SigmoidSegLoss", "SigmoidStatsMeter", "CurveMeter", "VolumeSurfaceMeter", "VolumePostprocess",
           "LesionMeter", "BoundaryLoss", "HausdorffDTLoss", "distance_maps", "LovaszLoss", "lovasz_ranks", "RegionLoss",
           "region_sums", "VolumeSlicer", "SoftSegLoss", "DistillLoss", "MixedTarget", "DeviceMix",
           "HardPixelLoss", "hard_pixel_values"]

"""The subjects of the busy-stream tests (tests/busy.py) of the hard-pixel criterion: HardPixelLoss under both heads, in its top-k and
its OHEM form, per batch and per image, and hard_pixel_values.  Three valid inputs A, B, C of the geometry of tests/busy_cases.py and
the reference of each from tests/hard_ref.py; importable without a GPU (tests/test_hard_cpu.py runs busy.check_discrimination on
them).  The bounds are those of tests/test_hard_kernels_gpu.py: 1e-5 |ref| for the loss, 1e-4 max |ref| for the gradient taken on the
device's own selection, hard_ref.VALUES_BAR * max(1, l) per value; the selection record must be EQUAL to numpy's on the device's own
values."""
import numpy as np

import busy_cases as K
import hard_ref as R
from busy import Subject  # noqa: F401

CONFIGS = {
    "HardPixelLoss-softmax-keep": dict(head="softmax", keep=0.1, weight=K.W_CE, scale=0.5),
    "HardPixelLoss-softmax-ohem-per_image": dict(head="softmax", thresh=0.7, min_kept=500, per_image=True),
    "HardPixelLoss-sigmoid-keep-per_image": dict(head="sigmoid", keep=0.25, per_image=True),
    "HardPixelLoss-sigmoid-ohem": dict(head="sigmoid", thresh=0.6, min_kept=1000, weight=K.W_DICE),
}
NAMES = sorted(CONFIGS)
VALUES_NAME = "hard_pixel_values-softmax"
VALUES_CONFIG = dict(head="softmax", keep=0.1, per_image=True)


def _outputs(r, kw, got):
    """values (-1 at a void element) and the record: numpy's selection on the device's own values, or float64's own without them"""
    vals = np.where(r.valid, r.values, -1.0)
    bar = np.where(r.valid, R.VALUES_BAR * np.maximum(1.0, r.values), 0.0)
    sel = {k: kw.get(k) for k in ("keep", "thresh")}
    src = got[-2] if got is not None else vals.astype(np.float32)
    rec = R.record_of(src, r.valid, kw.get("per_image", False), min_kept=kw.get("min_kept", 0), **sel)
    return [("values", vals, bar), ("selection", rec, None)]


def _criterion(name):
    kw = CONFIGS[name]

    def ref(arrays, got=None):
        r = R.loss_and_grad(arrays[0], arrays[1], K.C, device=None if got is None else (got[2], got[3]), **kw)
        return K._loss_grad(r.loss, r.grad) + _outputs(r, kw, got)
    target = (lambda k: K.label_map(k, void=True, dtype=np.uint8)) if kw["head"] == "softmax" else (lambda k: K.planes(k, void=True))
    return K._subject(name, lambda k: [K.logits(k), target(k)], ref, exact=True, no_growth=True)


def _values():
    def ref(arrays, got=None):
        r = R.loss_and_grad(arrays[0], arrays[1], K.C, **VALUES_CONFIG)
        return _outputs(r, VALUES_CONFIG, got)
    return K._subject(VALUES_NAME, lambda k: [K.logits(k), K.label_map(k, void=True, dtype=np.uint8)], ref, exact=True)


def subjects():
    out = [_criterion(n) for n in NAMES] + [_values()]
    return {s.name: s for s in out}

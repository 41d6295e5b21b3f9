"""The subjects of the busy-stream tests (tests/busy.py) of the soft-target classes: SoftSegLoss under both readers, DistillLoss under
both heads and both teacher types, DeviceMix.  Three valid inputs A, B, C of the geometry of tests/busy_cases.py and the reference of
each from tests/soft_ref.py; importable without a GPU (tests/test_soft_cpu.py runs busy.check_discrimination on them).  The bounds are
those of tests/test_soft_kernels_gpu.py: 1e-5 |ref| for the loss (1e-5 * magnitude for the distillation term), 1e-4 max |ref| for the
gradient; the mixer's outputs must be EQUAL."""
import numpy as np

import busy_cases as K
import soft_ref as R
from busy import Subject

T = 2.0
SEG = dict(w_ce=(1.0, 2.0, 0.5, 1.5), w_dice=(1.0, 0.5, 2.0, 1.5), eps=0.1)
NAMES = ["SoftSegLoss-probs", "SoftSegLoss-pair", "DistillLoss-softmax-f32", "DistillLoss-softmax-bf16", "DistillLoss-sigmoid-f32",
         "DistillLoss-sigmoid-bf16"]
MIX_NAME = "DeviceMix"


def probs(case):
    """unnormalised fp32 probabilities with void pixels (NaN)"""
    rng = K._rng(case, 7)
    q = (rng.random((K.B, K.C, K.H, K.W)) ** 2 * np.asarray(K._PROBS[case], np.float64)[None, :, None, None]).astype(np.float32)
    q[:, 0][rng.random((K.B, K.H, K.W)) < K._VOID[case]] = np.nan
    return q


def teacher(case, bf16):
    zt = (K.logits(case) + K._SCALE[case] * K._rng(case, 8).standard_normal((K.B, K.C, K.H, K.W))).astype(np.float32)
    return R.bf16_round(zt) if bf16 else zt


def lam(case):
    return (np.asarray([0.3, 0.8], np.float32) * np.float32({"A": 1.0, "B": 0.5, "C": 0.25}[case])).astype(np.float32)


def _seg(reader):
    def ref(arrays, got=None):
        if reader == "probs":
            r = R.SimpleNamespace(lg=arrays[0], q=arrays[1])
        else:
            r = R.SimpleNamespace(lg=arrays[0], ya=arrays[1], yb=arrays[2], lam=arrays[3])
        out = R.loss_and_grad(r, reader, **SEG)
        return K._loss_grad(out.loss, out.grad)
    if reader == "probs":
        make = lambda k: [K.logits(k), probs(k)]
    else:
        make = lambda k: [K.logits(k), K.label_map(k, void=True, dtype=np.uint8), K.label_map(k, void=True, dtype=np.uint8)[::-1].copy(), lam(k)]
    return K._subject("SoftSegLoss-%s" % reader, make, ref, no_growth=True)


def _distill(head, bf16):
    def ref(arrays, got=None):
        out = R.distill(arrays[0], arrays[1], head, arrays[2], T)
        return K._loss_grad(out.loss, out.grad, loss_scale=out.magnitude)
    valid = (lambda k: K.label_map(k, void=True, dtype=np.uint8)) if head == "softmax" else (lambda k: K.planes(k, void=True))
    return K._subject("DistillLoss-%s-%s" % (head, "bf16" if bf16 else "f32"), lambda k: [K.logits(k), teacher(k, bf16), valid(k)], ref, no_growth=True)


def mix_rows(case):
    """row 0: Mixup with the case's lam, row 1: CutMix with the case's box"""
    from lm_net_amd import hip
    y0 = {"A": 0, "B": 5, "C": 17}[case]
    return hip.mix_rows([1, 0], [R.MIXUP, R.CUTMIX], lam(case), [(0, 0, 0, 0), (y0, 3, y0 + 20, 47)])


def device_mix():
    def ref(arrays, got=None, host=None):
        return [(name, a, None) for name, a in zip(("x_out", "ya", "yb", "lam"), R.mix(arrays[0], arrays[1], host))]
    s = K._subject(MIX_NAME, lambda k: [K.logits(k, 3), K.label_map(k, void=True, dtype=np.uint8)], ref, exact=True, no_growth=True)
    s.host = {k: mix_rows(k) for k in K.CASES}
    return s


def subjects():
    out = [_seg("probs"), _seg("pair")] + [_distill(h, b) for h in ("softmax", "sigmoid") for b in (False, True)] + [device_mix()]
    return {s.name: s for s in out}

"""tests/golden/soft_ref.npz from the REAL reference code (build container only, where the reference tree exists): DiceLoss._dice_loss
of utils/loss.py (lines 183-191) applied to FLOAT targets -- the Dice term of lm_net_amd.loss.SoftSegLoss -- on float64 copies of the
inputs of tests/soft_ref.py::inputs(3, C, 5, 7, reader, seed=11 + C, void=0.2) at C = 2 and 4 under the probability reader and the
Mixup-pair reader: per class the method is called on softmax(z)[:, c], q[:, c] and the mask of the void pixels, the results are
weighted and averaged over the classes as DiceLoss.forward does.

The reference casts the target to fp32 and sums its squares in fp32, so the golden's targets are made multiples of 1 / 8 (q under
the probability reader, lam under the pair reader): cast, products and sums are then exact and the float64 restatement can be held to
1e-12.

The module is loaded the way tools/make_golden_region.py loads it (tests/void_ref.py::reference_modules).  The inputs are a recipe,
so only the expected numbers are stored: the Dice term (float64) and its d / d logits (float64)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import soft_ref as R  # noqa: E402
import void_ref as V  # noqa: E402


def weights(C):
    return [1.0 + 1.5 * k for k in range(C)]


def case(C, reader):
    """(inputs, q float64 with 0 at void pixels, valid) of one golden case"""
    r = R.inputs(3, C, 5, 7, reader, seed=11 + C, void=0.2)
    if reader == "probs":
        r.q = (np.round(r.q * 8) / 8).astype(np.float32)          # (NaN and -1 stay what they are)
    else:
        r.lam = (np.round(r.lam * 8) / 8).astype(np.float32)
    if reader == "probs":
        valid = R.probs_valid(r.q)
        q = np.where(valid[:, None], r.q.astype(np.float64), 0.0)
    else:
        q, valid = R.pair_q(r.ya, r.yb, r.lam, C)
    return r, q, valid


def compute():
    """{name: array} of the golden, from the reference tree"""
    ref_loss, _ = V.reference_modules()
    out = {}
    for C in (2, 4):
        for reader in ("probs", "pair"):
            r, q, valid = case(C, reader)
            crit = ref_loss.DiceLoss(C)
            z = torch.from_numpy(r.lg).double().requires_grad_(True)
            p = torch.softmax(z, 1)
            ignore = torch.from_numpy(~valid)
            loss = sum(crit._dice_loss(p[:, c], torch.from_numpy(q[:, c]), ignore) * w for c, w in enumerate(weights(C))) / C
            loss.backward()
            out["dice_%s/%d/loss" % (reader, C)] = np.array([float(loss.detach())])
            out["dice_%s/%d/dlogits" % (reader, C)] = z.grad.numpy()
    return out


def main():
    out = compute()
    path = os.path.join(ROOT, "tests", "golden", "soft_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), {k: v.tolist() for k, v in out.items() if v.size <= 4})


if __name__ == "__main__":
    main()

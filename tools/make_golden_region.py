"""tests/golden/region_ref.npz from the REAL reference code (build container only, where the reference tree exists): the three Dice
classes of utils/loss.py on float64 copies of the inputs of tests/region_ref.py::inputs(3, C, 5, 7, seed=11 + C) at C = 2 and 4:

  * DiceLoss with class weights, without void labels ("dice") and with 20 % void labels passed as its `ignore` mask ("dice_void");
  * BCEDiceLoss (0.4 CE + 0.6 (1 - dice), the Dice per (image, class) with the linear denominator and e = 1e-7), without void labels;
  * offical_DiceLoss (a per-sample squared Dice with smooth = 1, summed over the batch), without void labels: its denominator ignores
    the valid mask, a quirk the package does not reproduce.

The module is loaded the way tools/make_golden_void.py loads it (tests/void_ref.py::reference_modules).  The inputs are a recipe, so
only the expected numbers are stored: the loss (float64) and d loss / d logits (float64)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import region_ref as R  # noqa: E402
import void_ref as V  # noqa: E402


def weights(C):
    return [1.0 + 1.5 * k for k in range(C)]


def compute():
    """{name: array} of the golden, from the reference tree"""
    ref_loss, _ = V.reference_modules()
    out = {}
    for C in (2, 4):
        for tag, void in (("", 0.0), ("_void", 0.2)):
            lg, y = R.inputs(3, C, 5, 7, seed=11 + C, void=void)
            yt = torch.from_numpy(y)
            cases = {"dice" + tag: lambda z: ref_loss.DiceLoss(C)(z, yt.unsqueeze(1).float(), weight=weights(C), ignore=(yt == R.VOID))}
            if not void:
                cases["bcedice"] = lambda z: ref_loss.BCEDiceLoss(n_classes=C)(z, yt)
                cases["offical"] = lambda z: ref_loss.offical_DiceLoss()(z, yt)
            for name, fn in cases.items():
                z = torch.from_numpy(lg).double().requires_grad_(True)
                loss = fn(z)
                loss.backward()
                out["%s/%d/loss" % (name, C)] = np.array([float(loss.detach())])
                out["%s/%d/dlogits" % (name, C)] = z.grad.numpy()
    return out


def main():
    out = compute()
    path = os.path.join(ROOT, "tests", "golden", "region_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), {k: v.tolist() for k, v in out.items() if v.size <= 4})


if __name__ == "__main__":
    main()

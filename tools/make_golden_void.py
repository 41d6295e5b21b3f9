"""tests/golden/void_loss_stats.npz from the REAL reference code (build container only, where the reference tree exists):

  * utils/loss.py::DiceLoss with its `ignore` mask plus F.cross_entropy(weight, label_smoothing, ignore_index=255) at C = 2 and 9 with
    20 % void pixels: loss value (float64) and d loss / d logits (stored as float32);
  * utils/loss.py::FocalLoss at C = 3 without void labels.  torchvision is not installed here: the module's import of
    torchvision.ops.focal_loss.sigmoid_focal_loss is served by tests/void_ref.py::sigmoid_focal_loss, written from torchvision's
    documented formula -- parity with torchvision's own code is therefore NOT pinned by this golden;
  * utils/functional.py::get_stats(mode="multiclass", ignore_index=255) on argmax(logits) at C in {2, 4, 5, 64}, and every metric
    function of that file under every reduction: once on float64 copies of the statistics ("s64/...": float64 throughout) and once
    on the int64 statistics as the reference's callers pass them ("s32/...": its arithmetic is then float32).

Inputs are tools/detweights recipes built by tests/void_ref.py (loss_case, stats_case), so only the expected numbers are stored."""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import void_ref as V  # noqa: E402


def main():
    ref_loss, ref_fn = V.reference_modules()
    out = {}
    for tag in ("k2", "k9", "f3"):
        lg, y, wce, wdice, kw = V.loss_case(tag)
        l64 = lg.double().requires_grad_(True)
        if tag == "f3":
            loss = ref_loss.FocalLoss(num_classes=lg.shape[1])(l64, y)
        else:
            loss = V.reference_loss(ref_loss, l64, y, wce, wdice, kw["eps"], kw["ignore_index"])
        loss.backward()
        out["%s/loss" % tag] = np.array([float(loss.detach())])
        out["%s/dlogits" % tag] = l64.grad.float().numpy()
    for C in V.STATS_C:
        lg, y = V.stats_case(C)
        pred = lg.argmax(1)
        tp, fp, fn, tn = ref_fn.get_stats(pred, y, mode="multiclass", ignore_index=255, num_classes=C)
        out["stats/%d" % C] = torch.stack([tp, fp, fn, tn], -1).numpy().astype(np.int64)
        cw = V.stats_class_weights(C)
        for prec, conv in (("s64", lambda t: t.double()), ("s32", lambda t: t)):
            vals = []
            for m in V.METRICS:
                name, kw = V.REFERENCE_NAMES.get(m, (m, {}))
                for r in V.REDUCTIONS:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        v = getattr(ref_fn, name)(conv(tp), conv(fp), conv(fn), conv(tn), reduction=r,
                                                  class_weights=cw if "weighted" in r else None, **kw)
                    vals.append(float(v))
            out["%s/%d" % (prec, C)] = np.array(vals, dtype=np.float64).reshape(len(V.METRICS), len(V.REDUCTIONS))
    path = os.path.join(ROOT, "tests", "golden", "void_loss_stats.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), {k: v.tolist() for k, v in out.items() if v.size <= 4})


if __name__ == "__main__":
    main()

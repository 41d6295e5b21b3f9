"""Goldens of LM_Net at other input-channel / class counts, from the REAL reference in float64 (build container only):

  * train steps, in the format of tools/make_golden_wide.py (per parameter [max|g|, ||g||_2] and 128 sampled elements, up to 32768
    sampled logits, the input gradient's digest and sample, the BatchNorm running statistics after the step; samples as float32):

        python tools/make_golden_multiclass.py step 1 9 64 2 5   -> tests/golden/mc_c1_k9_64_b2.npz
        python tools/make_golden_multiclass.py all               -> every fixture tests/test_multiclass_model_gpu.py reads

  * loss and metrics at C = 9 and C = 33 (tests/golden/mc_loss_metrics.npz): utils/loss.py::DiceLoss(C)(..., weight) +
    nn.CrossEntropyLoss(weight, label_smoothing) (the loss of utils/train_eval_utils.py:141) with its d loss / d logits, and the
    reference Evaluator's metrics (utils/train_eval_utils.py:55-118) on argmax(logits), labels outside [0, C) included.

Weights / inputs: tools/detweights.py (seed, key names) -- nothing but the recipe and the expected numbers is stored.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.detweights import det_input, fill_module, uniform  # noqa: E402
from tools.make_golden_f64 import sample_index  # noqa: E402

STEPS = [(1, 2, 64, 2, 5), (1, 9, 64, 2, 5), (4, 4, 64, 2, 5), (3, 14, 64, 2, 5), (1, 9, 352, 2, 5)]
LOSS_CASES = {"k9": (9, 2, 40, 56, 3.0), "k33": (33, 2, 24, 40, 2.0)}


def step_key(channel, n_classes, size, B):
    return "mc_c%d_k%d_%d_b%d" % (channel, n_classes, size, B)


def class_labels(B, H, W, C, key):
    """Labels in [0, C) from the detweights stream."""
    u = uniform(key, B * H * W)
    return torch.from_numpy(np.minimum((u * C).astype(np.int64), C - 1).reshape(B, H, W))


def make_step(channel, n_classes, size, B, seed):
    from tools.ref_import import import_reference_lmnet
    LM_Net = import_reference_lmnet()
    m = LM_Net(channel, n_classes)
    fill_module(m, seed)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    m = m.double().train()
    key = step_key(channel, n_classes, size, B)
    x = det_input((B, channel, size, size), key + "/x").double().requires_grad_(True)
    t0 = time.time()
    y = m(x)
    G = det_input(tuple(y.shape), key + "/G").double()
    (y * G).sum().backward()
    print("%s: reference fp64 step %.1f s" % (key, time.time() - t0), flush=True)
    yf = y.detach().flatten()
    out = {"logits/stat": np.array([yf.abs().max().item(), yf.norm().item()]),
           "logits/sample": yf[torch.from_numpy(sample_index(yf.numel(), 32768))].float().numpy(),
           "meta": np.array([size, B, seed, channel, n_classes], dtype=np.int64)}
    gx = x.grad.detach().flatten()
    out["gx/stat"] = np.array([gx.abs().max().item(), gx.norm().item()])
    out["gx/sample"] = gx[torch.from_numpy(sample_index(gx.numel()))].float().numpy()
    for k, p in m.named_parameters():
        g = p.grad.detach().flatten()
        out["gstat/" + k] = np.array([g.abs().max().item(), g.norm().item()])
        out["gsamp/" + k] = g[torch.from_numpy(sample_index(g.numel()))].float().numpy()
    for k, v in m.state_dict().items():
        if "running_" in k:
            out["state/" + k] = v.detach().float().numpy()
    path = os.path.join(ROOT, "tests", "golden", key + ".npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))


def make_loss_metrics():
    from tools.make_golden_loss import _stub
    for n in ("torchvision", "torchvision.ops"):
        _stub(n)
    _stub("torchvision.ops.focal_loss", sigmoid_focal_loss=None)
    _stub("cv2")
    _stub("skimage")
    _stub("skimage.metrics", hausdorff_distance=None)
    _stub("sklearn")
    _stub("sklearn.metrics", accuracy_score=None, precision_score=None, recall_score=None, f1_score=None)
    _stub("tqdm", tqdm=lambda x, **k: x)
    from tools.ref_import import REFERENCE_ROOT
    sys.path.insert(0, REFERENCE_ROOT)
    from utils.loss import DiceLoss                      # noqa: E402  (the reference's class)
    from utils.train_eval_utils import Evaluator          # noqa: E402
    out = {}
    for tag, (C, B, H, W, scale) in LOSS_CASES.items():
        lg = (det_input((B, C, H, W), "mc_loss/%s" % tag) * scale).double().requires_grad_(True)
        y = class_labels(B, H, W, C, "mc_loss/%s/y" % tag)
        wce = torch.from_numpy(0.5 + uniform("mc_loss/%s/wce" % tag, C)).double()
        wdice = torch.from_numpy(0.5 + 2 * uniform("mc_loss/%s/wdice" % tag, C)).double()
        ce = torch.nn.CrossEntropyLoss(weight=wce, label_smoothing=0.001)
        loss = ce(lg, y) + DiceLoss(C)(lg, y.unsqueeze(1).float(), weight=wdice.tolist())     # train_eval_utils.py:141
        loss.backward()
        out["%s/meta" % tag] = np.array([C, B, H, W, scale])
        out["%s/wce" % tag] = wce.float().numpy()
        out["%s/wdice" % tag] = wdice.float().numpy()
        out["%s/loss" % tag] = np.array([loss.item()])
        out["%s/dlogits" % tag] = lg.grad.float().numpy()
        # the Evaluator on argmax(logits), with some labels outside [0, C) (dropped by _generate_matrix)
        gt = y.numpy().copy()
        gt.reshape(-1)[::97] = 255
        gt.reshape(-1)[5::89] = -1
        ev = Evaluator(C)
        ev.add_batch(gt, lg.detach().argmax(1).numpy())
        out["%s/labels" % tag] = gt.astype(np.int16)
        out["%s/confusion" % tag] = np.asarray(ev.confusion_matrix, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            for name in ("Accuracy", "Mean_Accuracy", "Mean_Recall", "Precision", "Recall", "Specificity", "Dice", "Mean_Dice",
                         "Mean_Intersection_over_Union", "Frequency_Weighted_Intersection_over_Union"):
                out["%s/ev/%s" % (tag, name)] = np.array([float(getattr(ev, name)())])
    path = os.path.join(ROOT, "tests", "golden", "mc_loss_metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path))


def main():
    torch.set_num_threads(8)
    if sys.argv[1:] == ["all"]:
        for fx in STEPS:
            make_step(*fx)
        make_loss_metrics()
    elif sys.argv[1] == "loss":
        make_loss_metrics()
    else:
        make_step(*(int(v) for v in sys.argv[2:7]))


if __name__ == "__main__":
    main()

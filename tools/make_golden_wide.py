"""Gradient goldens of the WIDE LM_Net variants from the REAL reference run in float64 (build container only), in the format of
tools/make_golden_f64.py (per parameter [max|g|, ||g||_2] and 128 sampled elements, up to 32768 sampled logits, the input gradient's
digest and sample, the BatchNorm running statistics after the step).  The sampled values are stored as float32 (the stats stay
float64): the checks are relative to a tensor's largest element at 1e-4 and looser, far above float32 rounding, and it keeps each
fixture under 1 MB at 4x the default width):

    python tools/make_golden_wide.py W2 64 2 5      -> tests/golden/wide_W2_64_b2.npz
    python tools/make_golden_wide.py all            -> the five fixtures tests/test_wide_model_gpu.py reads

Widths: W2 [24,48,96,192,384], W3 [36,72,144,288,576], W4 [48,96,192,384,768], Wodd [12,36,60,84,120].  Weights / inputs:
tools/detweights.py (seed, key names) -- nothing but the recipe and the expected numbers is stored.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.detweights import det_input, fill_module  # noqa: E402
from tools.make_golden_f64 import sample_index  # noqa: E402

WIDE = {
    "W2": [24, 48, 96, 192, 384],
    "W3": [36, 72, 144, 288, 576],
    "W4": [48, 96, 192, 384, 768],
    "Wodd": [12, 36, 60, 84, 120],
}
FIXTURES = [("W2", 64, 2, 5), ("W3", 64, 2, 5), ("W4", 64, 2, 5), ("Wodd", 64, 2, 5), ("W2", 352, 2, 5)]


def key_of(name, size, B):
    return "wide_%s_%d_b%d" % (name, size, B)


def make(name, size, B, seed):
    from tools.ref_import import import_reference_lmnet
    LM_Net = import_reference_lmnet()
    m = LM_Net(3, 2, filters=WIDE[name])
    fill_module(m, seed)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    m = m.double().train()
    key = key_of(name, size, B)
    x = det_input((B, 3, size, size), key + "/x").double().requires_grad_(True)
    t0 = time.time()
    y = m(x)
    G = det_input(tuple(y.shape), key + "/G").double()
    (y * G).sum().backward()
    print("%s: reference fp64 step %.1f s" % (key, time.time() - t0), flush=True)
    yf = y.detach().flatten()
    out = {"logits/stat": np.array([yf.abs().max().item(), yf.norm().item()]),
           "logits/sample": yf[torch.from_numpy(sample_index(yf.numel(), 32768))].float().numpy(),
           "meta": np.array([size, B, seed], dtype=np.int64),
           "filters": np.array(WIDE[name], dtype=np.int64)}
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


def main():
    torch.set_num_threads(8)
    if sys.argv[1:] == ["all"]:
        for fx in FIXTURES:
            make(*fx)
    else:
        make(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))


if __name__ == "__main__":
    main()

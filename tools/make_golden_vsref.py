"""tests/golden/vsref_48x64.npz from the REAL reference (build container only; same import path as tools/make_golden.py).

LM_Net(3, 2) with the tools/detweights.py weights of seed 3 on the input recipe "vsref/x" (2x3x48x64): the eval-mode logits and
the train-mode logits (batch-stat BatchNorm, dropout off).  tests/test_oracle_vs_reference.py compares the oracle against them, so
the comparison runs wherever the repository does.  Only the expected outputs are stored; weights and input are regenerated from
their recipes.

    python tools/make_golden_vsref.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.detweights import det_input, fill_module  # noqa: E402
from tools.make_golden import GOLD  # noqa: E402
from tools.ref_import import import_reference_lmnet  # noqa: E402


def main():
    Ref = import_reference_lmnet()
    torch.set_num_threads(8)
    r = Ref(3, 2)
    fill_module(r, seed=3)
    x = det_input((2, 3, 48, 64), "vsref/x")
    r.eval()
    with torch.no_grad():
        y_eval = r(x)
    for m in r.modules():                 # every dropout-like probability to 0 (nn.Dropout and modules with a float `p`)
        if hasattr(m, "p") and isinstance(getattr(m, "p"), float):
            m.p = 0.0
    r.train()
    y_train = r(x).detach()
    out = {"eval_logits": y_eval.numpy().astype(np.float32), "train_logits": y_train.numpy().astype(np.float32)}
    path = os.path.join(GOLD, "vsref_48x64.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), {k: float(np.abs(v).max()) for k, v in out.items()})


if __name__ == "__main__":
    main()

"""CPU: oracle vs the real reference's logits at 2x3x48x64, eval and train mode (tests/golden/vsref_48x64.npz, made by
tools/make_golden_vsref.py from the reference run on CPU)."""
import torch

from tools.detweights import det_input, fill_module
from helpers import load_golden, no_dropout, rel_err


def test_eval_and_train_forward_match_reference():
    from oracle.lmnet_ref import LM_Net
    g = load_golden("vsref_48x64.npz")
    o = LM_Net(3, 2)
    fill_module(o, seed=3)
    x = det_input((2, 3, 48, 64), "vsref/x")
    o.eval()
    with torch.no_grad():
        assert rel_err(o(x), g["eval_logits"]) < 1e-5
    no_dropout(o)
    o.train()
    assert rel_err(o(x), g["train_logits"]) < 1e-5

"""CPU: the channel / class envelope of the HIP path (lm_net_amd.LM_Net.envelope_error, README "Input channels and classes"), the
ABI 15 entry point of the grayscale / class-id input pipeline, the host-side pieces of SegLoss, ConfusionMeter and DevicePreprocess
at other class / channel counts, and the oracle against the real reference at (channel, n_classes) = (1, 9) and (4, 4) (skipped when
the reference tree is not importable)."""
import math

import numpy as np
import pytest
import torch

from helpers import load_golden, no_dropout
from tools.detweights import det_input, fill_module


@pytest.mark.parametrize("channel, n_classes", [(1, 1), (1, 2), (1, 9), (3, 2), (4, 4), (3, 14), (16, 64), (16, 1)])
def test_envelope_accepts(channel, n_classes):
    from lm_net_amd.LM_Net import envelope_error
    assert envelope_error([12, 24, 48, 96, 192], 3, channel, n_classes) is None
    assert envelope_error([24, 48, 96, 192, 384], 3, channel=channel, n_classes=n_classes) is None


@pytest.mark.parametrize("kw, words", [
    (dict(channel=0), ["channel = 0", "1 <= channel <= 16"]),
    (dict(channel=17), ["channel = 17", "1 <= channel <= 16"]),
    (dict(n_classes=0), ["n_classes = 0", "1 <= n_classes <= 64"]),
    (dict(n_classes=65), ["n_classes = 65", "1 <= n_classes <= 64"]),
])
def test_envelope_rejects_with_named_limit(kw, words):
    from lm_net_amd.LM_Net import envelope_error
    msg = envelope_error([12, 24, 48, 96, 192], **kw)
    assert msg is not None
    for w in words:
        assert w in msg, (w, msg)


def test_envelope_defaults_unchanged():
    """The keyword arguments default to the 3-channel, 2-class model: existing two-argument calls keep their answers."""
    from lm_net_amd.LM_Net import envelope_error
    assert envelope_error([12, 24, 48, 96, 192]) is None
    assert "396" in envelope_error([12, 24, 48, 396, 192])
    # the filters limits still apply at other channel / class counts
    assert "396" in envelope_error([12, 24, 48, 396, 192], 3, 1, 9)


def test_outside_envelope_still_constructs():
    from lm_net_amd import LM_Net
    m = LM_Net(17, 2)
    assert m.channel == 17
    m = LM_Net(3, 65)
    assert m.output_layer.weight.shape[0] == 65
    with pytest.raises(RuntimeError):                 # the device check stays first
        m(torch.zeros(1, 3, 64, 64))


def test_preprocess_ex_exported_and_abi_15():
    from lm_net_amd import hip
    assert hip.ABI_VERSION == 15
    assert "lmn_preprocess_u8_ex" in hip.SYMBOLS
    lib = hip.load()
    assert lib.lmn_abi_version() == 15
    assert hasattr(lib, "lmn_preprocess_u8_ex")


def test_device_preprocess_arguments():
    from lm_net_amd.data import DevicePreprocess
    p = DevicePreprocess((64, 64))
    assert p.channels == 3 and p.mask_mode == "binary"
    g = DevicePreprocess((64, 64), mean=(0.5,), std=(0.25,), channels=1, mask_mode="labels")
    assert g.channels == 1 and g.mask_mode == "labels"
    with pytest.raises(ValueError):
        DevicePreprocess((64, 64), channels=2)
    with pytest.raises(ValueError):
        DevicePreprocess((64, 64), channels=1)              # 3-channel mean / std for one channel
    with pytest.raises(ValueError):
        DevicePreprocess((64, 64), mask_mode="ids")
    with pytest.raises(RuntimeError, match="no CPU path"):
        g(torch.zeros(1, 8, 8, dtype=torch.uint8))


def test_segloss_default_weights_and_class_range():
    from lm_net_amd.loss import SegLoss
    crit = SegLoss(None, None)
    assert crit.ce_weight is None and crit.dice_weight is None
    w = crit._weight(None, 9, torch.device("cpu"), "ce")
    assert w.shape == (9,) and bool((w == 1).all())
    lg, y = torch.zeros(1, 65, 32, 32), torch.zeros(1, 32, 32, dtype=torch.int64)
    with pytest.raises(ValueError, match="2..64"):
        crit(lg, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # still no CPU path at a new class count
        crit(torch.zeros(1, 9, 32, 32), y)
    assert SegLoss().ce_weight.tolist() == [1.0, 4.0]              # the default stays


def test_evaluator_metrics_against_reference_golden():
    """lm_net_amd.metrics.evaluator_metrics on the reference Evaluator's own confusion matrices (C = 9, 33; labels 255 and -1
    dropped) against the values its methods returned (tests/golden/mc_loss_metrics.npz), NaN for NaN."""
    from lm_net_amd.metrics import ConfusionMeter, evaluator_metrics
    g = load_golden("mc_loss_metrics.npz")
    for tag in ("k9", "k33"):
        C = int(g[tag + "/meta"][0])
        cm = g[tag + "/confusion"]
        assert cm.shape == (C, C)
        r = evaluator_metrics(cm)
        for k, v in r.items():
            ref = float(g["%s/ev/%s" % (tag, k)][0])
            assert (math.isnan(v) and math.isnan(ref)) or abs(v - ref) < 1e-12, (tag, k, v, ref)
        m = ConfusionMeter(C, device="cpu")
        m.total += torch.from_numpy(cm)
        out = m.compute()
        assert abs(out["accuracy"] - float(g[tag + "/ev/Accuracy"][0])) < 1e-12
        for k in r:
            assert k in out
    with pytest.raises(ValueError):
        ConfusionMeter(65, device="cpu")


def test_evaluator_metrics_nan_handling():
    """A class that never occurs (row and column 0) is NaN in the per-class vectors and left out by nanmean."""
    from lm_net_amd.metrics import evaluator_metrics
    cm = np.array([[5.0, 1.0, 0.0], [2.0, 7.0, 0.0], [0.0, 0.0, 0.0]])
    r = evaluator_metrics(cm)
    assert abs(r["Mean_Dice"] - np.mean([10 / 13, 14 / 17])) < 1e-12
    assert abs(r["Mean_Intersection_over_Union"] - np.mean([5 / 8, 7 / 10])) < 1e-12
    assert abs(r["Frequency_Weighted_Intersection_over_Union"] - (6 / 15 * 5 / 8 + 9 / 15 * 7 / 10)) < 1e-12


@pytest.mark.parametrize("channel, n_classes", [(1, 9), (4, 4)])
def test_oracle_matches_reference_at_other_channels_and_classes(channel, n_classes):
    """oracle/lmnet_ref.py against the real reference (tools/ref_import.py) on the same name-keyed weights: same state_dict keys and
    shapes, logits equal to 1e-5 in eval and train (batch statistics)."""
    from tools.ref_import import import_reference_lmnet, reference_available
    if not reference_available():
        pytest.skip("reference tree not present")
    RefLMNet = import_reference_lmnet()
    from oracle.lmnet_ref import LM_Net as Oracle
    ref = RefLMNet(channel, n_classes)
    ora = Oracle(channel, n_classes)
    sr, so = ref.state_dict(), ora.state_dict()
    assert list(sr) == list(so)
    assert all(tuple(sr[k].shape) == tuple(so[k].shape) for k in sr)
    fill_module(ref, 3)
    fill_module(ora, 3)
    no_dropout(ref)
    no_dropout(ora)
    x = det_input((2, channel, 64, 64), "mc_cpu/x")
    for train in (False, True):
        ref.train(train)
        ora.train(train)
        with torch.no_grad():
            yr, yo = ref(x), ora(x)
        assert yr.shape == (2, n_classes, 64, 64)
        err = float((yr - yo).abs().max() / yr.abs().max())
        assert err < 1e-5, (channel, n_classes, train, err)


@pytest.mark.parametrize("channel, n_classes", [(1, 9), (4, 4)])
def test_oracle_train_step_matches_reference_golden(channel, n_classes):
    """The CPU oracle's fp32 train step against the float64 reference golden of tests/test_multiclass_model_gpu.py (logits only, at
    the fp32 rounding distance): pins the golden and the oracle to each other without a GPU."""
    from oracle.lmnet_ref import LM_Net as Oracle
    from tools.make_golden_f64 import sample_index
    key = "mc_c%d_k%d_64_b2" % (channel, n_classes)
    g = load_golden(key + ".npz")
    size, B, seed, ch, nc = (int(v) for v in g["meta"])
    assert (ch, nc) == (channel, n_classes)
    ora = Oracle(channel, n_classes)
    fill_module(ora, seed)
    no_dropout(ora)
    ora.train()
    x = det_input((B, channel, size, size), key + "/x")
    with torch.no_grad():
        y = ora(x)
    yf = y.flatten().double()
    ys = yf[torch.from_numpy(sample_index(yf.numel(), 32768))].numpy()
    assert float(np.abs(ys - g["logits/sample"]).max()) < 1e-4 * float(g["logits/stat"][0])

"""CPU: the width envelope of the HIP path (lm_net_amd.LM_Net.envelope_error, checked by LM_Net.forward before its first launch) and
the oracle against the real reference at the four wide widths of tests/test_wide_model_gpu.py (skipped when the reference tree is
not importable)."""
import pytest
import torch

from helpers import no_dropout
from tools.detweights import det_input, fill_module

WIDE = {
    "W2": [24, 48, 96, 192, 384],
    "W3": [36, 72, 144, 288, 576],
    "W4": [48, 96, 192, 384, 768],
    "Wodd": [12, 36, 60, 84, 120],
}


@pytest.mark.parametrize("filters", [[12, 24, 48, 96, 192], [12] * 5] + list(WIDE.values())
                         + [[384, 384, 384, 372, 12], [12, 12, 12, 12, 1488], [96, 192, 384, 384, 480]])
def test_envelope_accepts(filters):
    from lm_net_amd.LM_Net import envelope_error
    assert envelope_error(filters) is None
    for K in (3, 5, 7):
        assert envelope_error(filters, K) is None


@pytest.mark.parametrize("filters, words", [
    ([12, 24, 48, 396, 192], ["filters[3] = 396", "head_dim 33"]),
    ([396, 24, 48, 96, 192], ["filters[0] = 396"]),
    ([48, 96, 192, 384, 828], ["sum(filters) = 1548", "1536"]),
    ([12, 24, 48, 96, 1380], ["sum(filters) = 1560"]),
    ([12, 24, 48, 96, 0], ["filters[4] = 0", "positive multiple of 12"]),
    ([12, 24, 48, 96], ["5 entries"]),
])
def test_envelope_rejects_with_named_limit(filters, words):
    from lm_net_amd.LM_Net import envelope_error
    msg = envelope_error(filters)
    assert msg is not None
    for w in words:
        assert w in msg, (w, msg)


def test_envelope_window_sizes():
    from lm_net_amd.LM_Net import envelope_error
    # the channel-quad head dims (1, 2, 4, 8, 16) keep every odd window the ctor accepts; the general kernels take 3, 5, 7
    assert envelope_error([12, 24, 48, 96, 192], 9) is None
    assert envelope_error([12, 24, 48, 96, 192], 13) is None
    msg = envelope_error(WIDE["W3"], 9)
    assert msg is not None and "na_kernel_size = 9" in msg
    assert envelope_error(WIDE["Wodd"], 11) is not None


def test_outside_envelope_still_constructs():
    """A model outside the envelope still constructs (the check lives in forward, not in the ctor); forward keeps its device check
    first (a CPU input raises RuntimeError, as before).  tests/test_wide_model_gpu.py checks the ValueError on the device."""
    from lm_net_amd import LM_Net
    m = LM_Net(3, 2, filters=[12, 24, 48, 396, 192])
    assert m.filters[3] == 396
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 64, 64))


@pytest.mark.parametrize("name", list(WIDE))
def test_oracle_matches_reference_at_wide_widths(name):
    """oracle/lmnet_ref.py against the real reference (tools/ref_import.py) on the same name-keyed weights: same state_dict keys and
    shapes, logits equal to 1e-5 in eval and train (batch statistics)."""
    from tools.ref_import import import_reference_lmnet, reference_available
    if not reference_available():
        pytest.skip("reference tree not present")
    RefLMNet = import_reference_lmnet()
    from oracle.lmnet_ref import LM_Net as Oracle
    f = WIDE[name]
    ref = RefLMNet(3, 2, filters=f)
    ora = Oracle(3, 2, filters=f)
    sr, so = ref.state_dict(), ora.state_dict()
    assert list(sr) == list(so)
    assert all(tuple(sr[k].shape) == tuple(so[k].shape) for k in sr)
    fill_module(ref, 3)
    fill_module(ora, 3)
    no_dropout(ref)
    no_dropout(ora)
    x = det_input((2, 3, 64, 64), "wide_cpu/x")
    for train in (False, True):
        ref.train(train)
        ora.train(train)
        with torch.no_grad():
            yr, yo = ref(x), ora(x)
        err = float((yr - yo).abs().max() / yr.abs().max())
        assert err < 1e-5, (name, train, err)

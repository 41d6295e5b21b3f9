"""GPU: HardPixelLoss and hard_pixel_values on a caller's stream that is still busy (tests/busy.py): every call is issued twice behind a
gate on a side stream whose input buffers are rewritten between the calls.  Every call returns before the gate has drained (nothing
waits for the stream, although K is formed from device data), the results are those of the inputs the STREAM held at that point,
nothing is allocated after the warm-up, and -- with deterministic mode off and on: the family has no float atomics -- the bits are
those of a plain default-stream call.  References and bounds: tests/hard_busy_cases.py."""
import pytest
import torch

import busy
import hard_busy_cases as S

pytestmark = pytest.mark.gpu
_SIDE = []                       # one side stream for the file


def _side():
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream())
    return _SIDE[0]


def _make(name):
    import lm_net_amd as L
    crit = L.HardPixelLoss(S.K.C, **S.CONFIGS[name]).cuda()

    def make(bufs):
        z = bufs[0].requires_grad_(True)

        def call():
            z.grad = None
            loss = crit(z, bufs[1])
            loss.backward()
            return loss.detach(), z.grad, crit.values, crit.selection
        return call
    return make


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("name", S.NAMES)
def test_hard_criterion_on_a_busy_stream(name, deterministic):
    from lm_net_amd import hip
    was = hip.get_deterministic()
    hip.set_deterministic(deterministic)
    try:
        busy.run(S.subjects()[name], _make(name), _side())
    finally:
        hip.set_deterministic(was)


def test_hard_pixel_values_on_a_busy_stream():
    from lm_net_amd import hard_pixel_values

    def make(bufs):
        return lambda: hard_pixel_values(bufs[0], bufs[1], S.K.C, **S.VALUES_CONFIG)
    busy.run(S.subjects()[S.VALUES_NAME], make, _side())

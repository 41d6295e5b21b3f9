"""GPU: SoftSegLoss, DistillLoss and DeviceMix on a caller's stream that is still busy (tests/busy.py): every call is issued twice behind
a gate on a side stream whose input buffers are rewritten between the calls.  Every call returns before the gate has drained (nothing
waits for the stream), the results are those of the inputs the STREAM held at that point, nothing is allocated after the warm-up, and
-- the mixer always, the criteria in deterministic mode -- the bits are those of a plain default-stream call.  References and bounds:
tests/soft_busy_cases.py."""
import pytest
import torch

import busy
import soft_busy_cases as S

pytestmark = pytest.mark.gpu
_SIDE = []                       # one side stream for the file: deterministic mode keeps a scratch per stream for the process's life


def _side():
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream())
    return _SIDE[0]


def _make(name):
    import lm_net_amd as L
    part = name.split("-")
    if part[0] == "SoftSegLoss":
        crit = L.SoftSegLoss(S.K.C, ce_weight=S.SEG["w_ce"], dice_weight=S.SEG["w_dice"], label_smoothing=S.SEG["eps"]).cuda()
        target = (lambda bufs: bufs[1]) if part[1] == "probs" else (lambda bufs: L.MixedTarget(bufs[1], bufs[2], bufs[3]))
        run = lambda z, bufs: crit(z, target(bufs))
    else:
        crit = L.DistillLoss(S.K.C, temperature=S.T, head=part[1])
        run = lambda z, bufs: crit(z, bufs[1].to(torch.bfloat16) if part[2] == "bf16" else bufs[1], bufs[2])

    def make(bufs):
        z = bufs[0].requires_grad_(True)

        def call():
            z.grad = None
            loss = run(z, bufs)
            loss.backward()
            return loss.detach(), z.grad
        return call
    return make


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("name", S.NAMES)
def test_soft_criterion_on_a_busy_stream(name, deterministic):
    from lm_net_amd import hip
    s = S.subjects()[name]
    was = hip.get_deterministic()
    hip.set_deterministic(deterministic)
    try:
        if deterministic:                                            # deterministic mode promises the bits of a default-stream call
            s = busy.Subject(s.name, s.inputs, s.ref, exact=True, no_growth=s.no_growth)
        busy.run(s, _make(name), _side())
    finally:
        hip.set_deterministic(was)


def test_device_mix_on_a_busy_stream():
    from lm_net_amd import DeviceMix
    mixer = DeviceMix(mixup_alpha=0.4, cutmix_alpha=1.0, generator=0)

    def make(bufs):
        def call(rows):
            x, t = mixer.mix(bufs[0], bufs[1], rows=rows)
            return x, t.ya, t.yb, t.lam
        return call
    busy.run(S.subjects()[S.MIX_NAME], make, _side())

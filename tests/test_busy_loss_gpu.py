"""GPU: the criteria on a caller's stream that is still busy (tests/busy.py): forward and backward of every loss class, and the three
monitoring functions, issued twice behind a gate on a side stream whose input buffers are rewritten between the calls.  Every call
returns before the gate has drained (nothing waits for the stream: not torch, not the runtime, not the library), loss and dlogits
are those of the inputs the STREAM held at that point, and -- LovaszLoss, distance_maps, and everything in deterministic mode --
the bits are those of a plain default-stream call.  LovaszLoss and RegionLoss allocate nothing after the warm-up.  References and
bounds: tests/busy_cases.py."""
import pytest
import torch

import busy
import busy_cases as K

pytestmark = pytest.mark.gpu
_SIDE = []                       # one side stream for the file: deterministic mode keeps a scratch per stream for the process's life


def _side():
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream())
    return _SIDE[0]


def _backward(crit, bufs, extra=None, **kw):
    """call(): loss.backward() inside the gated region -> (loss, logits.grad [, what extra() returns])"""
    z = bufs[0].requires_grad_(True)

    def call():
        z.grad = None
        loss = crit(z, bufs[1], **(kw and {k: v() for k, v in kw.items()}))
        loss.backward()
        return (loss.detach(), z.grad) + (tuple(t.clone() for t in extra()) if extra else ())
    return call


def _make(name):
    import lm_net_amd as L
    from lm_net_amd.loss import distance_maps, lovasz_ranks, region_sums
    part = name.split("-")
    if name == "SegLoss":
        crit = L.SegLoss(ce_weight=K.W_CE, dice_weight=K.W_DICE).cuda()
    elif name == "SegLoss-extended":
        crit = L.SegLoss(ce_weight=K.W_CE, dice_weight=K.W_DICE, **K.SEG_EXT).cuda()
    elif name == "FocalLoss":
        crit = L.FocalLoss(K.C, ignore_index=K.VOID).cuda()
    elif name == "SigmoidSegLoss":
        crit = L.SigmoidSegLoss().cuda()
    elif name in ("BoundaryLoss", "HausdorffDTLoss"):
        crit = getattr(L, name)(K.C)
        return lambda bufs: _backward(crit, bufs, maps=lambda: crit.target_maps(bufs[1]))
    elif part[0] == "LovaszLoss":
        crit = L.LovaszLoss(K.C, head=part[1], per_image="per_image" in part, scale=0.5)
        return lambda bufs: _backward(crit, bufs, extra=lambda: crit.ranks[:2])
    elif part[0] == "RegionLoss":
        crit = L.RegionLoss(K.C, kind=part[1], per_image="per_image" in part, **K.REGION_KINDS[part[1]]).cuda()
    elif name == "distance_maps":
        return lambda bufs: lambda: distance_maps(bufs[0], K.C)
    elif part[0] == "lovasz_ranks":
        return lambda bufs: lambda: lovasz_ranks(bufs[0], bufs[1], K.C, part[1], "present", True)
    elif name == "region_sums":
        return lambda bufs: lambda: region_sums(bufs[0], bufs[1], K.C, per_image=True)
    else:
        raise KeyError(name)
    return lambda bufs: _backward(crit, bufs)


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("name", K.LOSS_NAMES)
def test_criterion_on_a_busy_stream(name, deterministic):
    from lm_net_amd import hip
    s = K.subjects()[name]
    was = hip.get_deterministic()
    hip.set_deterministic(deterministic)
    try:
        if deterministic and not s.exact:                            # deterministic mode promises the bits of a default-stream call
            s = busy.Subject(s.name, s.inputs, s.ref, exact=True, no_growth=s.no_growth)
        busy.run(s, _make(name), _side())
    finally:
        hip.set_deterministic(was)

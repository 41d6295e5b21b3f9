"""GPU: LM_Net under a caller's stream that is still busy (tests/busy.py), in deterministic mode: a training step (forward, SegLoss,
backward, FusedAdamW.step() with clipping and EMA) and an eval forward, each launch by launch and with enable_plans().  In the
plans variant the plan of the shape was recorded under the default stream; the gated calls come under the side stream and get a
plan of their own (LM_Net._plan_key).  The reference is the SAME sequence of calls of an identically filled twin on the default
stream: logits, loss, updated parameters and EMA must carry its bits (the step's float64 parity is tests/test_model_gpu.py's).
The discrimination precondition cannot be taken from a CPU restatement here; it is asserted on the twin's own results: the logits
of any two cases differ in more than half of their elements.  The host-launched training step is documented to wait for a
stalled stream when its reduce job tables miss their cache; it is held to stream order and the twin's bits, and a wait is accepted
only with that cause."""
import numpy as np
import pytest
import torch

import busy
import busy_cases as K
from helpers import no_dropout

pytestmark = pytest.mark.gpu
_SIDE = []
SHAPE = (2, 3, 64, 96)


def _side():
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream())
    return _SIDE[0]


@pytest.fixture
def deterministic():
    from lm_net_amd import hip
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    yield
    hip.set_deterministic(was)


def _inputs():
    return {k: [K.logits(k, shape=SHAPE), K.label_map(k, shape=(SHAPE[0],) + SHAPE[2:], n=2)] for k in K.CASES}


class _Step:
    """one model with its criterion and optimizer; step(x, y) is a whole training step, infer(x) an eval forward"""

    def __init__(self, plans, train):
        from lm_net_amd import LM_Net, SegLoss
        from lm_net_amd.optim import FusedAdamW
        from tools.detweights import fill_module
        net = LM_Net(3, 2, filters=[12] * 5)
        fill_module(net, 7)
        no_dropout(net)
        self.net = net.cuda().train(train)
        if plans:
            self.net.enable_plans()
        self.seg = SegLoss().cuda()
        self.opt = FusedAdamW(self.net, lr=1e-3, max_norm=1.0, ema_decay=0.99) if train else None

    def step(self, x, y):
        self.opt.zero_grad(set_to_none=True)
        logits = self.net(x)
        loss = self.seg(logits, y)
        loss.backward()
        self.opt.step()
        return logits.detach().clone(), loss.detach().clone(), self.opt.flat_p.clone(), self.opt.ema.clone()

    def infer(self, x, y=None):
        with torch.no_grad():
            return (self.net(x).clone(),)


def _run(name, plans, train):
    inputs = _inputs()
    ours, twin = _Step(plans, train), _Step(plans, train)
    fn = "step" if train else "infer"
    a = [torch.from_numpy(v).cuda() for v in inputs["A"]]
    for m in (ours, twin):                                            # the plan of this shape is recorded HERE, under the default stream
        for _ in range(4):
            getattr(m, fn)(*a)
    torch.cuda.synchronize()
    seen = {}

    def ref(arrays, got=None):
        """the twin repeats the calls busy.run makes -- five on case A (warm-up and timing), then B, then C -- on the default stream"""
        if not seen:
            for _ in range(5):
                seen["A"] = [t.cpu().numpy() for t in getattr(twin, fn)(*a)]
        case = "B" if "B" not in seen else "C"
        seen[case] = [t.cpu().numpy() for t in getattr(twin, fn)(*[torch.from_numpy(v).cuda() for v in arrays])]
        return [("output %d" % i, o, None) for i, o in enumerate(seen[case])]

    # no growth: under plans the pass lives in the plan's arena, so the step as a whole -- FusedAdamW.step() with it -- is held to
    # "nothing allocated after the first steps".  The eager schedule hands its intermediates to its side streams (record_stream);
    # while the caller's stream is stalled torch's allocator cannot recycle them and takes new segments, by design.
    s = busy.Subject(name, inputs, ref, no_growth=train and plans)
    if train and not plans:
        # documented (hip.wgrad_reduce_flush, LM_Net.enable_plans): behind a stalled stream the allocator hands the host-launched step
        # other blocks than last step, its reduce job tables miss their cache and go up with a blocking copy.  Measured: call 1 returns
        # after 400 ms behind a 385 ms gate, call 2 after 20 ms.  A wait is accepted only where new tables were uploaded.
        from lm_net_amd import hip
        s.waits = lambda: len(hip._RTABLES)
    busy.run(s, lambda bufs: lambda: getattr(ours, fn)(*bufs), _side())
    for p, q in (("A", "B"), ("A", "C"), ("B", "C")):                 # the precondition, on the twin's own logits
        share = busy.distance(seen[p][0], seen[q][0])[1]
        assert share > 0.5, (p, q, share)


@pytest.mark.parametrize("plans", [False, True], ids=["eager", "plans"])
def test_training_step_on_a_busy_stream(plans, deterministic):
    _run("LM_Net-train-%s" % ("plans" if plans else "eager"), plans, True)


@pytest.mark.parametrize("plans", [False, True], ids=["eager", "plans"])
def test_eval_forward_on_a_busy_stream(plans, deterministic):
    _run("LM_Net-eval-%s" % ("plans" if plans else "eager"), plans, False)

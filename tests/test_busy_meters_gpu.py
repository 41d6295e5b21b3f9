"""GPU: the device-side halves of the meters (update / push / close_case / raw()) on a caller's stream that is still busy
(tests/busy.py).  compute() synchronises by design and is not part of the gated region.  Every meter counts integers: the raw
statistics equal the restatement's and carry the bits of a plain default-stream call; the float64 sums of the surface meters keep
the 1e-9 bar of their own tests.  Also the instrument's gate itself, in both constructions.  References: tests/busy_cases.py."""
import pytest
import torch

import busy
import busy_cases as K

pytestmark = pytest.mark.gpu
_SIDE = []


def _side():
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream())
    return _SIDE[0]


def _make(name):
    from lm_net_amd import metrics as M
    if name.startswith("ConfusionMeter"):
        m = M.ConfusionMeter(K.C)

        def call_of(bufs):
            def call():
                m.reset()
                m.update(bufs[0], bufs[1])
                return (m.total.clone(),)
            return call
        return call_of
    if name == "SigmoidStatsMeter":
        m = M.SigmoidStatsMeter(K.C, threshold=0.3)

        def call_of(bufs):
            def call():
                m.reset()
                m.update(bufs[0], bufs[1])
                return (m.raw(), M.sigmoid_labels(bufs[0], 0.3))
            return call
        return call_of
    if name == "ImageStatsMeter":
        m, feed = M.ImageStatsMeter(K.C, ignore_index=K.VOID), "update"
    elif name == "CurveMeter":
        m, feed = M.CurveMeter(K.C, scores="sigmoid", thresholds=K.CURVE_THRESHOLDS), "update"
    elif name == "SurfaceDistanceMeter":
        m, feed = M.SurfaceDistanceMeter(K.C), "update"
    elif name == "VolumeSurfaceMeter":
        m, feed = M.VolumeSurfaceMeter(K.C, spacing=(2, 1, 1)), "push"
    elif name == "LesionMeter":
        m, feed = M.LesionMeter(K.C, connectivity=26, **K.LESION_CAP), "push"
    else:
        raise KeyError(name)

    def call_of(bufs):
        def call():
            m.reset()
            getattr(m, feed)(bufs[0], bufs[1])
            if feed == "push":                                       # the case in two pushes is out of scope here: one push, then close
                m.close_case()
            out = m.raw()
            return out if isinstance(out, tuple) else (out,)
        if name == "LesionMeter":
            call.finish = K.lesion_finish
        return call
    return call_of


@pytest.mark.parametrize("name", K.METER_NAMES)
def test_meter_on_a_busy_stream(name):
    busy.run(K.subjects()[name], _make(name), _side())


@pytest.mark.parametrize("kind", ["sleep", "matmul"])
def test_the_gate_holds_and_drains(kind):
    """An event behind a 20 ms gate is not complete when gate() returns and is complete after a synchronise; the measured length is
    within a factor of two of the request (calibration: two events around one unit of work)."""
    if kind == "sleep" and not hasattr(torch.cuda, "_sleep"):
        kind = "matmul"
    side = _side()
    busy.gate(side, 1.0, kind)                                       # calibrates
    side.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        start.record()
    ev = busy.gate(side, 20.0, kind)
    early = not ev.query()
    end = torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        end.record()
    side.synchronize()
    ms = start.elapsed_time(end)
    print("gate %s: asked 20 ms, took %.2f ms" % (kind, ms))
    assert early and ev.query() and 10.0 <= ms <= 40.0, (early, ms)

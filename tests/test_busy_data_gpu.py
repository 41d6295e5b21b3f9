"""GPU: the input and output side of the pipeline on a caller's stream that is still busy (tests/busy.py): DevicePreprocess,
DeviceAugment without and with the OneOf block (the parameter arrays and tables of a call are host memory: their upload must
neither wait for the stream nor read memory a later call has replaced, so the two gated calls carry different parameters),
VolumeSlicer (open_case, batch, restore), DevicePostprocess (called and components), VolumePostprocess and TiledPredictor.  All of it
is integer arithmetic or a fixed function of integers: the outputs equal the restatements' and carry the bits of a plain
default-stream call; VolumeSlicer's images keep the bound of tests/test_slices_kernels_gpu.py.  VolumeSlicer and TiledPredictor
allocate nothing after the warm-up.  References: tests/busy_cases.py."""
import numpy as np
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
    from lm_net_amd import VolumeSlicer
    from lm_net_amd.data import DeviceAugment, DevicePreprocess
    from lm_net_amd.post import DevicePostprocess, VolumePostprocess
    if name == "DevicePreprocess":
        pre = DevicePreprocess((K.H, K.W), mask_mode="labels")
        return lambda bufs: lambda: pre(bufs[0], bufs[1], bufs[2])
    if name.startswith("DeviceAugment"):
        aug = DeviceAugment((K.H, K.W), mask_mode="labels", one_of="reference" if name.endswith("oneof") else None)

        def call_of(bufs):
            def call(params):
                x, y = aug(bufs[0], bufs[1], params=params)
                return x, y, aug.last_gray_sum
            return call
        return call_of
    if name == "VolumeSlicer":
        s = VolumeSlicer(**K.SLICER)

        def call_of(bufs):
            def call(params):
                s.open_case(bufs[0], bufs[1])
                x, y = s.batch(K.SLICER_Z, params)
                back = s.restore(bufs[2])
                return tuple(t.clone() for t in (s.stats, s.table, x, y, back))     # (the slicer's own buffers: the next call overwrites them)
            return call
        return call_of
    if name == "DevicePostprocess":
        post = DevicePostprocess(K.C, connectivity=8, alpha=0.4, overlay="contour", **K.POST_CLEAN)

        def call_of(bufs):
            def call():
                out = post(bufs[0], K.POST_HW, bufs[1])
                return (out.labels_net, out.stats, out.labels, out.overlay) + tuple(post.components(bufs[0]))
            call.finish = K.post_finish
            return call
        return call_of
    if name == "VolumePostprocess":
        post = VolumePostprocess(K.C, connectivity=26, **K.VOLPOST_CLEAN)

        def call_of(bufs):
            def call():
                out = post(bufs[0])
                return (out.labels, out.stats) + tuple(post.components(bufs[0]))
            call.finish = K.volpost_finish
            return call
        return call_of
    raise KeyError(name)


def test_tiled_predictor_on_a_busy_stream():
    """TiledPredictor around LM_Net(3, 2) with recorded plans in deterministic mode: 70 x 100 frames in 64 x 64 tiles with the "h" copies, batches of 4.
    The reference is tests/test_tiles_model_gpu.py's: the float64 blend (tests/tiles_ref.py) of the model's own outputs on the
    restatement's tiles, within tiles_ref.tol; the labels are the map's arg-max; the map carries the bits of a default-stream
    call, and nothing is allocated after the warm-up.  The restatement needs the model, so the discrimination precondition is
    asserted here, on the references the device-fed restatement gives."""
    import tiles_ref as R
    from lm_net_amd import LM_Net, hip
    from lm_net_amd.infer import TiledPredictor
    from test_tiles_model_gpu import reference
    from tools.detweights import fill_module
    net = LM_Net(3, 2, filters=[12] * 5)
    fill_module(net, 5)
    net = net.cuda().eval().enable_plans()      # the pass lives in the plan's arena: what is left to allocate is the predictor's own
    kw = dict(tile=(64, 64), stride=(32, 32), flips=("h",), tile_batch=4)
    inputs = {k: [K.logits(k, shape=(1, 3, 70, 100))] for k in K.CASES}
    refs = {}

    def ref(arrays, got=None):
        key = arrays[0].tobytes()
        if key not in refs:
            want, zmax = reference(net, torch.from_numpy(arrays[0]), kw["tile"], kw["stride"], kw["flips"], tile_batch=kw["tile_batch"])
            refs[key] = (want, R.tol("logits", zmax))
        want, tol = refs[key]
        return [("map", want, tol)]

    was = hip.get_deterministic()
    hip.set_deterministic(True)
    try:
        s = busy.Subject("TiledPredictor", inputs, ref, exact=True, no_growth=True)
        busy.check_discrimination(s)
        pred = TiledPredictor(net, **kw)

        def call_of(bufs):
            def call():
                out = pred(bufs[0])
                return out.map.clone(), out.labels.clone()           # (the geometry's own buffers: the next call overwrites them)

            def finish(outs):                                        # the labels come out of the blend launch that writes the map
                assert outs[1].dtype == np.uint8 and np.array_equal(outs[1], outs[0].argmax(1))
                return [outs[0]]
            call.finish = finish
            return call
        busy.run(s, call_of, _side())
    finally:
        hip.set_deterministic(was)


@pytest.mark.parametrize("name", K.DATA_NAMES)
def test_data_stage_on_a_busy_stream(name):
    busy.run(K.subjects()[name], _make(name), _side())

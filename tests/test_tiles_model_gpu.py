"""GPU: lm_net_amd.infer.TiledPredictor around LM_Net(3, 2) and LM_Net(3, 1) (filters [12] * 5, seeded weights) against the float64
restatement tests/tiles_ref.py fed with the MODEL'S OWN tile outputs: the restatement's gather, pushed through the model in the same
batches (the repeated fill entry included), blended in float64.  The comparisons that need the two sets of tile outputs to be the
same numbers run in deterministic mode (bit-reproducible forwards); the tolerance is the blend's own (tests/tiles_ref.py: tol)."""
import contextlib
import functools
import gc

import numpy as np
import pytest
import torch

import tiles_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ALL = ("h", "v", "hv")


@pytest.fixture(scope="module")
def model():
    """model(C): LM_Net(3, C) with seeded weights in eval mode, built once per class count and released when this module is done, so
    that no model, arena or stream of these tests is still alive while later test modules run"""
    from lm_net_amd import LM_Net
    from tools.detweights import fill_module
    nets = {}

    def get(C):
        if C not in nets:
            net = LM_Net(3, C, filters=[12] * 5)
            fill_module(net, 5)
            nets[C] = net.to(DEV).eval()
        return nets[C]

    yield get
    nets.clear()
    gc.collect()


@functools.lru_cache(maxsize=None)
def frame(B, H, W):
    from tools.detweights import det_input
    return det_input((B, 3, H, W), "tiles/%dx%d" % (H, W))


@contextlib.contextmanager
def deterministic():
    from lm_net_amd import hip
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    try:
        yield
    finally:
        hip.set_deterministic(was)


def reference(net, x, tile, stride, flips=(), pad="reflect", average="logits", tile_batch=8, window="gaussian"):
    """-> (float64 blend of the model's own outputs on the restatement's tiles, max |tile output|)"""
    tiles = R.gather(x.numpy(), tile, stride, pad, flips)
    zs = []
    with torch.no_grad():
        for e0 in range(0, tiles.shape[0], tile_batch):
            part = tiles[e0:e0 + tile_batch]
            k = part.shape[0]
            if k < tile_batch:
                part = np.concatenate([part, np.repeat(part[-1:], tile_batch - k, axis=0)])
            zs.append(net(torch.from_numpy(part).to(DEV))[:k].float().cpu().numpy())
    z = np.concatenate(zs)
    B, _, H, W = x.shape
    return R.blend(z, B, H, W, tile, stride, flips, R.window(tile[0], window), R.window(tile[1], window), average), float(np.abs(z).max())


def check(res, ref, tol, C, average):
    got = res.map.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - ref).max())
    print("max abs err %.3e, tolerance %.3e" % (err, tol))
    assert got.shape == ref.shape and res.map.dtype == torch.float32 and err <= tol, (err, tol)
    if C == 1 or average == "sigmoid":
        assert res.labels is None
        return
    assert res.labels.dtype == torch.uint8 and tuple(res.labels.shape) == (ref.shape[0],) + ref.shape[2:]
    assert torch.equal(res.labels.long(), res.map.argmax(1))
    sure = R.top2_gap(ref) > 2 * tol
    assert np.array_equal(res.labels.cpu().numpy()[sure], ref.argmax(1)[sure])


@pytest.mark.parametrize("C", [2, 1])
def test_frame_100x150_with_every_flip(C, model):
    """3 x 4 tiles of 64x64 at stride 32, four copies each: 48 entries in batches of 4.  The model itself refuses this size."""
    from lm_net_amd.infer import TiledPredictor
    net, x = model(C), frame(1, 100, 150)
    with pytest.raises(ValueError, match="multiples of 16"):
        net(x.to(DEV))
    pred = TiledPredictor(net, tile=(64, 64), overlap=0.5, flips=ALL, tile_batch=4)
    assert pred.stride == (32, 32)
    with deterministic():
        res = pred(x.to(DEV))
        ref, zmax = reference(net, x, (64, 64), (32, 32), ALL, tile_batch=4)
    assert tuple(res.map.shape) == (1, C, 100, 150)
    check(res, ref, R.tol("logits", zmax), C, "logits")


def test_single_tile_equals_the_model(model):
    """a 64x64 frame, one tile, no flips, one entry per model call: (w z) / w rounds once or twice"""
    from lm_net_amd.infer import TiledPredictor
    net, x = model(2), frame(1, 64, 64).to(DEV)
    with deterministic(), torch.no_grad():
        y = net(x)
        res = TiledPredictor(net, tile=64, tile_batch=1)(x)
    err = float((res.map - y).abs().max())
    assert err <= 4 * R.EPS * float(y.abs().max()), err
    assert torch.equal(res.labels.long(), res.map.argmax(1))


@pytest.mark.parametrize("C,average,pad", [(2, "logits", "reflect"), (2, "softmax", "zero"), (2, "softmax", "reflect"), (1, "sigmoid", "reflect"),
                                           (2, "sigmoid", "zero")])
def test_frame_40x50_is_padded_on_both_axes(C, average, pad, model):
    """one 64x64 tile around a 40x50 frame: 12 rows and 7 columns of padding before, the rest after; "h" and "hv" copies; the three
    averaging modes; a short batch of 3 entries filled up to 8"""
    from lm_net_amd.infer import TiledPredictor
    net, x = model(C), frame(1, 40, 50)
    pred = TiledPredictor(net, tile=64, overlap=0.25, flips=("h", "hv"), average=average, pad=pad)
    with deterministic():
        res = pred(x.to(DEV))
        ref, zmax = reference(net, x, (64, 64), (48, 48), ("h", "hv"), pad, average)
    assert tuple(res.map.shape) == (1, C, 40, 50)
    check(res, ref, R.tol(average, zmax), C, average)


def test_two_calls_are_bit_identical_and_allocate_nothing(model):
    from lm_net_amd.infer import TiledPredictor
    net, x = model(2), frame(2, 100, 150).to(DEV)
    pred = TiledPredictor(net, tile=(64, 64), overlap=0.5, flips=("v",), average="softmax")
    with deterministic():
        first = pred(x)
        m1, l1 = first.map.clone(), first.labels.clone()
        second = pred(x)
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        third = pred(x)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == held
    assert third.map.data_ptr() == second.map.data_ptr() == first.map.data_ptr()          # the geometry's own buffers
    assert torch.equal(m1.view(torch.int32), third.map.view(torch.int32)) and torch.equal(l1, third.labels)


def test_workspace_limit_and_image_groups(model):
    """one 100x150 frame needs 24 entries x 2 x 64 x 64 x 4 bytes = 786432: a limit below that raises with both figures; a limit of one
    image blends a batch of two in two launches with the same result as one launch"""
    from lm_net_amd.infer import TiledPredictor
    net, x = model(2), frame(2, 100, 150).to(DEV)
    kw = dict(tile=(64, 64), overlap=0.5, flips=("h",))
    with pytest.raises(ValueError, match="786432 bytes.*workspace_mb=0.5 allows 524288"):
        TiledPredictor(net, workspace_mb=0.5, **kw)(x)
    with deterministic():
        one = TiledPredictor(net, workspace_mb=1.0, **kw)
        a = one(x).map.clone()
        assert one._cache[(tuple(x.shape), x.device)]["group"] == 1
        b = TiledPredictor(net, **kw)(x).map
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_graph_replays_agree_with_the_first_call():
    """model.enable_graphs(): every tile batch has one shape, so the third call of a geometry replays ONE captured graph per batch"""
    from lm_net_amd.infer import TiledPredictor
    from lm_net_amd import LM_Net
    from tools.detweights import fill_module
    net = LM_Net(3, 2, filters=[12] * 5)
    fill_module(net, 5)
    net = net.to(DEV).eval()
    x = frame(1, 40, 50).to(DEV)
    pred = TiledPredictor(net, tile=64, flips=("h",), tile_batch=2)
    eager = pred(x).map.clone()
    with torch.no_grad():
        zmax = float(net(pred._cache[(tuple(x.shape), x.device)]["batch"]).abs().max())
    net.enable_graphs()
    try:
        outs = [pred(x).map.clone() for _ in range(3)]
    finally:
        net.enable_graphs(False)
    tol = R.tol("logits", zmax)
    for k, o in enumerate(outs):
        err = float((o - eager).abs().max())
        print("call %d: max abs difference %.3e, tolerance %.3e" % (k + 1, err, tol))
        assert err <= tol, (k, err)

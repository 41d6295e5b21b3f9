"""CPU: the host side of tiled inference (include/tiles/lmnet_tiles.h, lm_net_amd.infer.TiledPredictor): registry and header agree, the
struct mirror, the geometry and the partition of unity of the float64 restatement
tests/tiles_ref.py, the share of pixels the label comparison of tests/test_tiles_kernels_gpu.py leaves out, and the argument checks
of the two entries (rejected before any HIP call, with fake device pointers).  No GPU needed."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import tiles_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- ABI
def test_registry_header_and_struct_agree():
    """The feature's own part of the registry: the literal list, its place in hip.HEADERS, the one struct with its size and field
    offsets, and the #defines, which hip mirrors partly as dicts.  (Header / export / layout / return-type checks: tests/test_host_cpu.py.)"""
    from lm_net_amd import hip
    lib = hip.load()
    assert hip.SYMBOLS_TILES == ["lmn_sizeof_tile_param", "lmn_tile_gather", "lmn_tile_blend"]
    assert hip.HEADERS["tiles/lmnet_tiles.h"] is hip.SYMBOLS_TILES and (hip.TileParam, "lmn_sizeof_tile_param") in hip.STRUCTS
    header = open(os.path.join(ROOT, "include", "tiles", "lmnet_tiles.h")).read()
    assert re.findall(r"^\}\s*(lmn_\w+_t)\s*;", header, re.M) == ["lmn_tile_param_t"]
    defs = {k: int(v) for k, v in re.findall(r"^#define (LMN_TILE_\w+) (\d+)\b", header, re.M)}
    assert lib.lmn_sizeof_tile_param() == ctypes.sizeof(hip.TileParam) == defs["LMN_TILE_PARAM_BYTES"] == hip.TILE_PARAM_BYTES == 96
    for name in ("MIN", "MAX", "MAX_LEN", "MAX_CLASSES", "MAX_FLIPS"):
        assert defs["LMN_TILE_" + name] == getattr(hip, "TILE_" + name), name
    assert {k: defs["LMN_TILE_PAD_" + k.upper()] for k in hip.TILE_PADS} == hip.TILE_PADS
    assert {k: defs["LMN_TILE_AVG_" + k.upper()] for k in hip.TILE_AVERAGES} == hip.TILE_AVERAGES
    assert hip.TILE_FLIPS == dict(h=defs["LMN_TILE_FLIP_H"], v=defs["LMN_TILE_FLIP_V"], hv=defs["LMN_TILE_FLIP_H"] | defs["LMN_TILE_FLIP_V"])
    offs = {f[0]: getattr(hip.TileParam, f[0]).offset for f in hip.TileParam._fields_}
    assert offs == dict(batch=0, channels=4, height=8, width=12, tile_h=16, tile_w=20, stride_h=24, stride_w=28, pad=32, n_flip=36, flip=40,
                        average=56, _pad=60)


def test_tile_param_and_window_tables():
    from lm_net_amd import hip
    from lm_net_amd.infer import window_table
    p = hip.tile_param(3, 2, 100, 150, (64, 48), (32, 24), "zero", ("hv", "h"), "softmax")
    assert (p.batch, p.channels, p.height, p.width, p.tile_h, p.tile_w, p.stride_h, p.stride_w) == (3, 2, 100, 150, 64, 48, 32, 24)
    assert (p.pad, p.n_flip, list(p.flip), p.average) == (0, 3, [0, 3, 1, 0], 1)
    assert hip.tile_entries(p) == 3 * 6 * 3                                     # rows: ceil(36 / 32) + 1, columns: ceil(102 / 24) + 1
    for bad in (dict(pad="edge"), dict(average="mean"), dict(flips=("x",)), dict(flips=("h", "h"))):
        with pytest.raises(ValueError, match="tile_param"):
            hip.tile_param(1, 1, 32, 32, (32, 32), (16, 16), **bad)
    for L, t, s in ((32, 32, 32), (33, 32, 16), (20, 32, 16), (97, 32, 24), (8192, 32, 1)):
        V, pb, starts = R.axis(L, t, s)
        assert hip.tile_axis(L, t, s) == (V, pb, len(starts)), (L, t, s)
    for t in (32, 48, 352):
        for kind in ("gaussian", "constant"):
            assert np.array_equal(window_table(t, kind), R.window(t, kind)) and window_table(t, kind).dtype == np.float32
        w = window_table(t, "gaussian")
        assert np.array_equal(w, w[::-1]) and w.min() > 3e-4 and w.min() ** 2 > 1e-7 and w.max() <= 1.0    # symmetric, far from underflow
    with pytest.raises(ValueError, match="window"):
        window_table(32, "hann")


# ---------------------------------------------------------------- the restatement: geometry
@pytest.mark.parametrize("L,t,s", [(32, 32, 32), (33, 32, 16), (47, 32, 8), (20, 32, 16), (21, 32, 16), (97, 32, 24), (70, 48, 12)])
def test_geometry_of_the_restatement(L, t, s):
    V, p, starts = R.axis(L, t, s)
    assert V == max(L, t) and p == (V - L) // 2 and len(starts) == math.ceil((V - t) / s) + 1
    assert starts[0] == 0 and starts[-1] == V - t and starts == sorted(set(starts))     # pulled back to the edge, no tile twice
    covered = np.zeros(V, dtype=np.int64)
    for a in starts:
        assert 0 <= a and a + t <= V
        covered[a:a + t] += 1
    assert covered.min() >= 1 and covered.max() <= t // s + 1                     # every pixel is covered
    if L >= t:
        assert V == L and p == 0                                                   # an axis of at least one tile is never padded


def test_reflect_index_equals_numpy_pad_for_pads_larger_than_the_axis():
    for L in (2, 3, 5, 20, 21):
        for before, after in ((0, 0), (1, 2), (L - 1, L), (3 * L + 1, 2 * L + 5), (40, 41)):
            ref = np.pad(np.arange(L), (before, after), mode="reflect")
            mine = [R.reflect_index(i - before, L) for i in range(before + L + after)]
            assert mine == ref.tolist(), (L, before, after)
    # ... and the padded frame of the restatement is numpy.pad's: the 20-pixel axis under a 32-pixel tile, 6 before and 6 after
    src = R.seeded((1, 2, 20, 21), 1)
    v = R.padded(src, (32, 32), "reflect")
    assert v.shape == (1, 2, 32, 32) and np.array_equal(v[0, 1, 6:26, 5:26], src[0, 1])
    assert np.array_equal(v[0, 0, :, 0], [src[0, 0, R.reflect_index(y - 6, 20), R.reflect_index(-5, 21)] for y in range(32)])
    z = R.padded(src, (32, 32), "zero")
    assert np.array_equal(z[0, :, 6:26, 5:26], src[0]) and float(np.abs(z).sum()) == float(np.abs(src).sum())


def test_gather_of_the_restatement_orders_entries_and_mirrors():
    src = R.seeded((2, 3, 33, 47), 2)
    g = R.gather(src, (32, 32), (16, 16), "reflect", ("h", "hv"))
    ys, xs = R.axis(33, 32, 16)[2], R.axis(47, 32, 16)[2]
    assert (ys, xs) == ([0, 1], [0, 15]) and g.shape == (2 * 2 * 2 * 3, 3, 32, 32) and g.dtype == np.float32
    e = ((1 * 2 + 1) * 2 + 0) * 3                                               # image 1, tile row 1, tile column 0
    assert np.array_equal(g[e], src[1, :, 1:33, 0:32])
    assert np.array_equal(g[e + 1], src[1, :, 1:33, 0:32][:, :, ::-1])          # h: left-right
    assert np.array_equal(g[e + 2], src[1, :, 1:33, 0:32][:, ::-1, ::-1])       # hv: both


# ---------------------------------------------------------------- the restatement: partition of unity
@pytest.mark.parametrize("window", ["gaussian", "constant"])
@pytest.mark.parametrize("flips", R.FLIP_SUBSETS, ids=lambda f: "+".join(f) or "none")
def test_blend_of_gathered_tiles_returns_the_map(window, flips):
    """Tile "outputs" cut out of a random map by the restatement's gather, blended in "logits" mode, are the map again: the weights
    of every pixel sum to one and the mirrors are undone."""
    for (H, W), tile, stride in (((33, 47), (32, 32), (16, 16)), ((20, 70), (32, 48), (8, 24)), ((97, 64), (32, 32), (24, 24))):
        M = np.random.default_rng(7).standard_normal((2, 3, H, W))
        for pad in ("reflect", "zero"):
            z = R.gather(M, tile, stride, pad, flips)
            out = R.blend(z, 2, H, W, tile, stride, flips, R.window(tile[0], window), R.window(tile[1], window), "logits")
            assert out.shape == M.shape and float(np.abs(out - M).max()) < 1e-12, (H, W, pad)


def test_probability_modes_of_the_restatement():
    z = R.seeded((1, 5, 32, 32), 3)
    ones = np.ones(32, dtype=np.float32)
    sm = R.blend(z, 1, 32, 32, (32, 32), (32, 32), (), ones, ones, "softmax")
    assert float(np.abs(sm - torch.softmax(torch.from_numpy(z).double(), 1).numpy()).max()) < 1e-15 and abs(float(sm.sum(1).max()) - 1) < 1e-15
    sg = R.blend(z, 1, 32, 32, (32, 32), (32, 32), (), ones, ones, "sigmoid")
    assert float(np.abs(sg - torch.sigmoid(torch.from_numpy(z).double()).numpy()).max()) < 1e-15
    # flip averaging in a probability mode is NOT the probability of the averaged logits
    zz = R.seeded((2, 5, 32, 32), 4)
    a = R.blend(zz, 1, 32, 32, (32, 32), (32, 32), ("h",), ones, ones, "softmax")
    b = R.blend(zz, 1, 32, 32, (32, 32), (32, 32), ("h",), ones, ones, "logits")
    assert float(np.abs(a - torch.softmax(torch.from_numpy(b), 1).numpy()).max()) > 1e-3
    gap = R.top2_gap(np.array([3.0, -1.0, 2.5, 0.0]).reshape(1, 4, 1, 1))
    assert gap.shape == (1, 1, 1) and float(gap[0, 0, 0]) == 0.5


# ---------------------------------------------------------------- the cases of the GPU tests
def test_the_kernel_cases_cover_what_they_claim():
    cs = R.blend_cases()
    assert len(cs) == len(R.gather_cases()) == len(R.IMAGES) * len(R.TILES) * 4 == 40
    assert {(c["C"], c["average"]) for c in cs} == {(C, m) for C in R.BLEND_CLASSES for m in R.MODES}
    assert {(c["window"], 1 + len(c["flips"])) for c in cs} == {(w, F) for w in ("gaussian", "constant") for F in (1, 2, 4)}
    assert {c["pad"] for c in cs} == {"reflect", "zero"} and {c["B"] for c in cs} == {1, 3}
    assert {(c["C"], c["B"]) for c in cs} >= {(64, 3), (64, 1), (1, 1), (1, 3)}
    gs = R.gather_cases()
    assert {c["flips"] for c in gs} == set(R.FLIP_SUBSETS) and {c["channel"] for c in gs} == {1, 3, 16} and {c["B"] for c in gs} == {1, 3}
    # at most 5 x 5 tiles cover a pixel: the term count behind the tolerance
    for image, tile, stride in R.geometries():
        for L, t, s in zip(image, tile, stride):
            V, _, starts = R.axis(L, t, s)
            cover = np.zeros(V, dtype=np.int64)
            for a in starts:
                cover[a:a + t] += 1
            assert cover.max() <= 5, (L, t, s)


def test_label_comparison_leaves_out_few_pixels():
    """tests/test_tiles_kernels_gpu.py compares labels where the restatement's top-two gap exceeds twice the tolerance; on the seeded
    inputs of every case that rule must leave out fewer than 0.5 % of the pixels (the restatement alone, no kernel)."""
    worst = 0.0
    for k, c in enumerate(R.blend_cases()):
        if c["C"] < 2 or c["average"] == "sigmoid":
            continue
        _, z, _, _, ref = R.blend_case(k)
        share = float((R.top2_gap(ref) <= 2 * R.tol(c["average"], float(np.abs(z).max()))).mean())
        worst = max(worst, share)
        assert share < 0.005, (R.case_id(c), share)
    print("largest share of pixels left out: %.4f %%" % (100 * worst))


# ---------------------------------------------------------------- argument checks
GOOD = dict(batch=2, channels=3, height=33, width=47, tile=(32, 32), stride=(16, 16), pad="reflect", flips=("h", "v", "hv"), average="logits")


def _entry(which, null=None, first=0, count=1, labels=False, **kw):
    """lmn_tile_gather / lmn_tile_blend with fake device pointers: every case here must be rejected before any HIP call."""
    from lm_net_amd import hip
    lib = hip.load()
    fake = ctypes.c_void_p(0x1000)
    raw = {k[4:]: kw.pop(k) for k in list(kw) if k.startswith("raw_")}
    p = hip.tile_param(**dict(GOOD, **kw))
    for k, v in raw.items():
        if k.startswith("flip"):
            p.flip[int(k[4:])] = v
        else:
            setattr(p, k, v)
    if which == "gather":
        a = dict(src=fake, param=ctypes.byref(p), tiles=fake)
        if null:
            a[null] = None
        rc = lib.lmn_tile_gather(a["src"], a["param"], ctypes.c_int64(first), ctypes.c_int64(count), a["tiles"], None)
    else:
        a = dict(z=fake, param=ctypes.byref(p), wy=fake, wx=fake, map=fake)
        if null:
            a[null] = None
        rc = lib.lmn_tile_blend(a["z"], a["param"], a["wy"], a["wx"], a["map"], fake if labels else None, None)
    return rc, lib.lmn_last_error().decode()


@pytest.mark.parametrize("which", ["gather", "blend"])
def test_entries_reject_bad_arguments(which):
    what = "tile_" + which
    for name in (("src", "param", "tiles") if which == "gather" else ("z", "param", "wy", "wx", "map")):
        rc, err = _entry(which, null=name)
        assert rc == -1 and err == what + ": null pointer", (name, err)
    for tile in ((40, 32), (32, 40), (16, 32), (32, 1040), (0, 32), (-32, 32)):
        rc, err = _entry(which, tile=tile, stride=(1, 1))
        assert rc == -1 and err.startswith(what) and "multiples of 16 in [32, 1024]" in err, (tile, err)
    for stride in ((0, 16), (16, 0), (33, 16), (16, 33), (-1, 16)):
        rc, err = _entry(which, stride=stride)
        assert rc == -1 and "outside [1, tile]" in err, (stride, err)
    for hw in ((0, 47), (33, 0), (8193, 47), (33, 8193), (-5, 47)):
        rc, err = _entry(which, height=hw[0], width=hw[1])
        assert rc == -1 and "sides must be in [1, 8192]" in err, (hw, err)
    for hw in ((1, 47), (33, 1)):                                               # a reflected axis shorter than the tile, one pixel long
        rc, err = _entry(which, height=hw[0], width=hw[1])
        assert rc == -1 and "a reflected axis needs length >= 2" in err, (hw, err)
    for kw, msg in ((dict(raw_pad=2), "unknown pad mode 2"), (dict(raw_pad=-1), "unknown pad mode -1"), (dict(raw_n_flip=0), "n_flip=0"),
                    (dict(raw_n_flip=5), "n_flip=5"), (dict(raw_flip0=1), "entry 0 is the identity"), (dict(raw_flip2=4), "unknown flip 4"),
                    (dict(raw_flip2=0), "unknown flip 0"), (dict(raw_flip3=1), "flip 1 twice"), (dict(raw_batch=0), "batch=0")):
        rc, err = _entry(which, **kw)
        assert rc == -1 and msg in err and err.startswith(what), (kw, err)
    if which == "gather":
        entries = 2 * 2 * 2 * 4                                                   # two images of 2 x 2 tiles, four copies each
        for first, count in ((0, 0), (0, -1), (-1, 2), (entries, 1), (entries - 1, 2), (0, entries + 1), (2 ** 62, 2 ** 62)):
            rc, err = _entry(which, first=first, count=count)
            assert rc == -1 and "outside [0, %d)" % entries in err, (first, count, err)
        rc, err = _entry(which, channels=0)
        assert rc == -1 and "channels=0" in err
    else:
        for C in (0, 65, -1):
            rc, err = _entry(which, channels=C)
            assert rc == -1 and "C=%d not in [1, 64]" % C in err, (C, err)
        for mode in (3, -1):
            rc, err = _entry(which, raw_average=mode)
            assert rc == -1 and "unknown mode %d" % mode in err, (mode, err)
        for kw in (dict(channels=1), dict(average="sigmoid")):
            rc, err = _entry(which, labels=True, **kw)
            assert rc == -1 and "labels are defined for C >= 2" in err, (kw, err)


def test_python_wrappers_check_sizes_before_the_library():
    from lm_net_amd import hip
    p = hip.tile_param(1, 2, 33, 47, (32, 32), (16, 16), flips=("h",))
    E = hip.tile_entries(p)
    assert E == 2 * 2 * 2
    src, tiles, w = torch.zeros(1, 2, 33, 47), torch.zeros(3, 2, 32, 32), torch.ones(32)
    with pytest.raises(ValueError, match="tile_gather: tensor sizes"):
        hip.tile_gather(src, p, 0, 2, tiles)
    with pytest.raises(ValueError, match="tile_gather: tensor sizes"):
        hip.tile_gather(src[:, :1], p, 0, 3, tiles)
    with pytest.raises(RuntimeError, match="tile_gather: contiguous torch.float32 device tensor required"):
        hip.tile_gather(src, p, 0, 3, tiles)
    z, out = torch.zeros(E, 2, 32, 32), torch.zeros(1, 2, 33, 47)
    for bad in (dict(z=z[1:]), dict(wy=w[1:]), dict(out=out[:, :1]), dict(labels=torch.zeros(1, 33, 46, dtype=torch.uint8))):
        a = dict(dict(z=z, wy=w, wx=w, out=out, labels=None), **bad)
        with pytest.raises(ValueError, match="tile_blend: tensor sizes"):
            hip.tile_blend(a["z"], p, a["wy"], a["wx"], a["out"], a["labels"])
    with pytest.raises(RuntimeError, match="tile_blend: contiguous torch.float32 device tensor required"):
        hip.tile_blend(z, p, w, w, out)


def test_predictor_refuses_what_it_cannot_run():
    from lm_net_amd import LM_Net
    from lm_net_amd.infer import TiledPredictor
    net = LM_Net(3, 2, filters=[12] * 5)
    with pytest.raises(RuntimeError, match="training mode"):
        TiledPredictor(net)
    net.eval()
    with pytest.raises(ValueError, match=r"overlap=0.8 outside \[0, 0.75\]"):
        TiledPredictor(net, overlap=0.8)
    with pytest.raises(ValueError, match="tile 40x40"):
        TiledPredictor(net, tile=40)
    for kw, msg in ((dict(tile=(32, 1040)), "tile 32x1040"), (dict(stride=(0, 8)), "stride 0x8"), (dict(tile=64, stride=65), "stride 65x65"),
                    (dict(window="hann"), "window='hann'"), (dict(flips=("d",)), "flips"), (dict(average="mean"), "average"),
                    (dict(pad="edge"), "pad"), (dict(tile_batch=0), "tile_batch"), (dict(sigma_scale=0.0), "sigma_scale")):
        with pytest.raises(ValueError, match=msg):
            TiledPredictor(net, **kw)
    pred = TiledPredictor(net, tile=(64, 48), overlap=0.5, flips=("h",))
    assert pred.stride == (32, 24) and TiledPredictor(net, tile=352, overlap=0.75).stride == (88, 88)
    assert TiledPredictor(net, tile=64, overlap=0.0).stride == (64, 64) and TiledPredictor(net, tile=64, stride=(1, 64)).stride == (1, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pred(torch.zeros(1, 3, 100, 150))
    net.train()
    with pytest.raises(RuntimeError, match="training mode"):                    # ... also when the model is switched back later
        pred(torch.zeros(1, 3, 100, 150))

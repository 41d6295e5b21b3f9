"""GPU: lmn_tile_gather and lmn_tile_blend alone (include/tiles/lmnet_tiles.h) against the float64 restatement tests/tiles_ref.py; no
model.

Geometries: images 32x32 (one tile), 33x47 (last tile pulled back by an odd amount), 20x70 and 21x33 (an axis shorter than the tile:
even and odd padding), 97x64 (several blocks); tiles 32x32 and 32x48; strides t, t/2, t/4 and 24 -- one case each, the other axes
(flip sets, channels, classes, windows, modes, pads, batch) cycling through them (tests/tiles_ref.py, asserted in test_tiles_cpu.py).

Tolerance: the blend is a convex combination of at most 5 x 5 tiles x 4 copies = 100 terms, so its fp32 error is bounded by the
roundings of that sum: 128 * 2^-24 * max|z| absolute for "logits"; the probability modes add the softmax's own at most C + 8
roundings on values in [0, 1]: 256 * 2^-24 absolute.  Labels must equal the restatement's arg-max wherever its top-two gap exceeds
twice the tolerance; test_tiles_cpu.py asserts that this leaves out fewer than 0.5 % of the pixels of every case."""
import numpy as np
import pytest
import torch

import tiles_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def entries_of(image, tile, stride, flips):
    return len(R.axis(image[0], tile[0], stride[0])[2]) * len(R.axis(image[1], tile[1], stride[1])[2]) * (1 + len(flips))


# ---------------------------------------------------------------- gather
@pytest.mark.parametrize("k", range(len(R.gather_cases())), ids=[R.case_id(c) for c in R.gather_cases()])
def test_gather_equals_the_restatement_bit_for_bit(k):
    from lm_net_amd import hip
    c = R.gather_cases()[k]
    (H, W), tile, stride, flips, ch, B = c["image"], c["tile"], c["stride"], c["flips"], c["channel"], c["B"]
    src = R.seeded((B, ch, H, W), c["seed"])
    d = torch.from_numpy(src).to(DEV)
    E = entries_of((H, W), tile, stride, flips)
    n = B * E
    for pad in ("reflect", "zero"):
        ref = R.gather(src, tile, stride, pad, flips)
        p = hip.tile_param(B, ch, H, W, tile, stride, pad, flips)
        assert hip.tile_entries(p) == E and ref.shape[0] == n
        out = torch.full((n, ch) + tile, float("nan"), device=DEV)
        hip.tile_gather(d, p, 0, n, out)
        assert np.array_equal(out.cpu().numpy().view(np.int32), ref.view(np.int32)), pad
        # a run that starts and ends mid-image (for B = 3: inside the first and inside the last image)
        first = E // 2 + (1 if E > 2 else 0)
        count = max(1, n - first - (E // 3 + 1)) if n - first > 1 else n - first
        if count >= 1 and first + count <= n:
            part = torch.full((count + 1, ch) + tile, float("nan"), device=DEV)
            hip.tile_gather(d, p, first, count, part[:count])
            assert np.array_equal(part[:count].cpu().numpy().view(np.int32), ref[first:first + count].view(np.int32)), (pad, first, count)
            assert bool(torch.isnan(part[count]).all())                          # nothing past the run is written
    assert torch.equal(d.cpu(), torch.from_numpy(src))                          # the source is read-only


# ---------------------------------------------------------------- blend
def device_blend(c, z, wy, wx, labels=True, B=None, z_dev=None):
    from lm_net_amd import hip
    (H, W), C = c["image"], c["C"]
    B = c["B"] if B is None else B
    p = hip.tile_param(B, C, H, W, c["tile"], c["stride"], c["pad"], c["flips"], c["average"])
    out = torch.full((B, C, H, W), float("nan"), device=DEV)
    lab = torch.full((B, H, W), 255, dtype=torch.uint8, device=DEV) if labels and C >= 2 and c["average"] != "sigmoid" else None
    dev = lambda a: torch.tensor(a, device=DEV)                                  # (a copy: the cached case arrays are read-only)
    hip.tile_blend(dev(z) if z_dev is None else z_dev, p, dev(wy), dev(wx), out, lab)
    return out, lab


@pytest.mark.parametrize("k", range(len(R.blend_cases())), ids=[R.case_id(c) for c in R.blend_cases()])
def test_blend_against_the_restatement(k):
    c, z, wy, wx, ref = R.blend_case(k)
    out, lab = device_blend(c, z, wy, wx)
    got = out.cpu().numpy().astype(np.float64)
    tol = R.tol(c["average"], float(np.abs(z).max()))
    err = float(np.abs(got - ref).max())
    print("%s: max abs err %.3e, tolerance %.3e" % (R.case_id(c), err, tol))
    assert np.isfinite(got).all() and err <= tol, (err, tol)
    if c["average"] == "softmax":
        assert float(np.abs(got.sum(1) - 1.0).max()) <= c["C"] * tol
    if lab is None:
        assert c["C"] == 1 or c["average"] == "sigmoid"
        return
    sure = R.top2_gap(ref) > 2 * tol
    assert float((~sure).mean()) <= 0.005
    lab = lab.cpu().numpy()
    assert np.array_equal(lab[sure], ref.argmax(1)[sure]) and int(lab.max()) < c["C"]
    assert np.array_equal(lab, out.argmax(1).cpu().numpy())                     # everywhere: the arg-max of the map it wrote, lowest class first
    # two calls are bit-identical, with and without the labels
    again, _ = device_blend(c, z, wy, wx, labels=False)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))


def test_labels_take_the_lowest_class_on_a_tie():
    """all classes equal in every tile: the blend is exactly that value for every class (w v / w with one rounding each way is the same
    for every class), and the label is class 0"""
    c = dict(image=(33, 47), tile=(32, 32), stride=(16, 16), pad="reflect", flips=("h",), average="logits", C=5, B=1)
    n = entries_of(c["image"], c["tile"], c["stride"], c["flips"])
    z = np.repeat(R.seeded((n, 1, 32, 32), 9), 5, axis=1)
    out, lab = device_blend(c, z, R.window(32, "gaussian"), R.window(32, "gaussian"))
    assert all(torch.equal(out[:, 0], out[:, j]) for j in range(1, 5)) and int(lab.max()) == 0


@pytest.mark.parametrize("k", [8, 17, 32])
def test_batch_equals_single_images_bit_for_bit(k):
    """B = 3 in one launch against three launches of one image each (cases with B = 3: 33x47 logits, 20x70 softmax with 64 classes, 97x64 softmax)"""
    c, z, wy, wx, _ = R.blend_case(k)
    assert c["B"] == 3
    E = z.shape[0] // 3
    out, lab = device_blend(c, z, wy, wx)
    for b in range(3):
        one, lab1 = device_blend(c, np.ascontiguousarray(z[b * E:(b + 1) * E]), wy, wx, B=1)
        assert torch.equal(out[b:b + 1].view(torch.int32), one.view(torch.int32)), b
        assert lab is None or torch.equal(lab[b:b + 1], lab1), b


# ---------------------------------------------------------------- the two kernels together
@pytest.mark.parametrize("k", range(0, len(R.gather_cases()), 3), ids=[R.case_id(c) for c in R.gather_cases()[::3]])
def test_round_trip_gather_then_blend_returns_the_map(k):
    """A random map gathered and blended as if the tiles were outputs, "logits" mode: any disagreement between the two kernels about
    starts, padding offsets or mirrors shows as an error of the order of the values."""
    from lm_net_amd import hip
    g = R.gather_cases()[k]
    (H, W), tile, stride, flips, C, B = g["image"], g["tile"], g["stride"], g["flips"], g["channel"], g["B"]
    M = R.seeded((B, C, H, W), 500 + k)
    d = torch.from_numpy(M).to(DEV)
    n = B * entries_of((H, W), tile, stride, flips)
    for pad, window in (("reflect", "gaussian"), ("zero", "constant")):
        tiles = torch.empty((n, C) + tile, device=DEV)
        hip.tile_gather(d, hip.tile_param(B, C, H, W, tile, stride, pad, flips), 0, n, tiles)
        c = dict(image=(H, W), tile=tile, stride=stride, pad=pad, flips=flips, average="logits", C=C, B=B)
        out, _ = device_blend(c, None, R.window(tile[0], window), R.window(tile[1], window), labels=False, z_dev=tiles)
        err = float((out - d).abs().max())
        assert err <= R.tol("logits", float(np.abs(M).max())), (pad, window, err)

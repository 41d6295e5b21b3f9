"""CPU: the OneOf restatement (tests/oneof_ref.py) on hand-checkable cases and against scipy, the integer LAB tables against the
float64 textbook formulas, the host-side sampler of lm_net_amd.data.DeviceAugment(one_of=...), the exports of
include/lmnet_oneof.h and the argument checks of lmn_augment_oneof_u8 (no GPU needed)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import oneof_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rng(seed):
    return np.random.default_rng(seed)


# ---------------------------------------------------------------- sampler
def test_one_of_none_draws_what_the_parent_drew():
    """Values recorded from the sampler before the OneOf block existed (same seed, same calls)."""
    from lm_net_amd.data import DeviceAugment
    ds = DeviceAugment((64, 96), generator=2024).sample_dicts(3, (150, 170))
    assert [d["crop"] for d in ds] == [(13, 8, 136, 162), (9, 4, 135, 161), (1, 2, 136, 164)]
    assert [d["angle"] for d in ds] == [-25.27646797428006, -25.74709294619059, -16.298965814655755]
    assert [d["flips"] for d in ds] == [0, 1, 3] and [d["order"] for d in ds] == [[0, 3, 2, 1], [0, 1, 3, 2], [2, 0, 3, 1]]
    assert ds[0]["cj"] == [1.0262924204103323, 0.8018518573313543, 0.9860476797635289, 0.19024887905141508] and ds[1]["cj"] is None
    assert ds[2]["M"] is None and all("oneof" not in d for d in ds)
    # with one_of set, the OneOf draws follow the sample's own: sample 0 keeps every existing key
    ds1 = DeviceAugment((64, 96), generator=2024, one_of="reference").sample_dicts(3, (150, 170))
    assert {k: v for k, v in ds1[0].items() if k != "oneof"} == ds[0] and "oneof" in ds1[0]
    assert ds1[1]["crop"] != ds[1]["crop"]


def _binomial_ok(got, n, p):
    return abs(got - n * p) <= 5 * math.sqrt(n * p * (1 - p))


def test_oneof_rates_within_5_sigma():
    from lm_net_amd.data import ONEOF_REFERENCE, DeviceAugment
    n, seed = 20000, 12
    # the bound itself, on a plain sampler with the same seed: fire with 0.4, then a uniform member
    g = _rng(seed)
    fire = g.random(n) < 0.4
    member = g.integers(9, size=n)[fire]
    assert _binomial_ok(fire.sum(), n, 0.4) and all(_binomial_ok((member == k).sum(), n, 0.4 / 9) for k in range(9))
    ds = DeviceAugment((32, 32), generator=seed, one_of="reference").sample_dicts(n, (40, 40))
    ops = [d["oneof"]["op"] for d in ds if d["oneof"] is not None]
    assert _binomial_ok(len(ops), n, 0.4), len(ops)
    for name in ONEOF_REFERENCE:
        assert _binomial_ok(ops.count(name), n, 0.4 / 9), (name, ops.count(name))


def test_drawn_values_stay_in_range():
    from lm_net_amd.data import DeviceAugment, pack_oneof
    aug = DeviceAugment((40, 56), generator=4, one_of="reference", p_oneof=1.0)
    ds = aug.sample_dicts(300, (60, 70))
    seen = set()
    for d in ds:
        o = d["oneof"]
        seen.add(o["op"])
        if o["op"] == "rgb_shift":
            assert all(abs(v) <= 20 for v in o["shift"])
        elif o["op"] == "hsv":
            assert abs(o["shift"][0]) <= 20 and abs(o["shift"][1]) <= 30 and abs(o["shift"][2]) <= 20
        elif o["op"] == "gaussian_blur":
            assert o["k"] in (3, 5, 7)
        elif o["op"] == "clahe":
            assert 1 <= o["clip"] <= 4
        elif o["op"] == "channel_shuffle":
            assert sorted(o["perm"]) == [0, 1, 2]
        elif o["op"] == "grid_distortion":
            assert len(o["xsteps"]) == len(o["ysteps"]) == 6 and all(0.7 <= v <= 1.3 for v in o["xsteps"] + o["ysteps"])
        elif o["op"] == "elastic":
            assert o["alpha"] == 1.0 and o["sigma"] == 50.0 and 0 <= o["seed"] < 2 ** 32
    assert len(seen) == 9
    assert {d["oneof"]["k"] for d in ds if d["oneof"]["op"] == "gaussian_blur"} == {3, 5, 7}
    arr, tables, n_el = pack_oneof(ds[:12], (40, 56))
    assert len(arr) == 12 and n_el == sum(d["oneof"]["op"] == "elastic" for d in ds[:12])
    again = pack_oneof(ds[:12], (40, 56))
    assert bytes(arr) == bytes(again[0]) and (tables is None or np.array_equal(tables, again[1]))


def test_constructor_rejects_bad_one_of():
    from lm_net_amd.data import DeviceAugment, pack_oneof
    for kw in ({"one_of": "albumentations"}, {"one_of": []}, {"one_of": ["sharpen"]}, {"one_of": [("hsv", {"hue": 300})]},
               {"one_of": [("gaussian_blur", {"blur_limit": (3, 8)})]}, {"one_of": [("gaussian_blur", {"sigma": 1})]},
               {"one_of": [("elastic", {"sigma": 0})]}, {"one_of": [("clahe", {"clip_limit": (0.5, 4)})]},
               {"one_of": [("grid_dropout", {"ratio": 0})]}, {"one_of": [("grid_distortion", {"num_steps": 0})]},
               {"one_of": [("rgb_shift", {"r": -1})]}, {"one_of": "reference", "p_oneof": 1.5},
               {"one_of": ["to_gray"], "channels": 1, "mean": (0.5,), "std": (0.2,)}):
        with pytest.raises(ValueError):
            DeviceAugment(**dict({"size": (32, 32)}, **kw))
    with pytest.raises(ValueError) as e:
        DeviceAugment((32, 32), (0.5,), (0.2,), channels=1, one_of="reference")
    assert all(name in str(e.value) for name in ("to_gray", "hsv", "channel_shuffle", "rgb_shift"))
    DeviceAugment((32, 32), (0.5,), (0.2,), channels=1, one_of=["grid_distortion", "elastic", "clahe", "grid_dropout", "gaussian_blur"])
    for bad in ({"op": "sharpen"}, {"op": "gaussian_blur", "k": 4}, {"op": "channel_shuffle", "perm": [0, 0, 1]},
                {"op": "elastic", "seed": 1, "alpha": 1, "sigma": -1}, {"op": "clahe", "clip": 0.1},
                {"op": "rgb_shift", "shift": [0, 0, 300]}):
        with pytest.raises(ValueError):
            pack_oneof([{"oneof": bad}], (32, 32))


# ---------------------------------------------------------------- restatement: known answers
@pytest.mark.parametrize("k", [3, 5, 7])
def test_blur_constant_and_impulse(k):
    const = np.full((11, 13, 3), 201, dtype=np.uint8)
    assert np.array_equal(R.gaussian_blur(const, k), const)
    w, shift = R.BLUR[k]
    assert sum(w) ** 2 == 1 << shift
    img = np.zeros((15, 17, 1), dtype=np.uint8)
    img[7, 8] = 255
    out = R.gaussian_blur(img, k)[..., 0].astype(np.int64)
    r = k // 2
    want = (np.outer(w, w) * 255 + (1 << (shift - 1))) >> shift
    assert np.array_equal(out[7 - r:8 + r, 8 - r:9 + r], want)
    out[7 - r:8 + r, 8 - r:9 + r] = 0
    assert not out.any()


def test_pointwise_members_known_answers():
    white = np.full((3, 4, 3), 255, dtype=np.uint8)
    assert (R.to_gray(white) == 255).all()
    px = np.array([[[10, 200, 250]]], dtype=np.uint8)
    assert R.rgb_shift(px, [-20.5, 7.9, 10.0]).tolist() == [[[0, 207, 255]]]
    assert R.channel_shuffle(px, [2, 0, 1]).tolist() == [[[250, 10, 200]]]
    assert np.array_equal(R.hsv_shift(white, [0.0, 0.0, 0.0]), white)
    red = np.array([[[255, 0, 0]]], dtype=np.uint8)
    assert R.hsv_shift(red, [60.0, 0.0, 0.0]).tolist() == [[[0, 255, 0]]]      # +60 of 180: red -> green
    assert R.hsv_shift(red, [0.0, -255.0, 0.0]).tolist() == [[[255, 255, 255]]]
    assert R.hsv_shift(red, [0.0, 0.0, -255.0]).tolist() == [[[0, 0, 0]]]


def test_grid_dropout_zeroes_the_predicted_pixels():
    img = _rng(1).integers(1, 256, (36, 52, 3), dtype=np.uint8)
    out = R.grid_dropout(img, 0.5)
    unit, hole = 3, 1                                   # max(2, 36 // 10), min(max(int(1.5), 1), 2)
    want = np.array([[(x % unit < hole) and (y % unit < hole) for x in range(52)] for y in range(36)])
    assert np.array_equal((out == 0).all(axis=2), want) and np.array_equal(out[~want], img[~want])
    lab = _rng(2).integers(0, 5, (36, 52))
    assert R.oneof_apply(img, lab, {"op": "grid_dropout", "ratio": 0.5})[1] is lab


def test_geometric_members_identities():
    rng = _rng(3)
    img = rng.integers(0, 256, (33, 47, 3), dtype=np.uint8)
    lab = rng.integers(0, 9, (33, 47)).astype(np.int64)
    ones = [1.0] * 6
    out, lo = R.oneof_apply(img, lab, {"op": "grid_distortion", "num_steps": 5, "xsteps": ones, "ysteps": ones})
    assert np.array_equal(out, img) and np.array_equal(lo, lab)
    out, lo = R.oneof_apply(img, lab, {"op": "elastic", "seed": 5, "alpha": 0.0, "sigma": 3.0})
    assert np.array_equal(out, img) and np.array_equal(lo, lab)


def test_elastic_at_the_reference_defaults_is_the_identity():
    """alpha = 1, sigma = 50: the blurred U[-1, 1) field stays below 1/64 pixel, which the 1/32-pixel remap rounds to zero."""
    rng = _rng(4)
    img = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    lab = rng.integers(0, 3, (64, 96)).astype(np.int64)
    d = {"op": "elastic", "seed": 77, "alpha": 1.0, "sigma": 50.0}
    mx, my = R.elastic_maps(64, 96, d)
    x, y = np.arange(96, dtype=np.float32)[None, :], np.arange(64, dtype=np.float32)[:, None]
    assert max(np.abs(mx - x).max(), np.abs(my - y).max()) < 1.0 / 64.0
    out, lo = R.oneof_apply(img, lab, d)
    assert np.array_equal(out, img) and np.array_equal(lo, lab)


def _plain_equalisation_luts(pad, th, tw):
    """[8,8,256] float64: plain histogram equalisation of every tile of the padded plane (cdf * 255 / area, rounded)."""
    luts = np.zeros((8, 8, 256))
    for ty in range(8):
        for tx in range(8):
            cdf = np.cumsum(np.bincount(pad[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].reshape(-1), minlength=256))
            luts[ty, tx] = np.clip(np.rint(cdf.astype(np.float32) * (np.float32(255) / np.float32(th * tw))), 0, 255)
    return luts


def test_clahe_constant_and_plain_equalisation():
    const = np.full((36, 52, 1), 90, dtype=np.uint8)
    out = R.clahe(const, 2.0)
    assert (out == out[0, 0, 0]).all()
    assert R.clahe(np.full((36, 52, 3), 128, dtype=np.uint8), 3.0).std() == 0
    # a clip nobody reaches: every tile's LUT is plain histogram equalisation of the tile.  32 x 48: tiles of 4 x 6, no padding;
    # pixel (4 ty + 2, 6 tx + 3) sits at tile coordinate (ty, tx) exactly and takes its own tile's LUT alone -- every tile
    v = _rng(5).integers(0, 256, (32, 48)).astype(np.int64)
    out = R.clahe_plane(v, 1e6)
    luts = _plain_equalisation_luts(v, 4, 6)
    for ty in range(8):
        for tx in range(8):
            cy, cx = ty * 4 + 2, tx * 6 + 3
            assert out[cy, cx] == luts[ty, tx, v[cy, cx]], (ty, tx)


def test_clahe_padded_frame_and_blend_against_a_plain_loop():
    """36 x 52 (tiles of 5 x 7 on a frame padded to 40 x 56 by np.pad's reflect mode): every pixel against a per-pixel loop that
    blends the four neighbouring plain-equalisation LUTs in float64.  The restatement blends in float32: a result within 1e-3 of
    a rounding tie may round the other way, so the two may differ by one level there and nowhere else."""
    v = _rng(7).integers(0, 256, (36, 52)).astype(np.int64)
    out = R.clahe_plane(v, 1e6)
    luts = _plain_equalisation_luts(np.pad(v, ((0, 4), (0, 4)), mode="reflect"), 5, 7)
    for y in range(36):
        for x in range(52):
            ty, tx = y / 5.0 - 0.5, x / 7.0 - 0.5
            y1, x1 = math.floor(ty), math.floor(tx)
            wy, wx = ty - y1, tx - x1
            y2, x2, y1, x1 = min(y1 + 1, 7), min(x1 + 1, 7), max(y1, 0), max(x1, 0)
            k = v[y, x]
            ref = ((luts[y1, x1, k] * (1 - wx) + luts[y1, x2, k] * wx) * (1 - wy)
                   + (luts[y2, x1, k] * (1 - wx) + luts[y2, x2, k] * wx) * wy)
            near_tie = abs(ref - math.floor(ref) - 0.5) < 1e-3
            assert abs(out[y, x] - ref) <= 0.5 + (1e-3 if near_tie else 1e-4), (y, x, out[y, x], ref)


# ---------------------------------------------------------------- scipy cross-checks
def test_blurred_field_matches_scipy():
    """fp32 taps and accumulation against scipy's float64 filter: a few float32 ulps of a value below 1."""
    from scipy import ndimage as ndi
    from lm_net_amd.data import elastic_noise
    for (H, W), sigma in (((32, 48), 3.0), ((32, 48), 4.0), ((36, 52), 9.0)):     # radius 16 and 36 exceed half of 32 rows
        f = elastic_noise(9, H, W)[0]
        ref = ndi.gaussian_filter(f.astype(np.float64), sigma, mode="mirror", truncate=4.0)
        assert np.abs(R.blur_field(f, sigma) - ref).max() < 2e-6


def _remap_cases(rng):
    return ({"op": "elastic", "seed": 3, "alpha": 30.0, "sigma": 3.0},
            {"op": "grid_distortion", "num_steps": 5, "xsteps": list(1 + rng.uniform(-0.3, 0.3, 6)), "ysteps": list(1 + rng.uniform(-0.3, 0.3, 6))})


def test_remap_matches_map_coordinates():
    """cv2.remap's 1/32-pixel coordinates against exact bilinear interpolation, on a 3-channel frame.  A coordinate moves by at
    most 1/64 pixel on each axis, so a byte can move by up to (1/64 + 1/64) * 255 = 7.97 grey levels plus the roundings.
    Measured on this restatement: worst |difference| 5.341 levels (alpha 30 / sigma 3 and the grid distortion below).
    Asserted: the measured value plus one grey level."""
    from scipy import ndimage as ndi
    rng = _rng(6)
    img = rng.integers(0, 256, (36, 52, 3), dtype=np.uint8)
    worst = 0.0
    for d in _remap_cases(rng):
        mx, my = R.elastic_maps(36, 52, d) if d["op"] == "elastic" else R.grid_distortion_maps(36, 52, d)
        out, _ = R.remap(img, None, np.ascontiguousarray(mx, dtype=np.float32), np.ascontiguousarray(my, dtype=np.float32))
        for c in range(3):
            ref = ndi.map_coordinates(img[..., c].astype(np.float64), [my.astype(np.float64), mx.astype(np.float64)], order=1, mode="mirror")
            worst = max(worst, np.abs(out[..., c] - ref).max())
    print("remap vs map_coordinates: worst %.3f grey levels" % worst)
    assert worst <= 5.341 + 1.0


def test_remap_labels_against_an_explicit_gather():
    """Labels take the pixel at round-half-even of the map, reflect-101 outside: against a per-pixel gather from a frame padded
    by np.pad's reflect mode, with Python's round()."""
    rng = _rng(8)
    lab = rng.integers(0, 200, (36, 52)).astype(np.int64)
    P = 70
    pad = np.pad(lab, P, mode="reflect")
    moved = 0
    for d in _remap_cases(rng) + ({"op": "elastic", "seed": 4, "alpha": 40.0, "sigma": 4.0},):
        mx, my = R.elastic_maps(36, 52, d) if d["op"] == "elastic" else R.grid_distortion_maps(36, 52, d)
        mx, my = np.ascontiguousarray(mx, dtype=np.float32), np.ascontiguousarray(my, dtype=np.float32)
        _, out = R.remap(None, lab, mx, my)
        assert -P <= np.rint(mx).min() and np.rint(mx).max() < 52 + P and -P <= np.rint(my).min() and np.rint(my).max() < 36 + P
        want = np.array([[pad[round(float(my[y, x])) + P, round(float(mx[y, x])) + P] for x in range(52)] for y in range(36)])
        assert np.array_equal(out, want)
        moved += int((out != lab).sum())
    assert moved > 500                                     # the maps really move labels
    # a half-way coordinate goes to the even pixel; one pixel outside the frame reflects to pixel 1 / n - 2
    mx = np.array([[0.5, 1.5, 2.5, -1.0, 4.0]], dtype=np.float32)
    row = np.array([[10, 11, 12, 13]], dtype=np.int64)
    assert R.remap(None, row, mx[:, :4], np.zeros((1, 4), np.float32))[1].tolist() == [[10, 12, 12, 11]]
    assert R.remap(None, row, mx[:, 1:], np.zeros((1, 4), np.float32))[1].tolist() == [[12, 12, 11, 12]]


def test_grid_distortion_map_known_answers():
    """n = 10, two cells of 5 pixels stretched by 1.2 and 0.8: the first runs 0 .. 6 and the second 6 .. 10 in steps of a fifth of
    their length (end point left out); a third factor belongs to the pixels past the last whole cell (n = 11: one, at 10)."""
    from lm_net_amd.data import grid_distortion_map
    want = np.array([0, 1.2, 2.4, 3.6, 4.8, 6, 6.8, 7.6, 8.4, 9.2])
    got = grid_distortion_map(10, 2, [1.2, 0.8, 1.0])
    assert got.dtype == np.float32 and np.abs(got - want).max() < 1e-6
    got = grid_distortion_map(11, 2, [1.2, 0.8, 1.5])
    assert np.abs(got - np.append(want, 10.0)).max() < 1e-6
    got = grid_distortion_map(7, 3, [0.5, 1.5, 1.0, 2.0])    # cells of 2: 0 .. 1, 1 .. 4, 4 .. 6, then pixel 6 from 6 to 7
    assert np.abs(got - np.array([0, 0.5, 1, 2.5, 4, 5, 6])).max() < 1e-6


# ---------------------------------------------------------------- LAB tables
def _lab_f64(rgb):
    v = rgb.astype(np.float64) / 255.0
    lin = np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
    M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    xyz = lin @ M.T / M.sum(axis=1)
    f = np.where(xyz > 0.008856, np.cbrt(xyz), 7.787 * xyz + 16.0 / 116.0)
    return 116.0 * f[..., 1] - 16.0, 500.0 * (f[..., 0] - f[..., 1]), 200.0 * (f[..., 1] - f[..., 2])


def _rgb_f64(L8, a8, b8):
    fy = (L8 / 2.55 + 16.0) / 116.0
    fx, fz = fy + (a8 - 128.0) / 500.0, fy - (b8 - 128.0) / 200.0
    M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    xyz = np.stack([np.where(f > 6.0 / 29.0, f ** 3, (f - 16.0 / 116.0) / 7.787) for f in (fx, fy, fz)], axis=-1) * M.sum(axis=1)
    lin = np.clip(xyz @ np.linalg.inv(M).T, 0.0, 1.0)
    return np.clip(np.rint(255.0 * np.where(lin <= 0.0031308, lin * 12.92, 1.055 * lin ** (1.0 / 2.4) - 0.055)), 0, 255)


def test_integer_lab_against_float64():
    """64^3 lattice.  L8 within 1 of round(2.55 L*).  The inverse is within 1 of the float64 inverse of the SAME 8-bit triple.
    The round trip itself is limited by the 8-bit a / b, not by the integer path: a step of 1 in a8 is 1/500 in fx, which the cube
    and the steep start of the sRGB curve turn into up to 26 levels on a channel near 0 of a saturated colour ((0, 255, 243) ->
    (26, 255, 243)); the float64 inverse of the same triples measures the same 26, and so does the integer path.  Asserted: 26."""
    g = np.round(np.linspace(0, 255, 64)).astype(np.uint8)
    rgb = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    L, a, b = R.rgb2lab(rgb)
    Lf, af, bf = _lab_f64(rgb)
    assert np.abs(L - np.rint(2.55 * Lf)).max() <= 1
    assert np.abs(a - np.rint(af + 128)).max() <= 2 and np.abs(b - np.rint(bf + 128)).max() <= 2
    back = R.lab2rgb(L, a, b).astype(np.int64)
    ref = _rgb_f64(L.astype(np.float64), a.astype(np.float64), b.astype(np.float64))
    assert np.abs(back - ref).max() <= 1
    trip, trip_ref = np.abs(back - rgb.astype(np.int64)).max(), np.abs(ref - rgb).max()
    print("LAB round trip: integer %d, float64 %d" % (trip, trip_ref))
    assert trip_ref == 26 and trip <= 26
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    Lg, ag, bg = R.rgb2lab(grey)
    assert (ag == 128).all() and (bg == 128).all() and Lg[0] == 0 and Lg[255] == 255 and (np.diff(Lg) >= 0).all()
    assert np.abs(R.lab2rgb(Lg, ag, bg).astype(int) - grey).max() <= 1


# ---------------------------------------------------------------- ABI and argument checks
def test_exports_and_struct_sizes():
    from lm_net_amd import hip
    lib = hip.load()
    assert hip.SYMBOLS_ONEOF == ["lmn_sizeof_oneof_param", "lmn_oneof_workspace", "lmn_augment_oneof_u8"]
    assert hip.HEADERS["lmnet_oneof.h"] is hip.SYMBOLS_ONEOF       # (the header / export / layout checks: tests/test_host_cpu.py)
    assert lib.lmn_sizeof_oneof_param() == ctypes.sizeof(hip.OneOfParam) == 72
    assert lib.lmn_sizeof_aug_param() == ctypes.sizeof(hip.AugParam) == 176 and hip.ABI_VERSION == 15
    assert hip.oneof_workspace(3, 36, 52, 3, 2) == 3 * 64 * 256 + 2 * 4 * 36 * 52 * 4
    assert hip.oneof_workspace(1, 8, 8, 1, 0) == 64 * 256
    with pytest.raises(ValueError):
        hip.oneof_workspace(2, 8, 8, 3, 3)
    header = open(os.path.join(ROOT, "include", "lmnet_oneof.h")).read()
    for name, op in hip.ONEOF_OPS.items():
        assert re.search(r"#define LMN_ONEOF_%s %d\b" % (name.upper(), op), header), name
    for name in ("GAMMA", "CBRT", "FY", "DA", "DB", "FWD", "INV", "INVGAMMA", "TABLE_INTS"):
        assert re.search(r"#define LMN_LAB_%s %d\b" % (name, getattr(hip, "LAB_" + name)), header), name


def _entry(oneof, tables=None, channels=3, ws_bytes=None, B=1, H=32, W=32, lab=True, labels_tmp=True):
    """Call lmn_augment_oneof_u8 with fake device pointers: every case here must be rejected before any HIP call."""
    from lm_net_amd import hip
    from lm_net_amd.data import pack_params
    lib = hip.load()
    fake = ctypes.c_void_p(0x1000)
    mean, std = (ctypes.c_double * 3)(0.5, 0.5, 0.5), (ctypes.c_double * 3)(0.2, 0.2, 0.2)
    params = pack_params([{"crop": (0, 0, 50, 60)}] * B)
    n_el = sum(q.op == hip.ONEOF_OPS["elastic"] for q in oneof)
    if ws_bytes is None:
        ws_bytes = hip.oneof_workspace(B, H, W, channels, n_el)
    nt = 0 if tables is None else tables.size
    tab = None if tables is None else tables.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    rc = lib.lmn_augment_oneof_u8(fake, fake, params, None, fake, B, 50, 60, H, W, channels, 0, mean, std, fake, fake, fake, fake,
                                  oneof, fake, tab, ctypes.c_int64(nt), fake if nt else None, fake if lab else None, fake,
                                  fake if labels_tmp else None, fake, ctypes.c_int64(ws_bytes), None)
    return rc, lib.lmn_last_error().decode()


def test_c_entry_rejects_bad_arguments():
    from lm_net_amd import hip
    from lm_net_amd.data import pack_oneof

    def one(d, size=(32, 32)):
        return pack_oneof([{"oneof": d}], size)

    arr, _, _ = one(None)
    arr[0].op = 10
    rc, err = _entry(arr)
    assert rc == -1 and "unknown op" in err
    arr[0].op = -1
    assert "unknown op" in _entry(arr)[1]
    for d in ({"op": "to_gray"}, {"op": "hsv", "shift": [1, 2, 3]}, {"op": "channel_shuffle", "perm": [0, 1, 2]},
              {"op": "rgb_shift", "shift": [1, 2, 3]}):
        rc, err = _entry(one(d)[0], channels=1)
        assert rc == -1 and "colour member" in err, (d, err)
    arr = one({"op": "gaussian_blur", "k": 5})[0]
    for k in (4, 9, 1, 0):
        arr[0].k = k
        assert "gaussian_blur k" in _entry(arr)[1]
    arr = one({"op": "channel_shuffle", "perm": [0, 1, 2]})[0]
    arr[0].perm[:] = [0, 2, 2]
    assert "permutation" in _entry(arr)[1]
    arr, tab, _ = one({"op": "elastic", "seed": 1, "alpha": 1.0, "sigma": 2.0})
    assert "workspace" in _entry(arr, tab, ws_bytes=hip.oneof_workspace(1, 32, 32, 3, 1) - 1)[1]
    assert "labels_tmp" in _entry(arr, tab, labels_tmp=False)[1]
    assert "tables" in _entry(arr, tab[:-1].copy())[1]
    arr[0].v[1] = 0.0
    assert "sigma" in _entry(arr, tab)[1]
    arr[0].v[1], arr[0].radius = 2.0, hip.ONEOF_MAX_RADIUS + 1
    assert "radius" in _entry(arr, tab)[1]
    arr[0].radius, arr[0].slot = 8, 1
    assert "slot" in _entry(arr, tab)[1]
    arr, tab, _ = one({"op": "grid_distortion", "num_steps": 5, "xsteps": [1.0] * 6, "ysteps": [1.0] * 6})
    assert "tables" in _entry(arr, tab[:-1].copy())[1]
    arr[0].tab_off = -1
    assert "tables" in _entry(arr, tab)[1]
    arr = one({"op": "grid_dropout"})[0]
    arr[0].hole = arr[0].unit
    assert "grid_dropout" in _entry(arr)[1]
    arr = one({"op": "clahe", "clip": 2.0})[0]
    assert "lab_tables" in _entry(arr, lab=False)[1]
    arr[0].v[0] = 0.5
    assert "clip" in _entry(arr)[1]
    assert "workspace" in _entry(one(None)[0], ws_bytes=64 * 256 - 1)[1]
    # and the checks it shares with lmn_augment_u8
    rc, err = _entry(one(None)[0], channels=2, ws_bytes=64 * 256)
    assert rc == -1 and "channels" in err


def test_host_errors_raise_value_error():
    import torch
    from lm_net_amd.data import DeviceAugment, pack_oneof
    img = torch.zeros(2, 30, 40, 3, dtype=torch.uint8)              # CPU tensors: the checks run before the device check
    with pytest.raises(ValueError):
        DeviceAugment((16, 16))(img, None, oneof=pack_oneof([{}] * 2, (16, 16)))            # one_of not set
    aug = DeviceAugment((16, 16), one_of=["gaussian_blur"])
    with pytest.raises(ValueError):
        aug(img, None, params=aug.sample(2, (30, 40)), oneof=pack_oneof([{}] * 3, (16, 16)))
    with pytest.raises(ValueError):
        aug(img, None, params=[{"crop": (0, 0, 30, 40), "oneof": {"op": "gaussian_blur", "k": 6}}] * 2)
    with pytest.raises(RuntimeError, match="HIP device only"):
        aug(img, None)
    gray = DeviceAugment((16, 16), (0.5,), (0.2,), channels=1, one_of=["clahe"])
    with pytest.raises(ValueError):
        gray(img[..., 0], None, params=[{"crop": (0, 0, 30, 40), "oneof": {"op": "to_gray"}}] * 2)

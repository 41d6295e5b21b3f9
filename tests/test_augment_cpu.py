"""CPU: the training-augmentation restatement (tests/augment_ref.py) on hand-checkable cases, the host-side sampler of
lm_net_amd.data.DeviceAugment, the lmn_augment_u8 exports and its argument checks (no GPU needed)."""
import ctypes
import math

import numpy as np
import pytest

import augment_ref as A
from oracle import preprocess_ref as P


def _rng(seed):
    return np.random.default_rng(seed)


# ---------------------------------------------------------------- restatement
@pytest.mark.parametrize("C,mm", [(3, 0), (1, 1)])
def test_identity_params_reproduce_preprocess(C, mm):
    rng = _rng(1)
    img = rng.integers(0, 256, (37, 53, C), dtype=np.uint8)
    mask = rng.integers(0, 256 if mm == 0 else 64, (37, 53), dtype=np.uint8)
    mean, std = (0.485, 0.456, 0.406)[:C], (0.229, 0.224, 0.225)[:C]
    for fl in range(4):
        p = {"crop": (0, 0, 37, 53), "M": [1, 0, 0, 0, 1, 0], "flips": fl, "cj": [1.0, 1.0, 1.0, 0.0], "order": [3, 1, 0, 2]}
        x, y, g = A.augment_one(img, mask, p, (32, 48), mean, std, mm)
        im = P.resize_linear_u8(img, 32, 48)
        mk = P.resize_nearest((mask > 127).astype(np.uint8) if mm == 0 else mask, 32, 48)
        if fl & 1:
            im, mk = im[:, ::-1], mk[:, ::-1]
        if fl & 2:
            im, mk = im[::-1], mk[::-1]
        assert np.array_equal(x, P.normalize(np.ascontiguousarray(im), mean, std).transpose(2, 0, 1))
        assert np.array_equal(y, mk.astype(np.int64)) and g is None
    if C == 3:   # and the oracle's own batch entry
        xr, yr = P.preprocess(img[None], mask[None], (32, 48))
        x, y, _ = A.augment(img[None], mask[None], [{"crop": (0, 0, 37, 53)}], (32, 48), mean, std)
        assert np.array_equal(x, xr) and np.array_equal(y, yr)


def test_rotation_180_about_pixel_centre_is_both_flips():
    rng = _rng(2)
    H, W = 24, 31
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    cx, cy = W / 2 - 0.5, H / 2 - 0.5
    M = [-1.0, 0.0, 2 * cx, 0.0, -1.0, 2 * cy]   # getRotationMatrix2D((cx, cy), 180, 1) with cos = -1, sin = 0 exactly
    assert np.array_equal(A.warp_affine(img, M, True), img[::-1, ::-1])
    assert np.array_equal(A.warp_affine(img[..., 0], M, False), img[::-1, ::-1, 0])


@pytest.mark.parametrize("tx,ty", [(3, 0), (-2, 5), (7, -4)])
def test_integer_shift_is_shifted_copy_with_zero_border(tx, ty):
    rng = _rng(3)
    H, W = 20, 26
    img = rng.integers(1, 256, (H, W, 3), dtype=np.uint8)
    ref = np.zeros_like(img)
    ys, yd = (slice(0, H - ty), slice(ty, H)) if ty >= 0 else (slice(-ty, H), slice(0, H + ty))
    xs, xd = (slice(0, W - tx), slice(tx, W)) if tx >= 0 else (slice(-tx, W), slice(0, W + tx))
    ref[yd, xd] = img[ys, xs]
    M = [1.0, 0.0, float(tx), 0.0, 1.0, float(ty)]
    assert np.array_equal(A.warp_affine(img, M, True), ref)
    assert np.array_equal(A.warp_affine(img[..., 1], M, False), ref[..., 1])


def test_remap_table_and_the_plain_products_blend_alike():
    t = A.remap_table()
    assert (t.sum(axis=2) == 32768).all()
    fy, fx = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    plain = np.stack([(32 - fy) * (32 - fx), (32 - fy) * fx, fy * (32 - fx), fy * fx], axis=-1) * 32
    diff = np.argwhere((t != plain).any(axis=2))
    assert diff.tolist() == [[0, 0]] and t[0, 0].tolist() == [32767, 0, 0, 1]
    # the kernel blends with the plain products: the (0, 0) entry gives the same byte for every pair of neighbours
    v = np.arange(256)[:, None]
    w = np.arange(256)[None, :]
    assert ((v * 32767 + w + 16384) >> 15 == v).all() and ((v * 32768 + 16384) >> 15 == v).all()


def test_colour_factor_identities():
    img = _rng(4).integers(0, 256, (17, 19, 3), dtype=np.uint8)
    assert A.adjust_brightness(img, 1.0) is img and A.adjust_contrast(img, 1.0) is img
    assert A.adjust_saturation(img, 1.0) is img and A.adjust_hue(img, 0.0) is img
    out, g = A.color_jitter(img, [1.0, 1.0, 1.0, 0.0], [2, 0, 3, 1])
    assert out is img and g is None
    gray = img[..., :1]
    assert A.adjust_saturation(gray, 0.5) is gray and A.adjust_hue(gray, 0.3) is gray


def test_colour_ops_hand_values():
    img = np.array([[[100, 150, 200], [0, 255, 10]]], dtype=np.uint8)
    assert A.adjust_brightness(img, 0.5).tolist() == [[[50, 75, 100], [0, 127, 5]]]
    assert A.adjust_brightness(img, 2.0).tolist() == [[[200, 255, 255], [0, 255, 20]]]
    assert (A.adjust_brightness(img, 0.0) == 0).all()
    g = A.rgb2gray(img)
    assert g.tolist() == [[(100 * 4899 + 150 * 9617 + 200 * 1868 + 8192) >> 14, (255 * 9617 + 10 * 1868 + 8192) >> 14]]
    m = g.mean()
    assert (A.adjust_contrast(img, 0.0) == int(m + 0.5)).all()
    assert A.adjust_contrast(img, 0.5)[0, 0, 0] == int(100 * 0.5 + m * 0.5)
    sat0 = A.adjust_saturation(img, 0.0)
    assert (sat0 == g[..., None]).all()


def test_hsv_primaries_secondaries_greys():
    cases = {(255, 0, 0): (0, 255, 255), (0, 255, 0): (60, 255, 255), (0, 0, 255): (120, 255, 255),
             (255, 255, 0): (30, 255, 255), (0, 255, 255): (90, 255, 255), (255, 0, 255): (150, 255, 255)}
    for v in (0, 1, 77, 128, 255):
        cases[(v, v, v)] = (0, 0, v)
    rgb = np.array([list(cases)], dtype=np.uint8)
    hsv = A.rgb2hsv(rgb)
    assert [tuple(int(c) for c in p) for p in hsv[0]] == list(cases.values())
    assert np.array_equal(A.hsv2rgb(hsv), rgb)


def test_hsv_round_trip_bound():
    g = np.arange(0, 256, 5)
    rgb = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(1, -1, 3).astype(np.uint8)
    back = A.hsv2rgb(A.rgb2hsv(rgb))
    err = np.abs(back.astype(int) - rgb.astype(int)).max()
    # hue is quantised to 180 steps (2 degrees): a channel between min and max moves by at most ~ diff * 6 / 360 + rounding
    assert err <= 6, err


def test_hue_shift_rotates_primaries():
    red = np.array([[[255, 0, 0]]], dtype=np.uint8)
    assert A.adjust_hue(red, 1.0 / 3.0).tolist() == [[[0, 255, 0]]]      # +60 of 180: red -> green
    assert A.adjust_hue(red, -1.0 / 3.0).tolist() == [[[0, 0, 255]]]     # -60: red -> blue


# ---------------------------------------------------------------- sampler
def test_sampler_limits_and_fallback():
    from lm_net_amd.data import DeviceAugment
    aug = DeviceAugment((64, 64), generator=7)
    B = 400
    hw = np.stack([_rng(8).integers(20, 300, B), _rng(9).integers(20, 300, B)], axis=1)
    for d, (hs, ws) in zip(aug.sample_dicts(B, hw), hw):
        y0, x0, h, w = d["crop"]
        assert 0 <= y0 and 0 <= x0 and 0 < h and 0 < w and y0 + h <= hs and x0 + w <= ws
        area, ratio = h * w / (hs * ws), w / h
        fallback = (h == hs or w == ws) and y0 == (hs - h) // 2 and x0 == (ws - w) // 2
        # int(round()) of both sides: allow one pixel of rounding on each
        ok = ((0.8 * hs * ws - h - w - 1) / (hs * ws) <= area <= (1.0 * hs * ws + h + w + 1) / (hs * ws)
              and 3 / 4 * (1 - 1.0 / min(h, w)) - 1e-9 <= ratio * (1 + 1.0 / min(h, w)) and ratio * (1 - 1.0 / min(h, w)) <= 4 / 3 + 1e-9)
        assert ok or fallback, (d["crop"], hs, ws)
        assert -30 <= d["angle"] <= 30 and 0.9 <= d["scale"] <= 1.1 and abs(d["dx"]) <= 0.1 and abs(d["dy"]) <= 0.1
        assert d["flips"] in (0, 1, 2, 3) and sorted(d["order"]) == [0, 1, 2, 3]
    # a very thin frame forces the centre-crop fallback
    d = aug.sample_dicts(1, (10, 400))[0]
    assert d["crop"] == (0, (400 - round(10 * 4 / 3)) // 2, 10, round(10 * 4 / 3))


def test_sampler_factor_ranges_and_matrix():
    from lm_net_amd.data import DeviceAugment, ssr_matrix
    aug = DeviceAugment((96, 128), generator=np.random.default_rng(11), p_ssr=1.0, p_cj=1.0)
    for d in aug.sample_dicts(300, (200, 240)):
        b, c, s, h = d["cj"]
        assert 0.8 <= b <= 1.2 and 0.8 <= c <= 1.2 and 0.8 <= s <= 1.2 and -0.2 <= h <= 0.2
        a = math.radians(d["angle"])
        al, be = math.cos(a) * d["scale"], math.sin(a) * d["scale"]
        M = d["M"]
        assert np.allclose(M, [al, be, (1 - al) * 64 - be * 48 + d["dx"] * 128, -be, al, be * 64 + (1 - al) * 48 + d["dy"] * 96])
    assert ssr_matrix(10, 20, 0.0, 1.0, 0.1, -0.2) == [1.0, 0.0, 2.0, -0.0, 1.0, -2.0]


def test_sampler_rates_within_3_sigma():
    from lm_net_amd.data import DeviceAugment
    n = 20000
    aug = DeviceAugment((32, 32), generator=12, p_ssr=0.5, p_hflip=0.3, p_vflip=0.7, p_cj=0.4)
    ds = aug.sample_dicts(n, (40, 40))
    for got, p in ((sum(d["M"] is not None for d in ds), 0.5), (sum(d["flips"] & 1 for d in ds), 0.3),
                   (sum(d["flips"] >> 1 for d in ds), 0.7), (sum(d["cj"] is not None for d in ds), 0.4)):
        assert abs(got - n * p) <= 3 * math.sqrt(n * p * (1 - p)), (got, p)


def test_sampler_seed_reproducible():
    import torch
    from lm_net_amd.data import DeviceAugment
    a = DeviceAugment((64, 64), generator=5).sample(6, (100, 120))
    b = DeviceAugment((64, 64), generator=5).sample(6, (100, 120))
    assert bytes(a) == bytes(b)
    c = DeviceAugment((64, 64), generator=torch.Generator().manual_seed(9)).sample(6, (100, 120))
    d = DeviceAugment((64, 64), generator=torch.Generator().manual_seed(9)).sample(6, (100, 120))
    assert bytes(c) == bytes(d) and bytes(a) != bytes(c)


def test_packed_inverse_matches_restatement():
    from lm_net_amd.data import DeviceAugment
    ps = DeviceAugment((64, 80), generator=3, p_ssr=1.0).sample_dicts(20, (90, 90))
    from lm_net_amd.data import pack_params
    arr = pack_params(ps)
    for p, d in zip(arr, ps):
        assert list(p.iM) == A.invert_affine(d["M"]) and list(p.M) == list(d["M"]) and p.apply_ssr == 1


# ---------------------------------------------------------------- ABI and argument checks
def test_exports_and_struct_size():
    from lm_net_amd import hip
    assert "lmn_augment_u8" in hip.SYMBOLS and "lmn_sizeof_aug_param" in hip.SYMBOLS
    lib = hip.load()
    assert lib.lmn_sizeof_aug_param() == ctypes.sizeof(hip.AugParam) == 176
    assert hip.ABI_VERSION == 15 and lib.lmn_abi_version() == 15


def _entry(params, src_hw=None, B=1, Hs=50, Ws=60, H=32, W=32, channels=3, mask_mode=0):
    """Call lmn_augment_u8 with fake device pointers: every case here must be rejected before any HIP call."""
    from lm_net_amd import hip
    lib = hip.load()
    fake = ctypes.c_void_p(0x1000)
    mean, std = (ctypes.c_double * 3)(0.5, 0.5, 0.5), (ctypes.c_double * 3)(0.2, 0.2, 0.2)
    hw = None if src_hw is None else (ctypes.c_int32 * (2 * B))(*[v for p in src_hw for v in p])
    rc = lib.lmn_augment_u8(fake, fake, params, hw, fake, B, Hs, Ws, H, W, channels, mask_mode, mean, std, fake, fake, fake, fake, None)
    return rc, lib.lmn_last_error().decode()


def test_c_entry_rejects_bad_arguments():
    from lm_net_amd.data import pack_params
    good = {"crop": (0, 0, 50, 60)}
    for kw, crop, hw, words in [({"channels": 2}, None, None, "channels"), ({"mask_mode": 2}, None, None, "mask_mode"),
                                ({"H": 0}, None, None, "output size"), ({}, (10, 20, 41, 10), None, "crop window"),
                                ({}, (0, 0, 30, 30), [(20, 60)], "crop window"), ({}, (0, 0, 10, 10), [(51, 60)], "src_hw")]:
        params = pack_params([{"crop": crop} if crop else good])
        rc, err = _entry(params, hw, **kw)
        assert rc == -1 and words in err, (kw, crop, err)
    p = pack_params([good])
    p[0].h = 0
    assert "crop window" in _entry(p)[1]
    p = pack_params([{"crop": (0, 0, 50, 60), "cj": [1, 1, 1, 0]}])
    p[0].order[:] = [0, 1, 1, 3]
    assert "permutation" in _entry(p)[1]
    p = pack_params([{"crop": (0, 0, 50, 60), "M": [1, 0, 0, 0, 1, 0]}])
    p[0].iM[2] = 1e9
    assert "SSR" in _entry(p)[1]
    p = pack_params([good])
    p[0].flips = 4
    assert "flips" in _entry(p)[1]


def test_host_argument_errors_raise_value_error():
    import torch
    from lm_net_amd.data import DeviceAugment, pack_params
    for kw in ({"channels": 2}, {"mask_mode": "soft"}, {"mean": (0.5,)}, {"p_ssr": 1.5}, {"scale": (1.0, 0.5)},
               {"cj": (0.2, 0.2, 0.2, 0.7)}, {"generator": "seed"}, {"size": (0, 4)}):
        with pytest.raises(ValueError):
            DeviceAugment(**dict({"size": (32, 32)}, **kw))
    for bad in ({"crop": (0, 0, 0, 5)}, {"crop": (-1, 0, 5, 5)}, {"crop": (0, 0, 5, 5), "flips": 4},
                {"crop": (0, 0, 5, 5), "cj": [1, 1, 1, 0], "order": [0, 0, 1, 2]}, {"crop": (0, 0, 5, 5), "cj": [-1, 1, 1, 0]},
                {"crop": (0, 0, 5, 5), "M": [1, 0, 0, 0, 1]}, {"crop": (0, 0, 5, 5), "M": [1, 0, float("nan"), 0, 1, 0]}):
        with pytest.raises(ValueError):
            pack_params([bad])
    aug = DeviceAugment((16, 16))
    img = torch.zeros(2, 30, 40, 3, dtype=torch.uint8)          # CPU tensors: the checks run before the device check
    with pytest.raises(ValueError):
        aug(img, None, params=[{"crop": (0, 0, 30, 41)}, {"crop": (0, 0, 5, 5)}])
    with pytest.raises(ValueError):
        aug(img, None, params=[{"crop": (0, 0, 20, 20)}, {"crop": (0, 0, 21, 5)}], src_hw=[[30, 40], [20, 40]])
    with pytest.raises(ValueError):
        aug(img, None, src_hw=[[31, 40], [20, 40]])
    with pytest.raises(ValueError):
        aug(img, torch.zeros(2, 30, 41, dtype=torch.uint8))
    with pytest.raises(ValueError):
        DeviceAugment((16, 16), channels=1, mean=(0.5,), std=(0.2,))(img)
    with pytest.raises(RuntimeError, match="HIP device only"):
        aug(img, None, params=[{"crop": (0, 0, 30, 40)}, {"crop": (0, 0, 5, 5)}])

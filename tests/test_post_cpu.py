"""CPU: the numpy restatement of the post-processing (tests/post_ref.py) against scipy.ndimage and hand-made cases, the new C-ABI
symbols, the workspace arithmetic and the argument checks of lm_net_amd.post.DevicePostprocess.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import post_ref as R
import surface_ref as S

GEN = [(8, 352, 352, 2), (8, 352, 352, 9), (2, 512, 512, 4), (3, 64, 96, 5), (2, 128, 160, 33), (3, 37, 53, 3)]
S8 = np.ones((3, 3), int)


def _maps():
    for B, H, W, Cn in GEN:
        yield "ellipses %dx%dx%dx%d" % (B, H, W, Cn), R.punched_ellipses(B, H, W, Cn), Cn
    yield "tiling", S.tiling_case()[0], 64
    yield "noise", R.noise_case(), 2
    yield "serpentine", R.serpentine(256, 250), 2
    yield "checkerboard", R.checkerboard(128, 128), 2
    yield "one class", np.full((1, 40, 56), 3, np.int64), 5
    yield "background", np.zeros((1, 40, 56), np.int64), 5


# ---------------------------------------------------------------- the restatement against scipy
@pytest.mark.parametrize("connectivity", [8, 4])
def test_components_rank_equals_scipy_label(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    st = S8 if connectivity == 8 else None
    for name, maps, Cn in _maps():
        for L in R.label_map(maps, Cn):
            roots, areas = R.components(L, connectivity)
            for k in np.unique(L):
                lab, n = ndi.label(L == k, structure=st)
                assert np.array_equal(R.rank_labels(roots, L == k), lab), (name, int(k))
                rk = np.flatnonzero((roots.ravel() == np.arange(L.size)) & (L.ravel() == k))
                assert n == rk.size and np.array_equal(areas.ravel()[rk], np.bincount(lab.ravel())[1:]), (name, int(k))
            assert areas.sum() == L.size and (areas.ravel()[roots.ravel()] > 0).all()
            assert (roots.ravel() <= np.arange(L.size)).all()


@pytest.mark.parametrize("connectivity", [8, 4])
def test_filled_set_equals_binary_fill_holes(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    filled_total = 0
    for name, maps, Cn in _maps():
        for L in R.label_map(maps, Cn):
            L1, L2, stats, removed, holes = R.clean_one(L, Cn, connectivity, keep_largest=True, min_area=12, fill_holes=True)
            want = ndi.binary_fill_holes(L1 != 0, structure=None if connectivity == 8 else S8)
            assert np.array_equal(L2 != 0, want), name
            assert np.array_equal(L2[L1 != 0], L1[L1 != 0]) and stats[0, 3] == holes
            assert stats[:, 2].sum() == L.size and (stats[:, 1] <= stats[:, 0]).all()
            filled_total += holes
    assert filled_total > 100


def test_large_worst_cases_finish_and_have_the_known_answer():
    snake = R.serpentine()[0]
    roots, areas = R.components(snake, 8)
    assert (roots[snake == 1] == 0).all() and areas[0, 0] == (snake == 1).sum()
    r4, _ = R.components(snake, 4)
    assert (r4[snake == 1] == 0).all()
    board = R.checkerboard()[0]
    r8, a8 = R.components(board, 8)
    assert np.unique(r8).tolist() == [0, 1] and a8[0, 0] == a8[0, 1] == board.size // 2
    r4, a4 = R.components(board, 4)
    assert np.array_equal(r4.ravel(), np.arange(board.size)) and (a4 == 1).all()


def test_hand_made_cases():
    # two equal rectangles: the first in raster order survives keep_largest
    L = np.zeros((20, 30), np.uint8)
    L[2:6, 3:9] = 1
    L[10:14, 15:21] = 1
    _, L2, stats, removed, _ = R.clean_one(L, 2, 8, keep_largest=True)
    assert L2[2:6, 3:9].all() and not L2[10:14, 15:21].any() and removed == 1 and stats[1].tolist() == [2, 1, 24, 0]
    # a ring with an island inside: the ring's hole is filled with the ring's class, the island keeps its class
    L = np.zeros((20, 20), np.uint8)
    L[3:15, 3:15] = 1
    L[5:13, 5:13] = 0
    L[8:10, 8:10] = 2
    _, L2, stats, _, holes = R.clean_one(L, 3, 8, fill_holes=True)
    assert holes == 1 and (L2[3:15, 3:15] != 0).all() and (L2[8:10, 8:10] == 2).all()
    assert (L2[5:13, 5:13][L[5:13, 5:13] == 0] == 1).all() and stats[:, 2].tolist() == [400 - 144, 140, 4]
    # a hole that touches the frame is not filled; neither is one larger than the limit
    L = np.zeros((12, 12), np.uint8)
    L[0:6, 2:8] = 1
    L[0:3, 4:6] = 0                                   # open to the top frame
    assert np.array_equal(R.clean_one(L, 2, 8, fill_holes=True)[1], L)
    L = np.zeros((16, 16), np.uint8)
    L[2:12, 2:12] = 1
    L[4:7, 4:7] = 0                                   # 9 pixels
    L[9, 9] = 0                                       # 1 pixel
    L2 = R.clean_one(L, 2, 8, fill_holes=8)[1]
    assert L2[9, 9] == 1 and not L2[4:7, 4:7].any()
    assert R.clean_one(L, 2, 8, fill_holes=9)[1][2:12, 2:12].all()
    # a one-pixel diagonal chain: one component at 8, n at 4
    n = 9
    L = np.eye(n, dtype=np.uint8)
    r8, a8 = R.components(L, 8)
    r4, a4 = R.components(L, 4)
    assert (r8[L == 1] == 0).all() and a8[0, 0] == n
    assert np.array_equal(r4[L == 1], np.flatnonzero(L.ravel())) and (a4[L == 1] == 1).all()
    assert R.clean_one(L, 2, 4, min_area=2)[3] == n and R.clean_one(L, 2, 8, min_area=2)[3] == 0
    # the dual connectivity of the background: a diagonal gap leaks at connectivity 4 (background 8) and not at 8 (background 4)
    L = np.zeros((7, 7), np.uint8)
    L[1:6, 1:6] = 1
    L[2:5, 2:5] = 0
    L[1, 1] = 0
    assert R.clean_one(L, 2, 8, fill_holes=True)[4] == 1 and R.clean_one(L, 2, 4, fill_holes=True)[4] == 0
    # the 2x2 checkerboard tiling
    L = np.array([[0, 1], [1, 0]], np.uint8)
    assert R.components(L, 8)[0].tolist() == [[0, 1], [1, 0]] and R.components(L, 4)[0].tolist() == [[0, 1], [2, 3]]
    L = np.tile(L, (3, 4))
    assert np.unique(R.components(L, 8)[0]).size == 2 and np.unique(R.components(L, 4)[0]).size == L.size


def test_resize_and_overlay_restatement():
    L2 = np.arange(12, dtype=np.uint8).reshape(1, 3, 4) % 3
    lab = R.resize_back(L2, [(6, 8)], 7, 9)
    assert np.array_equal(lab[0, :6, :8], np.repeat(np.repeat(L2[0], 2, 0), 2, 1)) and not lab[0, 6].any() and not lab[0, :, 8].any()
    frames = np.random.default_rng(0).integers(0, 256, (1, 7, 9, 3)).astype(np.uint8)
    pal = R.default_palette(3)
    ov = R.overlay(lab, frames, [(6, 8)], pal, 1.0, "fill")
    want = frames.copy()
    for k in (1, 2):
        want = np.where((lab == k)[..., None], pal[k], want)
    want[:, 6:] = 0
    want[:, :, 8:] = 0
    assert np.array_equal(ov, want)
    half = R.overlay(lab, frames, [(6, 8)], pal, 0.5, "fill")
    y, x = np.argwhere(lab[0] == 1)[0]
    assert half[0, y, x].tolist() == [(128 * int(frames[0, y, x, c]) + 128 * int(pal[1, c]) + 128) >> 8 for c in range(3)]
    cont = R.overlay(lab, frames, [(6, 8)], pal, 1.0, "contour")
    blob = np.zeros((1, 8, 8), np.uint8)
    blob[0, 2:7, 2:7] = 1
    c = R.overlay(blob, np.zeros((1, 8, 8, 3), np.uint8), [(8, 8)], pal, 1.0, "contour")
    assert c[0, 2, 2].tolist() == [0, 0, 255] and not c[0, 4, 4].any() and (c[0, ..., 2] > 0).sum() == 16
    assert cont.shape == ov.shape


# ---------------------------------------------------------------- the C ABI
def test_symbols_abi_and_struct_size():
    from lm_net_amd import hip
    lib = hip.load()
    for name in ("lmn_post_workspace", "lmn_cc_label", "lmn_post_clean", "lmn_sizeof_post_param", "lmn_post_render",
                 "lmn_confusion_labels"):
        assert name in hip.SYMBOLS and hasattr(lib, name), name
    assert hip.ABI_VERSION == 15 and lib.lmn_abi_version() == 15
    assert lib.lmn_sizeof_post_param() == C.sizeof(hip.PostParam) == 280


def test_workspace_is_monotone_and_bounded():
    from lm_net_amd import hip
    base = hip.post_workspace(2, 100, 120)
    assert base >= 2 * 100 * 120 * 10
    assert hip.post_workspace(3, 100, 120) > base and hip.post_workspace(2, 101, 120) > base and hip.post_workspace(2, 100, 121) > base
    prev = 0
    for side in (2, 3, 64, 352, 1000, 1024):
        cur = hip.post_workspace(1, side, side)
        assert cur >= prev and (side < 64 or cur > prev)          # (sizes are rounded up to 256 bytes)
        prev = cur
    assert hip.post_workspace(1, 1024, 1024) < 16 << 20
    for bad in ((0, 64, 64), (1, 1, 64), (1, 64, 1), (1, 1025, 64), (1, 64, 1025), (65536, 64, 64)):
        with pytest.raises(ValueError, match="outside"):
            hip.post_workspace(*bad)


def test_entries_reject_bad_arguments_before_any_launch():
    from lm_net_amd import hip
    lib = hip.load()
    prm = hip.PostParam()
    prm.connectivity = 8
    one = C.c_void_p(256)                             # never dereferenced: every check below fails first
    assert lib.lmn_cc_label(one, 1, 64, 64, 6, None, C.c_int64(0), one, one, None) != 0
    assert b"connectivity" in lib.lmn_last_error()
    assert lib.lmn_cc_label(one, 1, 64, 2048, 8, None, C.c_int64(0), one, one, None) != 0
    prm.class_mask = 1
    assert lib.lmn_post_clean(one, None, None, 1, 4, 64, 64, C.byref(prm), one, C.c_int64(1 << 30), one, one, None) != 0
    assert b"class 0" in lib.lmn_last_error()
    prm.class_mask = 2
    prm.min_area[1] = -1
    assert lib.lmn_post_clean(one, None, None, 1, 4, 64, 64, C.byref(prm), one, C.c_int64(1 << 30), one, one, None) != 0
    assert b"min_area" in lib.lmn_last_error()
    prm.min_area[1] = 0
    assert lib.lmn_post_clean(one, None, None, 1, 4, 64, 64, C.byref(prm), one, C.c_int64(16), one, one, None) != 0
    assert b"too small" in lib.lmn_last_error()
    assert lib.lmn_post_clean(one, one, None, 1, 4, 64, 64, C.byref(prm), one, C.c_int64(1 << 30), one, one, None) != 0
    assert lib.lmn_post_clean(one, None, None, 1, 4, 64, 64, C.byref(prm), one, C.c_int64(1 << 30), one, None, None) != 0
    assert b"stats may be NULL only" in lib.lmn_last_error()      # labels-only form: nothing may be cleaned or filled
    hw = (C.c_int32 * 2)(65, 10)
    pal = (C.c_uint8 * 12)()
    assert lib.lmn_post_render(one, 1, 64, 64, hw, 64, 64, one, 3, pal, 4, 256, 0, one, one, None) != 0
    assert b"src_hw" in lib.lmn_last_error()
    assert lib.lmn_post_render(one, 1, 64, 64, None, 64, 40000, one, 3, pal, 4, 256, 0, one, one, None) != 0
    assert lib.lmn_post_render(one, 1, 64, 64, None, 64, 64, one, 3, pal, 4, 257, 0, one, one, None) != 0
    assert b"alpha256" in lib.lmn_last_error()
    assert lib.lmn_confusion_labels(one, one, 1, 65, C.c_int64(16), one, None) != 0


# ---------------------------------------------------------------- the module's host side
def test_device_postprocess_rejects_bad_arguments():
    from lm_net_amd.post import DevicePostprocess
    for kw in (dict(connectivity=6), dict(classes=[0, 1]), dict(classes=[1, 1]), dict(classes=[4]), dict(min_area=-1),
               dict(min_area=[1, 2]), dict(alpha=1.5), dict(alpha=-0.1), dict(palette=np.zeros((3, 3), np.uint8)),
               dict(palette=np.zeros((4, 4), np.uint8)), dict(overlay="edges"), dict(fill_holes=-3), dict(keep_largest=[3], classes=[1, 2])):
        with pytest.raises(ValueError):
            DevicePostprocess(4, **kw)
    for n in (1, 65):
        with pytest.raises(ValueError, match=r"\[2, 64\]"):
            DevicePostprocess(n)
    post = DevicePostprocess(4, keep_largest=[2], min_area=[3, 4, 5], fill_holes=50, classes=[1, 2, 3])
    assert post.params.class_mask == 0b1110 and post.params.keep_largest_mask == 0b100 and post.params.hole_limit == 50
    assert list(post.params.min_area[:5]) == [0, 3, 4, 5, 0] and post.params.connectivity == 8
    assert DevicePostprocess(4, fill_holes=True).params.hole_limit == 2 ** 31 - 1
    with pytest.raises(RuntimeError, match="no CPU path"):
        post(torch.zeros(1, 4, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        post.components(torch.zeros(1, 8, 8, dtype=torch.uint8))


def test_palette_and_alpha_host_arithmetic():
    from lm_net_amd import post
    assert [post.alpha256(a) for a in (0.0, 0.4, 0.5, 1.0, 0.998, 1 / 512)] == [0, 102, 128, 256, 255, 1]
    assert all(post.alpha256(a) == R.alpha256(a) for a in np.linspace(0, 1, 1001))
    pal = post.default_palette(64)
    assert pal.dtype == np.uint8 and pal.shape == (64, 3) and np.array_equal(pal, R.default_palette(64))
    assert pal[:4].tolist() == [[0, 0, 0], [0, 0, 255], [0, 255, 0], [255, 0, 0]]
    assert pal[4].tolist() == [0, 0, 128] and pal[7].tolist() == [128, 128, 128] and pal[8].tolist() == [64, 0, 0]
    assert len({tuple(c) for c in pal.tolist()}) == 64              # all distinct, none but class 0 black
    assert post.default_palette(2).tolist() == [[0, 0, 0], [0, 0, 255]]

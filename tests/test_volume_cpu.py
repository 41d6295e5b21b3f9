"""CPU: the host side of the per-case 3D metrics (include/volume/lmnet_volume.h, lm_net_amd.metrics.VolumeSurfaceMeter): registry and
header agree, the argument checks of the C entries (rejected before any HIP call, with fake device
pointers), the meter's float64 arithmetic on hand-made raw statistics and against the restatement tests/volume_ref.py, and that
restatement against the scipy recipe medpy uses (binary_erosion + distance_transform_edt with a sampling).  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import volume_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- ABI
def test_registry_and_header_agree():
    """The feature's own part of the registry: the literal list, its place in hip.HEADERS, the number and values of its #defines, the
    header's citations and the meter's record.  (Header / export / layout / return-type / constants checks: tests/test_host_cpu.py.)"""
    from lm_net_amd import hip
    assert hip.SYMBOLS_VOLUME == ["lmn_volume_workspace", "lmn_volume_labels", "lmn_volume_dist"]
    assert hip.HEADERS["volume/lmnet_volume.h"] is hip.SYMBOLS_VOLUME
    header = open(os.path.join(ROOT, "include", "volume", "lmnet_volume.h")).read()
    assert len(re.findall(r"^#define LMN_VOLUME_\w+ \d+\b", header, re.M)) == 3
    assert (hip.VOLUME_MAX_SIDE, hip.VOLUME_NSTAT_I, hip.VOLUME_NSTAT_F) == (1024, 9, 2)
    # the reference lines and the medpy functions the entries stand in for
    for cite in ("utils/train_eval_utils.py:7", ":178-179", ":14-52", "medpy.metric.binary", "hd95", "assd", "generate_binary_structure(3, 1)"):
        assert cite in header, cite
    from lm_net_amd import VolumeSurfaceMeter
    from lm_net_amd.metrics import SurfaceDistanceMeter
    assert VolumeSurfaceMeter.RAW_I == SurfaceDistanceMeter.RAW_I + ("n_both",) == R.RAW_I


# ---------------------------------------------------------------- argument checks
FAKE = ctypes.c_void_p(0x1000)


def _labels(null=None, logits=True, **kw):
    """lmn_volume_labels with fake device pointers: every case here must be rejected before any HIP call."""
    from lm_net_amd import hip
    lib = hip.load()
    a = dict(pred_logits=FAKE if logits else None, pred_labels=None if logits else FAKE, target=FAKE, lab_pred=FAKE, lab_target=FAKE)
    if null:
        a[null] = None
    g = dict(dict(n=4, C=9, H=33, W=65, D_cap=17, z0=5), **kw)
    rc = lib.lmn_volume_labels(a["pred_logits"], a["pred_labels"], a["target"], g["n"], g["C"], g["H"], g["W"], a["lab_pred"], a["lab_target"],
                               g["D_cap"], g["z0"], None)
    return rc, lib.lmn_last_error().decode()


def _dist(null=None, classes=(1, 2, 3), **kw):
    from lm_net_amd import hip
    lib = hip.load()
    a = dict(lab_pred=FAKE, lab_target=FAKE, classes=(ctypes.c_int32 * len(classes))(*classes), workspace=FAKE, stats_i=FAKE, stats_f=FAKE)
    if null:
        a[null] = None
    g = dict(dict(D=17, H=33, W=65, C=9, kz=1, ky=1, kx=1, ws_bytes=1 << 40), **kw)
    rc = lib.lmn_volume_dist(a["lab_pred"], a["lab_target"], g["D"], g["H"], g["W"], g["C"], a["classes"], len(classes), g["kz"], g["ky"],
                             g["kx"], a["workspace"], ctypes.c_int64(g["ws_bytes"]), a["stats_i"], a["stats_f"], None)
    return rc, lib.lmn_last_error().decode()


def test_entries_reject_bad_arguments():
    for name in ("target", "lab_pred", "lab_target"):
        rc, err = _labels(null=name)
        assert rc == -1 and err == "volume_labels: null pointer", (name, err)
    rc, err = _labels(null="pred_logits")
    assert rc == -1 and "exactly one of pred_logits, pred_labels" in err
    lib_rc, err = _labels(logits=False, null="pred_labels")
    assert lib_rc == -1 and "exactly one of" in err
    for kw, msg in ((dict(C=1), "C=1 not in [2, 64]"), (dict(C=65), "C=65 not in [2, 64]"), (dict(H=1), "size 1x65 outside [2, 1024]"),
                    (dict(W=1025), "size 33x1025 outside [2, 1024]"), (dict(D_cap=0), "D_cap=0 not in [1, 1024]"),
                    (dict(D_cap=1025), "D_cap=1025 not in [1, 1024]"), (dict(n=0), "slices [5, 5 + 0)"), (dict(z0=-1), "slices [-1, -1 + 4)"),
                    (dict(z0=14), "slices [14, 14 + 4) outside the case buffer of 17 slices"), (dict(n=2 ** 31 - 1), "outside the case buffer")):
        rc, err = _labels(**kw)
        assert rc == -1 and msg in err and err.startswith("volume_labels: "), (kw, err)
    for name in ("lab_pred", "lab_target", "classes", "workspace", "stats_i", "stats_f"):
        rc, err = _dist(null=name)
        assert rc == -1 and err == "volume_dist: null pointer", (name, err)
    for kw, msg in ((dict(C=1), "C=1 not in [2, 64]"), (dict(C=65), "C=65"), (dict(D=0), "D=0 not in [1, 1024]"), (dict(D=1025), "D=1025"),
                    (dict(H=1), "size 1x65 outside [2, 1024]"), (dict(W=1025), "size 33x1025"), (dict(classes=()), "nk=0 not in [1, 64]"),
                    (dict(classes=tuple(range(65)), C=64), "nk=65"), (dict(classes=(1, 9)), "classes[1] = 9 outside [0, 9)"),
                    (dict(classes=(-1,)), "classes[0] = -1"), (dict(kz=0), "pitches (0, 1, 1) must be positive"), (dict(kx=-3), "pitches (1, 1, -3)"),
                    (dict(ky=2 ** 31 - 1), "must be < 2^31"), (dict(kz=2000, ky=1000, kx=500), "= 3072000000 must be < 2^31 = 2147483648"),
                    (dict(ws_bytes=1000), "workspace of 1000 bytes too small")):
        rc, err = _dist(**kw)
        assert rc == -1 and msg in err and err.startswith("volume_dist: "), (kw, err)
    # the bound itself, on (2, 2, 2): 3 * 26754^2 = 2147329548 < 2^31 <= 3 * 26755^2; the first passes every check up to the workspace
    rc, err = _dist(D=2, H=2, W=2, kz=26754, ky=26754, kx=26754, ws_bytes=0)
    assert rc == -1 and "workspace of 0 bytes too small" in err, err
    rc, err = _dist(D=2, H=2, W=2, kz=26755, ky=26755, kx=26755, ws_bytes=0)
    assert rc == -1 and "= 2147490075 must be < 2^31" in err, err
    rc, err = _dist(D=1, H=2, W=2, kz=2 ** 31 - 1, ws_bytes=0)                     # one slice: the pitch along z multiplies nothing
    assert rc == -1 and "workspace of 0 bytes too small" in err, err


def test_workspace_is_host_arithmetic():
    from lm_net_amd import hip
    up = lambda v: (v + 255) // 256 * 256
    for D, H, W, nk in ((1, 2, 2, 1), (17, 66, 130, 8), (128, 352, 352, 8), (1024, 1024, 1024, 64)):
        V, rows = D * H * W, D * H
        assert hip.volume_workspace(D, H, W, nk) == up(4 * nk * V) + 2 * up(8 * nk * V) + up(8 * nk * rows) + up(2 * nk * rows)
    assert 20 * 128 * 352 * 352 <= hip.volume_workspace(128, 352, 352, 1) <= 20.1 * 128 * 352 * 352       # about 20 bytes per voxel and class
    for args, msg in (((0, 8, 8, 1), "D=0"), ((1025, 8, 8, 1), "D=1025"), ((4, 1, 8, 1), "1x8"), ((4, 8, 1025, 1), "8x1025"),
                      ((4, 8, 8, 0), "nk=0"), ((4, 8, 8, 65), "nk=65")):
        with pytest.raises(ValueError, match="volume_workspace"):
            hip.volume_workspace(*args)
        assert msg in hip.load().lmn_last_error().decode()
    assert hip.volume_span((2, 2, 2), (26754,) * 3) == 2147329548 < 2 ** 31 <= hip.volume_span((2, 2, 2), (26755,) * 3)
    assert hip.volume_span((128, 352, 352), (50, 13, 13)) == 6350 ** 2 + 2 * 4563 ** 2 < 2 ** 31


def test_python_wrappers_check_sizes_before_the_library():
    from lm_net_amd import hip
    lp, lt = torch.zeros(6, 5, 7, dtype=torch.uint8), torch.zeros(6, 5, 7, dtype=torch.uint8)
    z, t = torch.zeros(4, 3, 5, 7), torch.zeros(4, 5, 7, dtype=torch.int64)
    for args, msg in (((z, t, 3, lp, lt[:5]), "two uint8 volumes"), ((z, t[:3], 3, lp, lt), "do not match"), ((z, t[:, :4], 3, lp, lt), "do not match"),
                      ((z, t, 4, lp, lt), "logits with 4 channels"), ((z, t, 3, lp, lt, 3), r"slices \[3, 7\) outside the case buffer of 6"),
                      ((z, t, 3, lp, lt, -1), "outside the case buffer")):
        with pytest.raises(ValueError, match=msg):
            hip.volume_labels(*args)
    with pytest.raises(RuntimeError):                                # right sizes reach the pointer helpers, which refuse CPU tensors
        hip.volume_labels(z, t, 3, lp, lt, 2)
    ws, si, sf = torch.zeros(8, dtype=torch.uint8), torch.zeros(2, 9, dtype=torch.int64), torch.zeros(2, 2, dtype=torch.float64)
    for args, msg in (((lp, lt[:, :4], 3, [1, 2], (1, 1, 1), ws, si, sf), "two uint8 volumes"), ((lp, lt, 3, [1], (1, 1, 1), ws, si, sf), "do not match 1 classes"),
                      ((lp, lt, 3, [1, 2], (1, 1), ws, si, sf), "three positive integers"), ((lp, lt, 3, [1, 2], (1, 0.5, 1), ws, si, sf), "three positive integers"),
                      ((lp, lt, 3, [1, 2], (1, 1, 0), ws, si, sf), "three positive integers")):
        with pytest.raises(ValueError, match=msg):
            hip.volume_dist(*args)
    with pytest.raises(RuntimeError):
        hip.volume_dist(lp, lt, 3, [1, 2], (1, 1, 1), ws, si, sf)


def test_meter_refuses_what_it_cannot_run():
    from lm_net_amd import VolumeSurfaceMeter
    for kw, msg in ((dict(n_classes=1), "outside"), (dict(n_classes=65), "outside"), (dict(n_classes=3, classes=[1, 1]), "distinct"),
                    (dict(n_classes=3, classes=[3]), "distinct"), (dict(n_classes=3, classes=[]), "distinct"),
                    (dict(n_classes=2, spacing=(1.5, 1, 1)), "positive integers"), (dict(n_classes=2, spacing=(0, 1, 1)), "positive integers"),
                    (dict(n_classes=2, spacing=1), "positive integers"), (dict(n_classes=2, spacing=(1, 1)), "positive integers"),
                    (dict(n_classes=2, spacing=(1, 1, 2 ** 31)), "positive integers"), (dict(n_classes=2, unit=0.0), "unit"),
                    (dict(n_classes=2, workspace_mb=0), "workspace_mb")):
        with pytest.raises(ValueError, match=msg):
            VolumeSurfaceMeter(device="cpu", **kw)
    m = VolumeSurfaceMeter(9, spacing=(50.0, 13, 13), unit=0.06, device="cpu")    # integral floats are integers
    assert m.classes == list(range(1, 9)) and m.spacing == (50, 13, 13) and m.unit == 0.06
    assert tuple(m.raw()[0].shape) == (0, 8, 9) and tuple(m.raw()[1].shape) == (0, 8, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.update(torch.zeros(4, 9, 8, 8), torch.zeros(4, 8, 8, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.push(torch.zeros(4, 8, 8, dtype=torch.int64), torch.zeros(4, 8, 8, dtype=torch.int64))
    with pytest.raises(ValueError, match="no slices were pushed"):
        m.close_case()
    with pytest.raises(ValueError, match="add_raw"):
        m.add_raw(torch.zeros(1, 8, 8, dtype=torch.int64), torch.zeros(1, 8, 2, dtype=torch.float64))
    assert m.chunking(128, 352, 352) == 3                           # 1 GiB holds three classes of 317 MB each
    with pytest.raises(ValueError, match=r"needs \d+ bytes of scratch, workspace_mb allows %d" % (64 << 20)):
        VolumeSurfaceMeter(9, device="cpu", workspace_mb=64).chunking(128, 352, 352)
    assert VolumeSurfaceMeter(9, device="cpu", workspace_mb=4096).chunking(128, 352, 352) == 8


# ---------------------------------------------------------------- host arithmetic
def test_compute_on_hand_made_statistics():
    """Two cases x two classes.  Case 0: class 1 valid with 10 + 11 = 21 border voxels (95 * 20 = 1900: rank 19 exactly), class 2 an
    empty prediction; case 1: class 1 valid with 4 + 2 border voxels (rank 4.75), class 2 empty in both."""
    from lm_net_amd import VolumeSurfaceMeter
    m = VolumeSurfaceMeter(3, spacing=(4, 1, 1), unit=0.5, device="cpu")
    si = torch.tensor([[[30, 20, 10, 11, 49, 36, 25, 49, 15], [0, 7, 0, 5, 0, 0, 0, 0, 0]],
                       [[8, 16, 4, 2, 9, 16, 9, 16, 8], [0, 0, 0, 0, 0, 0, 0, 0, 0]]], dtype=torch.int64)
    sf = torch.tensor([[[20.0, 33.0], [0.0, 0.0]], [[6.0, 5.0], [0.0, 0.0]]], dtype=torch.float64)
    m.add_raw(si[:1], sf[:1])
    m.add_raw(si[1:], sf[1:])
    r = m.compute()
    pc = r["per_case"]
    assert pc is r["per_sample"] and set(pc) == {"hd", "hd95", "assd", "rvd", "dice", "jaccard"}
    assert all(pc[k].shape == (2, 2) and pc[k].dtype == np.float64 for k in pc)
    nan = np.nan
    want = {"hd": [[3.5, nan], [2.0, nan]], "hd95": [[2.5, nan], [0.5 * (3 + 0.75), nan]],
            "assd": [[0.5 * (2.0 + 3.0) / 2, nan], [0.5 * (1.5 + 2.5) / 2, nan]], "rvd": [[0.5, -1.0], [-0.5, 0.0]],
            "dice": [[30 / 50, 0.0], [16 / 24, nan]], "jaccard": [[15 / 35, 0.0], [0.5, nan]]}
    for k, w in want.items():
        assert np.allclose(pc[k], np.array(w), rtol=0, atol=1e-15, equal_nan=True) and np.array_equal(np.isnan(pc[k]), np.isnan(np.array(w))), (k, pc[k])
    assert r["classes"] == [1, 2] and r["valid"] == [2, 0] and r["empty_pred"] == [0, 1] and r["empty_target"] == [0, 0] and r["empty_both"] == [0, 1]
    assert r["hd"][0] == 2.75 and np.isnan(r["hd"][1]) and r["mean_hd"] == 2.75
    assert abs(r["dice"][0] - (0.6 + 2 / 3) / 2) < 1e-15 and r["dice"][1] == 0.0 and abs(r["mean_dice"] - (0.6 + 2 / 3) / 4) < 1e-15
    assert abs(r["jaccard"][0] - (15 / 35 + 0.5) / 2) < 1e-15 and r["jaccard"][1] == 0.0
    assert set(r) >= {"classes", "hd", "hd95", "assd", "rvd", "rvd_total", "valid", "empty_pred", "empty_target", "empty_both", "mean_hd",
                      "mean_hd95", "mean_assd", "per_sample", "dice", "jaccard", "mean_dice", "per_case"}
    m.reset()
    assert tuple(m.raw()[0].shape) == (0, 2, 9) and np.isnan(m.compute()["mean_dice"])


def test_meter_arithmetic_equals_the_restatement():
    """The meter's host half on the restatement's raw statistics gives the restatement's metrics, scaled by the unit."""
    from lm_net_amd import VolumeSurfaceMeter
    cases = [R.ellipsoid_case(9, 24, 30, 4), R.ellipsoid_case(6, 20, 26, 4, seed=1)]
    cases[1][0][cases[1][0] == 2] = 0                                 # an empty prediction
    classes, spacing, unit = [1, 2, 3], (3, 1, 2), 0.7
    si, sf, met = R.cases_stats(cases, classes, spacing)
    m = VolumeSurfaceMeter(4, spacing=spacing, unit=unit, device="cpu")
    m.add_raw(torch.from_numpy(si), torch.from_numpy(sf))
    pc = m.compute()["per_case"]
    for k in R.METRICS:
        want = met[k] * (unit if k in ("hd", "hd95", "assd") else 1.0)
        assert np.array_equal(np.isnan(pc[k]), np.isnan(want)), k
        assert np.allclose(pc[k], want, rtol=1e-13, atol=0, equal_nan=True), (k, pc[k], want)
    assert np.isnan(met["hd"][1, 1]) and met["dice"][1, 1] == 0.0 and not np.isnan(met["hd"][0]).any()


# ---------------------------------------------------------------- the restatement
def test_border_definition():
    one = np.zeros((1, 5, 6), bool)
    one[0, 1:4, 1:5] = True
    assert np.array_equal(R.border(one), one)                       # one slice: every mask voxel is a border voxel
    full = np.ones((4, 5, 6), bool)
    shell = full.copy()
    shell[1:-1, 1:-1, 1:-1] = False
    assert np.array_equal(R.border(full), shell)                    # a mask that fills the volume: the border is the shell
    cross = np.zeros((3, 3, 3), bool)
    cross[1, 1, :] = cross[1, :, 1] = cross[:, 1, 1] = True
    cube = np.ones((3, 3, 3), bool)
    cube[0, 0, 0] = False                                            # a diagonal neighbour does not count: the centre stays interior
    assert not R.border(np.pad(cube, 1))[2, 2, 2] and R.border(np.pad(cube, 1)).sum() == 25
    assert not R.border(np.pad(cross, 1))[2, 2, 2] and R.border(np.pad(cross, 1)).sum() == 6     # six neighbours are enough


def test_two_voxels_in_opposite_corners():
    p, t = R.corner_voxels(2, 2, 2)
    si, sf, met = R.pair_stats(p == 1, t == 1, (26754,) * 3)
    assert si.tolist() == [1, 1, 1, 1, 2147329548, 2147329548, 2147329548, 2147329548, 0]
    assert met["hd"] == float(np.sqrt(np.float64(2147329548))) and met["dice"] == 0.0
    p, t = R.corner_voxels(3, 4, 5)
    assert R.pair_stats(p == 1, t == 1, (4, 1, 3))[0][4] == 8 ** 2 + 3 ** 2 + 12 ** 2


@pytest.mark.parametrize("spacing", [(1, 1, 1), (3, 1, 1), (5, 2, 2)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("shape", [(1, 8, 8), (2, 2, 2), (5, 16, 12), (7, 33, 65)], ids=lambda s: "x".join(map(str, s)))
def test_restatement_against_scipy(shape, spacing):
    """The recipe of medpy's __surface_distances: border = mask ^ binary_erosion(mask, generate_binary_structure(3, 1)),
    distance_transform_edt(~border, sampling): round(edt^2) must equal the integer d2 exactly, at every voxel and at the border
    voxels of the other mask as sq_dists returns them."""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(sum(shape) + 10 * sum(spacing))
    lab = rng.integers(0, 3, shape)
    blob = np.zeros(shape, bool)
    blob[:max(1, shape[0] // 2), 1:max(2, shape[1] - 2), :max(1, shape[2] * 2 // 3)] = True
    for a, b in ((lab == 1, lab == 2), (blob, lab == 1), (np.ones(shape, bool), blob), (rng.random(shape) < 0.5, rng.random(shape) < 0.5)):
        st = ndi.generate_binary_structure(3, 1)
        ba, bb = (m ^ ndi.binary_erosion(m, structure=st, iterations=1) for m in (a, b))
        assert np.array_equal(R.border(a), ba) and np.array_equal(R.border(b), bb)
        edt = ndi.distance_transform_edt(~bb, sampling=spacing)
        want = np.rint(edt.astype(np.float64) ** 2).astype(np.int64)
        assert np.abs(edt ** 2 - want).max() < 1e-6                  # (the float transform is that close to an integer)
        assert np.array_equal(R.dist2_map(bb, spacing), want)
        assert np.array_equal(R.sq_dists(a, b, spacing), want[ba])


def test_generators_score_every_pair():
    """The condition the GPU tests rest on, decided here on the CPU: every (case, class) pair of the ellipsoid and tiling cases is
    valid."""
    for D, H, W, C in ((17, 66, 130, 9), (17, 66, 130, 2), (17, 66, 130, 4), (24, 64, 80, 9), (65, 9, 7, 2), (65, 9, 7, 9), (3, 5, 70, 2), (3, 5, 70, 4),
                       (3, 5, 70, 9), (6, 64, 96, 9)):
        p, t = R.ellipsoid_case(D, H, W, C)
        assert R.valid_share(p, t, range(1, C)) == (C - 1, C - 1), (D, H, W, C)
    p, t = R.tiling_case()
    assert R.valid_share(p, t, range(64)) == (64, 64) and (p != t).any()

"""CPU: the surface-distance restatement (tests/surface_ref.py) against scipy and on hand-worked cases, the lmn_surface_* exports
and argument checks, and the host half of lm_net_amd.metrics.SurfaceDistanceMeter (no GPU needed)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import surface_ref as S

CASES = [(8, 352, 352, 2), (8, 352, 352, 9), (2, 512, 512, 4), (3, 64, 96, 5), (2, 128, 160, 33), (3, 37, 53, 3)]


# ---------------------------------------------------------------- restatement against the scipy / medpy recipe
def _scipy_pair(P, T):
    """medpy.metric.binary's __surface_distances, hd, hd95 and assd, on scipy."""
    from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure
    fp = generate_binary_structure(2, 1)
    bp, bt = P ^ binary_erosion(P, structure=fp, iterations=1), T ^ binary_erosion(T, structure=fp, iterations=1)
    pt, tp = distance_transform_edt(~bt)[bp], distance_transform_edt(~bp)[bt]
    return bp, bt, pt, tp, max(pt.max(), tp.max()), np.percentile(np.hstack((pt, tp)), 95), (pt.mean() + tp.mean()) / 2


def _check_against_scipy(P, T):
    bp, bt, pt, tp, hd, hd95, assd = _scipy_pair(P, T)
    assert np.array_equal(S.border(P), bp) and np.array_equal(S.border(T), bt)
    d_pt, d_tp = S.sq_dists(P, T), S.sq_dists(T, P)
    assert np.array_equal(d_pt, np.rint(pt * pt).astype(np.int64)) and np.array_equal(d_tp, np.rint(tp * tp).astype(np.int64))
    assert np.array_equal(np.sqrt(d_pt.astype(np.float64)), pt)          # every distance, bit for bit
    _, _, m = S.pair_stats(P, T)
    assert m["hd"] == hd
    assert abs(m["hd95"] - hd95) <= 1.2e-13 and abs(m["assd"] - assd) <= 1.2e-13, (m, hd95, assd)


@pytest.mark.parametrize("B,H,W,C", CASES)
def test_reference_matches_scipy_on_the_generator_cases(B, H, W, C):
    pytest.importorskip("scipy")
    pred, target = S.ellipse_case(B, H, W, C)
    n = 0
    for b in range(B):
        for k in range(1, C):
            P, T = pred[b] == k, target[b] == k
            if P.any() and T.any():
                _check_against_scipy(P, T)
                n += 1
    assert n == S.valid_share(pred, target, range(1, C))[0] and n > 0


def test_reference_matches_scipy_on_random_small_masks():
    pytest.importorskip("scipy")
    rng = np.random.default_rng(7)
    n = 0
    while n < 200:
        H, W = rng.integers(3, 41, 2)
        p = rng.uniform(0.05, 0.95)
        P, T = rng.random((H, W)) < p, rng.random((H, W)) < rng.uniform(0.05, 0.95)
        if n % 3 == 0:                                             # blobs that touch the image edge
            P[:, 0] = True
            T[-1, :] = True
        if P.any() and T.any():
            _check_against_scipy(P, T)
            n += 1


@pytest.mark.parametrize("B,H,W,C", CASES)
def test_generator_cases_leave_at_most_a_fifth_of_the_pairs_unscored(B, H, W, C):
    """At 33 classes later ellipses cover some earlier ones (53 of 64 pairs stay valid); every other case keeps all its pairs."""
    pred, target = S.ellipse_case(B, H, W, C)
    v, t = S.valid_share(pred, target, range(1, C))
    assert t == B * (C - 1) and v >= 0.8 * t and (v == t or C == 33)


def test_tiling_case_scores_every_pair_at_64_classes():
    pred, target = S.tiling_case()
    assert S.valid_share(pred, target, range(1, 64)) == (126, 126)
    assert pred.max() == 63 and not np.array_equal(pred, target)


# ---------------------------------------------------------------- known answers
def test_known_answers():
    P, T = np.zeros((6, 7), bool), np.zeros((6, 7), bool)
    P[0, 0], T[3, 4] = True, True
    si, sf, m = S.pair_stats(P, T)
    assert m["hd"] == m["hd95"] == m["assd"] == 5.0 and m["rvd"] == 0.0
    assert si.tolist() == [1, 1, 1, 1, 25, 25, 25, 25] and sf.tolist() == [5.0, 5.0]
    blob = np.zeros((20, 30), bool)
    blob[4:15, 6:22] = True
    blob[0:6, 10:12] = True                                        # touches the top edge
    _, _, m = S.pair_stats(blob, blob)
    assert m["hd"] == m["hd95"] == m["assd"] == 0.0
    full, rect = np.ones((32, 48), bool), np.zeros((32, 48), bool)
    rect[10:20, 10:30] = True
    assert S.border(full).sum() == 2 * 32 + 2 * 48 - 4               # a mask that fills the image: the frame
    si, _, m = S.pair_stats(full, rect)
    assert m["hd"] == math.sqrt(468) and si[4] == 468               # frame corner (31, 47) to rectangle corner (19, 29)
    assert m["rvd"] == (32 * 48 - 200) / 200
    si, _, m = S.pair_stats(rect, np.zeros_like(rect))
    assert math.isnan(m["hd"]) and m["rvd"] == 0.0 and si.tolist() == [200, 0, 56, 0, 0, 0, 0, 0]


def test_percentile_rank_arithmetic():
    v = np.sqrt(np.arange(21, dtype=np.float64))                   # n = 21: 95 * 20 = 1900, a multiple of 100 -> v[19] itself
    assert S.percentile95(v) == v[19] == np.percentile(v, 95)
    v = np.sqrt(np.arange(8, dtype=np.float64))                    # n = 8: 95 * 7 = 665 -> v[6] + 0.65 (v[7] - v[6])
    want = v[6] + (v[7] - v[6]) * 65 / 100
    assert S.percentile95(v) == want and abs(want - np.percentile(v, 95)) < 1e-15
    assert S.percentile95(np.array([3.0])) == 3.0


# ---------------------------------------------------------------- ABI and argument checks
def test_exports():
    from lm_net_amd import hip
    assert "lmn_surface_workspace" in hip.SYMBOLS and "lmn_surface_dist" in hip.SYMBOLS
    lib = hip.load()
    assert hasattr(lib, "lmn_surface_workspace") and hasattr(lib, "lmn_surface_dist")
    assert hip.ABI_VERSION == 15 and lib.lmn_abi_version() == 15    # additive: new symbols under ABI 15


def test_workspace_is_monotone_and_bounds_the_chunk():
    from lm_net_amd import hip
    from lm_net_amd.metrics import SurfaceDistanceMeter
    base = (4, 8, 100, 120)
    w0 = hip.surface_workspace(*base)
    assert w0 >= 4 * 8 * 100 * 120 * 12                            # uint16 + int32 per pixel, map and pair
    for i in range(4):
        prev = 0
        for v in range(2, 40):
            a = list(base)
            a[i] = v
            w = hip.surface_workspace(*a)
            assert w >= prev
            prev = w
    for bad in [(0, 1, 8, 8), (1, 0, 8, 8), (1, 65, 8, 8), (1, 1, 1, 8), (1, 1, 8, 1025), (1024, 64, 8, 8)]:
        with pytest.raises(ValueError):
            hip.surface_workspace(*bad)
    for mb, nc, B, H, W in [(256, 9, 8, 352, 352), (8, 9, 8, 352, 352), (256, 64, 4, 1024, 1024), (16, 64, 2, 1024, 1024),
                            (1, 5, 7, 64, 96), (0.25, 3, 5, 37, 53)]:
        m = SurfaceDistanceMeter(nc, device="cpu", workspace_mb=mb)
        bs, ks = m.chunking(B, H, W)
        assert 1 <= bs <= B and 1 <= ks <= nc - 1 and (bs == 1 or ks == nc - 1)
        assert hip.surface_workspace(bs, ks, H, W) <= mb * (1 << 20)
    assert SurfaceDistanceMeter(9, device="cpu").chunking(8, 352, 352) == (8, 8)
    assert SurfaceDistanceMeter(64, device="cpu", workspace_mb=16).chunking(2, 1024, 1024) == (1, 1)
    with pytest.raises(ValueError):
        SurfaceDistanceMeter(2, device="cpu", workspace_mb=4).chunking(1, 1024, 1024)


def _entry(B=2, C=4, H=32, W=48, classes=(1, 2, 3), ws_bytes=1 << 30, logits=True, labels=False):
    """Call lmn_surface_dist with fake device pointers: every case here must be rejected before any HIP call."""
    from lm_net_amd import hip
    lib = hip.load()
    fake = ctypes.c_void_p(0x1000)
    ids = (ctypes.c_int32 * max(len(classes), 1))(*classes)
    rc = lib.lmn_surface_dist(fake if logits else None, fake if labels else None, fake, B, C, H, W, ids, len(classes), fake,
                              ctypes.c_int64(ws_bytes), fake, fake, None)
    return rc, lib.lmn_last_error().decode()


def test_c_entry_rejects_bad_arguments():
    from lm_net_amd import hip
    for kw, words in [({"H": 1}, "size"), ({"H": 1025}, "size"), ({"W": 1}, "size"), ({"W": 1025}, "size"), ({"classes": ()}, "nk"),
                      ({"classes": (1, 4)}, "class id"), ({"classes": (-1,)}, "class id"), ({"C": 65}, "C=65"), ({"C": 1}, "C=1"),
                      ({"B": 0}, "B=0"), ({"B": 30000}, "B * nk"), ({"logits": False}, "exactly one"), ({"labels": True}, "exactly one"),
                      ({"ws_bytes": hip.surface_workspace(2, 3, 32, 48) - 1}, "too small")]:
        rc, err = _entry(**kw)
        assert rc == -1 and words in err, (kw, err)


# ---------------------------------------------------------------- the meter's host half
def test_meter_has_no_cpu_fallback_and_checks_its_arguments():
    from lm_net_amd.metrics import SurfaceDistanceMeter
    m = SurfaceDistanceMeter(3, device="cpu")
    assert m.classes == [1, 2]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.update(torch.zeros(1, 3, 16, 16), torch.zeros(1, 16, 16, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.update(torch.zeros(1, 16, 16, dtype=torch.int64), torch.zeros(1, 16, 16, dtype=torch.int64))
    for kw in ({"n_classes": 1}, {"n_classes": 65}, {"classes": []}, {"classes": [1, 1]}, {"classes": [3]}, {"classes": [-1]},
               {"spacing": 0.0}, {"workspace_mb": 0}):
        with pytest.raises(ValueError):
            SurfaceDistanceMeter(**dict({"n_classes": 3, "device": "cpu"}, **kw))
    r = m.compute()                                                 # nothing seen yet
    assert r["valid"] == [0, 0] and math.isnan(r["mean_hd"]) and r["per_sample"]["hd"].shape == (0, 2) and r["rvd_total"] == [0.0, 0.0]


def test_compute_on_injected_raw_statistics():
    """Three samples, classes (1, 2), spacing 0.5; the raw statistics are written by hand (RAW_I order)."""
    from lm_net_amd.metrics import SurfaceDistanceMeter
    m = SurfaceDistanceMeter(3, spacing=0.5, device="cpu")
    assert m.RAW_I == S.RAW_I
    si = torch.tensor([[[10, 8, 6, 4, 25, 9, 16, 25], [0, 5, 0, 5, 0, 0, 0, 0]],
                       [[4, 8, 4, 4, 4, 1, 1, 4], [7, 0, 6, 0, 0, 0, 0, 0]],
                       [[1, 1, 1, 1, 100, 100, 100, 100], [0, 0, 0, 0, 0, 0, 0, 0]]], dtype=torch.int64)
    sf = torch.tensor([[[18.0, 8.0], [0.0, 0.0]], [[6.0, 2.0], [0.0, 0.0]], [[10.0, 10.0], [0.0, 0.0]]], dtype=torch.float64)
    m.add_raw(si[:2], sf[:2])
    m.add_raw(si[2:], sf[2:])
    r = m.compute()
    assert r["classes"] == [1, 2]
    assert r["valid"] == [3, 0] and r["empty_pred"] == [0, 1] and r["empty_target"] == [0, 1] and r["empty_both"] == [0, 1]
    # sample 0: n = 10, 95 * 9 = 855 -> lo 8, rem 55: 4 + (5 - 4) * 0.55; sample 1: n = 8, 665 -> rem 65: 1 + (2 - 1) * 0.65
    hd = np.array([5.0, 2.0, 10.0]) * 0.5
    hd95 = np.array([4 + 0.55, 1 + 0.65, 10.0]) * 0.5
    assd = np.array([(18 / 6 + 8 / 4) / 2, (6 / 4 + 2 / 4) / 2, 10.0]) * 0.5
    ps = r["per_sample"]
    assert np.array_equal(ps["hd"][:, 0], hd) and np.allclose(ps["hd95"][:, 0], hd95, rtol=0, atol=1e-15)
    assert np.allclose(ps["assd"][:, 0], assd, rtol=0, atol=1e-15)
    assert np.isnan(ps["hd"][:, 1]).all() and np.isnan(ps["hd95"][:, 1]).all() and np.isnan(ps["assd"][:, 1]).all()
    assert abs(r["hd"][0] - hd.mean()) < 1e-15 and abs(r["hd95"][0] - hd95.mean()) < 1e-15 and abs(r["assd"][0] - assd.mean()) < 1e-15
    assert math.isnan(r["hd"][1]) and math.isnan(r["hd95"][1]) and math.isnan(r["assd"][1])
    assert r["mean_hd"] == r["hd"][0] and r["mean_hd95"] == r["hd95"][0] and r["mean_assd"] == r["assd"][0]
    rvd = np.array([[2 / 8, -1.0], [-4 / 8, 0.0], [0.0, 0.0]])     # spacing does not touch RVD; |T| = 0 -> 0
    assert np.array_equal(ps["rvd"], rvd) and np.allclose(r["rvd"], rvd.mean(0), rtol=0, atol=1e-15)
    assert r["rvd_total"] == [(15 - 17) / 17, (7 - 5) / 5]
    m.reset()
    assert m.compute()["valid"] == [0, 0]
    with pytest.raises(ValueError):
        m.add_raw(si[:, :1], sf[:, :1])


def test_host_metrics_agree_with_the_reference_formulas():
    """surface_metrics on the reference's own raw statistics reproduces the reference's metrics (the GPU test's comparison, host only)."""
    from lm_net_amd.metrics import surface_metrics
    pred, target = S.ellipse_case(3, 64, 96, 5)
    pred[0][pred[0] == 2] = 0                                        # one empty prediction
    si, sf, met = S.batch_stats(pred, target, [1, 2, 3, 4])
    r = surface_metrics(si, sf, [1, 2, 3, 4])
    assert r["empty_pred"] == [0, 1, 0, 0]
    for k in ("hd", "hd95", "assd", "rvd"):
        a, b = r["per_sample"][k], met[k]
        assert np.array_equal(np.isnan(a), np.isnan(b))
        ok = ~np.isnan(b)
        if k == "hd":
            assert np.array_equal(a[ok], b[ok])
        else:
            assert (np.abs(a[ok] - b[ok]) <= 1e-9 * np.maximum(1, np.abs(b[ok]))).all()

"""GPU: lm_net_amd.metrics.VolumeSurfaceMeter (lmn_volume_labels, lmn_volume_dist) against the numpy restatement (tests/volume_ref.py)
on host copies.  Every integer raw statistic must be equal and HD equal (the square root of an exactly known integer); the float64
sums, HD95, ASSD, RVD, Dice and Jaccard within 1e-9 * max(1, |reference|), the bar tests/test_surface_gpu.py holds the 2D meter to:
HD95, RVD and Dice are a handful of float64 operations on exact integers, the sums float64 sums of at most 2^18 non-negative terms
here (relative error <= n * 2^-53 ~ 3e-11 for any fixed order).

The shapes, each for what can go wrong at it: (1, 2, 2) and (2, 2, 2) the minimum; (3, 5, 70) x crosses a 64-lane boundary;
(65, 9, 7) z crosses a 64-slice segment; (17, 66, 130) more than one x tile, rows that are no multiple of the 8 rows in flight.  The
restatement of every case is computed once per process and shared."""
import functools

import numpy as np
import pytest
import torch

import volume_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 2), (2, 2, 2), (3, 5, 70), (65, 9, 7), (17, 66, 130)]
_ids = lambda s: "x".join(map(str, s))


def _meter(n_classes, **kw):
    from lm_net_amd import VolumeSurfaceMeter
    return VolumeSurfaceMeter(n_classes, **kw)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                     # (a copy: the shared cases are read-only)


@functools.lru_cache(maxsize=None)
def _ellipsoids(D, H, W, C):
    if min(D, H, W) <= 2:                                            # the minimum shapes: no room for ellipsoids, random labels
        rng = np.random.default_rng(D + C)
        pred, target = rng.integers(0, C, (D, H, W)), rng.integers(0, C, (D, H, W))
    else:
        pred, target = R.ellipsoid_case(D, H, W, C)
    for a in (pred, target):
        a.setflags(write=False)
    return pred, target


@functools.lru_cache(maxsize=None)
def _reference(D, H, W, C, spacing):
    pred, target = _ellipsoids(D, H, W, C)
    return R.cases_stats([(pred, target)], list(range(1, C)), spacing)


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    ok = ~np.isnan(b)
    err = np.abs(a[ok] - b[ok]) / np.maximum(1, np.abs(b[ok]))
    print("%s: max error %.3e over %d values (bar 1e-9)" % (what, err.max() if err.size else 0.0, err.size))
    assert (err <= 1e-9).all(), (what, float(err.max()))


def _compare(m, ref, all_valid=False):
    """The meter's raw statistics and metrics (all cases so far) against ref = (si, sf, metrics) of the restatement."""
    si_r, sf_r, met = ref
    valid = (si_r[..., 0] > 0) & (si_r[..., 1] > 0)
    print("valid pairs: %d of %d" % (valid.sum(), valid.size))
    if all_valid:
        assert valid.all()                                           # on the restatement's own count, before anything is compared
    si, sf = (t.cpu().numpy() for t in m.raw())
    assert si.shape == si_r.shape and sf.shape == sf_r.shape
    bad = np.argwhere(si != si_r)
    assert bad.size == 0, (bad[:5].tolist(), si[tuple(bad[0][:2])].tolist(), si_r[tuple(bad[0][:2])].tolist())
    _close(sf, sf_r, "sums of sqrt(D2)")
    r = m.compute()
    pc = r["per_case"]
    assert np.array_equal(np.isnan(pc["hd"]), ~valid) and np.array_equal(pc["hd"][valid], met["hd"][valid] * m.unit)
    for k in ("hd95", "assd"):
        _close(pc[k], met[k] * m.unit, k)
    for k in ("rvd", "dice", "jaccard"):
        _close(pc[k], met[k], k)
    assert r["valid"] == valid.sum(0).tolist()
    return r


# ---------------------------------------------------------------- generator cases
@pytest.mark.parametrize("C", [2, 9])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_shapes_match_the_restatement(shape, C):
    pred, target = _ellipsoids(*shape, C)
    m = _meter(C)
    m.update(_dev(pred), _dev(target))
    _compare(m, _reference(*shape, C, (1, 1, 1)), all_valid=min(shape) > 2)


@pytest.mark.parametrize("spacing", [(4, 1, 1), (1, 3, 2)], ids=_ids)
@pytest.mark.parametrize("shape", SHAPES[2:], ids=_ids)
def test_anisotropic_pitches(shape, spacing):
    pred, target = _ellipsoids(*shape, 9)
    m = _meter(9, spacing=spacing, unit=0.75)
    m.update(_dev(pred), _dev(target))
    _compare(m, _reference(*shape, 9, spacing), all_valid=True)


def test_64_classes_on_the_block_tiling():
    pred, target = R.tiling_case()
    m = _meter(64, classes=list(range(64)))
    m.update(_dev(pred), _dev(target))
    r = _compare(m, R.cases_stats([(pred, target)], list(range(64))), all_valid=True)
    assert r["valid"] == [1] * 64 and r["classes"] == list(range(64))


def test_realistic_case_of_nine_classes():
    """24 x 64 x 80 with shifted, rescaled ellipsoids at thick slices, 3.0 x 0.78 x 0.78 mm as (50, 13, 13) steps of 0.06 mm."""
    pred, target = _ellipsoids(24, 64, 80, 9)
    m = _meter(9, spacing=(50, 13, 13), unit=0.06)
    m.update(_dev(pred), _dev(target))
    r = _compare(m, _reference(24, 64, 80, 9, (50, 13, 13)), all_valid=True)
    assert r["valid"] == [1] * 8 and 0.0 < r["mean_dice"] < 1.0 and r["mean_hd95"] <= r["mean_hd"]


# ---------------------------------------------------------------- corner cases
@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 5, 70), (65, 9, 7)], ids=_ids)
def test_two_voxels_in_opposite_corners(shape):
    """The nearest border voxel lies in another slice and another row; on (2, 2, 2) with pitch 26754 d2 = 3 * 26754^2 = 2147329548,
    just under 2^31: the top bits of the select and the no-overflow rule."""
    spacing = (26754,) * 3 if shape == (2, 2, 2) else (3, 2, 5)
    pred, target = R.corner_voxels(*shape)
    m = _meter(2, spacing=spacing)
    m.update(_dev(pred), _dev(target))
    ref = R.cases_stats([(pred, target)], [1], spacing)
    d2 = sum((k * (n - 1)) ** 2 for k, n in zip(spacing, shape))
    assert ref[0][0, 0].tolist() == [1, 1, 1, 1, d2, d2, d2, d2, 0] and (shape != (2, 2, 2) or d2 == 2147329548)
    _compare(m, ref, all_valid=True)


def test_one_pitch_step_above_the_bound_raises():
    pred, target = R.corner_voxels(2, 2, 2)
    m = _meter(2, spacing=(26755,) * 3)
    with pytest.raises(ValueError, match=r"\(kz \(D-1\)\)\^2 \+ \(ky \(H-1\)\)\^2 \+ \(kx \(W-1\)\)\^2 = 2147490075 .* 2\^31 = 2147483648"):
        m.update(_dev(pred), _dev(target))
    assert m.raw()[0].shape[0] == 0
    m.push(_dev(pred), _dev(target))                                  # the bound is checked when the case is closed
    with pytest.raises(ValueError, match="2147490075"):
        m.close_case()
    with pytest.raises(ValueError, match="no slices were pushed"):   # ... and the case is gone
        m.close_case()


def test_half_density_noise():
    """Nearly every voxel is a border voxel: long rows of results, runs of 0 / 1 / 2 in the histograms."""
    rng = np.random.default_rng(11)
    pred, target = ((rng.random((9, 20, 70)) < 0.5).astype(np.int64) for _ in range(2))
    m = _meter(2, spacing=(2, 1, 1))
    m.update(_dev(pred), _dev(target))
    ref = R.cases_stats([(pred, target)], [1], (2, 1, 1))
    assert ref[0][0, 0, 2] > 0.45 * 9 * 20 * 70 and ref[0][0, 0, 2] > 0.95 * ref[0][0, 0, 0]
    _compare(m, ref, all_valid=True)


def test_filled_volume_touching_corners_and_empty_masks():
    """Cases in sequence through one meter: a class that fills the volume (the border is the shell) against a blob; two blobs that
    touch opposite corners of the volume; a one-slice volume; an empty prediction, an empty target, both empty; labels that belong to
    no class."""
    D, H, W = 6, 10, 70
    z = np.zeros((D, H, W), np.int64)
    blob, blob2, c1, c2, oor = z.copy(), z.copy(), z.copy(), z.copy(), z.copy()
    blob[1:4, 2:7, 10:40] = 1
    blob2[2:6, 4:9, 30:68] = 1
    c1[:2, :3, :5] = 1
    c1[-1, -1, -1] = 1
    c2[-2:, -3:, -5:] = 1
    c2[0, 0, 0] = 1
    oor[...] = blob
    oor[0, :4, :8] = 77
    oor[5, 6:, 60:] = -3
    cases = [(np.ones_like(z), blob), (blob, np.ones_like(z)), (c1, c2), (z, blob), (blob, z), (z, z), (blob2, oor), (blob, blob)]
    m = _meter(2, spacing=(3, 1, 1))
    for p, t in cases:
        m.update(_dev(p), _dev(t))
    one = (blob[2:3] | blob2[2:3], blob[2:3])                          # one slice: every mask voxel is a border voxel
    m.update(_dev(one[0]), _dev(one[1]))
    ref = R.cases_stats(cases + [one], [1], (3, 1, 1))
    r = _compare(m, ref)
    shell = D * H * W - (D - 2) * (H - 2) * (W - 2)
    assert ref[0][0, 0, 2] == shell and ref[0][1, 0, 3] == shell
    assert ref[0][8, 0, 2] == ref[0][8, 0, 0] and ref[0][8, 0, 3] == ref[0][8, 0, 1]
    assert (r["empty_pred"], r["empty_target"], r["empty_both"], r["valid"]) == ([1], [1], [1], [6])
    pc = r["per_case"]
    assert pc["dice"][3, 0] == 0.0 and pc["dice"][4, 0] == 0.0 and np.isnan(pc["dice"][5, 0]) and pc["dice"][7, 0] == 1.0
    assert pc["hd"][7, 0] == 0.0 and pc["assd"][7, 0] == 0.0


@pytest.mark.parametrize("shape", [(2, 1024, 3), (1024, 2, 3), (2, 3, 1024)], ids=_ids)
def test_longest_sides(shape):
    """1024 along one axis: 64 slices per segment along z, the 128 KiB strip along y, 16 waves along x."""
    rng = np.random.default_rng(sum(shape))
    pred, target = ((rng.random(shape) < 0.03).astype(np.int64) for _ in range(2))
    pred.flat[0] = target.flat[-1] = 1
    m = _meter(2)
    m.update(_dev(pred), _dev(target))
    _compare(m, R.cases_stats([(pred, target)], [1]), all_valid=True)


# ---------------------------------------------------------------- input forms, chunking, reproducibility
def test_logits_input_equals_label_input_and_ties_pick_the_first_maximum():
    pred, target = _ellipsoids(17, 66, 130, 9)
    logits = np.random.default_rng(3).normal(size=(17, 9, 66, 130)).astype(np.float32)
    np.put_along_axis(logits, pred[:, None], 9.0, 1)               # arg-max = pred
    a, b = _meter(9), _meter(9)
    a.update(_dev(logits), _dev(target))
    b.update(_dev(pred), _dev(target))
    assert all(torch.equal(x, y) for x, y in zip(a.raw(), b.raw()))
    _compare(a, _reference(17, 66, 130, 9, (1, 1, 1)), all_valid=True)
    ties = np.random.default_rng(4).integers(0, 2, (5, 4, 12, 70)).astype(np.float32)      # two values: ties in most voxels
    tgt = np.random.default_rng(5).integers(0, 4, (5, 12, 70))
    m = _meter(4, classes=[0, 1, 2, 3])
    m.update(_dev(ties), _dev(tgt))
    _compare(m, R.cases_stats([(ties.argmax(1), tgt)], [0, 1, 2, 3]))      # np.argmax: the first maximum


def test_push_in_uneven_batches_equals_one_update():
    pred, target = _ellipsoids(17, 66, 130, 9)
    p, t = _dev(pred), _dev(target)
    whole = _meter(9, spacing=(4, 1, 1))
    whole.update(p, t)
    parts = _meter(9, spacing=(4, 1, 1))
    for a, b in ((0, 5), (5, 6), (6, 17)):                            # 5 + 1 + 11: the case buffers grow twice
        parts.push(p[a:b], t[a:b])
    parts.close_case()
    parts.push(p[:3], t[:3])                                          # a second case through the same meter, then a third
    with pytest.raises(ValueError, match="open case"):
        parts.push(p[3:5, :, :64], t[3:5, :, :64])
    with pytest.raises(ValueError, match="close_case"):
        parts.update(p, t)
    parts.close_case()
    parts.update(p, t)
    si, sf = parts.raw()
    wi, wf = whole.raw()
    assert si.shape == (3, 8, 9)
    for k in (0, 2):
        assert torch.equal(si[k], wi[0]) and torch.equal(sf[k].view(torch.int64), wf[0].view(torch.int64))
    ref3 = R.cases_stats([(pred[:3], target[:3])], list(range(1, 9)), (4, 1, 1))
    assert np.array_equal(si[1].cpu().numpy(), ref3[0][0])
    parts.push(p[:2], t[:2])
    parts.reset()                                                     # reset() drops the open case too
    assert parts.raw()[0].shape[0] == 0
    with pytest.raises(ValueError, match="no slices were pushed"):
        parts.close_case()


def test_statistics_do_not_depend_on_the_class_chunking():
    pred, target = _ellipsoids(17, 66, 130, 9)
    p, t = _dev(pred), _dev(target)
    from lm_net_amd import hip
    one = hip.volume_workspace(17, 66, 130, 1)
    big, small, mid = _meter(9), _meter(9, workspace_mb=one / 2 ** 20), _meter(9, workspace_mb=3.5 * one / 2 ** 20)
    assert (big.chunking(17, 66, 130), small.chunking(17, 66, 130), mid.chunking(17, 66, 130)) == (8, 1, 3)
    for m in (big, small, mid):
        m.update(p, t)
    bi, bf = big.raw()
    for m in (small, mid):
        oi, of = m.raw()
        assert torch.equal(oi, bi) and torch.equal(of.view(torch.int64), bf.view(torch.int64))
    with pytest.raises(ValueError, match=r"needs %d bytes of scratch, workspace_mb allows %d" % (one, one - 1)):
        _meter(9, workspace_mb=(one - 1) / 2 ** 20).update(p, t)


def test_two_calls_are_bit_identical_in_both_deterministic_modes():
    from lm_net_amd import hip
    pred, target = _ellipsoids(17, 66, 130, 9)
    rng = np.random.default_rng(7)
    noise = tuple((rng.random((9, 20, 70)) < 0.5).astype(np.int64) for _ in range(2))
    before = hip.get_deterministic()
    out = []
    try:
        for det in (False, True, False, True):
            hip.set_deterministic(det)
            m = _meter(9, spacing=(1, 3, 2))
            m.update(_dev(pred), _dev(target))
            m.update(_dev(noise[0]), _dev(noise[1]))
            out.append(tuple(x.cpu() for x in m.raw()))
    finally:
        hip.set_deterministic(before)
    for si, sf in out[1:]:
        assert torch.equal(si, out[0][0]) and torch.equal(sf.view(torch.int64), out[0][1].view(torch.int64))
    side = torch.cuda.Stream()                                        # ... and on a non-default torch stream
    side.wait_stream(torch.cuda.current_stream())
    ms = _meter(9, spacing=(1, 3, 2))
    with torch.cuda.stream(side):
        ms.update(_dev(pred), _dev(target))
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(ms.raw()[0].cpu(), out[0][0][:1]) and torch.equal(ms.raw()[1].cpu().view(torch.int64), out[0][1][:1].view(torch.int64))

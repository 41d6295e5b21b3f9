"""GPU: lm_net_amd.metrics.SurfaceDistanceMeter (lmn_surface_dist) against the numpy restatement (tests/surface_ref.py) on host
copies.  Every integer raw statistic must be equal and HD equal (the square root of an exactly known integer); HD95, ASSD, RVD and
the float64 sums within 1e-9 * max(1, |reference|): HD95 and RVD are a handful of float64 operations on exact integers, ASSD a
float64 sum of at most 2^21 non-negative terms (relative error <= n * 2^-53 ~ 2.3e-10 for any fixed order)."""
import numpy as np
import pytest
import torch

import surface_ref as S

pytestmark = pytest.mark.gpu

CASES = [(8, 352, 352, 2), (8, 352, 352, 9), (2, 512, 512, 4), (3, 64, 96, 5), (2, 128, 160, 33), (3, 37, 53, 3)]


def _meter(n_classes, **kw):
    from lm_net_amd.metrics import SurfaceDistanceMeter
    return SurfaceDistanceMeter(n_classes, **kw)


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    ok = ~np.isnan(b)
    err = np.abs(a[ok] - b[ok]) / np.maximum(1, np.abs(b[ok]))
    print("%s: max error %.3e over %d values (bar 1e-9)" % (what, err.max() if err.size else 0.0, err.size))
    assert (err <= 1e-9).all(), (what, float(err.max()))


def _compare(m, pred, target, min_valid=0.0):
    """The meter's raw statistics and metrics against the reference on the label maps pred / target (numpy, all updates so far)."""
    si_r, sf_r, met = S.batch_stats(pred, target, m.classes)
    valid = (si_r[..., 0] > 0) & (si_r[..., 1] > 0)
    print("valid pairs: %d of %d" % (valid.sum(), valid.size))
    assert valid.sum() >= min_valid * valid.size                  # on the reference's own count, before anything is compared
    si, sf = (t.cpu().numpy() for t in m.raw())
    bad = np.argwhere(si != si_r)
    assert bad.size == 0, (bad[:5].tolist(), si[tuple(bad[0][:2])].tolist(), si_r[tuple(bad[0][:2])].tolist())
    _close(sf, sf_r, "sums of sqrt(D2)")
    r = m.compute()
    ps = r["per_sample"]
    assert np.array_equal(np.isnan(ps["hd"]), ~valid) and np.array_equal(ps["hd"][valid], met["hd"][valid] * m.spacing)
    _close(ps["hd95"], met["hd95"] * m.spacing, "HD95")
    _close(ps["assd"], met["assd"] * m.spacing, "ASSD")
    _close(ps["rvd"], met["rvd"], "RVD")
    assert r["valid"] == valid.sum(0).tolist()
    for j in range(len(m.classes)):
        if valid[:, j].any():
            _close(r["hd95"][j], (met["hd95"][valid[:, j], j]).mean() * m.spacing, "class HD95")
            assert abs(r["hd"][j] - met["hd"][valid[:, j], j].mean() * m.spacing) <= 1e-12 * max(1, r["hd"][j])
        else:
            assert np.isnan(r["hd"][j]) and np.isnan(r["hd95"][j]) and np.isnan(r["assd"][j])
    return r, si_r


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("B,H,W,C", CASES)
def test_generator_cases_match_the_reference(B, H, W, C):
    pred, target = S.ellipse_case(B, H, W, C)
    m = _meter(C)
    m.update(_dev(pred), _dev(target))
    _compare(m, pred, target, min_valid=0.8)


def test_64_classes_on_the_rectangle_tiling():
    pred, target = S.tiling_case()
    m = _meter(64, spacing=0.75)
    m.update(_dev(pred), _dev(target))
    r, _ = _compare(m, pred, target, min_valid=0.8)
    assert r["valid"] == [2] * 63 and r["classes"] == list(range(1, 64))


def test_logits_input_equals_label_input_and_ties_pick_the_first_maximum():
    pred, target = S.ellipse_case(3, 64, 96, 5)
    logits = np.random.default_rng(3).normal(size=(3, 5, 64, 96)).astype(np.float32)
    np.put_along_axis(logits, pred[:, None], 9.0, 1)               # arg-max = pred
    a, b = _meter(5), _meter(5)
    a.update(_dev(logits), _dev(target))
    b.update(_dev(pred), _dev(target))
    assert all(torch.equal(x, y) for x, y in zip(a.raw(), b.raw()))
    _compare(a, pred, target, min_valid=0.8)
    ties = np.random.default_rng(4).integers(0, 2, (2, 4, 48, 80)).astype(np.float32)      # two values: ties in most pixels
    assert ((ties == ties.max(1, keepdims=True)).sum(1) > 1).mean() > 0.5
    tgt = np.random.default_rng(5).integers(0, 4, (2, 48, 80))
    m = _meter(4, classes=[0, 1, 2, 3])
    m.update(_dev(ties), _dev(tgt))
    _compare(m, ties.argmax(1), tgt)                               # np.argmax: the first maximum


def test_corner_cases():
    H, W = 40, 56
    z = np.zeros((H, W), np.int64)
    blob = z.copy()
    blob[10:25, 12:30] = 1
    blob2 = z.copy()
    blob2[13:30, 9:27] = 1
    pixel, line, cut = z.copy(), z.copy(), z.copy()
    pixel[7, 50] = 1
    line[5:35, 20] = 1
    cut[30:, 40:] = 1                                              # a blob cut by the image corner
    cut[0:4, 10:20] = 1
    oor = blob.copy()
    oor[0:8, 0:8] = 77                                             # target values that belong to no class
    oor[30:36, 30:36] = -3
    pairs = [(z, blob), (blob, z), (z, z), (np.ones_like(z), blob), (blob, np.ones_like(z)), (pixel, blob), (pixel, pixel),
             (line, blob2), (cut, blob2), (blob2, oor), (line, cut)]
    pred, target = np.stack([p for p, _ in pairs]), np.stack([t for _, t in pairs])
    m = _meter(2)
    m.update(_dev(pred), _dev(target))
    r, si_r = _compare(m, pred, target)
    assert (r["empty_pred"], r["empty_target"], r["empty_both"], r["valid"]) == ([1], [1], [1], [8])
    assert si_r[3, 0, 2] == 2 * H + 2 * W - 4                        # the class that fills the image: its border is the frame


def test_half_density_noise_at_352():
    rng = np.random.default_rng(11)
    pred, target = (rng.random((2, 352, 352)) < 0.5).astype(np.int64), (rng.random((2, 352, 352)) < 0.5).astype(np.int64)
    m = _meter(2)
    m.update(_dev(pred), _dev(target))
    _, si_r = _compare(m, pred, target, min_valid=1.0)
    assert si_r[:, 0, 2].min() > 50000                               # about half of all pixels are border pixels


def test_repeatable_chunked_accumulating_and_streams():
    pred, target = S.ellipse_case(3, 64, 96, 5)
    p, t = _dev(pred), _dev(target)
    m = _meter(5)
    m.update(p, t)
    m.update(p, t)
    si, sf = m.raw()
    assert si.shape == (6, 4, 8) and torch.equal(si[:3], si[3:]) and torch.equal(sf[:3].view(torch.int64), sf[3:].view(torch.int64))
    # 64x96: 12 bytes per pixel and pair + 2 per pixel and sample -> 0.2 MB holds one sample of two classes, 0.7 MB two whole samples
    small = _meter(5, workspace_mb=0.2)
    assert small.chunking(3, 64, 96) == (1, 2)
    small.update(p, t)
    mid = _meter(5, workspace_mb=0.7)
    assert mid.chunking(3, 64, 96) == (2, 4)
    mid.update(p, t)
    for other in (small, mid):
        oi, of = other.raw()
        assert torch.equal(oi, si[:3]) and torch.equal(of.view(torch.int64), sf[:3].view(torch.int64))
    # updates of different B, H, W accumulate in order; reset() clears
    pred2, target2 = S.ellipse_case(2, 128, 160, 5)
    m.reset()
    assert m.raw()[0].shape == (0, 4, 8)
    m.update(p[:1], t[:1])
    m.update(_dev(pred2), _dev(target2))
    s1, _, _ = S.batch_stats(pred[:1], target[:1], m.classes)
    s2, _, _ = S.batch_stats(pred2, target2, m.classes)
    assert np.array_equal(m.raw()[0].cpu().numpy(), np.concatenate([s1, s2]))
    assert m.compute()["per_sample"]["hd"].shape == (3, 4)
    # a non-default torch stream that is still busy when the updates are issued: the inputs reach the buffers only in stream order, so
    # a launch on any other stream counts another case; the call returns before the stream has drained; the bits are those of a
    # default-stream call (tests/busy.py)
    import busy
    import busy_cases as K
    from test_busy_meters_gpu import _make, _side
    busy.run(K.subjects()["SurfaceDistanceMeter"], _make("SurfaceDistanceMeter"), _side())


def test_largest_size_in_class_chunks():
    """1024 rows (64-row segments in the column pass), a width that is no multiple of 64, and a workspace that holds one pair."""
    pred, target = S.ellipse_case(1, 1024, 1000, 3)
    pred[0, :3, :] = 1                                              # borders on the first rows and in the last column
    target[0, :, -2:] = 2
    m = _meter(3, workspace_mb=16)
    assert m.chunking(1, 1024, 1000) == (1, 1)
    m.update(_dev(pred), _dev(target))
    _compare(m, pred, target, min_valid=1.0)


def test_end_to_end_on_the_models_logits():
    from lm_net_amd import LM_Net
    from tools.detweights import det_input, fill_module
    net = LM_Net(3, 4, filters=[12] * 5)
    fill_module(net, 5)
    net = net.cuda().eval()
    x = det_input((2, 3, 64, 96), "surface/x").cuda()
    with torch.no_grad():
        logits = net(x).float().contiguous()
    target = S.ellipse_case(2, 64, 96, 4)[1]
    m = _meter(4, classes=[0, 1, 2, 3])
    m.update(logits, _dev(target))
    pred = logits.cpu().numpy().argmax(1)
    assert logits.shape == (2, 4, 64, 96)
    _compare(m, pred, target)

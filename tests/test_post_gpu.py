"""GPU: lm_net_amd.post.DevicePostprocess (lmn_cc_label, lmn_post_clean, lmn_post_render) against the numpy restatement
(tests/post_ref.py) on host copies.  Every output -- roots, areas, labels_net, stats, labels, overlay -- must be EQUAL, element for
element: the whole feature is integer arithmetic and a single differing pixel is a bug."""
import numpy as np
import pytest
import torch

import post_ref as R
import surface_ref as S

pytestmark = pytest.mark.gpu

CASES = [(8, 352, 352, 2), (8, 352, 352, 9), (2, 512, 512, 4), (3, 64, 96, 5), (2, 128, 160, 33), (3, 37, 53, 3)]
CLEAN = dict(keep_largest=True, min_area=12, fill_holes=True)


def _post(n_classes, **kw):
    from lm_net_amd.post import DevicePostprocess
    return DevicePostprocess(n_classes, **kw)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(got != want)
    print("%s: %d of %d elements differ" % (what, len(bad), want.size))
    assert len(bad) == 0, (what, bad[:5].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())


def _check(pred, C, connectivity, min_removed=0, min_holes=0, **kw):
    """components() and the cleaned map / stats of the label map or logits `pred` (numpy) against the restatement."""
    want_net, want_stats, removed, holes = R.clean(pred, C, connectivity=connectivity, **kw)
    print("restatement: %d components removed, %d holes filled" % (removed, holes))
    assert removed >= min_removed and holes >= min_holes          # on the restatement alone, before anything is compared
    post = _post(C, connectivity=connectivity, **kw)
    p = _dev(pred)
    roots, areas = post.components(p)
    want_roots, want_areas = R.batch_components(pred, C, connectivity)
    _same(roots, want_roots, "roots")
    _same(areas, want_areas, "areas")
    out = post(p)
    _same(out.labels_net, want_net, "labels_net")
    _same(out.stats, want_stats, "stats")
    assert out.labels is None and out.overlay is None
    return out, want_net


@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("B,H,W,C", CASES)
def test_organ_like_maps(B, H, W, C, connectivity):
    _check(R.punched_ellipses(B, H, W, C), C, connectivity, min_removed=10, min_holes=2, **CLEAN)


@pytest.mark.parametrize("connectivity", [8, 4])
def test_tiling_uniform_and_background_maps(connectivity):
    _check(S.tiling_case()[0], 64, connectivity, **CLEAN)
    _check(np.full((2, 40, 56), 3, np.int64), 5, connectivity, **CLEAN)
    _check(np.zeros((2, 40, 56), np.int64), 5, connectivity, **CLEAN)
    _check(np.full((1, 2, 2), 1, np.int64), 2, connectivity, **CLEAN)


@pytest.mark.parametrize("connectivity", [8, 4])
def test_half_density_noise_at_352(connectivity):
    pred = R.noise_case()
    n = [int((R.components(l, connectivity)[1] > 0).sum()) for l in pred.astype(np.uint8)]
    print("components per image:", n)
    assert min(n) > (500 if connectivity == 8 else 10000)
    _check(pred, 2, connectivity, min_removed=100, min_holes=10, **CLEAN)
    _check(pred, 2, connectivity, keep_largest=False, min_area=3, fill_holes=4)


@pytest.mark.parametrize("connectivity", [8, 4])
def test_serpentine_1024x1000(connectivity):
    """One component with the longest possible chains, in an image whose width is no multiple of the tile."""
    pred = R.serpentine(1024, 1000)
    out, _ = _check(pred, 2, connectivity, **CLEAN)
    assert out.stats.cpu()[0, 1].tolist() == [1, 1, int(pred.sum()), 0]


@pytest.mark.parametrize("connectivity", [8, 4])
def test_pixel_checkerboard_1024x1024(connectivity):
    """2 components at connectivity 8, H * W at 4 (every pixel a root: the select pass's worst case)."""
    pred = R.checkerboard(1024, 1024)
    out, _ = _check(pred, 2, connectivity, keep_largest=True, min_area=0, fill_holes=False)
    assert out.stats.cpu()[0, 1, :2].tolist() == ([1, 1] if connectivity == 8 else [1 << 19, 1])
    _check(pred[:, :300, :200], 2, connectivity, **CLEAN)


def test_logits_equal_label_maps_ties_and_out_of_range_labels():
    pred = R.punched_ellipses(3, 64, 96, 5)
    logits = np.random.default_rng(3).normal(size=(3, 5, 64, 96)).astype(np.float32)
    np.put_along_axis(logits, pred[:, None], 9.0, 1)               # arg-max = pred
    post = _post(5, **CLEAN)
    a, b, c = post(_dev(logits)), post(_dev(pred)), post(_dev(pred.astype(np.uint8)))
    for x, y in ((a, b), (a, c)):
        assert torch.equal(x.labels_net, y.labels_net) and torch.equal(x.stats, y.stats)
    _check(logits, 5, 8, min_removed=10, **CLEAN)
    ties = np.random.default_rng(4).integers(0, 2, (2, 4, 48, 80)).astype(np.float32)      # two values: ties in most pixels
    assert ((ties == ties.max(1, keepdims=True)).sum(1) > 1).mean() > 0.5
    _check(ties, 4, 8, min_area=2)
    _check(ties, 4, 4, **CLEAN)
    oor = pred.copy()
    oor[:, 5:9, 5:40] = 5                                          # >= C: background
    oor[:, 20:22, 10:30] = 77
    oor[:, 30:33, 50:60] = -2
    oor[:, 40, :] = 300
    assert (R.label_map(oor, 5)[:, 40] == 0).all()
    _check(oor, 5, 8, **CLEAN)
    o8 = oor.copy()
    o8[(o8 < 0) | (o8 > 255)] = 200
    want = R.clean(o8, 5, connectivity=8, **CLEAN)
    got = post(_dev(o8.astype(np.uint8)))
    _same(got.labels_net, want[0], "labels_net of a uint8 map with values >= C")
    _same(got.stats, want[1], "stats of a uint8 map with values >= C")


def test_per_class_parameters():
    pred = R.punched_ellipses(2, 128, 160, 33)
    classes = [1, 2, 5, 8, 20, 32]
    kw = dict(classes=classes, keep_largest=[2, 20], min_area=[0, 5, 9, 40, 1, 3000], fill_holes=6)
    for connectivity in (8, 4):
        _check(pred, 33, connectivity, min_removed=2, min_holes=2, **kw)


def test_ragged_frames_labels_and_overlays():
    B, H, W, C = 3, 64, 96, 5
    pred = R.punched_ellipses(B, H, W, C)
    src_hw = np.array([[150, 201], [40, 57], [97, 96]])            # larger than the net, smaller than it, hs a prime
    Hs, Ws = 150, 203                                              # a padded buffer wider than every sample; 203 = 7 * 29
    rng = np.random.default_rng(21)
    frames = rng.integers(0, 256, (B, Hs, Ws, 3)).astype(np.uint8)
    net = R.clean(pred, C, connectivity=8, **CLEAN)[0]
    want_labels = R.resize_back(net, src_hw, Hs, Ws)
    assert want_labels[0].any() and want_labels[1].any() and want_labels[2].any()
    for mode in ("fill", "contour"):
        for alpha in (1.0, 0.4):
            post = _post(C, alpha=alpha, overlay=mode, **CLEAN)
            out = post(_dev(pred), src_hw=src_hw, frames=_dev(frames))
            _same(out.labels_net, net, "labels_net")
            _same(out.labels, want_labels, "labels")
            want = R.overlay(want_labels, frames, src_hw, post.palette, alpha, mode)
            painted = (want != R.overlay(np.zeros_like(want_labels), frames, src_hw, post.palette)).any(-1)
            print("%s alpha %.1f: %d painted pixels" % (mode, alpha, painted.sum()))
            assert painted.sum() > 500
            _same(out.overlay, want, "overlay %s %.1f" % (mode, alpha))
            if alpha == 1.0 and mode == "fill":                    # the reference's np.where
                ref = frames.copy()
                for k in range(1, C):
                    ref = np.where((want_labels == k)[..., None], post.palette[k], ref)
                for b in range(B):
                    ref[b, src_hw[b, 0]:] = 0
                    ref[b, :, src_hw[b, 1]:] = 0
                _same(out.overlay, ref, "overlay against np.where")
    # labels alone: Hs, Ws = the largest h and w; a (h, w) pair for all samples; grayscale frames; a custom palette
    post = _post(C, **CLEAN)
    out = post(_dev(pred), src_hw=src_hw)
    assert out.overlay is None
    _same(out.labels, R.resize_back(net, src_hw, 150, 201), "labels without frames")
    out = post(_dev(pred), src_hw=(33, 47))
    _same(out.labels, R.resize_back(net, [(33, 47)] * B, 33, 47), "labels of one (h, w)")
    pal = rng.integers(0, 256, (C, 3)).astype(np.uint8)
    gray = frames[..., 0].copy()
    for fr in (gray, gray[..., None]):
        post = _post(C, palette=pal, alpha=0.4, overlay="contour", **CLEAN)
        out = post(_dev(pred), frames=_dev(fr))
        full = [(Hs, Ws)] * B
        _same(out.labels, R.resize_back(net, full, Hs, Ws), "labels at the full frame")
        _same(out.overlay, R.overlay(R.resize_back(net, full, Hs, Ws), gray, full, pal, 0.4, "contour"), "grayscale overlay")


def test_frames_view_that_is_not_16_byte_aligned():
    B, H, W, C = 2, 37, 53, 3
    pred = R.punched_ellipses(B + 1, H, W, C)[1:]
    buf = np.random.default_rng(9).integers(0, 256, (B + 1, 45, 61)).astype(np.uint8)       # 45 * 61 is odd
    view = _dev(buf)[1:]
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    post = _post(C, alpha=0.4, **CLEAN)
    out = post(_dev(pred), frames=view)
    net = R.clean(pred, C, connectivity=8, **CLEAN)[0]
    full = [(45, 61)] * B
    want = R.resize_back(net, full, 45, 61)
    _same(out.labels, want, "labels")
    _same(out.overlay, R.overlay(want, buf[1:], full, post.palette, 0.4, "fill"), "overlay of an unaligned grayscale view")


def test_large_frames_and_identity_size():
    pred = R.punched_ellipses(8, 352, 352, 9)
    net = R.clean(pred, 9, connectivity=8, **CLEAN)[0]
    frames = np.random.default_rng(5).integers(0, 256, (8, 704, 704, 3)).astype(np.uint8)
    post = _post(9, alpha=0.4, **CLEAN)
    out = post(_dev(pred), frames=_dev(frames))
    full = [(704, 704)] * 8
    want = R.resize_back(net, full, 704, 704)
    _same(out.labels, want, "labels 704")
    _same(out.overlay, R.overlay(want, frames, full, post.palette, 0.4, "fill"), "overlay 704")
    out = post(_dev(pred), src_hw=(352, 352))
    _same(out.labels, net, "labels at the network size")


def test_repeatable_and_on_a_side_stream():
    pred = R.punched_ellipses(8, 352, 352, 9)
    frames = _dev(np.random.default_rng(6).integers(0, 256, (8, 500, 620, 3)).astype(np.uint8))
    src_hw = np.array([[500 - 13 * b, 620 - 17 * b] for b in range(8)])
    post = _post(9, alpha=0.4, overlay="contour", **CLEAN)
    p = _dev(pred)
    a, b = post(p, src_hw, frames), post(p, src_hw, frames)
    ra, rb = post.components(p), post.components(p)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])
    # a side stream that is still busy when the calls are issued (tests/busy.py): cleaning, ragged contour overlays and components of
    # inputs that reach the buffers only in stream order -- a launch, memset or copy on any other stream sees another case -- with no
    # wait for the stream and the bits of a default-stream call
    import busy
    import busy_cases as K
    from test_busy_data_gpu import _make, _side
    busy.run(K.subjects()["DevicePostprocess"], _make("DevicePostprocess"), _side())


def test_meters_take_cleaned_label_maps():
    from lm_net_amd.metrics import ConfusionMeter, SurfaceDistanceMeter
    B, H, W, C = 3, 64, 96, 5
    pred, target = S.ellipse_case(B, H, W, C)
    target[0, :4, :4] = 9                                          # labels that belong to no class are dropped
    logits = np.random.default_rng(8).normal(size=(B, C, H, W)).astype(np.float32)
    np.put_along_axis(logits, pred[:, None], 9.0, 1)
    t = _dev(target)
    ok = (target >= 0) & (target < C)
    want = np.bincount((C * target[ok] + pred[ok]).ravel(), minlength=C * C).reshape(C, C)
    for p in (_dev(pred), _dev(pred.astype(np.uint8)), _dev(pred.astype(np.int32))):
        m = ConfusionMeter(C)
        m.update(p, t)
        m.update(p, t)
        assert np.array_equal(m.total.cpu().numpy(), 2.0 * want)
    mb = ConfusionMeter(2)
    mb.update(_dev(pred > 0), t.clamp(max=1))                      # a bool map
    assert np.array_equal(mb.total.cpu().numpy(), 1.0 * np.bincount((2 * np.minimum(target, 1) + (pred > 0)).ravel(), minlength=4).reshape(2, 2))
    with pytest.raises(ValueError, match="INTEGER label map"):
        ConfusionMeter(C).update(_dev(pred).float(), t)            # a 3-D float tensor is neither logits nor a label map
    ml = ConfusionMeter(C)
    ml.update(_dev(logits), t)
    assert np.array_equal(ml.total.cpu().numpy(), 1.0 * want)
    # a cleaned map as it is: uint8 labels_net into both meters
    post = _post(C, **CLEAN)
    out = post(_dev(R.punched_ellipses(B, H, W, C)))
    net = R.clean(R.punched_ellipses(B, H, W, C), C, connectivity=8, **CLEAN)[0]
    mc = ConfusionMeter(C)
    mc.update(out.labels_net, t)
    assert np.array_equal(mc.total.cpu().numpy(), 1.0 * np.bincount((C * target[ok] + net[ok]).ravel(), minlength=C * C).reshape(C, C))
    a, b = SurfaceDistanceMeter(C), SurfaceDistanceMeter(C)
    a.update(out.labels_net, t)
    b.update(_dev(net.astype(np.int64)), t)
    assert all(torch.equal(x, y) for x, y in zip(a.raw(), b.raw()))
    si, _, _ = S.batch_stats(net.astype(np.int64), target, a.classes)
    assert np.array_equal(a.raw()[0].cpu().numpy(), si)


def test_end_to_end_on_the_models_logits():
    from lm_net_amd import LM_Net
    from tools.detweights import det_input, fill_module
    net = LM_Net(3, 4, filters=[12] * 5)
    fill_module(net, 5)
    net = net.cuda().eval()
    x = det_input((2, 3, 64, 96), "surface/x").cuda()
    with torch.no_grad():
        logits = net(x).float().contiguous()
    assert logits.shape == (2, 4, 64, 96)
    host = logits.cpu().numpy()
    for kw in (dict(min_area=4, fill_holes=True), CLEAN):
        post = _post(4, **kw)
        out = post(logits, src_hw=[(100, 150), (64, 96)])
        want_net, want_stats, removed, holes = R.clean(host, 4, connectivity=8, **kw)
        print("end to end: %d components removed, %d holes filled" % (removed, holes))
        _same(out.labels_net, want_net, "labels_net")
        _same(out.stats, want_stats, "stats")
        _same(out.labels, R.resize_back(want_net, [(100, 150), (64, 96)], 100, 150), "labels")
        roots, areas = post.components(logits)
        want_roots, want_areas = R.batch_components(host, 4, 8)
        _same(roots, want_roots, "roots")
        _same(areas, want_areas, "areas")

"""GPU: the 3D labelling and cleaning kernels (lm_net_amd/csrc/volpost.hip) through lm_net_amd.post.VolumePostprocess, element for
element against the numpy restatement tests/volpost_ref.py.  The shapes are the smallest where the kernels can go wrong: (2, 2, 2);
(1, 8, 8), one slice; (3, 5, 70), where x crosses a 64-wide tile and lane boundary and the rows are odd; (17, 66, 130), with tile
seams along both in-plane axes; (65, 9, 7), deeper than 64 slices -- each at connectivity 6, 18 and 26 with 2, 4 and 9 classes, from
logits with ties and from label maps with out-of-range values.  Then the adversarial cases, each with what it has to show (the
restatement's side of that is decided in tests/test_volpost_cpu.py::test_adversarial_cases_show_what_they_must)."""
import functools

import numpy as np
import pytest
import torch

import volpost_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def _np(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ref_components(kind, shape, C, connectivity):
    pred = R.tie_logits(shape, C) if kind == "logits" else R.blob_labels(shape, C)
    return R.components(R.label_volume(pred, C), connectivity)


def _kw(C):
    """Cleaning parameters that use every path: two selection passes for class 1, a minimal volume, a finite hole limit."""
    keep = {1: 2} if C == 2 else {1: 2, C - 1: 1}
    return dict(keep_largest=keep, min_volume=2, fill_holes=6)


@functools.lru_cache(maxsize=None)
def _ref_clean(kind, shape, C, connectivity):
    pred = R.tie_logits(shape, C) if kind == "logits" else R.blob_labels(shape, C)
    L2, stats, _ = R.clean(pred, C, connectivity, **_kw(C))
    return L2, stats


def _device_pred(kind, shape, C):
    if kind == "logits":
        return torch.from_numpy(R.tie_logits(shape, C)).to(DEV)
    return torch.from_numpy(R.blob_labels(shape, C)).to(DEV)                # int64, values in [-2, C + 2)


@pytest.mark.parametrize("kind", ["logits", "labels"])
@pytest.mark.parametrize("C", [2, 4, 9])
@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_components_and_clean_equal_the_restatement(shape, connectivity, C, kind):
    from lm_net_amd import VolumePostprocess
    post = VolumePostprocess(C, connectivity=connectivity, **_kw(C))
    pred = _device_pred(kind, shape, C)
    roots, sizes = post.components(pred)
    want_r, want_s = _ref_components(kind, shape, C, connectivity)
    assert roots.dtype == sizes.dtype == torch.int32 and tuple(roots.shape) == shape
    assert np.array_equal(_np(roots), want_r) and np.array_equal(_np(sizes), want_s)
    out = post(pred)
    L2, stats = _ref_clean(kind, shape, C, connectivity)
    assert out.labels.dtype == torch.uint8 and out.stats.dtype == torch.int32 and tuple(out.stats.shape) == (C, 4)
    assert np.array_equal(_np(out.labels), L2) and np.array_equal(_np(out.stats), stats)
    if shape[0] == 1:
        assert stats[0, 3] == 0                                               # a one-slice volume has no holes


@pytest.mark.parametrize("C", [2, 4, 9])
@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_uint8_label_maps_with_out_of_range_values(connectivity, C):
    """uint8 input: values in [C, 255] become 0 (an int64 -1 has no uint8 form; 255 stands in for it)."""
    from lm_net_amd import VolumePostprocess
    shape = (3, 5, 70)
    lab = R.blob_labels(shape, C)
    lab8 = np.where(lab < 0, 255, lab).astype(np.uint8)
    out = VolumePostprocess(C, connectivity=connectivity, **_kw(C))(torch.from_numpy(lab8).to(DEV))
    L2, stats = _ref_clean("labels", shape, C, connectivity)
    assert (lab8 >= C).any() and np.array_equal(_np(out.labels), L2) and np.array_equal(_np(out.stats), stats)


ONE_SLICE_SHAPES = [(1, 8, 8), (1, 33, 65), (1, 70, 130)]


def _seam_pairs(roots):
    """Same-component pixel pairs of the restatement's roots across row 32 and across column 64 (the first tile seams)."""
    r = roots[0]
    return int((r[31] == r[32]).sum()), int((r[:, 63] == r[:, 64]).sum())


@pytest.mark.parametrize("shape", ONE_SLICE_SHAPES, ids=ids)
@pytest.mark.parametrize("connectivity", [6, 26])
def test_one_slice_equals_the_2d_cleaning(connectivity, shape):
    """One slice with fill_holes=False: labels, stats, roots and sizes equal DevicePostprocess(connectivity=4 | 8) on the same map.
    (1, 8, 8) is a single tile; (1, 33, 65) is one pixel past a tile seam in each direction; (1, 70, 130) has two seams along each
    axis and ragged last tiles, so the 2D and the 3D kernels feed the shared tile and seam passes with different pointers and bases.
    Decided on the restatement alone first: where the shape has seams a component crosses row 32 and one crosses column 64, and the
    cleaning removes a component -- otherwise a seam bug would hide."""
    from lm_net_amd import VolumePostprocess
    from lm_net_amd.post import DevicePostprocess
    for C in (2, 4, 9):
        if shape[1] > 32:                                                     # (both seam shapes have seams along both axes)
            want_r, _ = _ref_components("labels", shape, C, connectivity)
            _, want_stats, _ = R.clean(R.blob_labels(shape, C), C, connectivity, keep_largest=True, min_volume=2)
            rows, cols = _seam_pairs(want_r)
            assert rows >= 1 and cols >= 1 and (want_stats[:, 0] - want_stats[:, 1]).sum() >= 1
        pred = _device_pred("labels", shape, C)
        a = VolumePostprocess(C, connectivity=connectivity, keep_largest=True, min_volume=2)(pred)
        b = DevicePostprocess(C, connectivity=4 if connectivity == 6 else 8, keep_largest=True, min_area=2)(pred)
        assert torch.equal(a.labels, b.labels_net) and torch.equal(a.stats, b.stats[0])
        r3, s3 = VolumePostprocess(C, connectivity=connectivity).components(pred)
        r2, s2 = DevicePostprocess(C, connectivity=4 if connectivity == 6 else 8).components(pred)
        assert torch.equal(r3, r2) and torch.equal(s3, s2)


@pytest.mark.parametrize("C", [2, 4, 9])
@pytest.mark.parametrize("shape", R.ORGAN_SHAPES, ids=ids)
def test_organ_cases(shape, C):
    """The generator whose conditions tests/test_volpost_cpu.py::test_generator_conditions decides: components removed by min_volume,
    a cavity filled, a cavity open to a face, a cavity above the limit, in every class."""
    from lm_net_amd import VolumePostprocess
    L = R.organ_case(*shape, C)
    dev = torch.from_numpy(L).to(DEV)
    for conn in (6, 18, 26):
        for kw in (dict(min_volume=R.ORGAN_MIN_VOLUME, fill_holes=R.ORGAN_HOLE_LIMIT), dict(keep_largest=2, fill_holes=True)):
            out = VolumePostprocess(C, connectivity=conn, **kw)(dev)
            L2, stats, _ = R.clean(L, C, conn, **kw)
            assert np.array_equal(_np(out.labels), L2) and np.array_equal(_np(out.stats), stats), (conn, kw)


def _comp_count(post, L):
    return _np(post(torch.from_numpy(L).to(DEV)).stats)[:, 0].tolist()


def test_parity_checkerboard():
    """One component per voxel under 6 (every voxel a root: one global atomic per block and class in the selection); two components
    under 18 and 26."""
    from lm_net_amd import VolumePostprocess
    L = R.parity_checkerboard()
    n1 = int(L.sum())
    assert _comp_count(VolumePostprocess(2, connectivity=6, keep_largest=True), L) == [L.size - n1, n1]
    for conn in (6, 18, 26):
        post = VolumePostprocess(2, connectivity=conn, keep_largest=True)
        roots, sizes = post.components(torch.from_numpy(L).to(DEV))
        want_r, want_s = R.components(L, conn)
        assert np.array_equal(_np(roots), want_r) and np.array_equal(_np(sizes), want_s)
        out = post(torch.from_numpy(L).to(DEV))
        L2, stats, _ = R.clean(L, 2, conn, keep_largest=True)
        assert np.array_equal(_np(out.labels), L2) and np.array_equal(_np(out.stats), stats)
        if conn != 6:
            assert stats[:, 0].tolist() == [1, 1]
        else:
            assert stats[1].tolist() == [n1, 1, 1, 0]                           # ties: the smallest root, voxel 1, stays


def test_corner_and_edge_pairs_tell_the_connectivities_apart():
    from lm_net_amd import VolumePostprocess
    L = R.touching_pairs()
    got = [_comp_count(VolumePostprocess(3, connectivity=c), L)[1:] for c in (6, 18, 26)]
    assert got == [[2, 2], [2, 1], [1, 1]]


def test_serpentine_is_one_component():
    """The long-chain case for the finds: one one-voxel corridor through (9, 33, 65)."""
    from lm_net_amd import VolumePostprocess
    L = R.serpentine()
    for conn in (6, 18, 26):
        roots, sizes = VolumePostprocess(2, connectivity=conn).components(torch.from_numpy(L).to(DEV))
        want_r, want_s = R.components(L, conn)
        assert np.array_equal(_np(roots), want_r) and np.array_equal(_np(sizes), want_s)
        assert int(sizes.flatten()[0]) == int(L.sum()) and (_np(roots)[L == 1] == 0).all()


def test_noise_giant_and_dust():
    """50 % noise at (12, 40, 70) under 26: one percolating giant plus dust, contention on one root."""
    from lm_net_amd import VolumePostprocess
    L = R.noise_case()
    post = VolumePostprocess(2, connectivity=26, keep_largest=True, fill_holes=True)
    roots, sizes = post.components(torch.from_numpy(L).to(DEV))
    want_r, want_s = R.components(L, 26)
    assert np.array_equal(_np(roots), want_r) and np.array_equal(_np(sizes), want_s)
    out = post(torch.from_numpy(L).to(DEV))
    L2, stats, _ = R.clean(L, 2, 26, keep_largest=True, fill_holes=True)
    assert np.array_equal(_np(out.labels), L2) and np.array_equal(_np(out.stats), stats)
    assert want_s[L == 1].max() > 0.9 * L.sum() and stats[1, 0] > 1 and stats[1, 1] == 1


@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_shells(connectivity):
    """Closed: filled.  Opened by one voxel to a face: not filled.  Opened diagonally only: filled under background 6 (connectivity 18,
    26), open under background 26 (connectivity 6)."""
    from lm_net_amd import VolumePostprocess
    post = VolumePostprocess(2, connectivity=connectivity, fill_holes=True)
    for opening, holes in ((None, 1), ("face", 0), ("diagonal", 0 if connectivity == 6 else 1)):
        L = R.shell(opening)
        out = post(torch.from_numpy(L).to(DEV))
        L2, stats, _ = R.clean(L, 2, connectivity, fill_holes=True)
        assert np.array_equal(_np(out.labels), L2) and np.array_equal(_np(out.stats), stats)
        assert int(out.stats[0, 3]) == holes and int((out.labels[1:4, 3:6, 4:7] == 1).all()) == holes, opening
    out = VolumePostprocess(2, connectivity=connectivity, fill_holes=26)(torch.from_numpy(R.shell()).to(DEV))
    assert int(out.stats[0, 3]) == 0                                          # the cavity has 27 voxels: above a limit of 26
    out = VolumePostprocess(2, connectivity=connectivity, fill_holes=27)(torch.from_numpy(R.shell()).to(DEV))
    assert int(out.stats[0, 3]) == 1


def test_two_kidneys_and_size_ties():
    from lm_net_amd import VolumePostprocess
    L = R.kidneys()
    out = VolumePostprocess(2, keep_largest=2)(torch.from_numpy(L).to(DEV))
    L2, stats, info = R.clean(L, 2, 26, keep_largest=2)
    assert np.array_equal(_np(out.labels), L2) and np.array_equal(_np(out.stats), stats)
    assert stats[1].tolist()[:2] == [5, 2] and stats[1, 2] == np.sort(info["sizes"][1])[-2:].sum()     # both kidneys kept, debris removed
    L = R.size_ties()
    for n in (1, 2, 3, 4):
        out = VolumePostprocess(2, keep_largest=n)(torch.from_numpy(L).to(DEV))
        L2, stats, info = R.clean(L, 2, 26, keep_largest=n)
        assert np.array_equal(_np(out.labels), L2) and np.array_equal(_np(out.stats), stats)
        assert info["survive"][1].tolist() == [True, False] + [j < n - 1 for j in range(3)]            # equal sizes: the smaller roots first

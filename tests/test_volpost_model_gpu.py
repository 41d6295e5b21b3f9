"""GPU: lm_net_amd.post.VolumePostprocess as a user meets it: why the class exists (a tilted rod stays whole where the per-slice
cleaning cuts it), push in uneven batches, its labels scored by VolumeSurfaceMeter, bit-identical repeats and the scratch limit."""
import numpy as np
import pytest
import torch

import volpost_ref as R
import volume_ref as VR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _np(t):
    return t.cpu().numpy()


def test_tilted_rod_stays_whole_where_the_per_slice_cleaning_cuts_it():
    """The rod's slices are disjoint 2D islands beside a larger block: DevicePostprocess(keep_largest) deletes the rod's piece in every
    slice; in 3D the rod is one component and the two largest components are the rod and the block."""
    from lm_net_amd import VolumePostprocess
    from lm_net_amd.post import DevicePostprocess
    rod = R.tilted_rod()
    dev = torch.from_numpy(rod).to(DEV)
    out = VolumePostprocess(2, keep_largest=2)(dev)
    assert np.array_equal(_np(out.labels), rod) and _np(out.stats)[1].tolist() == [2, 2, int(rod.sum()), 0]
    per_slice = DevicePostprocess(2, keep_largest=True)(dev).labels_net
    assert np.array_equal(_np(per_slice), R.clean_slices(rod, 2, 8, keep_largest=True)[0])
    assert (_np(per_slice)[:, 3] == 0).all() and not torch.equal(per_slice, out.labels)
    roots, sizes = VolumePostprocess(2).components(dev)
    assert (_np(roots)[:, 3][rod[:, 3] == 1] == 3 * rod.shape[2] + 2).all() and int(sizes[0, 3, 2]) == 3 * rod.shape[0]


@pytest.mark.parametrize("form", ["logits", "labels"])
def test_push_in_uneven_batches_equals_one_call(form):
    from lm_net_amd import VolumePostprocess
    shape, C = (9, 33, 65), 4
    pred = torch.from_numpy(R.tie_logits(shape, C) if form == "logits" else R.blob_labels(shape, C)).to(DEV)
    kw = dict(connectivity=18, keep_largest={1: 2}, min_volume=3, fill_holes=True)
    whole = VolumePostprocess(C, **kw)(pred)
    post = VolumePostprocess(C, **kw)
    for z0, z1 in ((0, 3), (3, 4), (4, 9)):                          # 3 + 1 + 5 slices: the case buffer grows twice
        post.push(pred[z0:z1])
    with pytest.raises(ValueError, match="is open"):
        post(pred)
    parts = post.close_case()
    assert torch.equal(parts.labels, whole.labels) and torch.equal(parts.stats, whole.stats)
    L2, stats, _ = R.clean(_np(pred), C, 18, keep_largest={1: 2}, min_volume=3, fill_holes=True)
    assert np.array_equal(_np(parts.labels), L2) and np.array_equal(_np(parts.stats), stats)
    with pytest.raises(ValueError, match="no slices were pushed"):
        post.close_case()
    again = post(pred)                                                # the object is reusable after a case
    assert torch.equal(again.labels, whole.labels)


def test_labels_go_into_the_volume_meter_as_they_are():
    """labels[z0:z1] pushed into VolumeSurfaceMeter: the raw statistics equal the restatement of both steps."""
    from lm_net_amd import VolumePostprocess, VolumeSurfaceMeter
    D, H, W, C = 12, 40, 70, 4
    pred, target = VR.ellipsoid_case(D, H, W, C)
    kw = dict(keep_largest=True, fill_holes=True)
    out = VolumePostprocess(C, **kw)(torch.from_numpy(pred).to(DEV))
    L2, stats, _ = R.clean(pred, C, 26, **kw)
    assert np.array_equal(_np(out.labels), L2) and (stats[1:, 1] < stats[1:, 0]).any()      # the specks went
    meter = VolumeSurfaceMeter(C, spacing=(3, 1, 1))
    tgt = torch.from_numpy(target).to(DEV)
    for z0, z1 in ((0, 5), (5, 12)):
        meter.push(out.labels[z0:z1], tgt[z0:z1])
    meter.close_case()
    si, sf = meter.raw()
    want_i, want_f, _ = VR.case_stats(L2.astype(np.int64), target, [1, 2, 3], (3, 1, 1))
    assert np.array_equal(_np(si)[0], want_i) and np.allclose(_np(sf)[0], want_f, rtol=1e-9, atol=0)
    raw_i, _, _ = VR.case_stats(pred, target, [1, 2, 3], (3, 1, 1))
    assert not np.array_equal(raw_i, want_i)                          # the cleaning changes what the meter reports


@pytest.mark.parametrize("deterministic", [False, True])
def test_two_calls_are_bit_identical(deterministic):
    from lm_net_amd import VolumePostprocess, hip
    L = torch.from_numpy(R.noise_case(12, 40, 70, seed=5) * R.blob_labels((12, 40, 70), 4)).to(DEV)
    post = VolumePostprocess(4, connectivity=26, keep_largest=3, min_volume=2, fill_holes=50)
    before = hip.load().lmn_get_deterministic()
    hip.load().lmn_set_deterministic(int(deterministic))
    try:
        a, b = post(L), post(L)
        ra, rb = post.components(L), post.components(L)
    finally:
        hip.load().lmn_set_deterministic(before)
    assert torch.equal(a.labels, b.labels) and torch.equal(a.stats, b.stats)
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])
    assert int(a.stats[1:, 0].min()) > 3 and int(a.stats[0, 3]) > 0


def test_limits_are_checked_when_a_case_is_closed():
    from lm_net_amd import VolumePostprocess
    post = VolumePostprocess(2, workspace_mb=1)
    post.push(torch.zeros(8, 128, 128, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match=r"a 8x128x128 case needs \d+ bytes of scratch, workspace_mb allows %d" % (1 << 20)):
        post.close_case()
    with pytest.raises(ValueError, match="into an open case|no slices"):
        post.push(torch.zeros(0, 128, 128, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="pred must be"):
        post.push(torch.zeros(2, 8, 8, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="logits with 3 channels"):
        post.push(torch.zeros(2, 3, 8, 8, device=DEV))
    with pytest.raises(ValueError, match="outside 1 <= D"):
        post.push(torch.zeros(2, 1, 8, dtype=torch.uint8, device=DEV))
    small = VolumePostprocess(2, workspace_mb=1)(torch.ones(2, 2, 2, dtype=torch.uint8, device=DEV))
    assert _np(small.stats).tolist() == [[0, 0, 0, 0], [1, 1, 8, 0]]

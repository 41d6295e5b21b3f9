"""GPU: the lesion matching kernel (lm_net_amd/csrc/lesion.hip) through lm_net_amd.metrics.LesionMeter and hip.lesion_match: the
canonical records equal the numpy restatement tests/lesion_ref.py element for element.  The shapes are the smallest where the kernel
can go wrong: (2, 2, 2), eight voxels in two lanes; (1, 8, 8), one slice; (3, 5, 70), a second block that is almost empty and rows
that end on no 4-voxel boundary; (12, 40, 70) and (17, 66, 130), many blocks and lesions that cross them -- each at connectivity 6,
18 and 26 with 2, 4 and 9 classes.  Then the cases made for the table: identical and disjoint volumes, one pair that holds every
voxel, the checkerboard that overflows the block's table, and a global table that is exactly full.  (What the generators hold is
decided on the restatement alone in tests/test_lesion_cpu.py.)"""
import functools

import numpy as np
import pytest
import torch

import lesion_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)
NAMES = ("comp_keys", "comp_sizes", "pair_keys", "pair_counts", "ctrl")
CAP = dict(max_components=8192, max_pairs=4096)                            # (the largest case: 7464 lesions, 3250 pairs)


@functools.lru_cache(maxsize=None)
def _case(shape, C):
    return R.lesion_case(*shape, C)


@functools.lru_cache(maxsize=None)
def _want(shape, C, connectivity, classes=None):
    return R.records(*_case(shape, C), C, connectivity, None if classes is None else list(classes), CAP["max_components"],
                     2 * CAP["max_pairs"])


def _dev(L):
    return torch.from_numpy(np.ascontiguousarray(L)).to(DEV)


def _assert_records(meter, want, what=""):
    got = [t.cpu().numpy() for t in meter.raw()]
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and np.array_equal(g[-1], w), (what, name)


@pytest.mark.parametrize("C", [2, 4, 9])
@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_records_equal_the_restatement(shape, connectivity, C):
    from lm_net_amd import LesionMeter
    Lp, Lt = _case(shape, C)
    meter = LesionMeter(C, connectivity=connectivity, **CAP)
    meter.update(_dev(Lp), _dev(Lt))
    want = _want(shape, C, connectivity)
    _assert_records(meter, want)
    assert want[4][0] >= 2 and want[4][1] >= 1
    if shape == R.SHAPES[-1] and C == 9:
        assert want[4][0] > 4000 and want[4][1] > 1500                     # thousands of lesions: the table is really used


@pytest.mark.parametrize("connectivity", [6, 26])
def test_class_subset_and_metrics(connectivity):
    """A `classes` subset in another order; compute() equals lesion_metrics of the restatement's records."""
    from lm_net_amd import LesionMeter
    from lm_net_amd.metrics import LESION_COUNTS, LESION_SCORES, lesion_metrics
    shape, C, classes = (12, 40, 70), 9, (5, 2, 7)
    Lp, Lt = _case(shape, C)
    meter = LesionMeter(C, classes=classes, connectivity=connectivity, **CAP)
    meter.update(_dev(Lp), _dev(Lt))
    want = _want(shape, C, connectivity, classes)
    _assert_records(meter, want)
    assert want[4][0] < _want(shape, C, connectivity)[4][0]
    for kw in (dict(), dict(overlap=0.5, iou=0.7, min_size=3)):
        got, ref = meter.compute(**kw), lesion_metrics(R.stack([want]), list(classes), **kw)
        for key in LESION_COUNTS + LESION_SCORES:
            assert np.array_equal(got["per_case"][key], ref["per_case"][key], equal_nan=True), key
            assert np.array_equal(got["pooled"][key], ref["pooled"][key], equal_nan=True), key
    by = meter.sensitivity_by_size([1, 4, 50, 1e9])
    assert by["n_target"].sum() == meter.compute()["pooled"]["n_target"].sum() and by["sensitivity"].shape == (3, 3)


def test_unaligned_volumes_take_the_scalar_path():
    """Label volumes that start at an odd address: no 4-byte loads, the same records."""
    from lm_net_amd import hip
    shape, C, conn = (12, 40, 70), 4, 26
    Lp, Lt = _case(shape, C)
    V = Lp.size
    bufs = [torch.zeros(V + 3, dtype=torch.uint8, device=DEV) for _ in range(2)]
    views = []
    for buf, L, off in zip(bufs, (Lp, Lt), (1, 3)):
        v = buf[off:off + V].view(shape)
        v.copy_(_dev(L))
        assert v.data_ptr() % 4 == off and v.is_contiguous()
        views.append(v)
    got = _match(views[0], views[1], C, conn, CAP["max_components"], 2 * CAP["max_pairs"])
    for g, w, name in zip(got, _want(shape, C, conn), NAMES):
        assert np.array_equal(g, w), name


def _match(lp, lt, C, connectivity, M, S, mask=None):
    """hip.lesion_match on fresh buffers -> the canonical records as numpy arrays."""
    from lm_net_amd import hip
    from lm_net_amd.metrics import _canonical_records
    ws = torch.full((hip.lesion_workspace(*lp.shape),), 0xFF, dtype=torch.uint8, device=DEV)
    ck, cs = torch.empty(M, dtype=torch.int64, device=DEV), torch.empty(M, dtype=torch.int32, device=DEV)
    pk, pc = torch.empty(S, dtype=torch.int64, device=DEV), torch.empty(S, dtype=torch.int32, device=DEV)
    ctrl = torch.empty(4, dtype=torch.int32, device=DEV)
    hip.lesion_match(lp, lt, C, connectivity, (1 << C) - 2 if mask is None else mask, ws, ck, cs, pk, pc, ctrl)
    ck, cs = _canonical_records(ck, cs)
    pk, pc = _canonical_records(pk, pc)
    return [t.cpu().numpy() for t in (ck, cs, pk, pc, ctrl)]


def test_identical_and_disjoint_volumes():
    from lm_net_amd import LesionMeter
    shape, C = (12, 40, 70), 4
    Lp, Lt = _case(shape, C)
    meter = LesionMeter(C, **CAP)
    meter.update(_dev(Lp), _dev(Lp))
    want = R.records(Lp, Lp, C, 26, None, CAP["max_components"], 2 * CAP["max_pairs"])
    _assert_records(meter, want, "identical")
    m = meter.compute()["pooled"]
    assert want[4][1] * 2 == want[4][0] and (m["pq"] == 1.0).all() and (m["f1"] == 1.0).all() and (m["fp"] == 0).all()
    # disjoint: the prediction in the even slices, the target in the odd ones -- an empty table
    a, b = Lp.copy(), Lt.copy()
    a[1::2] = 0
    b[0::2] = 0
    meter = LesionMeter(C, **CAP)
    meter.update(_dev(a), _dev(b))
    want = R.records(a, b, C, 26, None, CAP["max_components"], 2 * CAP["max_pairs"])
    _assert_records(meter, want, "disjoint")
    raw = meter.raw()
    assert want[4].tolist()[1:] == [0, 0, 0] and want[4][0] > 0 and bool((raw[2] == -1).all()) and bool((raw[3] == 0).all())
    m = meter.compute()["pooled"]
    assert (m["det_tp"] == 0).all() and (m["pq"] == 0.0).all() and (m["sensitivity"] == 0.0).all()


def test_two_full_masks_make_one_pair():
    """Two all-ones volumes: one pair whose count is the whole volume, from 143 blocks that each insert once (the pre-reduction)."""
    shape = (17, 66, 130)
    ones = torch.ones(shape, dtype=torch.uint8, device=DEV)
    ck, cs, pk, pc, ctrl = _match(ones, ones, 2, 26, 64, 64)
    V = 17 * 66 * 130
    assert ctrl.tolist() == [2, 1, 0, 0] and ck[:2].tolist() == [1 << 32, 1 << 40 | 1 << 32] and cs[:2].tolist() == [V, V]
    assert pk[0] == 0 and pc[0] == V and (pk[1:] == -1).all() and (pc[1:] == 0).all() and (ck[2:] == -1).all()


@pytest.mark.parametrize("pair_slots", [16384, 8192])
def test_checkerboard_overflows_the_block_table(pair_slots):
    """The parity checkerboard under 6 against a solid target: every voxel of the prediction is a lesion and a pair, 512 or so in
    each block's 256 LDS slots, so half of the insertions take the global route; at 8192 slots the global table is 92 % full."""
    Lp, Lt = R.checkerboard_case()
    got = _match(_dev(Lp), _dev(Lt), 2, 6, 8192, pair_slots)
    want = R.records(Lp, Lt, 2, 6, None, 8192, pair_slots)
    for g, w, name in zip(got, want, NAMES):
        assert np.array_equal(g, w), name
    assert got[4].tolist() == [7508, 7507, 0, 0] and (got[3][:7507] == 1).all()


def test_full_table_edge():
    """pair_slots = 1024: grid_case's 1024 pairs fill the table to the last slot and nothing is dropped; one more isolated voxel and
    exactly one insertion finds it full; with max_components = 512 ctrl[0] still counts every lesion."""
    g = R.grid_case()
    solid = np.ones_like(g)
    got = _match(_dev(g), _dev(solid), 2, 6, 2048, 1024)
    want = R.records(g, solid, 2, 6, None, 2048, 1024)
    for a, w, name in zip(got, want, NAMES):
        assert np.array_equal(a, w), name
    assert got[4].tolist() == [1025, 1024, 0, 0] and (got[2] >= 0).all()
    g1 = g.copy()
    g1[1, 1, 1] = 1
    ck, cs, pk, pc, ctrl = _match(_dev(g1), _dev(solid), 2, 6, 2048, 1024)
    assert ctrl.tolist() == [1026, 1024, 1, 0] and (pk >= 0).all() and (pc == 1).all()
    all_pairs = set(R.records(g1, solid, 2, 6)[2].tolist())
    assert len(set(pk.tolist())) == 1024 and set(pk.tolist()) < all_pairs                   # 1024 of the 1025, whichever came first
    ck, cs, pk, pc, ctrl = _match(_dev(g1), _dev(solid), 2, 6, 512, 1024)
    full = R.records(g1, solid, 2, 6)
    assert ctrl.tolist() == [1026, 1024, 1, 0] and (ck >= 0).all() and len(set(ck.tolist())) == 512 and set(ck.tolist()) < set(full[0].tolist())
    size = dict(zip(full[0].tolist(), full[1].tolist()))
    assert [size[k] for k in ck.tolist()] == cs.tolist()


# ---------------------------------------------------------------- through the class
def test_compute_raises_with_both_figures():
    from lm_net_amd import LesionMeter
    g = R.grid_case()
    g[1, 1, 1] = 1
    solid = np.ones_like(g)
    meter = LesionMeter(2, connectivity=6, max_components=512, max_pairs=4096)
    meter.update(_dev(solid), _dev(solid))
    meter.update(_dev(g), _dev(solid))
    with pytest.raises(ValueError, match=r"case 1 has 1026 lesions, max_components allows 512"):
        meter.compute()
    meter = LesionMeter(2, connectivity=6, max_components=2048, max_pairs=512)
    assert meter.pair_slots == 1024
    meter.update(_dev(g), _dev(solid))
    with pytest.raises(ValueError, match=r"case 0 dropped 1 pair insertions: its table of 1024 slots"):
        meter.compute()
    with pytest.raises(ValueError, match=r"needs %d bytes of scratch, workspace_mb allows %d" % (16 * g.size, 1 << 16)):
        LesionMeter(2, workspace_mb=1 / 16).update(_dev(g), _dev(solid))


def test_raw_is_bit_identical_and_add_raw_joins_two_halves():
    from lm_net_amd import LesionMeter
    C, conn = 4, 18
    cases = [_case(s, C) for s in ((12, 40, 70), (3, 5, 70), (17, 66, 130), (1, 8, 8))]

    def run(sel):
        m = LesionMeter(C, connectivity=conn, **CAP)
        for Lp, Lt in sel:
            m.update(_dev(Lp), _dev(Lt))
        return m

    one, again = run(cases), run(cases)
    for a, b, name in zip(one.raw(), again.raw(), NAMES):
        assert a.shape[0] == 4 and torch.equal(a, b), name
    left, right = run(cases[:2]), run(cases[2:])
    left.add_raw(*right.raw())
    for a, b, name in zip(one.raw(), left.raw(), NAMES):
        assert torch.equal(a, b), name
    got, ref = left.compute(), one.compute()
    assert np.array_equal(got["pooled"]["pq"], ref["pooled"]["pq"]) and np.array_equal(got["mean"]["f1"], ref["mean"]["f1"])


def test_update_images_equals_one_update_per_image():
    """A [B, H, W] batch, each image a one-slice case; also pushed slice by slice as a volume, which is another case."""
    from lm_net_amd import LesionMeter
    C = 4
    Lp, Lt = _case((12, 40, 70), C)
    lp, lt = _dev(Lp[:5]).long(), _dev(Lt[:5]).long()
    a, b = LesionMeter(C, **CAP), LesionMeter(C, **CAP)
    a.update_images(lp, lt)
    for i in range(5):
        b.update(lp[i:i + 1], lt[i:i + 1])
    for x, y, name in zip(a.raw(), b.raw(), NAMES):
        assert x.shape[0] == 5 and torch.equal(x, y), name
    for i in range(5):
        want = R.records(Lp[i:i + 1], Lt[i:i + 1], C, 26, None, CAP["max_components"], 2 * CAP["max_pairs"])
        for x, w, name in zip(a.raw(), want, NAMES):
            assert np.array_equal(x[i].cpu().numpy(), w), (i, name)
    vol = LesionMeter(C, **CAP)
    vol.push(lp[:2], lt[:2])
    vol.push(lp[2:], lt[2:])
    vol.close_case()
    _assert_records(vol, R.records(Lp[:5], Lt[:5], C, 26, None, CAP["max_components"], 2 * CAP["max_pairs"]))
    with pytest.raises(ValueError, match="is open"):
        vol.push(lp[:1], lt[:1]) or vol.update_images(lp, lt)

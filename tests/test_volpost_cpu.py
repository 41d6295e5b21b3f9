"""CPU: the host side of the 3D cleaning (include/volpost/lmnet_volpost.h, lm_net_amd.post.VolumePostprocess): registry and header
agree, the argument checks of the C entries (rejected before any HIP call, with fake device
pointers), the workspace formula, the class's ValueErrors, the restatement tests/volpost_ref.py against scipy.ndimage (label with the
three structures, binary_fill_holes with the dual structure), and the conditions the GPU tests rest on, decided by the restatement
alone.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import volpost_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- ABI
def test_registry_and_header_agree():
    """The feature's own part of the registry: the literal list, its place in hip.HEADERS, the number and values of its #defines, the
    header's citations and the package's export.  (Header / export / layout / return-type / constants checks: tests/test_host_cpu.py.)"""
    from lm_net_amd import hip
    assert hip.SYMBOLS_VOLPOST == ["lmn_volpost_workspace", "lmn_cc3d_label", "lmn_volpost_clean"]
    assert hip.HEADERS["volpost/lmnet_volpost.h"] is hip.SYMBOLS_VOLPOST
    header = open(os.path.join(ROOT, "include", "volpost", "lmnet_volpost.h")).read()
    assert len(re.findall(r"^#define LMN_VOLPOST_\w+ \d+\b", header, re.M)) == 3
    assert (hip.VOLPOST_MAX_SIDE, hip.VOLPOST_MAX_KEEP, hip.VOLPOST_NSTAT) == (1024, 4, 4)
    for cite in ("generate_binary_structure(3,", "binary_fill_holes", "DUAL connectivity", "smallest linear", "x - 1"):
        assert cite in header, cite
    import lm_net_amd
    from lm_net_amd.post import VolumeOutput, VolumePostprocess
    assert lm_net_amd.VolumePostprocess is VolumePostprocess and "VolumePostprocess" in lm_net_amd.__all__
    assert VolumeOutput._fields == ("labels", "stats")
    assert "one-slice volume has no holes" in VolumePostprocess.__doc__


# ---------------------------------------------------------------- argument checks
FAKE = ctypes.c_void_p(0x1000)


def _label(null=None, **kw):
    """lmn_cc3d_label with fake device pointers: every case here must be rejected before any HIP call."""
    from lm_net_amd import hip
    lib = hip.load()
    a = dict(labels=FAKE, roots=FAKE, sizes=FAKE)
    if null:
        a[null] = None
    g = dict(dict(D=17, H=33, W=65, connectivity=26), **kw)
    rc = lib.lmn_cc3d_label(a["labels"], g["D"], g["H"], g["W"], g["connectivity"], a["roots"], a["sizes"], None)
    return rc, lib.lmn_last_error().decode()


def _clean(null=None, keep=None, minv=None, **kw):
    from lm_net_amd import hip
    lib = hip.load()
    g = dict(dict(D=17, H=33, W=65, C=4, connectivity=26, class_mask=0b1110, hole_limit=5, ws_bytes=1 << 40), **kw)
    keep = [0] * g["C"] if keep is None else keep
    minv = [0] * g["C"] if minv is None else minv
    a = dict(labels=FAKE, keep_largest=(ctypes.c_int32 * max(len(keep), 1))(*keep), min_volume=(ctypes.c_int32 * max(len(minv), 1))(*minv),
             workspace=FAKE, labels_out=FAKE, stats=FAKE)
    if null:
        a[null] = None
    rc = lib.lmn_volpost_clean(a["labels"], g["D"], g["H"], g["W"], g["C"], g["connectivity"], ctypes.c_uint64(g["class_mask"]), a["keep_largest"],
                               a["min_volume"], g["hole_limit"], a["workspace"], ctypes.c_int64(g["ws_bytes"]), a["labels_out"], a["stats"], None)
    return rc, lib.lmn_last_error().decode()


def test_entries_reject_bad_arguments():
    for name in ("labels", "roots", "sizes"):
        rc, err = _label(null=name)
        assert rc == -1 and err == "cc3d_label: null pointer", (name, err)
    for kw, msg in ((dict(D=0), "D=0 not in [1, 1024]"), (dict(D=1025), "D=1025 not in [1, 1024]"), (dict(H=1), "size 1x65 outside [2, 1024]"),
                    (dict(W=1025), "size 33x1025 outside [2, 1024]"), (dict(connectivity=8), "connectivity 8 is none of 6, 18, 26"),
                    (dict(connectivity=0), "connectivity 0")):
        rc, err = _label(**kw)
        assert rc == -1 and msg in err and err.startswith("cc3d_label: "), (kw, err)
    for name in ("labels", "keep_largest", "min_volume", "workspace", "labels_out", "stats"):
        rc, err = _clean(null=name)
        assert rc == -1 and err == "volpost_clean: null pointer", (name, err)
    for kw, msg in ((dict(C=1, class_mask=0), "C=1 not in [2, 64]"), (dict(C=65, class_mask=0), "C=65"), (dict(D=0), "D=0 not in [1, 1024]"),
                    (dict(D=1025), "D=1025"), (dict(H=1), "size 1x65 outside [2, 1024]"), (dict(W=1025), "size 33x1025"),
                    (dict(connectivity=4), "connectivity 4 is none of 6, 18, 26"), (dict(class_mask=0b1111), "class_mask names class 0"),
                    (dict(class_mask=0b10010), "a class >= C=4"), (dict(hole_limit=-1), "hole_limit -1 < 0"),
                    (dict(keep=[0, 5, 0, 0]), "keep_largest[1] = 5 outside [0, 4]"), (dict(keep=[0, 0, -1, 0]), "keep_largest[2] = -1"),
                    (dict(keep=[0, 0, 0, 2], class_mask=0b0110), "keep_largest[3] = 2 names a class outside class_mask"),
                    (dict(minv=[0, 0, -7, 0]), "min_volume[2] = -7 < 0"), (dict(ws_bytes=1000), "workspace of 1000 bytes too small")):
        rc, err = _clean(**kw)
        assert rc == -1 and msg in err and err.startswith("volpost_clean: "), (kw, err)
    rc, err = _clean(keep=[0, 4, 1, 0], minv=[0, 2 ** 31 - 1, 0, 0], hole_limit=2 ** 31 - 1, ws_bytes=0)     # the bounds themselves pass
    assert rc == -1 and "workspace of 0 bytes too small" in err, err


def test_workspace_is_host_arithmetic():
    from lm_net_amd import hip
    up = lambda v: (v + 255) // 256 * 256
    for D, H, W in ((1, 2, 2), (2, 2, 2), (3, 5, 70), (17, 66, 130), (128, 352, 352), (1024, 1024, 1024)):
        V = D * H * W
        assert hip.volpost_workspace(D, H, W) == up(V) + 2 * up(4 * V) + up(4 * ((V + 31) // 32)) + up(64 * 4 * 8)
    assert 9.125 * 128 * 352 * 352 <= hip.volpost_workspace(128, 352, 352) <= 9.13 * 128 * 352 * 352          # 9 bytes and one bit per voxel
    for args, msg in (((0, 8, 8), "D=0"), ((1025, 8, 8), "D=1025"), ((4, 1, 8), "1x8"), ((4, 8, 1025), "8x1025")):
        with pytest.raises(ValueError, match="volpost_workspace"):
            hip.volpost_workspace(*args)
        assert msg in hip.load().lmn_last_error().decode()


def test_python_wrappers_check_sizes_before_the_library():
    from lm_net_amd import hip
    lab = torch.zeros(6, 5, 7, dtype=torch.uint8)
    r, s = torch.zeros(6, 5, 7, dtype=torch.int32), torch.zeros(6, 5, 7, dtype=torch.int32)
    for args in ((lab, 26, r[:5], s), (lab, 26, r, s[:, :4]), (lab[0], 26, r[0], s[0])):
        with pytest.raises(ValueError, match="cc3d_label"):
            hip.cc3d_label(*args)
    with pytest.raises(RuntimeError):                                # right sizes reach the pointer helpers, which refuse CPU tensors
        hip.cc3d_label(lab, 26, r, s)
    ws, out, st = torch.zeros(8, dtype=torch.uint8), torch.zeros(6, 5, 7, dtype=torch.uint8), torch.zeros(3, 4, dtype=torch.int32)
    for args, msg in (((lab, 3, 26, 0b110, [0] * 3, [0] * 3, 0, ws, out[:5], st), "output buffers do not match"),
                      ((lab, 4, 26, 0b110, [0] * 4, [0] * 4, 0, ws, out, st), "output buffers do not match"),
                      ((lab, 3, 26, 0b110, [0] * 2, [0] * 3, 0, ws, out, st), "one entry per class"),
                      ((lab, 3, 26, 0b110, [0] * 3, [0] * 4, 0, ws, out, st), "one entry per class")):
        with pytest.raises(ValueError, match=msg):
            hip.volpost_clean(*args)
    with pytest.raises(RuntimeError):
        hip.volpost_clean(lab, 3, 26, 0b110, [0] * 3, [0] * 3, 0, ws, out, st)


def test_class_refuses_what_it_cannot_run():
    from lm_net_amd import VolumePostprocess
    for kw, msg in ((dict(n_classes=1), "outside"), (dict(n_classes=65), "outside"), (dict(n_classes=3, connectivity=8), "none of 6, 18, 26"),
                    (dict(n_classes=3, classes=[1, 1]), "distinct"), (dict(n_classes=3, classes=[0]), "distinct"), (dict(n_classes=3, classes=[3]), "distinct"),
                    (dict(n_classes=3, keep_largest=0), r"counts must be in \[1, 4\]"), (dict(n_classes=3, keep_largest=5), r"counts must be in \[1, 4\]"),
                    (dict(n_classes=3, keep_largest={2: 0}), "counts must be in"), (dict(n_classes=3, classes=[1], keep_largest={2: 1}), "names a class outside"),
                    (dict(n_classes=3, keep_largest=[1]), "a bool, an int"), (dict(n_classes=3, min_volume=[1]), "one entry per class"),
                    (dict(n_classes=3, min_volume=-1), "min_volume must be in"), (dict(n_classes=3, min_volume=2 ** 31), "min_volume must be in"),
                    (dict(n_classes=3, fill_holes=-1), "maximal hole volume"), (dict(n_classes=3, fill_holes=2 ** 31), "maximal hole volume"),
                    (dict(n_classes=3, workspace_mb=0), "workspace_mb")):
        with pytest.raises(ValueError, match=msg):
            VolumePostprocess(**kw)
    p = VolumePostprocess(9, connectivity=18, classes=[1, 2, 5], keep_largest={2: 2, 5: 1}, min_volume=[10, 0, 7], fill_holes=True)
    assert p.class_mask == 0b100110 and p._keep == [0, 0, 2, 0, 0, 1, 0, 0, 0] and p._minv == [0, 10, 0, 0, 0, 7, 0, 0, 0]
    assert p.hole_limit == 2 ** 31 - 1 and p.connectivity == 18
    assert VolumePostprocess(4, keep_largest=True)._keep == [0, 1, 1, 1] and VolumePostprocess(4, keep_largest=2)._keep == [0, 2, 2, 2]
    assert VolumePostprocess(4, fill_holes=100).hole_limit == 100 and VolumePostprocess(4).hole_limit == 0
    with pytest.raises(RuntimeError, match="no CPU path"):
        p.push(torch.zeros(4, 9, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        p(torch.zeros(4, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="no slices were pushed"):
        p.close_case()
    from lm_net_amd import hip
    assert p.scratch_bytes(128, 352, 352) == hip.volpost_workspace(128, 352, 352) < 2048 << 20
    with pytest.raises(ValueError, match=r"needs \d+ bytes of scratch, workspace_mb allows %d" % (64 << 20)):
        VolumePostprocess(9, workspace_mb=64).scratch_bytes(128, 352, 352)


# ---------------------------------------------------------------- the restatement
STRUCT_SHAPES = [(1, 8, 8), (2, 2, 2), (3, 5, 70), (7, 33, 65)]


@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("shape", STRUCT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_components_against_scipy_label(shape, connectivity):
    """ndimage.label with generate_binary_structure(3, 1 | 2 | 3), per label value: the same partition, numbered in the same raster
    order; the root is the smallest index of the component and sizes counts it."""
    ndi = pytest.importorskip("scipy.ndimage")
    st = ndi.generate_binary_structure(3, R.ORDER[connectivity])
    cases = [R.label_volume(R.blob_labels(shape, 4), 4), R.noise_case(*shape).astype(np.uint8), R.parity_checkerboard(*shape).astype(np.uint8)]
    for L in cases:
        roots, sizes = R.components(L, connectivity)
        idx = np.arange(L.size).reshape(L.shape)
        for k in np.unique(L):
            want, n = ndi.label(L == k, structure=st)
            assert np.array_equal(R.rank_labels(roots, L == k), want), (shape, connectivity, k)
            for c in range(1, n + 1):
                m = want == c
                r = idx[m].min()
                assert (roots[m] == r).all() and sizes.ravel()[r] == m.sum()
        assert sizes.sum() == L.size and ((sizes > 0) == (roots == idx)).all()


@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_fill_holes_against_scipy(connectivity):
    """binary_fill_holes(L1 > 0, structure = the dual): the filled voxels are exactly the voxels that turn non-zero."""
    ndi = pytest.importorskip("scipy.ndimage")
    dual = ndi.generate_binary_structure(3, R.ORDER[R.DUAL[connectivity]])
    cases = [R.shell(), R.shell("face"), R.shell("diagonal"), R.organ_case(12, 40, 70, 4), R.noise_case(6, 12, 14, seed=3), R.noise_case(1, 8, 8, seed=4),
             (R.noise_case(5, 9, 11, seed=5) + R.noise_case(5, 9, 11, seed=6) > 0).astype(np.int64)]
    filled_any = 0
    for L in cases:
        C = int(L.max()) + 1 if L.max() > 0 else 2
        L2, stats, info = R.clean(L, C, connectivity, fill_holes=True)
        want = ndi.binary_fill_holes(info["L1"] > 0, structure=dual)
        assert np.array_equal(L2 > 0, want), connectivity
        assert np.array_equal(L2[info["L1"] > 0], info["L1"][info["L1"] > 0])
        filled_any += int(stats[0, 3])
        assert stats[0, 3] == ndi.label(want & (info["L1"] == 0), structure=dual)[1]
        if L.shape[0] == 1:
            assert stats[0, 3] == 0                                    # a one-slice volume has no holes
    assert filled_any > 0


def test_adversarial_cases_show_what_they_must():
    """The table of the adversarial cases, decided by the restatement."""
    def n_comp(L, conn, k):
        return int(R.clean(L, int(L.max()) + 1, conn)[1][k, 0])
    cb = R.parity_checkerboard()
    assert n_comp(cb, 6, 0) + n_comp(cb, 6, 1) == cb.size and n_comp(cb, 18, 0) == n_comp(cb, 18, 1) == 1 and n_comp(cb, 26, 1) == 1
    tp = R.touching_pairs()
    assert [(n_comp(tp, c, 1), n_comp(tp, c, 2)) for c in (6, 18, 26)] == [(2, 2), (2, 1), (1, 1)]
    sp = R.serpentine()
    for c in (6, 18, 26):
        assert n_comp(sp, c, 1) == 1
    assert R.components(sp, 6)[1][0, 0, 0] == (sp == 1).sum() > 5 * 17 * 65                  # the corridor starts at voxel 0
    roots, sizes = R.components(R.noise_case(), 26)
    ones = np.sort(sizes[(R.noise_case() == 1) & (sizes > 0)])
    assert ones[-1] > 0.9 * (R.noise_case() == 1).sum() and ones.size > 1                  # one giant plus dust
    for conn in (6, 18, 26):
        assert R.clean(R.shell(), 2, conn, fill_holes=True)[1][0, 3] == 1
        assert R.clean(R.shell("face"), 2, conn, fill_holes=True)[1][0, 3] == 0
        assert R.clean(R.shell("diagonal"), 2, conn, fill_holes=True)[1][0, 3] == (0 if conn == 6 else 1)
    L2, stats, info = R.clean(R.kidneys(), 2, 26, keep_largest=2)
    big = np.sort(info["sizes"][1])[-2:]
    assert stats[1].tolist()[:2] == [5, 2] and stats[1, 2] == big.sum() and big[0] > 100 and big[0] != big[1]
    L2, stats, info = R.clean(R.size_ties(), 2, 26, keep_largest=2)
    assert info["sizes"][1].tolist() == [4, 2, 4, 4, 4] and info["survive"][1].tolist() == [True, False, True, False, False]
    # the tilted rod: one component in 3D; per slice its piece is the smaller island and goes
    rod = R.tilted_rod()
    L2, stats, _ = R.clean(rod, 2, 26, keep_largest=True)
    assert stats[1].tolist()[:2] == [2, 1] and (L2[:, 3] == 0).all()                       # (the block is the largest 3D component)
    L2, stats, _ = R.clean(rod, 2, 26, keep_largest=2)
    assert np.array_equal(L2, rod) and stats[1, 0] == 2
    per_slice, _ = R.clean_slices(rod, 2, 8, keep_largest=True)
    assert (per_slice[:, 3] == 0).all() and not np.array_equal(per_slice, L2)


@pytest.mark.parametrize("C", [2, 4, 9])
@pytest.mark.parametrize("shape", R.ORGAN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_generator_conditions(shape, C):
    """The conditions the GPU tests rest on, in every organ case and for every cleaned class (all of 1 .. C - 1), under each
    connectivity: L0 has at least 3 components of pairwise distinct sizes, at least one is removed by min_volume and at least one
    survives it; per class a cavity is filled, a cavity open to a face is not, and a cavity lies above the finite fill_holes limit."""
    L = R.organ_case(*shape, C)
    for conn in (6, 18, 26):
        L2, stats, info = R.clean(L, C, conn, min_volume=R.ORGAN_MIN_VOLUME, fill_holes=R.ORGAN_HOLE_LIMIT)
        for k in range(1, C):
            sz, ok = info["sizes"][k], info["survive"][k]
            assert sz.size >= 3 and len(set(sz.tolist())) == sz.size, (k, sz)
            assert (~ok).sum() >= 1 and ok.sum() >= 1 and (sz[~ok] < R.ORGAN_MIN_VOLUME).all()
        hs, op = info["hole_sizes"], info["hole_open"]
        n = C - 1
        assert stats[0, 3] == n == ((~op) & (hs <= R.ORGAN_HOLE_LIMIT)).sum()                # filled: one per class
        assert ((~op) & (hs > R.ORGAN_HOLE_LIMIT)).sum() == n                                # closed, above the limit: one per class
        assert (op & (hs == 3)).sum() == n                                                   # the pits: open to z = 0, not filled
        assert (L2 != info["L1"]).sum() == n
        full = R.clean(L, C, conn, keep_largest=2, fill_holes=True)
        assert full[1][0, 3] == 2 * n and (full[1][1:, 1] == 2).all()

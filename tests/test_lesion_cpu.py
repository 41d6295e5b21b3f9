"""CPU: the host side of the lesion matching (include/lesion/lmnet_lesion.h, lm_net_amd.metrics.LesionMeter): registry and header
agree, the argument checks of the C entry (rejected before any HIP call, with fake device
pointers), the workspace formula, the class's ValueErrors, the restatement tests/lesion_ref.py and lesion_metrics against an
independent scipy.ndimage.label with explicit loops over the label ids, hand-computed cases, and the conditions the GPU tests rest on,
decided by the restatement alone.  No GPU needed."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import lesion_ref as R
import volpost_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- ABI
def test_registry_and_header_agree():
    """The feature's own part of the registry: the literal list, its place in hip.HEADERS, the number and values of its #defines, the
    header's citations and the package's export.  (Header / export / layout / return-type / constants checks: tests/test_host_cpu.py.)"""
    from lm_net_amd import hip
    assert hip.SYMBOLS_LESION == ["lmn_lesion_workspace", "lmn_lesion_match"]
    assert hip.HEADERS["lesion/lmnet_lesion.h"] is hip.SYMBOLS_LESION
    header = open(os.path.join(ROOT, "include", "lesion", "lmnet_lesion.h")).read()
    assert len(re.findall(r"^#define LMN_LESION_\w+ \d+\b", header, re.M)) == 4
    assert (hip.LESION_MAX_SIDE, hip.LESION_MIN_SLOTS, hip.LESION_MAX_SLOTS, hip.LESION_NCTRL) == (1024, 64, 2 ** 22, 4)
    for cite in ("side << 40 | class << 32 | root", "root_p << 32 | root_g", "DEPENDS ON ARRIVAL ORDER", "smallest linear", "BraTS",
                 "without its dilation", "value >= C is read as 0", "theta >= 0.5", "lesion_match: "):
        assert cite in header, cite
    import lm_net_amd
    from lm_net_amd.metrics import LesionMeter
    assert lm_net_amd.LesionMeter is LesionMeter and "LesionMeter" in lm_net_amd.__all__
    for cite in ("VOID TARGET VOXELS ARE BACKGROUND", "BraTS", "without its", "smallest linear voxel index"):
        assert cite in LesionMeter.__doc__, cite


# ---------------------------------------------------------------- argument checks
FAKE = ctypes.c_void_p(0x1000)
POINTERS = ("pred", "target", "workspace", "comp_keys", "comp_sizes", "pair_keys", "pair_counts", "ctrl")


def _match(null=None, **kw):
    """lmn_lesion_match with fake device pointers: every case here must be rejected before any HIP call."""
    from lm_net_amd import hip
    lib = hip.load()
    a = {k: FAKE for k in POINTERS}
    if null:
        a[null] = None
    g = dict(dict(D=17, H=33, W=65, C=4, connectivity=26, class_mask=0b1110, ws_bytes=1 << 40, max_components=64, pair_slots=64), **kw)
    rc = lib.lmn_lesion_match(a["pred"], a["target"], g["D"], g["H"], g["W"], g["C"], g["connectivity"], ctypes.c_uint64(g["class_mask"]),
                              a["workspace"], ctypes.c_int64(g["ws_bytes"]), a["comp_keys"], a["comp_sizes"], g["max_components"],
                              a["pair_keys"], a["pair_counts"], g["pair_slots"], a["ctrl"], None)
    return rc, lib.lmn_last_error().decode()


def test_entry_rejects_bad_arguments():
    for name in POINTERS:
        rc, err = _match(null=name)
        assert rc == -1 and err == "lesion_match: null pointer", (name, err)
    for kw, msg in ((dict(C=1, class_mask=0), "C=1 not in [2, 64]"), (dict(C=65, class_mask=0), "C=65"), (dict(D=0), "D=0 not in [1, 1024]"),
                    (dict(D=1025), "D=1025"), (dict(H=1), "size 1x65 outside [2, 1024]"), (dict(H=1025), "size 1025x65"),
                    (dict(W=1), "size 33x1 outside"), (dict(W=1025), "size 33x1025"),
                    (dict(connectivity=8), "connectivity 8 is none of 6, 18, 26"), (dict(connectivity=0), "connectivity 0"),
                    (dict(class_mask=0b1111), "class_mask names class 0"), (dict(class_mask=0b10010), "a class >= C=4"),
                    (dict(pair_slots=96), "pair_slots 96 is no power of two in [64, 4194304]"), (dict(pair_slots=32), "pair_slots 32"),
                    (dict(pair_slots=1 << 23), "pair_slots 8388608"), (dict(pair_slots=0), "pair_slots 0"), (dict(pair_slots=-64), "pair_slots -64"),
                    (dict(max_components=0), "max_components 0 < 1"), (dict(max_components=-3), "max_components -3 < 1"),
                    (dict(ws_bytes=1000), "workspace of 1000 bytes too small")):
        rc, err = _match(**kw)
        assert rc == -1 and msg in err and err.startswith("lesion_match: "), (kw, err)
    # the bounds themselves pass: the last check, of the workspace, is reached
    from lm_net_amd import hip
    need = hip.lesion_workspace(1024, 1024, 1024)
    rc, err = _match(D=1024, H=1024, W=1024, C=64, class_mask=(1 << 64) - 2, pair_slots=1 << 22, max_components=2 ** 31 - 1, ws_bytes=need - 1)
    assert rc == -1 and "workspace of %d bytes too small, %d needed" % (need - 1, need) in err, err
    rc, err = _match(D=1, H=2, W=2, C=2, class_mask=0b10, connectivity=6, max_components=1, ws_bytes=0)
    assert rc == -1 and "workspace of 0 bytes too small" in err, err


def test_workspace_is_host_arithmetic():
    from lm_net_amd import hip
    up = lambda v: (v + 255) // 256 * 256
    for D, H, W in ((1, 2, 2), (2, 2, 2), (3, 5, 70), (17, 66, 130), (128, 352, 352), (1024, 1024, 1024)):
        assert hip.lesion_workspace(D, H, W) == 4 * up(4 * D * H * W)
    assert hip.lesion_workspace(1, 2, 2) == 1024 and hip.lesion_workspace(128, 352, 352) == 16 * 128 * 352 * 352
    for args, msg in (((0, 8, 8), "D=0"), ((1025, 8, 8), "D=1025"), ((4, 1, 8), "1x8"), ((4, 8, 1025), "8x1025")):
        with pytest.raises(ValueError, match="lesion_workspace"):
            hip.lesion_workspace(*args)
        assert msg in hip.load().lmn_last_error().decode()


def test_python_wrapper_checks_sizes_before_the_library():
    from lm_net_amd import hip
    lab = torch.zeros(6, 5, 7, dtype=torch.uint8)
    ws = torch.zeros(8, dtype=torch.uint8)
    ck, cs = torch.zeros(16, dtype=torch.int64), torch.zeros(16, dtype=torch.int32)
    pk, pc = torch.zeros(64, dtype=torch.int64), torch.zeros(64, dtype=torch.int32)
    ctrl = torch.zeros(4, dtype=torch.int32)
    for args, msg in (((lab[0], lab[0], 3, 26, 0b110, ws, ck, cs, pk, pc, ctrl), "two uint8 volumes"),
                      ((lab, lab[:5], 3, 26, 0b110, ws, ck, cs, pk, pc, ctrl), "two uint8 volumes"),
                      ((lab, lab, 3, 26, 0b110, ws, ck, cs[:15], pk, pc, ctrl), "record buffers"),
                      ((lab, lab, 3, 26, 0b110, ws, ck, cs, pk[:32], pc, ctrl), "record buffers"),
                      ((lab, lab, 3, 26, 0b110, ws, ck.view(4, 4), cs.view(4, 4), pk, pc, ctrl), "record buffers"),
                      ((lab, lab, 3, 26, 0b110, ws, ck, cs, pk, pc, ctrl[:3]), "record buffers")):
        with pytest.raises(ValueError, match=msg):
            hip.lesion_match(*args)
    with pytest.raises(RuntimeError):                                # right sizes reach the pointer helpers, which refuse CPU tensors
        hip.lesion_match(lab, lab, 3, 26, 0b110, ws, ck, cs, pk, pc, ctrl)


def test_class_refuses_what_it_cannot_run():
    from lm_net_amd import LesionMeter, hip
    for kw, msg in ((dict(n_classes=1), "outside"), (dict(n_classes=65), "outside"), (dict(n_classes=3, connectivity=8), "none of 6, 18, 26"),
                    (dict(n_classes=3, classes=[1, 1]), "distinct"), (dict(n_classes=3, classes=[0]), "distinct"), (dict(n_classes=3, classes=[3]), "distinct"),
                    (dict(n_classes=3, classes=[]), "distinct"), (dict(n_classes=3, max_components=0), "max_components"),
                    (dict(n_classes=3, max_components=2 ** 31), "max_components"), (dict(n_classes=3, max_pairs=0), "max_pairs"),
                    (dict(n_classes=3, max_pairs=2 ** 21 + 1), "max_pairs"), (dict(n_classes=3, workspace_mb=0), "workspace_mb")):
        with pytest.raises(ValueError, match=msg):
            LesionMeter(**kw)
    m = LesionMeter(9, classes=[1, 2, 5], connectivity=18, device="cpu")
    assert m.class_mask == 0b100110 and m.connectivity == 18 and (m.max_components, m.max_pairs, m.pair_slots) == (8192, 8192, 16384)
    assert [LesionMeter(2, max_pairs=n).pair_slots for n in (1, 32, 33, 4096, 4097, 2 ** 21)] == [64, 64, 128, 8192, 16384, 2 ** 22]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.push(torch.zeros(4, 9, 8, 8), torch.zeros(4, 8, 8, dtype=torch.int64))
    with pytest.raises(ValueError, match="no slices were pushed"):
        m.close_case()
    assert m.scratch_bytes(128, 352, 352) == hip.lesion_workspace(128, 352, 352) < 2048 << 20
    with pytest.raises(ValueError, match=r"needs %d bytes of scratch, workspace_mb allows %d" % (16 * 128 * 352 * 352, 64 << 20)):
        LesionMeter(9, workspace_mb=64).scratch_bytes(128, 352, 352)
    raw = m.raw()
    assert [tuple(t.shape) for t in raw] == [(0, 8192), (0, 8192), (0, 16384), (0, 16384), (0, 4)]
    assert [t.dtype for t in raw] == [torch.int64, torch.int32, torch.int64, torch.int32, torch.int32]
    with pytest.raises(ValueError, match="add_raw"):
        m.add_raw(*(t[:, :5] for t in raw))
    for kw, msg in ((dict(overlap=1.5), "overlap"), (dict(overlap=-0.1), "overlap"), (dict(iou=0.4), "iou"), (dict(iou=1.0), "iou"),
                    (dict(min_size=-1), "min_size"), (dict(min_size=1.5), "min_size")):
        with pytest.raises(ValueError, match=msg):
            m.compute(**kw)
    with pytest.raises(ValueError, match="size_bins"):
        m.sensitivity_by_size([3])


def test_compute_names_the_case_and_both_figures():
    """More lesions than max_components, or a dropped pair insertion: lesion_metrics (and so LesionMeter.compute) raises a ValueError
    with the case index and both figures."""
    from lm_net_amd.metrics import lesion_metrics
    Lp, Lt = R.lesion_case(1, 8, 8, 2)
    good = R.records(Lp, Lt, 2, 26, None, 16, 64)
    lesion_metrics(R.stack([good, good]), [1])
    over = tuple(a.copy() for a in good)
    over[4][0] = 17
    with pytest.raises(ValueError, match=r"case 1 has 17 lesions, max_components allows 16"):
        lesion_metrics(R.stack([good, over]), [1])
    full = tuple(a.copy() for a in good)
    full[4][2] = 3
    with pytest.raises(ValueError, match=r"case 0 dropped 3 pair insertions: its table of 64 slots"):
        lesion_metrics(R.stack([full, good]), [1])


# ---------------------------------------------------------------- the restatement against scipy, with explicit loops
STRUCT_SHAPES = [(1, 8, 8), (2, 2, 2), (3, 5, 70), (7, 33, 65)]


def _loops(Lp, Lt, C, connectivity, classes, overlap, iou, min_size):
    """The definitions once more: ndimage.label per class and side, explicit loops over the label ids, Python floats."""
    import scipy.ndimage as ndi
    st = ndi.generate_binary_structure(3, VR.ORDER[connectivity])
    Lp, Lt = R.clamp(Lp, C), R.clamp(Lt, C)
    out = []
    for k in classes:
        lp, n_p = ndi.label(Lp == k, structure=st)
        lt, n_t = ndi.label(Lt == k, structure=st)
        sp = {p: int((lp == p).sum()) for p in range(1, n_p + 1)}
        sg = {g: int((lt == g).sum()) for g in range(1, n_t + 1)}
        sp = {p: n for p, n in sp.items() if n >= min_size}
        sg = {g: n for g, n in sg.items() if n >= min_size}
        o_p, o_g, tp, s_iou, s_dice = dict.fromkeys(sp, 0), dict.fromkeys(sg, 0), 0, 0.0, 0.0
        for p in sp:
            under = np.bincount(lt[lp == p], minlength=n_t + 1)
            for g in sg:
                n = int(under[g])
                if n == 0:
                    continue
                o_p[p] += n
                o_g[g] += n
                if n / (sp[p] + sg[g] - n) > iou:
                    tp += 1
                    s_iou += n / (sp[p] + sg[g] - n)
                    s_dice += 2 * n / (sp[p] + sg[g])
        det_tp = sum(1 for g in sg if o_g[g] >= 1 and o_g[g] >= overlap * sg[g])
        det_fp = sum(1 for p in sp if not (o_p[p] >= 1 and o_p[p] >= overlap * sp[p]))
        nP, nG = len(sp), len(sg)
        nan = float("nan")
        s = det_tp / nG if nG else nan
        pr = (nP - det_fp) / nP if nP else nan
        f1 = (0.0 if s + pr == 0 else 2 * s * pr / (s + pr))
        fp, fn = nP - tp, nG - tp
        den = tp + fp / 2 + fn / 2
        out.append(dict(n_pred=nP, n_target=nG, det_tp=det_tp, det_fn=nG - det_tp, det_fp=det_fp, tp=tp, fp=fp, fn=fn, sensitivity=s,
                        precision=pr, f1=f1, sq=s_iou / tp if tp else nan, rq=tp / den if den else nan,
                        pq=(s_iou / tp * tp / den if tp else 0.0) if den else nan, lesion_dice=s_dice / (tp + fp + fn) if tp + fp + fn else nan))
    return out


def _same(got, want, what):
    if isinstance(want, int):
        assert int(got) == want, (what, got, want)
    elif math.isnan(want):
        assert math.isnan(float(got)), (what, got, want)
    else:
        assert abs(float(got) - want) <= 1e-12, (what, got, want)


@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("shape", STRUCT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_against_scipy_loops(shape, connectivity):
    pytest.importorskip("scipy.ndimage")
    from lm_net_amd.metrics import LESION_COUNTS, LESION_SCORES
    C = 4
    u8 = lambda L: np.where(L < 0, 255, L).astype(np.uint8)
    cases = [R.lesion_case(*shape, C), (u8(VR.blob_labels(shape, C, seed=0)), u8(VR.blob_labels(shape, C, seed=1)))]
    for classes in ([1, 2, 3], [3, 1]):
        for kw in (dict(overlap=0.0, iou=0.5, min_size=0), dict(overlap=0.5, iou=0.6, min_size=2), dict(overlap=1.0, iou=0.5, min_size=0)):
            got = R.metrics(cases, C, connectivity, classes, **kw)
            want = [_loops(Lp, Lt, C, connectivity, classes, **kw) for Lp, Lt in cases]
            assert got["classes"] == classes
            for n in range(len(cases)):
                for j in range(len(classes)):
                    for key in LESION_COUNTS + LESION_SCORES:
                        _same(got["per_case"][key][n, j], want[n][j][key], (shape, connectivity, classes, kw, n, j, key))
            for j in range(len(classes)):                             # pooled: the counts add up
                for key in LESION_COUNTS:
                    assert int(got["pooled"][key][j]) == sum(w[j][key] for w in want)
    # the per-size strata partition the targets
    by = R.metrics(cases, C, connectivity, size_bins=[1, 2, 5, 1e9])["by_size"]
    full = R.metrics(cases, C, connectivity)["pooled"]
    assert np.array_equal(by["n_target"].sum(0), full["n_target"]) and np.array_equal(by["det_tp"].sum(0), full["det_tp"])


# ---------------------------------------------------------------- hand-computed cases
def _plane(*cells):
    """(1, 8, 8) uint8 volume with class 1 at the given (y, x)."""
    L = np.zeros((1, 8, 8), np.uint8)
    for y, x in cells:
        L[0, y, x] = 1
    return L


SQUARE = [(1, 1), (1, 2), (2, 1), (2, 2)]


def _one(Lp, Lt, **kw):
    m = R.metrics([(Lp, Lt)], 2, 26, **kw)
    return {k: (v[0].item() if hasattr(v[0], "item") else v[0]) for k, v in m["pooled"].items()}


def test_hand_computed_cases():
    sq = _plane(*SQUARE)
    # identical masks
    m = _one(sq, sq)
    assert (m["tp"], m["fp"], m["fn"], m["det_tp"], m["det_fp"]) == (1, 0, 0, 1, 0)
    assert m["pq"] == m["sq"] == m["rq"] == m["f1"] == m["lesion_dice"] == m["sensitivity"] == m["precision"] == 1.0
    # a square and an L of 4 voxels that share 3: IoU 3/5, matched
    m = _one(sq, _plane((1, 1), (1, 2), (2, 1), (3, 1)))
    assert (m["tp"], m["fp"], m["fn"]) == (1, 0, 0) and abs(m["sq"] - 0.6) < 1e-15 and abs(m["pq"] - 0.6) < 1e-15
    assert abs(m["lesion_dice"] - 0.75) < 1e-15 and m["f1"] == 1.0
    # two squares that share 2 voxels: IoU 2/6 -- detected under the overlap rule, unmatched under the IoU rule
    shifted = _plane((1, 2), (1, 3), (2, 2), (2, 3))
    m = _one(sq, shifted)
    assert (m["det_tp"], m["det_fn"], m["det_fp"]) == (1, 0, 0) and m["f1"] == 1.0
    assert (m["tp"], m["fp"], m["fn"]) == (0, 1, 1) and m["pq"] == 0.0 and m["rq"] == 0.0 and math.isnan(m["sq"]) and m["lesion_dice"] == 0.0
    # overlap = 0.5: 2 of 4 voxels is enough, 0.75 is not
    assert _one(sq, shifted, overlap=0.5)["det_tp"] == 1 and _one(sq, shifted, overlap=0.5)["det_fp"] == 0
    m = _one(sq, shifted, overlap=0.75)
    assert (m["det_tp"], m["det_fn"], m["det_fp"]) == (0, 1, 1) and m["f1"] == 0.0 and m["sensitivity"] == 0.0
    # min_size: the one-voxel miss and the one-voxel false alarm go
    Lp, Lt = _plane(*SQUARE, (6, 6)), _plane(*SQUARE, (5, 0))
    m = _one(Lp, Lt)
    assert (m["n_pred"], m["n_target"], m["det_fn"], m["det_fp"], m["tp"]) == (2, 2, 1, 1, 1) and m["sensitivity"] == 0.5 and m["rq"] == 0.5
    m = _one(Lp, Lt, min_size=2)
    assert (m["n_pred"], m["n_target"], m["det_fn"], m["det_fp"]) == (1, 1, 0, 0) and m["pq"] == 1.0
    # ... and a pair goes with its dropped lesion: a one-voxel prediction inside the square
    m = _one(_plane((1, 1)), sq, min_size=2)
    assert (m["n_pred"], m["n_target"], m["det_tp"], m["det_fn"]) == (0, 1, 0, 1)
    # the nan rules
    empty = _plane()
    m = _one(empty, empty)
    assert all(math.isnan(m[k]) for k in ("sensitivity", "precision", "f1", "pq", "sq", "rq", "lesion_dice"))
    m = _one(sq, empty)
    assert math.isnan(m["sensitivity"]) and m["precision"] == 0.0 and math.isnan(m["f1"]) and m["pq"] == 0.0 and m["rq"] == 0.0
    m = _one(empty, sq)
    assert m["sensitivity"] == 0.0 and math.isnan(m["precision"]) and m["pq"] == 0.0 and (m["fn"], m["fp"]) == (1, 0)
    # a void target value is background: the prediction under it is a false alarm
    void = sq.copy()
    void[void == 1] = 255
    m = _one(sq, void)
    assert (m["n_target"], m["det_fp"]) == (0, 1)
    # reductions: 'mean' skips the nan of the empty case, 'pooled' adds the counts
    r = R.metrics([(sq, sq), (empty, empty), (sq, shifted)], 2, 26)
    assert r["mean"]["pq"].tolist() == [0.5] and r["pooled"]["tp"].tolist() == [1] and abs(r["pooled"]["pq"][0] - 0.5) < 1e-15
    assert np.isnan(r["per_case"]["pq"][1, 0]) and r["per_case"]["pq"].shape == (3, 1)


# ---------------------------------------------------------------- what the GPU tests rest on
ROOMY = [(s, C) for s in R.SHAPES[2:] for C in (2, 4, 9)] + [((1, 8, 8), 2)]
CRAMPED = [((1, 8, 8), 4), ((1, 8, 8), 9), ((2, 2, 2), 2), ((2, 2, 2), 4), ((2, 2, 2), 9)]


def _pair_table(shape, C, connectivity):
    ck, cs, pk, pc, ctrl = R.records(*R.lesion_case(*shape, C), C, connectivity)
    size = dict(zip(ck.tolist(), cs.tolist()))
    rows = []
    for key, n in zip(pk.tolist(), pc.tolist()):
        rp, rg = key >> 32, key & 0xFFFFFFFF
        k = next(c for c in range(1, C) if (c << 32 | rp) in size and (1 << 40 | c << 32 | rg) in size)
        n_p, n_g = size[k << 32 | rp], size[1 << 40 | k << 32 | rg]
        rows.append((k, rp, rg, n / (n_p + n_g - n)))
    return ck, rows


@pytest.mark.parametrize("shape,C", ROOMY, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_generator_conditions(shape, C):
    """Every scored class of lesion_case has a pair of IoU 1, a pair with 0.5 < IoU < 1, a pair with 0 < IoU <= 0.5, a prediction over
    two targets, a target under two predictions, a false positive and a miss, under each connectivity -- wherever the volume has
    room for the 2 (C - 1) motif rows, which is every case of the GPU tests but the five of test_cramped_cases."""
    for conn in (6, 18, 26):
        ck, rows = _pair_table(shape, C, conn)
        for k in range(1, C):
            mine = [r for r in rows if r[0] == k]
            ious = [r[3] for r in mine]
            assert any(v == 1.0 for v in ious) and any(0.5 < v < 1 for v in ious) and any(0 < v <= 0.5 for v in ious), (conn, k)
            ps, gs = [r[1] for r in mine], [r[2] for r in mine]
            assert max(ps.count(p) for p in set(ps)) >= 2 and max(gs.count(g) for g in set(gs)) >= 2, (conn, k)
            preds = {key & 0xFFFFFFFF for key in ck.tolist() if key >> 40 == 0 and (key >> 32) & 0xFF == k}
            targets = {key & 0xFFFFFFFF for key in ck.tolist() if key >> 40 == 1 and (key >> 32) & 0xFF == k}
            assert preds - set(ps) and targets - set(gs), (conn, k)     # a false positive and a miss


@pytest.mark.parametrize("shape,C", CRAMPED, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_cramped_cases(shape, C):
    """The volumes without room for every motif row.  (2, 2, 2) holds one row cut to two columns: an identical pair of class 1 and
    nothing else.  (1, 8, 8) holds four rows, A rows first: an identical pair, a pair of IoU 2/3, a false positive and a miss of the
    classes 1 .. min(C - 1, 4)."""
    ck, rows = _pair_table(shape, C, 26)
    if shape == (2, 2, 2):
        assert rows == [(1, 0, 0, 1.0)] and ck.tolist() == [1 << 32, 1 << 40 | 1 << 32]
    else:
        for k in range(1, min(C - 1, 4) + 1):
            assert {2 / 3, 1.0} <= {r[3] for r in rows if r[0] == k}
            paired = {(0, r[1]) for r in rows} | {(1, r[2]) for r in rows}
            alone = [key >> 40 for key in ck.tolist() if (key >> 32) & 0xFF == k and (key >> 40, key & 0xFFFFFFFF) not in paired]
            assert sorted(set(alone)) == [0, 1], k                    # a false positive and a miss


def test_kernel_cases_are_what_they_claim():
    """grid_case: 1024 isolated voxels, and (1, 1, 1) is isolated from them under 6.  The checkerboard under 6: 7507 pairs, 7508
    lesions, a load of 0.92 in 8192 slots."""
    g = R.grid_case()
    ck, cs, pk, pc, ctrl = R.records(g, np.ones_like(g), 2, 26)
    assert ctrl.tolist() == [1025, 1024, 0, 0] and (cs[:1024] == 1).all() and cs[1024] == g.size and (pc == 1).all()
    g1 = g.copy()
    g1[1, 1, 1] = 1
    assert R.records(g1, np.ones_like(g), 2, 6)[4].tolist() == [1026, 1025, 0, 0]
    assert R.records(g1, np.ones_like(g), 2, 26)[4].tolist()[1] < 1025                       # (under 26 it joins its neighbours)
    Lp, Lt = R.checkerboard_case()
    ctrl = R.records(Lp, Lt, 2, 6)[4]
    assert ctrl.tolist() == [7508, 7507, 0, 0] and 0.91 < 7507 / 8192 < 0.92

"""CPU: the host side of the volume slicer (include/slices/lmnet_slices.h; lm_net_amd.data.VolumeSlicer): registry and header agree,
the argument checks of the C entries (rejected before any HIP call, with fake device pointers) and of the class, and the restatement tests/slices_ref.py: against torch's F.interpolate in float64, against numpy's mean,
std and percentile, and float32 against float64 coordinates on the cases of the GPU tests.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import slices_ref as R
from lm_net_amd import VolumeSlicer, hip  # noqa: F401  (every test of this file belongs to the feature)
from lm_net_amd.data import resize_map, slice_param_row, ssr_matrix

assert callable(hip.slices_gather)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_ENTRIES = ["lmn_slices_stats", "lmn_slices_gather"]


# ---------------------------------------------------------------- ABI
def test_registry_and_header_agree():
    """The feature's own part of the registry: the literal list, its place in hip.HEADERS, the number of #defines, the header's
    citations and the package's export.  (Header / export / layout / return-type / constants checks: tests/test_host_cpu.py.)"""
    assert hip.SYMBOLS_SLICES == ["lmn_slices_workspace"] + DEVICE_ENTRIES
    assert hip.HEADERS["slices/lmnet_slices.h"] is hip.SYMBOLS_SLICES
    header = open(os.path.join(ROOT, "include", "slices", "lmnet_slices.h")).read()
    assert len(re.findall(r"^#define LMN_SLICES_\w+ \(?-?\d+\)?", header, re.M)) == 20
    for cite in ("r = (q_ppm * (n - 1)) / 1000000", "WITH n = 0 EVERY FIELD IS 0", "b = 0 WHEN n = 0", "b = 0 WHEN\n *      v_hi == v_lo",
                 "never NaN or infinite", "sx = __fadd_rn(__fadd_rn(__fmul_rn(m0, x), __fmul_rn(m1, y)), m2)", "floorf(__fadd_rn(s, 0.5f))",
                 "nearest-exact", "slices_workspace: ", "slices_stats: ", "slices_gather: "):
        assert cite in header, cite
    import lm_net_amd
    from lm_net_amd import data
    assert lm_net_amd.VolumeSlicer is data.VolumeSlicer and "VolumeSlicer" in lm_net_amd.__all__


# ---------------------------------------------------------------- argument checks
FAKE = ctypes.c_void_p(0x1000)


def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _stats(null=(), **kw):
    """lmn_slices_stats with fake device pointers: every case here must be rejected before any HIP call."""
    lib = hip.load()
    g = dict(dict(kind=0, M=2, D=9, Hs=33, Ws=47, fg=(-32769, 0), q_lo=5000, q_hi=995000, mod=(0, 0, 1), knd=(1, 0, 2), level=(0.0, 40.0, 0.0),
                  width=(1.0, 400.0, 1.0), ws_bytes=1 << 30), **kw)
    S = g.get("S", len(g["mod"]))
    a = dict(volume=FAKE, fg=_i32(*g["fg"]), mod=_i32(*g["mod"]), knd=_i32(*g["knd"]), level=(ctypes.c_double * len(g["level"]))(*g["level"]),
             width=(ctypes.c_double * len(g["width"]))(*g["width"]), workspace=FAKE, stats=FAKE, table=FAKE)
    for k in null:
        a[k] = None
    rc = lib.lmn_slices_stats(a["volume"], g["kind"], g["M"], g["D"], g["Hs"], g["Ws"], a["fg"], g["q_lo"], g["q_hi"], S, a["mod"], a["knd"],
                              a["level"], a["width"], a["workspace"], ctypes.c_int64(g["ws_bytes"]), a["stats"], a["table"], None)
    return rc, lib.lmn_last_error().decode()


def _gather(null=(), **kw):
    """lmn_slices_gather with fake device pointers"""
    lib = hip.load()
    g = dict(dict(kind=0, M=2, D=9, Hs=33, Ws=47, n=3, mod=(0, 0, 1), context=1, stride=1, edge=0, border=0, bval=(0.0, 0.0), label_border=0, h=32,
                  w=32, label_kind=0), **kw)
    S = g.get("S", len(g["mod"]))
    a = dict(volume=FAKE, labels=FAKE, z=FAKE, params=FAKE, table=FAKE, mod=_i32(*g["mod"]), bval=(ctypes.c_float * len(g["bval"]))(*g["bval"]),
             x=FAKE, y=FAKE)
    for k in null:
        a[k] = None
    rc = lib.lmn_slices_gather(a["volume"], g["kind"], a["labels"], g["M"], g["D"], g["Hs"], g["Ws"], a["z"], a["params"], g["n"], a["table"], S,
                               a["mod"], g["context"], g["stride"], g["edge"], g["border"], a["bval"], g["label_border"], g["h"], g["w"], a["x"],
                               a["y"], g["label_kind"], None)
    return rc, lib.lmn_last_error().decode()


VOLUME_CASES = [(dict(kind=2), "unknown volume kind 2"), (dict(M=0), "M=0 not in [1, 4]"), (dict(M=5), "M=5 not in [1, 4]"),
                (dict(D=0), "D=0 not in [1, 1024]"), (dict(D=1025), "D=1025 not in [1, 1024]"), (dict(Hs=1), "size 1x47 not in [2, 1024]"),
                (dict(Ws=1025), "size 33x1025 not in [2, 1024]"), (dict(mod=(0, 2, 1)), "spec 1 names modality 2 of 2"),
                (dict(mod=(1, 0, 1)), "modalities must not decrease"), (dict(S=0), "S=0 not in [1, 16]"), (dict(S=17), "S=17 not in [1, 16]")]


def test_stats_rejects_bad_arguments():
    for name in ("volume", "fg", "mod", "knd", "level", "width", "workspace", "stats", "table"):
        rc, err = _stats(null=(name,))
        assert rc == -1 and err == "slices_stats: null pointer", (name, err)
    need = hip.slices_workspace(2, 9, 33, 47)
    assert need == (2 * (64 + 4 * (1024 + 128 + 8)) + 255) // 256 * 256
    cases = VOLUME_CASES + [(dict(fg=(-32770, 0)), "foreground[0]=-32770 not in [-32769, 32767]"), (dict(fg=(0, 32768)), "foreground[1]=32768"),
                            (dict(q_lo=-1), "ranks -1, 995000 ppm"), (dict(q_lo=600000, q_hi=500000), "not 0 <= lo <= hi <= 1000000"),
                            (dict(q_hi=1000001), "ranks 5000, 1000001 ppm"), (dict(knd=(1, 3, 2)), "spec 1: unknown kind 3"),
                            (dict(width=(1.0, 0.0, 1.0)), "spec 1: window level=40, width=0"), (dict(width=(1.0, float("nan"), 1.0)), "spec 1: window"),
                            (dict(level=(0.0, float("inf"), 0.0)), "spec 1: window level=inf"),
                            (dict(ws_bytes=need - 1), "workspace of %d bytes too small, %d needed" % (need - 1, need))]
    for kw, msg in cases:
        rc, err = _stats(**kw)
        assert rc == -1 and msg in err and err.startswith("slices_stats: "), (kw, err)
    for args in ((0, 9, 33, 47), (2, 0, 33, 47), (2, 9, 1, 47), (2, 9, 33, 1025)):
        with pytest.raises(ValueError, match="slices_workspace"):
            hip.slices_workspace(*args)
    assert hip.slices_workspace(4, 1024, 1024, 1024) == (4 * 4704 + 255) // 256 * 256 and hip.slices_workspace(1, 1, 2, 2) == 4864


def test_gather_rejects_bad_arguments():
    for name in ("z", "params", "table", "mod", "bval"):
        rc, err = _gather(null=(name,))
        assert rc == -1 and err == "slices_gather: null pointer", (name, err)
    for null, msg in ((("volume", "labels", "x", "y"), "neither a volume nor labels"), (("x",), "a volume needs x"), (("volume",), "a volume needs x"),
                      (("y",), "labels need y"), (("labels",), "labels need y")):
        rc, err = _gather(null=null)
        assert rc == -1 and msg in err and err.startswith("slices_gather: "), (null, err)
    cases = VOLUME_CASES + [(dict(n=0), "n=0 not in [1, 65535]"), (dict(n=65536), "n=65536 not in"), (dict(h=0), "output size 0x32 not in [1, 4096]"),
                            (dict(w=4097), "output size 32x4097"), (dict(context=-1), "context=-1 not in [0, 7]"), (dict(context=8), "context=8"),
                            (dict(stride=0), "stride=0 not in [1, 1024]"), (dict(edge=2), "unknown edge 2"), (dict(border=-1), "unknown border -1"),
                            (dict(label_border=256), "label_border=256 not in [0, 255]"), (dict(label_kind=2), "unknown label kind 2"),
                            (dict(context=3), "3 specs x 7 slices = 21 channels, above 16"), (dict(bval=(0.0, 1e6)), "border_value[1]=1e+06"),
                            (dict(bval=(float("nan"), 0.0)), "border_value[0]=nan")]
    for kw, msg in cases:
        rc, err = _gather(**kw)
        assert rc == -1 and msg in err and err.startswith("slices_gather: "), (kw, err)


def test_class_rejects_bad_arguments():
    bad = [dict(modalities=0), dict(modalities=5), dict(size=(0, 32)), dict(size=(32, 5000)), dict(context=8), dict(stride=0), dict(edge="wrap"),
           dict(border="reflect"), dict(label_dtype=torch.int32), dict(label_border=256), dict(norm="minmax"), dict(norm=("window", 40)),
           dict(norm=("window", 40, 0)), dict(norm=("zscore", 1)), dict(norm=["zscore", "zscore"]), dict(modalities=2, norm=["zscore"]),
           dict(context=3, norm=[["zscore", "percentile", ("window", 0, 1)]]), dict(foreground=40000), dict(modalities=2, foreground=[0]),
           dict(clip=(5,)), dict(clip=(60, 40)), dict(clip=(0, 101)), dict(border_value=1e6), dict(modalities=2, border_value=[0, 0, 0]),
           dict(p_ssr=1.5), dict(scale_limit=1.0), dict(gain_limit=-0.1)]
    for kw in bad:
        with pytest.raises(ValueError, match="VolumeSlicer"):
            VolumeSlicer(**kw)
    with pytest.raises(ValueError, match="at most|limit"):
        VolumeSlicer(context=2, norm=[["zscore", "percentile", ("window", 0, 1), ("window", 0, 2)]])       # 20 channels
    s = VolumeSlicer(size=(32, 32), modalities=2, norm=[["zscore", ("window", 40, 400)], ("percentile",)], context=1, clip=(0.5, 99.5))
    assert s.channels == 9 and s.q_ppm == (5000, 995000)
    assert s.specs == [(0, hip.SLICES_ZSCORE, 0.0, 1.0), (0, hip.SLICES_WINDOW, 40.0, 400.0), (1, hip.SLICES_PERCENTILE, 0.0, 1.0)]
    for call in (lambda: s.slices(0, 1), lambda: s.batch([0]), lambda: s.restore(torch.zeros(1, 4, 4, dtype=torch.uint8))):
        with pytest.raises(ValueError, match="no case is open"):
            call()
    # the limits of open_case are checked before the device is touched, each named
    for shape, word in (((2, 1025, 4, 4), "D = 1025 outside the limit [1, 1024]"), ((2, 3, 1, 4), "outside the limit [2, 1024]"),
                        ((2, 3, 4, 1025), "outside the limit [2, 1024]"), ((3, 3, 4, 4), "modalities"), ((3, 4, 4), "modalities")):
        with pytest.raises(ValueError, match=re.escape(word)):
            s.open_case(torch.zeros(shape, dtype=torch.int16))
    with pytest.raises(ValueError, match="int16 or uint8"):
        s.open_case(torch.zeros(2, 3, 4, 4))
    with pytest.raises(ValueError, match="labels must be uint8"):
        s.open_case(torch.zeros(2, 3, 4, 4, dtype=torch.int16), torch.zeros(3, 4, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="parameter sets"):
        s.rows(3, s.sample(2, 0), (32, 32), (40, 48))
    with pytest.raises(ValueError, match="flips 0..3"):
        s.rows(1, [dict(flips=4)], (32, 32), (40, 48))
    a, b = s.sample(5, 7), s.sample(5, 7)
    assert a == b and {"M", "flips", "gain", "bias"} == set(a[0]) and a != s.sample(5, 8)


# ---------------------------------------------------------------- the restatement
def _rows64(n, dst, src):
    T = resize_map(dst, src)
    return np.tile(np.array([T[0, 0], T[0, 1], T[0, 2], T[1, 0], T[1, 1], T[1, 2], 1.0, 0.0]), (n, 1))


@pytest.mark.parametrize("src,dst", [((5, 7), (16, 16)), ((50, 60), (32, 32)), ((12, 16), (12, 16)), ((9, 11), (18, 33))])
def test_restatement_equals_interpolate_bilinear(src, dst):
    """float64 coordinates, identity table: the image is F.interpolate(bilinear, align_corners=False) in float64 to 1e-9 (of values
    up to 2^15) and the plain-resize row of the class is the float32 rounding of the same map."""
    g = np.random.default_rng(1)
    vol = g.integers(-32768, 32768, size=(1, 2, src[0], src[1])).astype(np.int16)
    tab = np.array([[-1e9, 1e9, 0.0, 1.0]])
    x, _, _ = R.gather(vol, None, [0, 1], _rows64(2, dst, src), tab, [0], 0, 1, dst, coord_dtype=np.float64)
    want = F.interpolate(torch.from_numpy(vol[0].astype(np.float64))[:, None], size=dst, mode="bilinear", align_corners=False)[:, 0].numpy()
    assert np.abs(x[:, 0] - want).max() <= 1e-9 * 32768
    assert np.array_equal(slice_param_row(dst, src), _rows64(1, dst, src)[0].astype(np.float32))


@pytest.mark.parametrize("src,dst", [((5, 7), (15, 14)), ((12, 16), (12, 16)), ((48, 60), (16, 20)), ((32, 32), (8, 16))])
def test_restatement_labels_equal_nearest_exact_at_integer_factors(src, dst):
    g = np.random.default_rng(2)
    lab = g.integers(0, 256, size=(3, src[0], src[1])).astype(np.uint8)
    want = F.interpolate(torch.from_numpy(lab.astype(np.float64))[:, None], size=dst, mode="nearest-exact")[:, 0].numpy().astype(np.int64)
    for dt in (np.float32, np.float64):
        rows = _rows64(3, dst, src) if dt is np.float64 else np.tile(slice_param_row(dst, src), (3, 1))
        _, y, _ = R.gather(None, lab, [0, 1, 2], rows, None, None, 0, 1, dst, coord_dtype=dt)
        assert np.array_equal(y, want), dt


def test_record_and_table_equal_numpy():
    """n, sums and extrema against numpy on int64, mean and std against numpy's float64 to 1e-12 relative (numpy's own pairwise sums
    are good to a few ulp), the order statistics against np.percentile(method="lower") where q (n - 1) is not within 1e-6 of an
    integer, and the edge rules."""
    g = np.random.default_rng(3)
    for shape, fg, q in (((1, 3, 5, 7), None, (0.5, 99.5)), ((2, 9, 33, 47), -900, (1.0, 99.0)), ((1, 2, 31, 17), 0, (2.5, 97.5)),
                         ((1, 1, 300, 300), None, (0.5, 99.5))):
        vol = g.integers(-2000, 3000, size=shape).astype(np.int16)
        vol[g.random(shape) < 0.4] = -1024
        fgs = [R.NO_FOREGROUND if fg is None else fg] * shape[0]
        ppm = (int(round(q[0] * 1e4)), int(round(q[1] * 1e4)))
        rec = R.record(vol, fgs, ppm)
        tab = R.table(rec, [(m, R.ZSCORE, 0.0, 1.0) for m in range(shape[0])])
        for m in range(shape[0]):
            v = vol[m].reshape(-1).astype(np.int64)
            v = v[v > fgs[m]]
            n = v.size
            assert rec[m][:5] == [n, int(v.sum()), int((v * v).sum()), int(v.min()), int(v.max())] and rec[m][7] == 0
            assert abs(tab[m, 2] - v.mean()) <= 1e-12 * abs(v.mean()) and abs(1.0 / tab[m, 3] - v.std()) <= 1e-12 * v.std()
            for k, qq in enumerate(q):
                pos = qq / 100.0 * (n - 1)
                assert abs(pos - round(pos)) > 1e-6, "choose another size: q (n - 1) is an integer here"
                assert rec[m][5 + k] == int(np.percentile(v, qq, method="lower"))
    const = np.full((1, 2, 4, 4), 7, dtype=np.int16)
    rec = R.record(const, [R.NO_FOREGROUND], (5000, 995000))
    assert rec == [[32, 224, 1568, 7, 7, 7, 7, 0]]
    tab = R.table(rec, [(0, R.ZSCORE, 0, 1), (0, R.PERCENTILE, 0, 1), (0, R.WINDOW, 40.0, 400.0)])
    assert tab.tolist() == [[7.0, 7.0, 7.0, 1e8], [7.0, 7.0, 7.0, 0.0], [-160.0, 240.0, -160.0, 0.0025]]      # std = 0 and v_hi == v_lo
    rec = R.record(const, [7], (0, 1000000))                                                                # a foreground that excludes everything
    assert rec == [[0] * 8] and not R.table(rec, [(0, R.ZSCORE, 0, 1), (0, R.PERCENTILE, 0, 1)]).any()


def _case_rows(name):
    case = R.GATHER_CASES[name]
    kw = dict(case["kw"])
    if kw.get("label_dtype") == "int64":
        kw["label_dtype"] = torch.int64
    s = VolumeSlicer(**kw)
    Hs, Ws = case["shape"][2:]
    return s, s.rows(len(case["z"]), R.case_params(case, s.size, ssr_matrix), s.size, (Hs, Ws))


@pytest.mark.parametrize("name", list(R.GATHER_CASES))
def test_float32_and_float64_coordinates_give_the_same_labels(name):
    """On every case of tests/test_slices_kernels_gpu.py the two restatements agree on every label whose coordinate is not within
    1e-4 of a tie, and those are under 0.5 % of the case's pixels."""
    case = R.GATHER_CASES[name]
    vol, lab = R.case_data(name)
    s, rows = _case_rows(name)
    kw = dict(border=s.border, label_border=s.label_border)
    _, y32, _ = R.gather(None, lab, case["z"], rows, None, None, 0, 1, s.size, coord_dtype=np.float32, **kw)
    _, y64, near = R.gather(None, lab, case["z"], rows, None, None, 0, 1, s.size, coord_dtype=np.float64, **kw)
    assert np.array_equal(y32[~near], y64[~near])
    assert near.mean() < 0.005, near.mean()
    assert vol.shape == case["shape"] and 0 < lab.max() <= 2

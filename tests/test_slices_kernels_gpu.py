"""GPU: the kernels of include/slices/lmnet_slices.h against tests/slices_ref.py.  The record is compared EXACTLY (integer arithmetic on
both sides) and the table to 1e-6 relative; for the gather the restatement runs on the device's own table with float32 coordinates,
labels are compared exactly with no pixel left out and images within slices_ref.tol, the derived device bound.  Every test prints its
measured maximum beside the bound."""
import numpy as np
import pytest
import torch

import slices_ref as R
from lm_net_amd import VolumeSlicer, hip
from lm_net_amd.data import ssr_matrix

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ALL3 = [(0, hip.SLICES_ZSCORE, 0.0, 1.0), (0, hip.SLICES_PERCENTILE, 0.0, 1.0), (0, hip.SLICES_WINDOW, 40.0, 400.0)]


def _stats(vol, fg, q_ppm, specs):
    """(record as lists of ints, table float64 [S, 4]) of the device for a numpy volume [M, D, Hs, Ws]"""
    M, D, Hs, Ws = vol.shape
    v = torch.from_numpy(vol).to(DEV)
    ws = torch.empty(hip.slices_workspace(M, D, Hs, Ws), device=DEV, dtype=torch.uint8).fill_(0xA5)
    stats = torch.empty(M, 8, device=DEV, dtype=torch.int64).fill_(-7)
    table = torch.full((len(specs), 4), float("nan"), device=DEV)
    hip.slices_stats(v, fg, q_ppm[0], q_ppm[1], specs, ws, stats, table)
    return stats.cpu().tolist(), table.cpu().numpy().astype(np.float64), stats, table


def _check_stats(vol, fg, q_ppm, specs, what):
    rec, tab, _, _ = _stats(vol, fg, q_ppm, specs)
    want = R.record(vol, fg, q_ppm)
    assert rec == want, (what, rec, want)
    ref = R.table(want, specs)
    assert np.isfinite(tab).all()
    err = float(np.max(np.abs(tab - ref) / np.maximum(np.abs(ref), 1e-30) * (ref != 0) + np.abs(tab) * (ref == 0)))
    print("%s: record exact; table max relative error %.3g (bound 1e-6)" % (what, err))
    assert err <= 1e-6, (what, tab, ref)
    return rec, tab


def _volume(shape, seed, lo=-2000, hi=3000, air=0.4, dtype=np.int16):
    g = np.random.default_rng(seed)
    vol = g.integers(lo, hi, size=shape).astype(dtype)
    if air:
        vol[g.random(shape) < air] = -1024 if dtype == np.int16 else 0
    return vol


NONE = R.NO_FOREGROUND
STATS_CASES = {
    "3x5x7_less_than_a_wave": lambda: (_volume((1, 3, 5, 7), 1), [NONE], (5000, 995000)),
    "9x33x47": lambda: (_volume((1, 9, 33, 47), 2), [-1000], (10000, 990000)),
    "two_modalities": lambda: (_volume((2, 4, 16, 24), 3), [-1000, NONE], (25000, 975000)),
    "constant_1x300x300": lambda: (np.full((1, 1, 300, 300), -1024, dtype=np.int16), [NONE], (5000, 995000)),
    "extremes": lambda: (np.concatenate([_volume((1, 2, 8, 9), 4).reshape(-1), np.array([-32768, 32767, -32768], dtype=np.int16)])
                         .reshape(1, 1, 3, 49), [NONE], (0, 1000000)),
    "both_ranks_in_one_coarse_bin": lambda: (_volume((1, 2, 9, 11), 5, 128, 192, air=0), [NONE], (100000, 900000)),
    "ranks_either_side_of_a_bin_boundary": lambda: (np.array([63, 64] * 35, dtype=np.int16).reshape(1, 2, 5, 7), [NONE], (250000, 750000)),
    "foreground_excludes_everything": lambda: (_volume((1, 2, 9, 11), 6), [32767], (5000, 995000)),
    "no_clip": lambda: (_volume((1, 2, 9, 11), 7), [-1000], (0, 1000000)),
    "uint8": lambda: (_volume((1, 3, 16, 16), 8, 0, 256, dtype=np.uint8), [0], (5000, 995000)),
    "uint8_odd": lambda: (_volume((1, 3, 5, 7), 9, 0, 256, dtype=np.uint8), [NONE], (5000, 995000)),
}


@pytest.mark.parametrize("name", list(STATS_CASES))
def test_statistics(name):
    vol, fg, q = STATS_CASES[name]()
    specs = [(m, k, lv, w) for m in range(vol.shape[0]) for _, k, lv, w in ALL3]
    rec, tab = _check_stats(vol, fg, q, specs, name)
    if name == "constant_1x300x300":
        assert rec[0] == [90000, -1024 * 90000, 1024 * 1024 * 90000, -1024, -1024, -1024, -1024, 0]
        assert tab[0].tolist() == [-1024.0, -1024.0, -1024.0, float(np.float32(1e8))] and tab[1, 3] == 0.0       # std = 0 exactly; v_hi == v_lo
    if name == "foreground_excludes_everything":
        assert rec == [[0] * 8] and not tab[:2].any()                                                           # n = 0: every field 0, b = 0
    if name == "ranks_either_side_of_a_bin_boundary":
        assert rec[0][5:7] == [63, 64]
    if name == "extremes":
        assert rec[0][3:7] == [-32768, 32767, -32768, 32767]


def test_statistics_are_bit_identical_from_call_to_call():
    vol = _volume((2, 5, 33, 47), 11)
    specs = [(m, k, lv, w) for m in range(2) for _, k, lv, w in ALL3]
    a = _stats(vol, [-1000, NONE], (5000, 995000), specs)
    b = _stats(vol, [-1000, NONE], (5000, 995000), specs)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3].view(torch.int32), b[3].view(torch.int32))


# ---------------------------------------------------------------- gather
def _slicer(name):
    case = R.GATHER_CASES[name]
    kw = dict(case["kw"])
    if kw.get("label_dtype") == "int64":
        kw["label_dtype"] = torch.int64
    s = VolumeSlicer(**kw)
    vol, lab = R.case_data(name)
    v = torch.from_numpy(vol).to(DEV)
    s.open_case(v[0] if vol.shape[0] == 1 else v, torch.from_numpy(lab).to(DEV))
    return case, s, vol, lab


def _reference(case, s, vol, lab, rows):
    tab = s.table.cpu().numpy().astype(np.float64)
    x, y, _ = R.gather(vol, lab, case["z"], rows, tab, [m for m, _, _, _ in s.specs], s.context, s.stride, s.size, edge=s.edge, border=s.border,
                       border_value=s.border_value, label_border=s.label_border, coord_dtype=np.float32)
    return x, y, R.tol(x, rows, tab, 2 * s.context + 1, R.vmax(vol, s.border_value, tab))


@pytest.mark.parametrize("name", list(R.GATHER_CASES))
def test_gather(name):
    case, s, vol, lab = _slicer(name)
    params = R.case_params(case, s.size, ssr_matrix)
    rows = s.rows(len(case["z"]), params)
    x, y = s.batch(case["z"], params)
    n, (h, w) = len(case["z"]), s.size
    assert tuple(x.shape) == (n, s.channels, h, w) and x.dtype == torch.float32 and tuple(y.shape) == (n, h, w) and y.dtype == s.label_dtype
    want_x, want_y, tol = _reference(case, s, vol, lab, rows)
    assert np.array_equal(y.cpu().numpy().astype(np.int64), want_y)                     # every pixel, none left out
    err = np.abs(x.cpu().numpy().astype(np.float64) - want_x)
    k = int(np.argmax(err / tol))
    print("%s: max |x - ref| %.3g (bound there %.3g, ratio %.3g), max |x| %.3g" % (name, err.max(), tol.reshape(-1)[k], (err / tol).max(),
                                                                                    np.abs(want_x).max()))
    assert np.isfinite(x.cpu().numpy()).all() and (err <= tol).all()
    # the same slices from a device index tensor, and (where they are consecutive and unwarped) from slices()
    x0, y0 = x.clone(), y.clone()
    x1, y1 = s.batch(torch.tensor(case["z"], dtype=torch.int32, device=DEV), params)
    assert torch.equal(x0, x1) and torch.equal(y0, y1)
    z = case["z"]
    if params is None and z == list(range(z[0], z[0] + n)):
        x2, y2 = s.slices(z[0], z[0] + n)
        assert torch.equal(x0, x2) and torch.equal(y0, y2)


def test_restore_32x32_to_50x60():
    """The way back to the source grid: label-only mode, nearest under the half-pixel rule, exactly the restatement's labels."""
    case, s, vol, lab = _slicer("down_50x60_to_32x32")
    g = np.random.default_rng(5)
    net = g.integers(0, 4, size=(3, 32, 32)).astype(np.uint8)
    out = s.restore(torch.from_numpy(net).to(DEV))
    assert tuple(out.shape) == (3, 50, 60) and out.dtype == torch.uint8
    rows = s.rows(3, None, (50, 60), (32, 32))
    _, want, _ = R.gather(None, net, [0, 1, 2], rows, None, None, 0, 1, (50, 60), coord_dtype=np.float32)
    assert np.array_equal(out.cpu().numpy().astype(np.int64), want)


def test_stats_and_table_of_the_open_case():
    case, s, vol, lab = _slicer("c12")
    want = R.record(vol, s.foreground, s.q_ppm)
    assert s.stats.cpu().tolist() == want and tuple(s.table.shape) == (4, 4)
    ref = R.table(want, s.specs)
    assert np.allclose(s.table.cpu().numpy().astype(np.float64), ref, rtol=1e-6, atol=0)

"""GPU: lmn_curve_hist (lm_net_amd/csrc/curves.hip) against the brute-force restatement tests/curves_ref.py.  Every comparison is
exact, cell for cell: the kernel counts integers and decides a bin only by fp32 comparisons against the edge table, which numpy
repeats bit for bit.  In the softmax form the inputs are drawn so that no probability lies within 1e-4 of an edge (the fp32
probability is within about 1e-6 of the float64 one), and no element is left out."""
import numpy as np
import pytest
import torch

import curves_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def device_hist(values, target, thresholds, scores="sigmoid", form="planes"):
    """hip.curve_hist on device tensors (values / target may be views) -> int64 numpy [B, C, 2, N + 1]"""
    from lm_net_amd import hip
    B, C = values.shape[:2]
    hw = values.numel() // (B * C)
    kind = hip.CURVE_SOFTMAX if scores == "softmax" else hip.CURVE_RAW
    edges = torch.from_numpy(hip.curve_edges(thresholds, "logit" if scores == "sigmoid" else "probability")).to(DEV)
    ws = torch.empty(hip.curve_workspace(kind, B, hw), device=DEV, dtype=torch.uint8) if kind == hip.CURVE_SOFTMAX else None
    hist = torch.full((B, C, 2, edges.numel() + 1), -7, device=DEV, dtype=torch.int64)         # (the entry zeroes it itself)
    hip.curve_hist(values, target, hip.CURVE_LABELS if form == "labels" else hip.CURVE_PLANES, kind, edges, hist, ws)
    return hist.cpu().numpy()


def check(z, t, thresholds, scores="sigmoid", form="planes"):
    got = device_hist(torch.from_numpy(z).to(DEV), torch.from_numpy(t).to(DEV), thresholds, scores, form)
    ref = R.hist(z, t, thresholds, scores, form)
    assert got.shape == ref.shape and np.array_equal(got, ref), "%d of %d cells differ" % (int((got != ref).sum()), ref.size)
    return got


# ---------------------------------------------------------------- RAW form: the launch geometry
@pytest.mark.parametrize("shape", [(1, 1, 3, 5), (2, 3, 17, 23), (2, 1, 64, 64), (2, 8, 264, 256)], ids=lambda s: "x".join(map(str, s)))
def test_raw_form_shapes(shape):
    """(1, 1, 3, 5): one partial trip, scalar loads; (2, 3, 17, 23): odd HW, several planes; (2, 1, 64, 64): vector loads;
    (2, 8, 264, 256): 16 planes of 67584 elements = 16896 four-element items = 66 blocks' worth, and a plane gets 1024 / 16 = 64 blocks
    under the entry's cap of 1024 blocks, so blocks 0 and 1 of every plane take a second trip."""
    z = R.logits(shape, "shapes/z/%d" % shape[-1])
    t = R.plane_targets(shape, "shapes/t/%d" % shape[-1])
    got = check(z, t, 101)
    assert got.sum() == ((t == 0) | (t == 1)).sum()
    if shape[-1] == 256:
        # both routes: the table starts at -inf and ends at +inf, so bins 1 and 100 are the populated end bins (ballots), 2 .. 99 take LDS atomics
        assert got[..., 2:-2].sum() > got.sum() // 4 and got[..., 1].sum() > 0 and got[..., -2].sum() > 0 and got[..., 0].sum() == 0


def test_raw_form_view_offset_by_four_bytes_takes_the_scalar_route():
    """HW % 4 == 0 but the values start 4 bytes (and the uint8 target 1 byte) off a 16-byte boundary: 16-byte loads would be
    misaligned, so the entry must fall back to one element per lane."""
    shape = (2, 2, 16, 24)
    z, t = R.logits(shape, "offset/z"), R.plane_targets(shape, "offset/t", dtype=np.uint8)
    n = z.size
    zb, tb = torch.zeros(n + 4, device=DEV), torch.zeros(n + 4, device=DEV, dtype=torch.uint8)
    zv, tv = zb[1:n + 1].view(shape), tb[1:n + 1].view(shape)
    zv.copy_(torch.from_numpy(z))
    tv.copy_(torch.from_numpy(t))
    assert zv.data_ptr() % 16 == 4 and tv.data_ptr() % 4 == 1 and zv.is_contiguous()
    ref = R.hist(z, t, 101)
    assert np.array_equal(device_hist(zv, tv, 101), ref)
    assert np.array_equal(device_hist(zv, torch.from_numpy(t).to(DEV), 101), ref)           # only the values are offset
    assert np.array_equal(device_hist(torch.from_numpy(z).to(DEV), tv, 101), ref)           # only the target


# ---------------------------------------------------------------- RAW form: contents
def special_logits(shape, key):
    z = R.logits(shape, key)
    flat = z.reshape(-1)
    idx = R.rng(key + "/special").permutation(flat.size)[:60]
    flat[idx[:20]], flat[idx[20:40]], flat[idx[40:]] = np.nan, np.inf, -np.inf
    return z


@pytest.mark.parametrize("form", ["planes", "labels"])
@pytest.mark.parametrize("dtype", [np.uint8, np.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("thresholds", [2, 101, 1024, [0.5]], ids=["2", "101", "1024", "one"])
def test_raw_form_contents(thresholds, dtype, form):
    """20 % void elements, logits with NaN, +inf and -inf, both target kinds and both target forms, at every table size."""
    shape = (2, 3, 17, 23)
    z = special_logits(shape, "contents/z")
    t = (R.plane_targets(shape, "contents/t", 0.2, dtype) if form == "planes" else R.label_targets((2, 17, 23), 3, "contents/l", 0.2, dtype))
    got = check(z, t, thresholds, "sigmoid", form)
    valid = ((t == 0) | (t == 1)).sum() if form == "planes" else 3 * ((t >= 0) & (t < 3)).sum()
    assert got.sum() == valid and 0.75 * t.size * (3 if form == "labels" else 1) < valid < 0.85 * t.size * (3 if form == "labels" else 1)


@pytest.mark.parametrize("value", [30.0, -30.0, float("inf"), float("nan"), 0.0])
def test_a_map_of_one_value_lands_in_one_bin(value):
    """Everything in one of the four end bins 100, 1, 101, 0: the ballot route alone (0.0 sits exactly on the edge of 0.5 and takes the
    LDS route alone).  The table of N = 101 runs from -inf to +inf: -30 passes edge 0 only, 30 every edge but the last."""
    shape = (2, 2, 64, 64)
    z = np.full(shape, value, dtype=np.float32)
    t = R.plane_targets(shape, "onevalue/t", 0.2, np.uint8)
    got = check(z, t, 101)
    b = {30.0: 100, -30.0: 1, float("inf"): 101, 0.0: 51}.get(value, 0)       # (NaN: bin 0)
    assert got[..., b].sum() == got.sum() == ((t == 0) | (t == 1)).sum()


def test_uniform_noise_fills_every_bin():
    """sigmoid(z) uniform over (0, 1): every element takes the LDS route, every bin is hit."""
    shape = (2, 2, 64, 64)
    u = R.rng("noise/u").random(shape)
    z = np.log(u / (1 - u)).astype(np.float32)
    got = check(z, R.plane_targets(shape, "noise/t"), 101)
    assert got[..., 0].sum() == 0 and got[..., 101].sum() == 0 and bool((got[..., 1:101].sum((0, 1, 2)) > 0).all())


@pytest.mark.parametrize("n", [101, 1024])
def test_logits_exactly_on_edges(n):
    """Every logit IS an entry of the table (drawn by index, the +-inf ends included): ties are decided by >= on identical bits."""
    from lm_net_amd import hip
    shape = (2, 2, 32, 32)
    edges = hip.curve_edges(n, "logit")
    k = R.rng("onedges/%d" % n).integers(0, n, shape)
    z = edges[k]
    t = R.plane_targets(shape, "onedges/t")
    got = check(z, t, n)
    valid = (t == 0) | (t == 1)
    want = np.bincount(k[valid] + 1, minlength=n + 1)             # on edge k: b = k + 1 (the table is strictly increasing)
    assert bool(np.all(np.diff(edges) > 0)) and np.array_equal(got.sum((0, 1, 2)), want)


def test_thresholds_of_one_half_equal_the_sigmoid_stats_meter():
    from lm_net_amd import CurveMeter
    from lm_net_amd.metrics import SigmoidStatsMeter
    shape = (2, 3, 17, 23)
    z = torch.from_numpy(special_logits(shape, "meter/z")).to(DEV)
    t = torch.from_numpy(R.plane_targets(shape, "meter/t")).to(DEV)
    cm, sm = CurveMeter(3, "sigmoid", [0.5]), SigmoidStatsMeter(3, 0.5)
    for _ in range(2):
        cm.update(z, t)
        sm.update(z, t)
    tp, fp, fn, tn = cm.counts(per_image=True)
    assert tp.shape == (4, 3, 1)
    assert np.array_equal(np.stack([tp, fp, fn, tn], -1)[:, :, 0, :], sm.raw().cpu().numpy())
    assert tuple(cm.raw().shape) == (4, 3, 2, 2) and cm.raw().is_cuda


def test_probability_edges_on_torch_sigmoid():
    """The kernel sees the fp32 probabilities as torch computed them: exact against the same values on the host."""
    from lm_net_amd import CurveMeter
    shape = (2, 2, 17, 23)
    p = torch.sigmoid(torch.from_numpy(R.logits(shape, "prob/z")).to(DEV))
    t = R.plane_targets(shape, "prob/t", dtype=np.uint8)
    m = CurveMeter(2, "probability", 101)
    m.update(p, torch.from_numpy(t).to(DEV))
    assert np.array_equal(m.raw().cpu().numpy(), R.hist(p.cpu().numpy(), t, 101, "probability"))


# ---------------------------------------------------------------- SOFTMAX form
@pytest.mark.parametrize("C,N", [(2, 65), (2, 257), (3, 65), (3, 257), (9, 65), (9, 257), (64, 65)])
def test_softmax_form(C, N):
    """Shapes (2, C, 17, 23) against int64 labels and (1, C, 64, 64) against uint8 labels and against int64 planes.  Logits in
    [-8, 8], every pixel redrawn until none of its float64 probabilities lies within 1e-4 of an edge k / (N - 1), k >= 1."""
    for shape, dtype in (((2, C, 17, 23), np.int64), ((1, C, 64, 64), np.uint8)):
        key = "softmax/%d/%d/%d" % (C, N, shape[-1])
        z, rounds = R.softmax_case(shape, N, key)
        assert rounds < 30 and float(np.abs(z).max()) <= 8.0
        t = R.label_targets((shape[0],) + shape[2:], C, key + "/t", 0.2, dtype)
        got = check(z, t, N, "softmax", "labels")
        assert got.sum() == C * ((t >= 0) & (t < C)).sum() and got[..., 0].sum() == 0            # every score is >= 0: no bin 0
    check(z, R.plane_targets(shape, key + "/p"), N, "softmax", "planes")


# ---------------------------------------------------------------- reproducibility
def test_two_calls_and_both_deterministic_modes_are_bit_identical():
    from lm_net_amd import hip
    shape = (2, 4, 64, 64)
    z, _ = R.softmax_case(shape, 65, "repro/z")
    zt, lt = torch.from_numpy(z).to(DEV), torch.from_numpy(R.label_targets((2, 64, 64), 4, "repro/t")).to(DEV)
    pt = torch.from_numpy(R.plane_targets(shape, "repro/p", dtype=np.uint8)).to(DEV)
    runs = []
    assert not hip.get_deterministic()
    try:
        for det in (False, False, True, True):
            hip.set_deterministic(det)
            runs.append((device_hist(zt, lt, 65, "softmax", "labels"), device_hist(zt, pt, 101, "sigmoid", "planes")))
    finally:
        hip.set_deterministic(False)
    for a, b in runs[1:]:
        assert np.array_equal(a, runs[0][0]) and np.array_equal(b, runs[0][1])
    assert runs[0][0].sum() > 0 and runs[0][1].sum() > 0

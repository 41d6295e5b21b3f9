"""GPU: the counting entries and meters stay EXACT when one call sees more than 2^24 pixels.

A float cell holds every integer up to 2^24 = 16 777 216 and only every second one above it, so a confusion matrix counted into float
cells cannot return an odd count above 2^24.  The data here makes cell (0, 0) exactly that: 4097 x 4097 = 16 785 409 pixels (odd, above
2^24) in ONE image, nearly all of them label 0 / prediction 0, with a sprinkling of the other classes, of void and out-of-range labels
and of forced arg-max ties (first maximum wins); a second shape has 5 images of 2049 x 2049 (20 992 005 pixels: each image below 2^24,
the batch above it).  The references are np.bincount on the host; every comparison is equality.

  * lm_net_amd.ConfusionMeter is exact on both shapes and both prediction forms (it splits into calls below 2^24 pixels: along the
    batch first, then along the pixels of one image);
  * hip.confusion / hip.confusion_labels refuse such a call by name of the limit (never an inexact count without saying so) and are
    exact on the largest call they accept, 2^24 - 1 pixels;
  * ImageStatsMeter (ballots at C <= 8, LDS atomics above), SigmoidStatsMeter, CurveMeter (both target forms) and the integer counts of
    region_sums and lovasz_ranks count in integers and claim exactness: pinned here at the extent where it matters."""
import numpy as np
import pytest
import torch

import extent as X

pytestmark = pytest.mark.gpu

LIMIT = 1 << 24
SHAPES = {"1x4097x4097": (1, 4097, 4097), "5x2049x2049": (5, 2049, 2049)}
VOID = np.array([-1, 255, 0, 1000, -(1 << 40)], dtype=np.int64)      # (entry 2 becomes C: the first label past the classes)


def _case(B, H, W, C):
    """-> lab int64 [B*H*W] (host), pred int64 [B*H*W] (host: the arg-max the logits below must give), special pixel indices and their
    fp32 logit vectors [n, C].  Every other pixel has logits (1, 0, ..., 0)."""
    n = B * H * W
    lab = np.zeros(n, np.int64)
    s = np.arange(0, n, 20011)
    lab[s] = (s // 20011) % C                                       # the other classes
    v = np.arange(3, n, 40009)
    void = VOID.copy()
    void[2] = C
    lab[v] = void[(v // 40009) % 5]                                   # void and out-of-range labels
    pos, vec = [], []
    p = np.arange(5, n, 19997)                                        # a different sprinkling: class k wins clearly
    k = (p // 19997) % C
    a = np.zeros((p.size, C), np.float32)
    a[:, 0] = 1.0
    a[np.arange(p.size), k] = 2.0
    pos.append(p), vec.append(a)
    q = np.arange(7, n, 29989)                                       # forced ties: the first maximum wins
    k = 1 + (q // 29989) % (C - 1)
    a = np.zeros((q.size, C), np.float32)
    a[:, 0] = 1.0
    a[np.arange(q.size), k] = 1.0                                    # class k ties class 0 -> 0
    hi = (q // 29989) % 2 == 1
    a[hi, 0] = -5.0                                                  # every second one: class 0 falls away ...
    a[hi, C - 1] = 1.0                                               # ... and the last class ties class k -> min(k, C - 1)
    pos.append(q), vec.append(a)
    d = s[(np.arange(s.size) // C) % 2 == 0]                          # labelled pixels that are predicted right: the diagonal
    a = np.zeros((d.size, C), np.float32)
    a[:, 0] = 1.0
    a[np.arange(d.size), lab[d]] = 2.0
    pos.append(d), vec.append(a)
    r = np.arange(11, n, 300007)                                     # every class ties: class 0
    pos.append(r), vec.append(np.full((r.size, C), 0.25, np.float32))
    pred = np.zeros(n, np.int64)
    for i, a in zip(pos, vec):                                       # (in this order on the device too: a later set overrides)
        pred[i] = np.argmax(a, axis=1)                               # numpy: the first maximum
    _odd_cell00(lab, pred)
    return lab, pred, pos, vec


def _odd_cell00(lab, pred):
    """Cell (0, 0) must be odd: make one of its pixels void if it is not."""
    if int(((lab == 0) & (pred == 0)).sum()) % 2 == 0:
        j = lab.size - 1
        while lab[j] != 0 or pred[j] != 0:
            j -= 1
        lab[j] = 255


def _logits(B, H, W, C, pos, vec):
    lg = torch.zeros(B, C, H * W, device="cuda")
    lg[:, 0] = 1.0
    for i, a in zip(pos, vec):
        lg[torch.from_numpy(i // (H * W)).cuda(), :, torch.from_numpy(i % (H * W)).cuda()] = torch.from_numpy(a).cuda()
    return lg.view(B, C, H, W)


def _confusion_ref(lab, pred, C):
    ok = (lab >= 0) & (lab < C) & (pred >= 0) & (pred < C)
    return np.bincount(lab[ok] * C + pred[ok], minlength=C * C).reshape(C, C)


@pytest.fixture(autouse=True)
def _one_case_alive():
    """The memory rules of tests/extent.py: one case alive at a time, at most 24 GiB at its peak, a skip only below 64 GiB."""
    total = torch.cuda.get_device_properties("cuda").total_memory
    if total < X.MIN_DEVICE:
        pytest.skip("device memory %.0f GiB below 64 GiB: the extent cases need a large device (an MI355X must run them: 0 skips there)"
                    % (total / 2 ** 30))
    X.release()
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    X.release()
    assert peak <= X.PEAK_LIMIT, "peak device memory %.1f GiB above the 24 GiB of one case" % (peak / 2 ** 30)


def _refused(fn):
    with pytest.raises(RuntimeError) as e:
        fn()
    assert "2^24" in str(e.value) and "pixels" in str(e.value), str(e.value)


def _stats_ref(lab, pred, B, C):
    """tp, fp, fn, tn per image and class ([B, C, 4]) from the per-image confusion matrices; a void label counts nowhere."""
    out = np.zeros((B, C, 4), np.int64)
    for b, (l, p) in enumerate(zip(lab.reshape(B, -1), pred.reshape(B, -1))):
        m = _confusion_ref(l, p, C)
        tp = np.diag(m)
        out[b] = np.stack([tp, m.sum(0) - tp, m.sum(1) - tp, m.sum() - m.sum(0) - m.sum(1) + tp], 1)
    return out


# the one-image shape at every kernel form: registers (C = 2, 3, 4) and the LDS histogram (C = 5, 64); the batch shape, which
# splits along the batch instead of along the pixels, at one form of each kind
@pytest.mark.parametrize("shape,C", [("1x4097x4097", C) for C in (2, 3, 4, 5, 64)] + [("5x2049x2049", 2), ("5x2049x2049", 5)])
def test_confusion_logits_exact(shape, C):
    from lm_net_amd import hip
    from lm_net_amd.metrics import ConfusionMeter
    B, H, W = SHAPES[shape]
    lab, pred, pos, vec = _case(B, H, W, C)
    want = _confusion_ref(lab, pred, C)
    assert want[0, 0] > LIMIT and want[0, 0] % 2 == 1 and want.sum() == ((lab >= 0) & (lab < C)).sum()
    assert (np.diag(want) > 0).all() and (want > 0).sum() > C            # every class is hit, and off-diagonal cells too
    lg, y = _logits(B, H, W, C, pos, vec), torch.from_numpy(lab).cuda().view(B, H, W)
    m = ConfusionMeter(C)
    m.update(lg, y)
    m.update(lg[:1, :, :3, :5], y[:1, :3, :5])                           # a small batch after a split one: the same accumulator
    small = _confusion_ref(lab.reshape(B, H, W)[:1, :3, :5].ravel(), pred.reshape(B, H, W)[:1, :3, :5].ravel(), C)
    got = m.total.cpu().numpy()
    print("confusion %s C=%d: cell(0,0) want %d got %d" % (shape, C, want[0, 0] + small[0, 0], got[0, 0]))
    assert np.array_equal(got, (want + small).astype(np.float64)), got - want - small
    assert m.compute()["confusion"] == (want + small).tolist()
    # the entry itself refuses the whole extent by name of its limit, and is exact on the largest call it accepts
    _refused(lambda: hip.confusion(lg, y, torch.zeros(C, C, device="cuda")))
    if B == 1:
        n = LIMIT - 1
        counts = torch.zeros(C, C, device="cuda")
        hip.confusion(lg.view(1, C, H * W)[..., :n].contiguous(), y.view(1, H * W)[:, :n].contiguous(), counts)
        assert np.array_equal(counts.cpu().numpy(), _confusion_ref(lab[:n], pred[:n], C).astype(np.float32))


@pytest.mark.parametrize("shape,C", [("1x4097x4097", 2), ("1x4097x4097", 64), ("5x2049x2049", 3)])
def test_confusion_label_map_exact(shape, C):
    """The label-map route: uint8 predictions, among them 255 ("no class") and values past the classes, which are dropped."""
    from lm_net_amd import hip
    from lm_net_amd.metrics import ConfusionMeter
    B, H, W = SHAPES[shape]
    lab, pred, _, _ = _case(B, H, W, C)
    u = np.arange(13, lab.size, 25013)
    pred[u] = np.where((u // 25013) % 2 == 0, 255, C)                     # (C = 64: 64 is past the classes as well)
    _odd_cell00(lab, pred)
    want = _confusion_ref(lab, pred, C)
    assert want[0, 0] > LIMIT and want[0, 0] % 2 == 1
    p8, y = torch.from_numpy(pred.astype(np.uint8)).cuda().view(B, H, W), torch.from_numpy(lab).cuda().view(B, H, W)
    m = ConfusionMeter(C)
    m.update(p8, y)
    got = m.total.cpu().numpy()
    print("confusion_labels %s C=%d: cell(0,0) want %d got %d" % (shape, C, want[0, 0], got[0, 0]))
    assert np.array_equal(got, want.astype(np.float64)), got - want
    m.reset()
    m.update(p8.long(), y)                                               # an int64 label map takes the same route
    assert np.array_equal(m.total.cpu().numpy(), want.astype(np.float64))
    _refused(lambda: hip.confusion_labels(p8, y, torch.zeros(C, C, device="cuda")))
    n = LIMIT - 1
    counts = torch.zeros(C, C, device="cuda")
    hip.confusion_labels(p8.view(1, -1)[:, :n].contiguous(), y.view(1, -1)[:, :n].contiguous(), counts)
    assert np.array_equal(counts.cpu().numpy(), _confusion_ref(lab[:n], pred[:n], C).astype(np.float32))


@pytest.mark.parametrize("shape,C", [("1x4097x4097", 2), ("1x4097x4097", 9), ("5x2049x2049", 8)])
def test_image_stats_exact(shape, C):
    """Wave ballots (C <= 8) and LDS atomics (C > 8); logits and label map."""
    from lm_net_amd import ImageStatsMeter
    B, H, W = SHAPES[shape]
    lab, pred, pos, vec = _case(B, H, W, C)
    want = _stats_ref(lab, pred, B, C)
    assert want[..., 3].max() > LIMIT or B > 1
    lg, y = _logits(B, H, W, C, pos, vec), torch.from_numpy(lab).cuda().view(B, H, W)
    m = ImageStatsMeter(C, ignore_index=255)
    m.update(lg, y)
    m.update(torch.from_numpy(pred.astype(np.uint8)).cuda().view(B, H, W), y)
    got = m.raw().cpu().numpy()
    assert np.array_equal(got[:B], want), got[:B] - want
    assert np.array_equal(got[B:], want), got[B:] - want
    assert int(want[0].sum(-1)[0]) == int(((lab.reshape(B, -1)[0] >= 0) & (lab.reshape(B, -1)[0] < C)).sum())


def _planes(B, H, W):
    """One-logit sigmoid data: logits from {-3, 0, 3} (0 is the tie at threshold 0.5: predicted on), targets 0 / 1 / void."""
    n = B * H * W
    z = np.full(n, -3.0, np.float32)
    z[np.arange(1, n, 50003)] = 3.0
    z[np.arange(2, n, 120011)] = 0.0
    z[np.arange(4, n, 900001)] = np.nan
    t = np.zeros(n, np.uint8)
    t[np.arange(0, n, 25013)] = 1
    t[np.arange(6, n, 30011)] = 7
    return z, t


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_sigmoid_stats_exact(shape):
    from lm_net_amd import SigmoidStatsMeter
    B, H, W = SHAPES[shape]
    z, t = _planes(B, H, W)
    m = SigmoidStatsMeter(1)
    m.update(torch.from_numpy(z).cuda().view(B, 1, H, W), torch.from_numpy(t).cuda().view(B, H, W))
    on, ok = (z >= 0.0).reshape(B, -1), (t <= 1).reshape(B, -1)          # (NaN >= 0 is False: predicted off)
    pos = (t == 1).reshape(B, -1)
    want = np.stack([(ok & on & pos).sum(1), (ok & on & ~pos).sum(1), (ok & ~on & pos).sum(1), (ok & ~on & ~pos).sum(1)], 1)[:, None]
    assert want.sum() > LIMIT and want.max() > (LIMIT if B == 1 else 0)
    got = m.raw().cpu().numpy()
    assert np.array_equal(got, want), got - want


def _curve_ref(score, pos, ok, edges):
    """tp, fp, fn, tn at every threshold: an element is predicted on when score >= edge (fp32; NaN: off)."""
    with np.errstate(invalid="ignore"):
        on = [score >= e for e in edges.astype(np.float32)]
    return tuple(np.array([int((ok & f(o) & g(pos)).sum()) for o in on])
                 for f, g in ((lambda o: o, lambda p: p), (lambda o: o, lambda p: ~p), (lambda o: ~o, lambda p: p), (lambda o: ~o, lambda p: ~p)))


def test_curve_meter_planes_exact():
    from lm_net_amd import CurveMeter
    B, H, W = SHAPES["1x4097x4097"]
    z, t = _planes(B, H, W)
    m = CurveMeter(1, scores="sigmoid", thresholds=5)
    z[np.arange(8, z.size, 70001)] = m.edges[1]                           # scores exactly on an edge: predicted on at it
    m.update(torch.from_numpy(z).cuda().view(B, 1, H, W), torch.from_numpy(t).cuda().view(B, H, W))
    want = _curve_ref(z, t == 1, t <= 1, m.edges)
    got = m.counts()
    assert want[3].max() > LIMIT
    for g, w in zip(got, want):
        assert np.array_equal(g[0], w), (g, w)


def test_curve_meter_label_map_exact():
    """Probabilities of two classes against an integer label map, one-vs-rest; a label outside [0, C) is void."""
    from lm_net_amd import CurveMeter
    B, H, W = SHAPES["1x4097x4097"]
    n = B * H * W
    lab, _, _, _ = _case(B, H, W, 2)
    p1 = np.zeros(n, np.float32)
    p1[np.arange(1, n, 50303)] = 1.0
    p1[np.arange(2, n, 120101)] = 0.25
    p1[np.arange(9, n, 130103)] = 0.5
    probs = np.stack([1.0 - p1, p1])                                     # (exact in fp32: quarters)
    m = CurveMeter(2, scores="probability", thresholds=[0.0, 0.25, 0.5, 0.75, 1.0])
    m.update(torch.from_numpy(probs).cuda().view(1, 2, H, W), torch.from_numpy(lab).cuda().view(1, H, W))
    got = m.counts()
    ok = (lab >= 0) & (lab < 2)
    for c in range(2):
        want = _curve_ref(probs[c], lab == c, ok, m.edges)
        assert max(w.max() for w in want) > LIMIT
        for g, w in zip(got, want):
            assert np.array_equal(g[c], w), (c, g, w)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_region_and_lovasz_counts_exact(shape):
    """The int32 counts beside the fp32 sums: labelled and valid elements per scored class (region_sums), valid and valid foreground
    elements per segment (lovasz_ranks)."""
    from lm_net_amd.loss import lovasz_ranks, region_sums
    B, H, W = SHAPES[shape]
    C = 2
    lab, _, pos, vec = _case(B, H, W, C)
    lg, y = _logits(B, H, W, C, pos, vec), torch.from_numpy(lab).cuda().view(B, H, W)
    valid = int(((lab >= 0) & (lab < C)).sum())
    fg = [int((lab == c).sum()) for c in range(C)]
    assert valid > LIMIT and fg[0] > LIMIT
    _, counts = region_sums(lg, y, C)
    assert counts.cpu().numpy().reshape(C, 2).tolist() == [[fg[c], valid] for c in range(C)]
    del counts
    _, _, counts = lovasz_ranks(lg, y, C, classes="all")
    assert counts.cpu().numpy().reshape(C, 2).tolist() == [[valid, fg[c]] for c in range(C)]

"""TEST INFRASTRUCTURE ONLY -- numpy restatement of lm_net_amd.metrics.LesionMeter (the components of a predicted and a target label
volume, one record per lesion, and the join of the two labellings), written from its specification on top of volpost_ref.components
(which tests/test_volpost_cpu.py pins to scipy.ndimage.label) and np.unique over the stacked roots, and the volume generators of its
tests.  It produces the canonical records of LesionMeter.raw() and hands them to the same lm_net_amd.metrics.lesion_metrics;
tests/test_lesion_cpu.py checks both against an independent scipy.ndimage.label with explicit loops."""
import numpy as np

import volpost_ref as VR

EMPTY = -1


def clamp(L, C):
    """A label volume as the meter reads it: values outside [0, C) are 0."""
    L = np.asarray(L).astype(np.int64)
    return np.where((L >= 0) & (L < C), L, 0)


def records(Lp, Lt, C, connectivity=26, classes=None, max_components=None, pair_slots=None):
    """The canonical records of ONE case: (comp_keys int64 [M], comp_sizes int32 [M], pair_keys int64 [S], pair_counts int32 [S], ctrl
    int32 [4]), sorted by key, padded with EMPTY / 0 to max_components and pair_slots where given (M and S are the numbers of
    records otherwise)."""
    Lp, Lt = clamp(Lp, C), clamp(Lt, C)
    classes = list(range(1, C)) if classes is None else list(classes)
    keys, sizes, roots = [], [], []
    for side, L in enumerate((Lp, Lt)):
        r, s = VR.components(L, connectivity)
        roots.append(r)
        at = np.flatnonzero((s.ravel() > 0) & np.isin(L.ravel(), classes))
        keys.append((side << 40) | (L.ravel()[at] << 32) | at)
        sizes.append(s.ravel()[at])
    ck, cs = np.concatenate(keys).astype(np.int64), np.concatenate(sizes).astype(np.int32)
    order = np.argsort(ck)
    ck, cs = ck[order], cs[order]
    both = (Lp == Lt) & np.isin(Lp, classes)
    pk, pc = np.unique((roots[0][both].astype(np.int64) << 32) | roots[1][both], return_counts=True)
    ctrl = np.array([ck.size, pk.size, 0, 0], np.int32)
    M = ck.size if max_components is None else max_components
    S = pk.size if pair_slots is None else pair_slots
    assert ck.size <= M and pk.size <= S
    pad = lambda a, n, v, dt: np.concatenate([a.astype(dt), np.full(n - a.size, v, dt)])
    return pad(ck, M, EMPTY, np.int64), pad(cs, M, 0, np.int32), pad(pk, S, EMPTY, np.int64), pad(pc, S, 0, np.int32), ctrl


def stack(cases):
    """The records of several cases (of one M and S) stacked as LesionMeter.raw() stacks them."""
    return tuple(np.stack(t) for t in zip(*cases))


def metrics(cases, C, connectivity=26, classes=None, **kw):
    """lesion_metrics of the cases [(Lp, Lt), ...] through the restatement's records."""
    from lm_net_amd.metrics import lesion_metrics
    classes = list(range(1, C)) if classes is None else list(classes)
    recs = [records(Lp, Lt, C, connectivity, classes) for Lp, Lt in cases]
    M, S = max(max(r[0].size for r in recs), 1), max(max(r[2].size for r in recs), 1)
    recs = [records(Lp, Lt, C, connectivity, classes, M, S) for Lp, Lt in cases]
    return lesion_metrics(stack(recs), classes, **kw)


# ---------------------------------------------------------------- inputs
SHAPES = [(1, 8, 8), (2, 2, 2), (3, 5, 70), (12, 40, 70), (17, 66, 130)]


def _motif(Lp, Lt, z, y, x0, k, kind):
    """One row of lesions of class k, eight voxels wide (cut at the volume's edge), at (z, y, x0 ..):
      A   pred  k . k k k . k .     an identical pair (IoU 1), a pair of IoU 2/3, a false positive (x0 + 6)
          target k . k k . k . .    ... and a miss (x0 + 5)
      B   pred  k k k . k . k .     a prediction over two targets (IoU 1/3 each),
          target k . k . k k k .    a target under two predictions (IoU 1/3 each)"""
    W = Lp.shape[2]
    p, t = ((0, 2, 3, 4, 6), (0, 2, 3, 5)) if kind == "A" else ((0, 1, 2, 4, 6), (0, 2, 4, 5, 6))
    for L, xs in ((Lp, p), (Lt, t)):
        for dx in xs:
            if x0 + dx < W:
                L[z, y, x0 + dx] = k


def lesion_case(D, H, W, C, seed=0):
    """(Lp, Lt) uint8 [D, H, W] with values >= C on both sides.  Motif rows A and B of every class 1 .. C - 1 (_motif) in cells of
    9 columns on every second row -- of slice 0 in a volume of at least 12 x 36 x 70, of every second slice otherwise -- as many as
    fit: all of them except at (1, 8, 8) with C > 2 and at (2, 2, 2) (tests/test_lesion_cpu.py::test_generator_conditions).  The
    large volumes hold, from slice 2 on, one box per class and side that crosses the tile seam x = 64 (IoU 5/7) and a region of
    random blobs with out-of-range values, shared by both sides and redrawn in 3 % of the voxels of each."""
    big = D >= 12 and H >= 36 and W >= 70
    Lp, Lt = np.zeros((D, H, W), np.int64), np.zeros((D, H, W), np.int64)
    items = [(k, kind) for kind in "AB" for k in range(1, C)]
    cells = [(z, y, x0) for z in range(0, 1 if big else D, 2) for y in range(0, H, 2) for x0 in range(0, max(W - 7, 1), 9)]
    for (k, kind), (z, y, x0) in zip(items, cells):
        _motif(Lp, Lt, z, y, x0, k, kind)
    if big:
        rng = np.random.default_rng(D + 3 * H + 7 * W + 101 * C + 1009 * seed)
        for k in range(1, C):
            Lp[2:8, 4 * (k - 1):4 * (k - 1) + 3, 56:68] = k
            Lt[2:8, 4 * (k - 1):4 * (k - 1) + 3, 58:70] = k
        base = VR.blob_labels((D - 2, H, 40), C, seed)
        for L in (Lp, Lt):
            b = base.copy()
            redraw = rng.random(b.shape) < 0.03
            b[redraw] = rng.integers(-2, C + 2, int(redraw.sum()))
            L[2:, :, 12:52] = b
    u8 = lambda L: np.where((L < 0) | (L > 255), 255, L).astype(np.uint8)
    return u8(Lp), u8(Lt)


def grid_case():
    """(4, 32, 64): one voxel of class 1 at every even coordinate -- 1024 isolated voxels under any connectivity."""
    L = np.zeros((4, 32, 64), np.uint8)
    L[::2, ::2, ::2] = 1
    assert int(L.sum()) == 1024
    return L


def checkerboard_case():
    """(7, 33, 65): the parity checkerboard against a solid target.  Under connectivity 6 every voxel of the prediction is a lesion:
    7507 of them plus the target, and 7507 pairs."""
    Lp = VR.parity_checkerboard(7, 33, 65).astype(np.uint8)
    assert int(Lp.sum()) == 7507
    return Lp, np.ones_like(Lp)

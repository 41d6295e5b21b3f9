"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the per-case 3D metrics of lm_net_amd.metrics.VolumeSurfaceMeter (Dice, Jaccard,
HD, HD95, ASSD, RVD in the medpy.metric.binary conventions dc / jc / hd / hd95 / assd / ravd, with integer voxel pitches) and the
volume generators of its tests.  No scipy: tests/test_volume_cpu.py checks this file against the scipy recipe where scipy is
installed."""
import numpy as np

from surface_ref import percentile95

BIG = 1 << 40                                                    # "no border voxel": far above every squared distance (< 2^31)
RAW_I = ("n_pred", "n_target", "border_pred", "border_target", "max_d2_pt", "max_d2_tp", "d2_lo", "d2_hi", "n_both")


def border(m):
    """Voxels of m [D, H, W] with a 6-neighbour outside m; outside the volume counts as outside (binary_erosion with
    generate_binary_structure(3, 1), border_value=0)."""
    p = np.pad(m, 1)
    c = (slice(1, -1),) * 3
    inner = np.ones_like(m)
    for ax in range(3):
        for s in (slice(0, -2), slice(2, None)):
            idx = list(c)
            idx[ax] = s
            inner = inner & p[tuple(idx)]
    return m & ~inner


def _axis_min(G, ax, k):
    """out[i] = min_j G[j] + (k (i - j))^2 along axis ax (int64; the separable step of the exact squared distance transform)."""
    G = np.moveaxis(G, ax, 0)
    out = G.copy()
    for d in range(1, G.shape[0]):
        dd = (k * d) ** 2
        np.minimum(out[d:], G[:-d] + dd, out=out[d:])
        np.minimum(out[:-d], G[d:] + dd, out=out[:-d])
    return np.moveaxis(out, 0, ax)


def dist2_map(bd, spacing=(1, 1, 1)):
    """Squared distance (kz dz)^2 + (ky dy)^2 + (kx dx)^2 of EVERY voxel to the nearest True voxel of bd, exact int64 (>= BIG where bd
    is empty)."""
    g = np.where(bd, 0, BIG).astype(np.int64)
    for ax in range(3):
        g = _axis_min(g, ax, spacing[ax])
    return g


def _bbox(m):
    return tuple(slice(int(np.nonzero(m.any(tuple(a for a in range(3) if a != ax)))[0][0]),
                       int(np.nonzero(m.any(tuple(a for a in range(3) if a != ax)))[0][-1]) + 1) for ax in range(3))


def sq_dists(a, b, spacing=(1, 1, 1)):
    """D2(a -> b): one int64 per border voxel of a, in row-major (z, y, x) order.  The same separable minimum as dist2_map, formed only
    where a border voxel of a needs it: inside the bounding box of the two borders (every source and every query voxel lies in it, so
    the crop changes nothing), along y only in the slices and along x only in the rows that hold a query voxel."""
    ba, bb = border(a), border(b)
    box = _bbox(ba | bb)
    ba, bb = ba[box], bb[box]
    g = np.where(bb, 0, BIG).astype(np.int64)
    for z in range(1, g.shape[0]):                                   # steps along z to the nearest source of the column, two sweeps
        np.minimum(g[z], g[z - 1] + 1, out=g[z])
    for z in range(g.shape[0] - 2, -1, -1):
        np.minimum(g[z], g[z + 1] + 1, out=g[z])
    g = np.where(g < BIG, (spacing[0] * g) ** 2, BIG)
    zs = ba.any((1, 2))
    g, ba = _axis_min(g[zs], 1, spacing[1]), ba[zs]
    rows = ba.any(2)
    return _axis_min(g[rows], 1, spacing[2])[ba[rows]]


def pair_stats(P, T, spacing=(1, 1, 1)):
    """(raw integer statistics [9], raw float64 sums [2], metrics dict in steps of the unit) of one pair of boolean volumes; the six
    distance statistics are 0 and hd / hd95 / assd are nan when P or T is empty; dice / jaccard are nan when both are."""
    P, T = np.asarray(P, bool), np.asarray(T, bool)
    n_p, n_t, n_b = int(P.sum()), int(T.sum()), int((P & T).sum())
    si = np.zeros(9, np.int64)
    sf = np.zeros(2, np.float64)
    si[:4] = n_p, n_t, int(border(P).sum()), int(border(T).sum())
    si[8] = n_b
    out = {"hd": np.nan, "hd95": np.nan, "assd": np.nan, "rvd": (n_p - n_t) / n_t if n_t else 0.0,
           "dice": 2 * n_b / (n_p + n_t) if n_p + n_t else np.nan, "jaccard": n_b / (n_p + n_t - n_b) if n_p + n_t else np.nan}
    if n_p and n_t:
        pt, tp = sq_dists(P, T, spacing), sq_dists(T, P, spacing)
        pooled = np.sort(np.concatenate([pt, tp]))
        n = len(pooled)
        lo = 95 * (n - 1) // 100
        si[4:8] = pt.max(), tp.max(), pooled[lo], pooled[min(lo + 1, n - 1)]
        rpt, rtp = np.sqrt(pt.astype(np.float64)), np.sqrt(tp.astype(np.float64))
        sf[:] = rpt.sum(), rtp.sum()
        out["hd"] = float(np.sqrt(np.float64(max(pt.max(), tp.max()))))
        out["hd95"] = float(percentile95(np.sqrt(pooled.astype(np.float64))))
        out["assd"] = float((rpt.mean() + rtp.mean()) / 2)
    return si, sf, out


METRICS = ("hd", "hd95", "assd", "rvd", "dice", "jaccard")


def case_stats(pred, target, classes, spacing=(1, 1, 1)):
    """pred, target: integer label volumes [D, H, W] of ONE case.  Returns si [nk, 9], sf [nk, 2] and METRICS as [nk] float64
    arrays (nan where the pair is not scored)."""
    nk = len(classes)
    si, sf = np.zeros((nk, 9), np.int64), np.zeros((nk, 2), np.float64)
    met = {k: np.full(nk, np.nan) for k in METRICS}
    for j, k in enumerate(classes):
        si[j], sf[j], m = pair_stats(pred == k, target == k, spacing)
        for key in met:
            met[key][j] = m[key]
    return si, sf, met


def cases_stats(cases, classes, spacing=(1, 1, 1)):
    """case_stats of a list of (pred, target) cases, stacked: si [N, nk, 9], sf [N, nk, 2], METRICS as [N, nk]."""
    parts = [case_stats(p, t, classes, spacing) for p, t in cases]
    return (np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]),
            {k: np.stack([p[2][k] for p in parts]) for k in METRICS})


# ---------------------------------------------------------------- inputs
def _ellipsoid(shape, c, r):
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 <= 1.0


def ellipsoid_case(D, H, W, C, seed=0):
    """One ellipsoid "organ" per class painted in class order into the target; the prediction paints the same ellipsoids with the
    centre moved by N(0, 4 % of the side) and the semi-axes scaled by U(0.8, 1.2), then six 1 x 3 x 3 specks of random classes."""
    rng = np.random.default_rng(1000 * D + H + 7 * W + 13 * C + 100003 * seed)
    shape = np.array([D, H, W], np.float64)
    pred, target = np.zeros((D, H, W), np.int64), np.zeros((D, H, W), np.int64)
    for k in range(1, C):
        c = rng.uniform(0.2, 0.8, 3) * shape
        r = np.maximum(rng.uniform(0.08, 0.2, 3) * shape, 1.0)
        target[_ellipsoid((D, H, W), c, r)] = k
        pred[_ellipsoid((D, H, W), c + rng.normal(0, 0.04, 3) * shape, r * rng.uniform(0.8, 1.2, 3))] = k
    for _ in range(6):
        z0, y0, x0, k = int(rng.integers(0, D)), int(rng.integers(0, H - 2)), int(rng.integers(0, W - 2)), int(rng.integers(1, C))
        pred[z0, y0:y0 + 3, x0:x0 + 3] = k
    return pred, target


def tiling_case(D=8, H=12, W=68, shift=(1, 2, 1)):
    """Target: a 4 x 4 x 4 grid of class blocks (class = 16 i + 4 j + l); prediction: the same grid rolled by a voxel or two along
    every axis, so each of the 64 classes is present in both volumes and every pair is valid by construction."""
    z, y, x = np.ogrid[:D, :H, :W]
    target = ((z * 4 // D) * 16 + (y * 4 // H) * 4 + (x * 4 // W)).astype(np.int64)
    return np.roll(target, shift, (0, 1, 2)).copy(), target.copy()


def corner_voxels(D, H, W):
    """Prediction: the single voxel (0, 0, 0); target: the single voxel (D-1, H-1, W-1).  The nearest border voxel lies in another
    slice and another row, and d2 is the largest the volume allows."""
    pred, target = np.zeros((D, H, W), np.int64), np.zeros((D, H, W), np.int64)
    pred[0, 0, 0] = 1
    target[-1, -1, -1] = 1
    return pred, target


def valid_share(pred, target, classes):
    """(valid pairs, all pairs) of one case: a pair is valid when the class is present in both volumes."""
    return sum(int((pred == k).any() and (target == k).any()) for k in classes), len(classes)

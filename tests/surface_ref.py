"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the surface-distance metrics of lm_net_amd.metrics.SurfaceDistanceMeter
(HD, HD95, ASSD, RVD in the medpy.metric.binary conventions hd / hd95 / assd / ravd) and the mask generators of its tests.
No scipy: tests/test_surface_cpu.py checks this file against the scipy / medpy recipe where scipy is installed."""
import numpy as np

INF = 1 << 15
RAW_I = ("n_pred", "n_target", "border_pred", "border_target", "max_d2_pt", "max_d2_tp", "d2_lo", "d2_hi")


def border(m):
    """Pixels of m with a 4-neighbour outside m; outside the image counts as outside (binary_erosion, border_value=0)."""
    p = np.pad(m, 1)
    return m & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])


def col_dist(bd):
    """Vertical distance to the nearest border pixel of the column, INF where the column has none."""
    H, W = bd.shape
    g = np.full((H, W), INF, np.int64)
    last = np.full(W, -INF, np.int64)
    for y in range(H):
        last = np.where(bd[y], y, last)
        g[y] = np.minimum(g[y], y - last)
    last = np.full(W, 3 * INF, np.int64)
    for y in range(H - 1, -1, -1):
        last = np.where(bd[y], y, last)
        g[y] = np.minimum(g[y], last - y)
    return np.minimum(g, INF)


def sq_dists(a, b):
    """D2(a -> b): one int64 per border pixel of a, in row-major order of the pixels."""
    g2 = col_dist(border(b)) ** 2
    x = np.arange(a.shape[1])
    dx2 = (x[:, None] - x[None, :]) ** 2
    ys, xs = np.nonzero(border(a))
    out = np.empty(len(ys), np.int64)
    for s in range(0, len(ys), 4096):                            # (blocks: the [n, W] intermediate stays small on noise)
        out[s:s + 4096] = (dx2[xs[s:s + 4096]] + g2[ys[s:s + 4096]]).min(1)
    return out


def percentile95(v):
    """numpy's default (linear) 95th percentile of the sorted float64 values v, with the rank arithmetic in integers."""
    n = len(v)
    lo, rem = divmod(95 * (n - 1), 100)
    hi = min(lo + 1, n - 1)
    return v[lo] + (v[hi] - v[lo]) * rem / 100


def pair_stats(P, T):
    """(raw integer statistics [8], raw float64 sums [2], metrics dict) of one pair of boolean masks; the six distance
    statistics are 0 and hd / hd95 / assd are nan when P or T is empty."""
    P, T = np.asarray(P, bool), np.asarray(T, bool)
    n_p, n_t = int(P.sum()), int(T.sum())
    si = np.zeros(8, np.int64)
    sf = np.zeros(2, np.float64)
    si[:4] = n_p, n_t, int(border(P).sum()), int(border(T).sum())
    out = {"hd": np.nan, "hd95": np.nan, "assd": np.nan, "rvd": (n_p - n_t) / n_t if n_t else 0.0}
    if n_p and n_t:
        pt, tp = sq_dists(P, T), sq_dists(T, P)
        pooled = np.sort(np.concatenate([pt, tp]))
        n = len(pooled)
        lo = 95 * (n - 1) // 100
        si[4:] = pt.max(), tp.max(), pooled[lo], pooled[min(lo + 1, n - 1)]
        rpt, rtp = np.sqrt(pt.astype(np.float64)), np.sqrt(tp.astype(np.float64))
        sf[:] = rpt.sum(), rtp.sum()
        out["hd"] = float(np.sqrt(np.float64(max(pt.max(), tp.max()))))
        out["hd95"] = float(percentile95(np.sqrt(pooled.astype(np.float64))))
        out["assd"] = float((rpt.mean() + rtp.mean()) / 2)
    return si, sf, out


def batch_stats(pred, target, classes):
    """pred, target: integer label maps [B, H, W].  Returns si [B, nk, 8], sf [B, nk, 2] and {'hd', 'hd95', 'assd', 'rvd'} as
    [B, nk] float64 arrays (nan where the pair is not scored)."""
    B, nk = pred.shape[0], len(classes)
    si, sf = np.zeros((B, nk, 8), np.int64), np.zeros((B, nk, 2), np.float64)
    met = {k: np.full((B, nk), np.nan) for k in ("hd", "hd95", "assd", "rvd")}
    for b in range(B):
        for j, k in enumerate(classes):
            si[b, j], sf[b, j], m = pair_stats(pred[b] == k, target[b] == k)
            for key in met:
                met[key][b, j] = m[key]
    return si, sf, met


# ---------------------------------------------------------------- inputs
def _ellipse(H, W, cy, cx, ry, rx):
    y, x = np.mgrid[:H, :W]
    return ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0


def ellipse_case(B, H, W, C):
    """Per image one ellipse per class painted in class order into the target; the prediction paints the same ellipses with the
    centre moved by N(0, 4 px) and the semi-axes scaled by U(0.8, 1.2), then six 3x3 specks of random classes."""
    rng = np.random.default_rng(B * 1000 + H + C)
    pred, target = np.zeros((B, H, W), np.int64), np.zeros((B, H, W), np.int64)
    for b in range(B):
        for k in range(1, C):
            cy, cx = rng.uniform(0.15, 0.85) * H, rng.uniform(0.15, 0.85) * W
            ry, rx = rng.uniform(0.05, 0.18) * H, rng.uniform(0.05, 0.18) * W
            target[b][_ellipse(H, W, cy, cx, ry, rx)] = k
            dy, dx = rng.normal(0, 4, 2)
            sy, sx = rng.uniform(0.8, 1.2, 2)
            pred[b][_ellipse(H, W, cy + dy, cx + dx, ry * sy, rx * sx)] = k
        for _ in range(6):
            y0, x0, k = int(rng.integers(0, H - 2)), int(rng.integers(0, W - 2)), int(rng.integers(1, C))
            pred[b, y0:y0 + 3, x0:x0 + 3] = k
    return pred, target


def tiling_case(B=2, H=96, W=128, C=64, shift=(2, 3)):
    """Target: an 8 x 8 grid of class rectangles (class = 8 * row + column); prediction: the same grid shifted by a few pixels, so
    every class is present in both maps and every pair is valid by construction."""
    assert C == 64
    y, x = np.mgrid[:H, :W]
    target = (y * 8 // H) * 8 + (x * 8 // W)
    pred = np.empty((B, H, W), np.int64)
    for b in range(B):
        dy, dx = shift[0] + b, shift[1] + 2 * b
        pred[b] = np.roll(np.roll(target, dy, 0), dx, 1)
    return pred, np.broadcast_to(target, (B, H, W)).astype(np.int64).copy()


def valid_share(pred, target, classes):
    """(valid pairs, all pairs): a pair is valid when the class is present in both maps of the sample."""
    v = sum(int((pred[b] == k).any() and (target[b] == k).any()) for b in range(pred.shape[0]) for k in classes)
    return v, pred.shape[0] * len(classes)

"""TEST INFRASTRUCTURE ONLY -- numpy restatement of lm_net_amd.post.DevicePostprocess (arg-max, connected components, cleaning, hole
filling, statistics, nearest resize back, overlay), written from its specification, and the input generators of its tests.
No scipy: tests/test_post_cpu.py checks this file against scipy.ndimage where scipy is installed."""
import numpy as np

INT32_MAX = 2 ** 31 - 1


# ---------------------------------------------------------------- step 1: components
def components(L, connectivity):
    """(roots, areas) of one label map L [H, W]: roots[y, x] = the smallest row-major index of the pixel's component (pixels joined
    by 4- or 8-neighbour steps through equal labels), areas = the component's pixel count at its root pixel, 0 elsewhere.

    Union-find over the whole edge list at once: parent[i] <= i always; a round hooks, for every edge whose ends have different
    roots, the larger root under the smaller (np.minimum.at), then shortens every chain to its root by pointer jumping.  When no edge
    joins different roots the root is constant on a component, and it is the component's smallest index because parent[i] <= i.
    Every round removes each root that has a smaller neighbouring root, so the number of roots of a component at least halves:
    O(log n) rounds also on the serpentine."""
    assert connectivity in (4, 8)
    H, W = L.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    pairs = [(idx[:, 1:], idx[:, :-1], L[:, 1:] == L[:, :-1]), (idx[1:], idx[:-1], L[1:] == L[:-1])]
    if connectivity == 8:
        pairs += [(idx[1:, 1:], idx[:-1, :-1], L[1:, 1:] == L[:-1, :-1]), (idx[1:, :-1], idx[:-1, 1:], L[1:, :-1] == L[:-1, 1:])]
    u = np.concatenate([a[m] for a, _, m in pairs])
    v = np.concatenate([b[m] for _, b, m in pairs])
    parent = np.arange(H * W, dtype=np.int64)
    while u.size:
        ru, rv = parent[u], parent[v]
        live = ru != rv
        if not live.any():
            break
        u, v, ru, rv = u[live], v[live], ru[live], rv[live]
        np.minimum.at(parent, np.maximum(ru, rv), np.minimum(ru, rv))
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    areas = np.bincount(parent, minlength=H * W)
    return parent.reshape(H, W), areas.reshape(H, W)


def rank_labels(roots, mask=None):
    """Components numbered 1.. in raster order of their first pixel (scipy.ndimage.label's numbering), 0 outside mask."""
    r = roots if mask is None else np.where(mask, roots, -1)
    uniq, inv = np.unique(r, return_inverse=True)
    inv = inv.reshape(r.shape)
    return inv if mask is not None and uniq[0] == -1 else inv + 1


# ---------------------------------------------------------------- steps 0-4 for one sample
def label_map(pred, C):
    """L0 [B, H, W] uint8 of logits [B, C, H, W] (np.argmax: the first maximum) or of an integer label map (outside [0, C) -> 0)."""
    pred = np.asarray(pred)
    if pred.ndim == 4:
        return pred.argmax(1).astype(np.uint8)
    p = pred.astype(np.int64)
    return np.where((p >= 0) & (p < C), p, 0).astype(np.uint8)


def clean_one(L0, C, connectivity=8, classes=None, keep_largest=False, min_area=0, fill_holes=False):
    """(L1, L2, stats [C, 4], removed components, holes filled) of one label map L0 [H, W]."""
    H, W = L0.shape
    classes = list(range(1, C)) if classes is None else list(classes)
    largest = (list(classes) if keep_largest else []) if isinstance(keep_largest, (bool, np.bool_)) else list(keep_largest)
    areas_min = {k: int(min_area) for k in classes} if np.isscalar(min_area) else dict(zip(classes, min_area))
    limit = (INT32_MAX if fill_holes else 0) if isinstance(fill_holes, (bool, np.bool_)) else int(fill_holes)
    roots, areas = components(L0, connectivity)
    fr, fa, fl = roots.ravel(), areas.ravel(), L0.ravel()
    root_px = np.flatnonzero(fr == np.arange(H * W))
    stats = np.zeros((C, 4), np.int64)
    survive = np.ones(H * W, bool)                                    # indexed by root
    for k in range(C):
        rk = root_px[fl[root_px] == k]                                # ascending: the first of equal areas is the smallest root
        stats[k, 0] = rk.size
        ok = np.ones(rk.size, bool)
        if k in classes:
            ok &= fa[rk] >= areas_min[k]
            if k in largest and rk.size:
                top = np.zeros(rk.size, bool)
                top[np.argmax(fa[rk])] = True                         # np.argmax: the first maximum
                ok &= top
        survive[rk] = ok
        stats[k, 1] = ok.sum()
    L1 = np.where(survive[fr], fl, 0).reshape(H, W).astype(np.uint8)
    L2, holes = L1.copy(), 0
    if limit > 0:
        hr, ha = components(L1, 4 if connectivity == 8 else 8)
        hr, ha = hr.ravel(), ha.ravel()
        touches = np.zeros(H * W, bool)
        frame = np.zeros((H, W), bool)
        frame[[0, -1], :] = True
        frame[:, [0, -1]] = True
        touches[hr[frame.ravel()]] = True
        zero = L1.ravel() == 0
        hole_px = zero & ~touches[hr] & (ha[hr] <= limit)
        flat = L2.ravel()
        flat[hole_px] = L1.ravel()[hr[hole_px] - 1]                  # the pixel left of the root pixel
        holes = int((hole_px & (hr == np.arange(H * W))).sum())
    stats[:, 2] = np.bincount(L2.ravel(), minlength=C)[:C]
    stats[0, 3] = holes
    removed = int((stats[:, 0] - stats[:, 1]).sum())
    return L1, L2, stats, removed, holes


def clean(pred, C, **kw):
    """(labels_net [B, H, W] uint8, stats [B, C, 4] int32, components removed, holes filled) of a batch."""
    L0 = label_map(pred, C)
    out = [clean_one(l, C, **kw) for l in L0]
    return (np.stack([o[1] for o in out]), np.stack([o[2] for o in out]).astype(np.int32), sum(o[3] for o in out),
            sum(o[4] for o in out))


def batch_components(pred, C, connectivity):
    L0 = label_map(pred, C)
    out = [components(l, connectivity) for l in L0]
    return np.stack([o[0] for o in out]).astype(np.int32), np.stack([o[1] for o in out]).astype(np.int32)


# ---------------------------------------------------------------- steps 5 and 6
def resize_back(L2, src_hw, Hs, Ws):
    """labels [B, Hs, Ws] uint8: nearest, floor(dst * (net / valid)) in double, 0 outside each sample's valid area."""
    B, H, W = L2.shape
    out = np.zeros((B, Hs, Ws), np.uint8)
    for b in range(B):
        hs, ws = int(src_hw[b][0]), int(src_hw[b][1])
        sy = np.minimum(np.floor(np.arange(hs) * (float(H) / hs)).astype(np.int64), H - 1)
        sx = np.minimum(np.floor(np.arange(ws) * (float(W) / ws)).astype(np.int64), W - 1)
        out[b, :hs, :ws] = L2[b][sy][:, sx]
    return out


def alpha256(alpha):
    return int(np.floor(float(alpha) * 256.0 + 0.5))


def default_palette(C):
    pal = np.zeros((C, 3), np.uint8)
    for k in range(C):
        for j in range(8):
            for c in range(3):
                pal[k, c] |= ((k >> (3 * j + c)) & 1) << (7 - j)
    for k, colour in ((1, (0, 0, 255)), (2, (0, 255, 0)), (3, (255, 0, 0))):
        if k < C:
            pal[k] = colour
    return pal


def overlay(labels, frames, src_hw, palette, alpha=1.0, mode="fill"):
    """[B, Hs, Ws, 3] uint8 of frame-resolution labels [B, Hs, Ws] over frames [B, Hs, Ws, 3] or [B, Hs, Ws] (replicated)."""
    B, Hs, Ws = labels.shape
    fr = frames if frames.ndim == 4 else frames[..., None]
    fr = np.broadcast_to(fr, (B, Hs, Ws, 3)).astype(np.int64)
    a = alpha256(alpha)
    out = np.zeros((B, Hs, Ws, 3), np.uint8)
    pal = np.asarray(palette, np.int64)
    for b in range(B):
        hs, ws = int(src_hw[b][0]), int(src_hw[b][1])
        l = labels[b, :hs, :ws].astype(np.int64)
        paint = l > 0
        if mode == "contour":
            p = np.pad(l, 1, constant_values=-1)                      # outside the valid area: a different label
            c = p[1:-1, 1:-1]
            paint &= (p[:-2, 1:-1] != c) | (p[2:, 1:-1] != c) | (p[1:-1, :-2] != c) | (p[1:-1, 2:] != c)
        px = fr[b, :hs, :ws]
        mixed = ((256 - a) * px + a * pal[l] + 128) >> 8
        out[b, :hs, :ws] = np.where(paint[..., None], mixed, px).astype(np.uint8)
    return out


# ---------------------------------------------------------------- inputs
def punched_ellipses(B, H, W, C):
    """surface_ref.ellipse_case's prediction with 1 % of its foreground pixels set to 0 (holes)."""
    import surface_ref
    pred, _ = surface_ref.ellipse_case(B, H, W, C)
    pred[(np.random.default_rng(7000 + 1000 * B + H + C).random(pred.shape) < 0.01) & (pred > 0)] = 0
    return pred


def noise_case(B=2, H=352, W=352, seed=11):
    return (np.random.default_rng(seed).random((B, H, W)) < 0.5).astype(np.int64)


def serpentine(H=1024, W=1000):
    """One one-pixel-wide corridor of class 1 through the whole image: even rows full, odd rows one pixel at alternating ends."""
    m = np.zeros((H, W), np.int64)
    m[0::2] = 1
    m[1::4, -1] = 1
    m[3::4, 0] = 1
    return m[None]


def checkerboard(H=1024, W=1024):
    y, x = np.mgrid[:H, :W]
    return ((y + x) & 1).astype(np.int64)[None]

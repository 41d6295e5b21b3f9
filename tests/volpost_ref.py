"""TEST INFRASTRUCTURE ONLY -- numpy restatement of lm_net_amd.post.VolumePostprocess (3D connected components under connectivity 6,
18 or 26, the n largest components of a class, a minimal volume, cavity filling under the dual connectivity, statistics), written from
its specification, and the volume generators of its tests.  No scipy: tests/test_volpost_cpu.py checks this file against
scipy.ndimage where scipy is installed."""
import numpy as np

INT32_MAX = 2 ** 31 - 1
ORDER = {6: 1, 18: 2, 26: 3}                                        # generate_binary_structure(3, ORDER[connectivity])
DUAL = {6: 26, 18: 6, 26: 6}


# ---------------------------------------------------------------- step 1: components
def _pair(d, n):
    """(slice of the voxels, slice of their neighbours at +d) along an axis of length n."""
    return slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d))


def components(L, connectivity):
    """(roots, sizes) of one label volume L [D, H, W]: roots = the smallest linear index (z * H + y) * W + x of the voxel's component
    (voxels joined by 6-, 18- or 26-neighbour steps through equal labels), sizes = the component's voxel count at its root voxel, 0
    elsewhere.

    Union-find over ROW RUNS: a run is a maximal stretch of equal labels along x, numbered in raster order, so the smaller run id
    starts at the smaller voxel index.  The edges are the pairs of runs that hold two neighbouring voxels of equal label in different
    rows (the 13 - 1 offsets of the half neighbourhood with dz < 0, or dz == 0 and dy < 0, that the connectivity allows), made unique.
    A round hooks, for every edge whose ends have different roots, the larger root under the smaller (np.minimum.at), then shortens
    every chain by pointer jumping; parent[i] <= i always, so when no edge joins different roots the root of a component is its
    smallest run, whose first voxel is the component's smallest index."""
    order = ORDER[connectivity]
    L = np.asarray(L)
    D, H, W = L.shape
    start = np.ones((D, H, W), bool)
    start[:, :, 1:] = L[:, :, 1:] != L[:, :, :-1]
    run = (np.cumsum(start.ravel()) - 1).reshape(D, H, W)
    first = np.flatnonzero(start.ravel())                             # the first voxel of every run
    us, vs = [], []
    for dz in (-1, 0):
        for dy in (-1, 0, 1):
            if (dz, dy) == (0, 0) or (dz == 0 and dy > 0):
                continue
            for dx in (-1, 0, 1):
                if abs(dz) + abs(dy) + abs(dx) > order:
                    continue
                (az, bz), (ay, by), (ax, bx) = _pair(dz, D), _pair(dy, H), _pair(dx, W)
                m = L[az, ay, ax] == L[bz, by, bx]
                us.append(run[az, ay, ax][m])
                vs.append(run[bz, by, bx][m])
    n = first.size
    parent = np.arange(n, dtype=np.int64)
    if us:
        e = np.unique(np.concatenate(us) * n + np.concatenate(vs))
        u, v = e // n, e % n
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
    roots = first[parent][run]
    sizes = np.bincount(roots.ravel(), minlength=D * H * W).reshape(D, H, W)
    return roots, sizes


def rank_labels(roots, mask):
    """Components of mask numbered 1.. in raster order of their first voxel (scipy.ndimage.label's numbering), 0 outside mask."""
    r = np.where(mask, roots, -1)
    uniq, inv = np.unique(r, return_inverse=True)
    inv = inv.reshape(r.shape)
    return inv if uniq[0] == -1 else inv + 1


def faces(shape):
    """The voxels on any of the six faces of the volume (all of them in a one-slice volume)."""
    f = np.zeros(shape, bool)
    f[[0, -1]] = True
    f[:, [0, -1]] = True
    f[:, :, [0, -1]] = True
    return f


# ---------------------------------------------------------------- steps 0-4 for one case
def label_volume(pred, C):
    """L0 [D, H, W] uint8 of logits [D, C, H, W] (np.argmax: the first maximum) or of an integer label volume (outside [0, C) -> 0)."""
    pred = np.asarray(pred)
    if pred.ndim == 4:
        return pred.argmax(1).astype(np.uint8)
    p = pred.astype(np.int64)
    return np.where((p >= 0) & (p < C), p, 0).astype(np.uint8)


def keep_table(classes, keep_largest):
    """{class: n} of the keep_largest argument (False, True, an int, a dict); 0 / absent = every component."""
    if isinstance(keep_largest, (bool, np.bool_)):
        return {k: 1 for k in classes} if keep_largest else {}
    if isinstance(keep_largest, dict):
        return {int(k): int(n) for k, n in keep_largest.items()}
    return {k: int(keep_largest) for k in classes}


def clean(pred, C, connectivity=26, classes=None, keep_largest=False, min_volume=0, fill_holes=False):
    """(L2 [D, H, W] uint8, stats [C, 4] int32, info) of one case; info: L0, L1, per class the component sizes in L0 (by ascending
    root) and which survive, and the sizes of the zero components of L1 under the dual connectivity with their face flags."""
    L0 = label_volume(pred, C)
    D, H, W = L0.shape
    V = D * H * W
    classes = list(range(1, C)) if classes is None else list(classes)
    keep = keep_table(classes, keep_largest)
    minv = {k: int(min_volume) for k in classes} if np.isscalar(min_volume) else dict(zip(classes, (int(v) for v in min_volume)))
    limit = (INT32_MAX if fill_holes else 0) if isinstance(fill_holes, (bool, np.bool_)) else int(fill_holes)
    roots, sizes = components(L0, connectivity)
    fr, fs, fl = roots.ravel(), sizes.ravel(), L0.ravel()
    root_vx = np.flatnonzero(fr == np.arange(V))
    stats = np.zeros((C, 4), np.int64)
    survive = np.ones(V, bool)                                        # indexed by root
    info = {"L0": L0, "sizes": {}, "survive": {}}
    for k in range(C):
        rk = root_vx[fl[root_vx] == k]                                # ascending roots
        stats[k, 0] = rk.size
        ok = np.ones(rk.size, bool)
        if k in classes:
            if keep.get(k, 0) > 0:
                top = np.lexsort((rk, -fs[rk]))[:keep[k]]             # largest first; equal sizes: the smaller root
                ok[:] = False
                ok[top] = True
            ok &= fs[rk] >= minv[k]
        survive[rk] = ok
        stats[k, 1] = ok.sum()
        info["sizes"][k], info["survive"][k] = fs[rk], ok
    L1 = np.where(survive[fr], fl, 0).reshape(D, H, W).astype(np.uint8)
    L2, holes = L1.copy(), 0
    zero = L1.ravel() == 0
    hr, hs = components((L1 != 0).astype(np.uint8), DUAL[connectivity])
    hr, hs = hr.ravel(), hs.ravel()
    touches = np.zeros(V, bool)
    touches[hr[faces((D, H, W)).ravel()]] = True
    zr = np.flatnonzero(zero & (hr == np.arange(V)))                  # the roots of the zero components
    info.update(L1=L1, hole_sizes=hs[zr], hole_open=touches[zr])
    if limit > 0:
        hole_vx = zero & ~touches[hr] & (hs[hr] <= limit)
        flat = L2.ravel()
        flat[hole_vx] = L1.ravel()[hr[hole_vx] - 1]                  # the voxel at x - 1 of the root voxel
        holes = int((hole_vx & (hr == np.arange(V))).sum())
    stats[:, 2] = np.bincount(L2.ravel(), minlength=C)[:C]
    stats[0, 3] = holes
    return L2, stats.astype(np.int32), info


def clean_slices(pred, C, connectivity=8, **kw):
    """DevicePostprocess on the slices of the same volume, restated with this file: every slice is a one-slice case (an in-plane
    connectivity of 4 is 6 in a one-slice volume, 8 is 18 or 26)."""
    L0 = label_volume(pred, C)
    out = [clean(l[None], C, 6 if connectivity == 4 else 26, **kw) for l in L0]
    return np.concatenate([o[0] for o in out]), np.stack([o[1] for o in out])


# ---------------------------------------------------------------- inputs
SHAPES = [(2, 2, 2), (1, 8, 8), (3, 5, 70), (17, 66, 130), (65, 9, 7)]


def blob_labels(shape, C, seed=0):
    """A label volume with out-of-range values: smooth-ish random blobs (a coarse random grid repeated 2 x 3 x 3) with 10 % of the
    voxels redrawn from [-2, C + 2), so that components of every size occur and every class is present in the larger shapes."""
    rng = np.random.default_rng(sum(shape) + 31 * C + 1009 * seed)
    D, H, W = shape
    coarse = rng.integers(0, C, ((D + 1) // 2, (H + 2) // 3, (W + 2) // 3))
    lab = np.repeat(np.repeat(np.repeat(coarse, 2, 0), 3, 1), 3, 2)[:D, :H, :W].astype(np.int64)
    redraw = rng.random(shape) < 0.1
    lab[redraw] = rng.integers(-2, C + 2, int(redraw.sum()))
    return lab


def tie_logits(shape, C, seed=0):
    """fp32 logits [D, C, H, W] with three values only: ties in most voxels (the first maximum wins)."""
    rng = np.random.default_rng(7 * sum(shape) + C + 1009 * seed)
    D, H, W = shape
    coarse = rng.integers(0, 3, ((D + 1) // 2, C, (H + 1) // 2, (W + 2) // 3))
    lg = np.repeat(np.repeat(np.repeat(coarse, 2, 0), 2, 2), 3, 3)[:D, :, :H, :W]
    return np.ascontiguousarray(lg).astype(np.float32)


ORGAN_SHAPES = [(12, 40, 70), (17, 66, 130)]
ORGAN_MIN_VOLUME = 3          # removes the debris of 1 and 2 voxels, keeps the debris of 5 and the organ
ORGAN_HOLE_LIMIT = 4          # fills the cavity of 1 voxel, leaves the cavity of 12


def organ_case(D, H, W, C):
    """One box "organ" per class k = 1 .. C - 1 in cell k - 1 of a 2 x 4 grid of cells over (y, x), each with
      * a closed cavity of 1 voxel and a closed cavity of 2 x 2 x 3 = 12 voxels;
      * a pit of 3 voxels open to the face z = 0 (a cavity that is NOT filled);
      * debris of 1, 2 and 5 voxels two slices above the organ, at least two voxels from everything else (separate under 26).
    Needs D >= 12, H >= 28, W >= 56 and C <= 9."""
    assert D >= 12 and H // 2 >= 14 and W // 4 >= 14 and 2 <= C <= 9
    L = np.zeros((D, H, W), np.int64)
    for k in range(1, C):
        y0, x0 = ((k - 1) // 4) * (H // 2), ((k - 1) % 4) * (W // 4)
        L[0:9, y0 + 1:y0 + 13, x0 + 1:x0 + 13] = k
        L[3, y0 + 3, x0 + 3] = 0                                      # closed, 1 voxel
        L[4:7, y0 + 6:y0 + 8, x0 + 6:x0 + 8] = 0                      # closed, 12 voxels
        L[0:3, y0 + 10, x0 + 3] = 0                                   # open to z = 0
        L[10, y0 + 1, x0 + 1] = k
        L[10, y0 + 1, x0 + 4:x0 + 6] = k
        L[10, y0 + 5, x0 + 1:x0 + 6] = k
    return L


def parity_checkerboard(D=9, H=33, W=65):
    z, y, x = np.ogrid[:D, :H, :W]
    return ((z + y + x) % 2).astype(np.int64)


def touching_pairs():
    """(4, 6, 12): two voxels of class 1 touching at a corner only, two of class 2 touching at an edge only."""
    L = np.zeros((4, 6, 12), np.int64)
    L[1, 1, 1] = L[2, 2, 2] = 1
    L[1, 3, 7] = L[2, 4, 7] = 2
    return L


def serpentine(D=9, H=33, W=65):
    """One one-voxel-wide corridor of class 1 through the whole volume: every even slice holds the 2D serpentine (even rows full, odd
    rows one voxel at alternating ends, from (0, 0) to (H - 1, W - 1)), every odd slice the one voxel that joins two of them."""
    assert H % 4 == 1 and D % 2 == 1
    s = np.zeros((H, W), np.int64)
    s[0::2] = 1
    s[1::4, -1] = 1
    s[3::4, 0] = 1
    L = np.zeros((D, H, W), np.int64)
    L[0::2] = s
    L[1::4, -1, -1] = 1
    L[3::4, 0, 0] = 1
    return L


def noise_case(D=12, H=40, W=70, seed=11):
    return (np.random.default_rng(seed).random((D, H, W)) < 0.5).astype(np.int64)


def shell(opening=None):
    """(7, 9, 11): a 5 x 5 x 5 shell of class 1 around a 3 x 3 x 3 cavity, pushed against the face z = 0.  opening: None (closed);
    "face": the wall voxel between the cavity and z = 0 removed; "diagonal": a corner voxel of the wall at z = 0 removed, which joins
    the cavity's corner voxel to the outside by a corner step only."""
    L = np.zeros((7, 9, 11), np.int64)
    L[0:5, 2:7, 3:8] = 1
    L[1:4, 3:6, 4:7] = 0
    if opening == "face":
        L[0, 4, 5] = 0
    elif opening == "diagonal":
        L[0, 2, 3] = 0
    else:
        assert opening is None
    return L


def kidneys():
    """(10, 24, 40): two ellipsoid "kidneys" of class 1 of different sizes plus debris of 1, 3 and 4 voxels."""
    z, y, x = np.ogrid[:10, :24, :40]
    L = np.zeros((10, 24, 40), np.int64)
    L[((z - 5) / 4.0) ** 2 + ((y - 12) / 7.0) ** 2 + ((x - 9) / 6.0) ** 2 <= 1] = 1
    L[((z - 4) / 3.0) ** 2 + ((y - 11) / 6.0) ** 2 + ((x - 29) / 5.0) ** 2 <= 1] = 1
    L[0, 0, 0] = 1
    L[9, 22, 17:20] = 1
    L[1, 1:3, 18:20] = 1
    return L


def size_ties():
    """(3, 6, 20): four components of class 1 of 4 voxels each (a row, a column, a 2 x 2 square, a stick along z plus one), and one
    of 2 voxels."""
    L = np.zeros((3, 6, 20), np.int64)
    L[1, 4, 14:18] = 1
    L[0, 0:4, 10] = 1
    L[2, 0:2, 2:4] = 1
    L[0:3, 5, 0] = 1
    L[0, 4, 0] = 1
    L[0, 0, 18:20] = 1
    return L


def tilted_rod(D=8, H=16, W=40):
    """A rod of class 1, three voxels long per slice, that moves two voxels along x per slice: its slices overlap by one voxel, so it
    is one 3D component -- beside a solid block of class 1 that is larger than the rod's piece in every slice."""
    L = np.zeros((D, H, W), np.int64)
    for z in range(D):
        L[z, 3, 2 + 2 * z:5 + 2 * z] = 1
    L[:, 9:13, 30:36] = 1
    return L


def bench_case(D=128, H=352, W=352, C=9):
    """The prediction of volume_ref.ellipsoid_case (ellipsoid organs plus 1 x 3 x 3 specks) with more debris -- 40 specks of 1 to 8
    voxels of random classes -- and cavities: 0.1 % of the organ voxels set to 0, and one 3 x 3 x 3 cavity near each organ's centre of
    mass."""
    import volume_ref
    pred, _ = volume_ref.ellipsoid_case(D, H, W, C)
    rng = np.random.default_rng(4242 + D + H + W + C)
    organs = pred > 0
    for k in range(1, C):
        vz, vy, vx = np.nonzero(pred == k)
        if vz.size:
            z, y, x = (int(np.clip(v.mean(), 2, n - 3)) for v, n in ((vz, D), (vy, H), (vx, W)))
            pred[z - 1:z + 2, y - 1:y + 2, x - 1:x + 2] = 0
    pred[organs & (rng.random(pred.shape) < 0.001)] = 0
    for _ in range(40):
        z, y, x, k, n = int(rng.integers(0, D)), int(rng.integers(0, H)), int(rng.integers(0, W - 8)), int(rng.integers(1, C)), int(rng.integers(1, 9))
        pred[z, y, x:x + n] = k
    return pred

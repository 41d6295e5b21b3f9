"""numpy restatement of include/slices/lmnet_slices.h (lm_net_amd.data.VolumeSlicer): the record by sorting and Python integers, the
normalisation table in float64, the gather with the coordinate arithmetic in float32 (every product and sum rounded once, as the
device's __fmul_rn / __fadd_rn: the same floor at every pixel) or in float64, the interpolation in float64 either way.

THE DEVICE BOUND tol().  The device reads four taps |v| <= Vmax exactly and runs, in fp32,
    top = fma(fx, v01 - v00, v00)    bot = fma(fx, v11 - v10, v10)    v = fma(fy, bot - top, top)
    u = (min(max(v, lo), hi) - a) * b            o = fma(u, gain, bias)
with e = 2^-24 the unit roundoff.  The tap differences are exact (integers below 2^17).  top and bot carry one rounding each of a
value <= Vmax, and enter v with weights 1 - fy and fy: Vmax e together.  bot - top rounds a value <= 2 Vmax, scaled by fy <= 1:
2 Vmax e.  The last fma rounds a value <= Vmax: Vmax e.  That is three lerps of at most two roundings each, 4 Vmax e in raw units; the
clamp passes an error on or cuts it.  v - a rounds a value <= 2 Vmax (Vmax bounds |a|, |lo| and |hi| too): 2 Vmax e.  Times |b| and
|gain|: 6 Vmax |b| |gain| e.  The product with b rounds u, |u| <= 2 Vmax |b|: after the gain 2 Vmax |b| |gain| e.  The last fma
rounds o: |o| e.  In all (8 Vmax |b| |gain| + |o|) e; the bound of the family is stated with 4 |o| for an implementation that does
not fuse its last two multiply-adds:

    tol = (8 Vmax |b| |gain| + 4 |o|) * 2^-24

The float64 interpolation of this file contributes 2^-53 relative, nothing at this scale.  Vmax is the largest magnitude among the
voxels, the border values and the finite lo, hi and a of the table."""
import math

import numpy as np

WINDOW, ZSCORE, PERCENTILE = 0, 1, 2
NO_FOREGROUND = -32769


def record(vol, foreground, q_ppm):
    """vol integer [M, D, Hs, Ws] -> M rows of eight Python ints: n, sum v, sum v^2, min, max, v_lo, v_hi, 0 of the foreground v >
    foreground[m]; v_lo / v_hi at the ranks (q_ppm * (n - 1)) // 10^6 of the sorted foreground; all 0 when it is empty."""
    out = []
    for m in range(vol.shape[0]):
        v = np.sort(vol[m].reshape(-1).astype(np.int64))
        v = v[v > int(foreground[m])]
        n = int(v.size)
        if n == 0:
            out.append([0] * 8)
            continue
        ints = [int(t) for t in v]
        r_lo, r_hi = (int(q_ppm[0]) * (n - 1)) // 1000000, (int(q_ppm[1]) * (n - 1)) // 1000000
        out.append([n, sum(ints), sum(t * t for t in ints), ints[0], ints[-1], ints[r_lo], ints[r_hi], 0])
    return out


def table(rec, specs):
    """float64 [S, 4]: (lo, hi, a, b) of each spec (modality, kind, level, width) from the records."""
    T = np.zeros((len(specs), 4), dtype=np.float64)
    for i, (m, kind, level, width) in enumerate(specs):
        n, s, q, _, _, v_lo, v_hi, _ = rec[m]
        if kind == WINDOW:
            T[i] = (level - 0.5 * width, level + 0.5 * width, level - 0.5 * width, 1.0 / width)
        elif kind == ZSCORE:
            if n:
                std = math.sqrt(n * q - s * s) / n            # (Python integers: exact until the square root)
                T[i] = (v_lo, v_hi, s / n, 1.0 / max(std, 1e-8))
            else:
                T[i] = (v_lo, v_hi, 0.0, 0.0)
        else:
            T[i] = (v_lo, v_hi, v_lo, 0.0 if v_hi == v_lo else 1.0 / (v_hi - v_lo))
    return T


def _coords(row, h, w, Hs, Ws, dt):
    """(sx, sy) [h, w] in dtype dt: every product and sum rounded once, then the clamp that keeps far outside just outside"""
    r = np.asarray(row[:6]).astype(dt)
    xs, ys = np.arange(w, dtype=dt)[None, :], np.arange(h, dtype=dt)[:, None]
    sx = ((r[0] * xs).astype(dt) + (r[1] * ys).astype(dt)).astype(dt) + r[2]
    sy = ((r[3] * xs).astype(dt) + (r[4] * ys).astype(dt)).astype(dt) + r[5]
    sx = np.minimum(np.maximum(sx.astype(dt), dt(-2)), dt(Ws + 1))
    sy = np.minimum(np.maximum(sy.astype(dt), dt(-2)), dt(Hs + 1))
    return sx, sy


def gather(vol, labels, z, rows, tab, spec_mod, context, stride, size, edge="replicate", border="replicate", border_value=None,
           label_border=0, coord_dtype=np.float32):
    """-> (x float64 [n, C, h, w] or None, y int64 [n, h, w] or None, near [n, h, w] bool: a label coordinate within 1e-4 of a tie).
    vol integer [M, D, Hs, Ws] or None, labels [D, Hs, Ws] or None, rows [n, 8] (m0 .. m5, gain, bias), tab [S, 4]."""
    ref = vol[0] if vol is not None else labels
    D, Hs, Ws = ref.shape
    h, w = size
    n, K = len(z), 2 * context + 1
    S = 0 if vol is None else len(spec_mod)
    x = np.zeros((n, S * K, h, w), dtype=np.float64) if vol is not None else None
    y = np.zeros((n, h, w), dtype=np.int64) if labels is not None else None
    near = np.zeros((n, h, w), dtype=bool)
    dt = coord_dtype
    for i in range(n):
        zc = min(max(int(z[i]), 0), D - 1)
        gain, bias = float(rows[i][6]), float(rows[i][7])
        sx, sy = _coords(rows[i], h, w, Hs, Ws, dt)
        x0, y0 = np.floor(sx), np.floor(sy)
        fx, fy = (sx - x0).astype(np.float64), (sy - y0).astype(np.float64)
        x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
        tx, ty = (sx + dt(0.5)).astype(dt), (sy + dt(0.5)).astype(dt)
        lx, ly = np.floor(tx).astype(np.int64), np.floor(ty).astype(np.int64)
        near[i] = (np.abs(tx - np.rint(tx)) < 1e-4) | (np.abs(ty - np.rint(ty)) < 1e-4)

        def tap(plane, yy, xx, fill):
            ok = (yy >= 0) & (yy < Hs) & (xx >= 0) & (xx < Ws)
            t = plane[np.clip(yy, 0, Hs - 1), np.clip(xx, 0, Ws - 1)].astype(np.float64)
            return t if border == "replicate" else np.where(ok, t, float(fill))

        if labels is not None:
            y[i] = tap(labels[zc], ly, lx, label_border).astype(np.int64)
        for s in range(S):
            m = spec_mod[s]
            lo, hi, a, b = (float(t) for t in tab[s])
            for k in range(K):
                zs = zc + (k - context) * stride
                if edge == "zero" and not 0 <= zs < D:
                    x[i, s * K + k] = 0.0 * gain + bias
                    continue
                p = vol[m, min(max(zs, 0), D - 1)]
                bv = 0.0 if border_value is None else border_value[m]
                top = (1.0 - fx) * tap(p, y0, x0, bv) + fx * tap(p, y0, x0 + 1, bv)
                bot = (1.0 - fx) * tap(p, y0 + 1, x0, bv) + fx * tap(p, y0 + 1, x0 + 1, bv)
                v = (1.0 - fy) * top + fy * bot
                x[i, s * K + k] = (np.minimum(np.maximum(v, lo), hi) - a) * b * gain + bias
    return x, y, near


def vmax(vol, border_value, tab):
    """the Vmax of tol(): voxels, border values and the table's lo, hi, a"""
    t = np.abs(np.asarray(tab, dtype=np.float64)[:, :3])
    return float(max(np.abs(vol.astype(np.int64)).max(), max(abs(float(b)) for b in (border_value or [0])), t.max() if t.size else 0.0))


def tol(x, rows, tab, K, v_max):
    """The device bound of the module docstring per element of x [n, C, h, w]: (8 Vmax |b| |gain| + 4 |o|) * 2^-24."""
    b = np.repeat(np.abs(np.asarray(tab, dtype=np.float64)[:, 3]), K)[None, :, None, None]
    gain = np.abs(np.asarray(rows, dtype=np.float64)[:, 6])[:, None, None, None]
    return (8.0 * v_max * b * gain + 4.0 * np.abs(x)) * 2.0 ** -24


def phantom(M, D, Hs, Ws, seed, dtype=np.int16, air=0.4):
    """An integer volume [M, D, Hs, Ws] with a large share of one value (air at -1024, or 0 for uint8), a smooth body and noise, and
    uint8 labels [D, Hs, Ws] of three classes."""
    g = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(np.arange(D), np.arange(Hs), np.arange(Ws), indexing="ij")
    r = np.sqrt(((yy - Hs / 2.0) / (0.45 * Hs)) ** 2 + ((xx - Ws / 2.0) / (0.45 * Ws)) ** 2)
    body = r < 1.0 - air * 0.5
    lab = (body.astype(np.uint8) + (r < 0.4).astype(np.uint8)).astype(np.uint8)
    vols = []
    for m in range(M):
        if dtype == np.uint8:
            v = np.where(body, 90 + 60 * m + g.integers(-40, 40, size=body.shape), 0)
            vols.append(np.clip(v, 0, 255).astype(np.uint8))
        else:
            v = np.where(body, 40 + 300 * m + 200 * np.sin(0.3 * xx + 0.2 * zz) + g.integers(-150, 150, size=body.shape), -1024)
            vols.append(v.astype(np.int16))
    return np.stack(vols), lab


# ---------------------------------------------------------------------------------------------------------------- the gather cases
# name -> shape (M, D, Hs, Ws) of the phantom, VolumeSlicer keywords, slice list, per-sample parameters (None: plain resize; "ssr" =
# (angle, scale, dx, dy) stands for ssr_matrix on the output grid).  Shared by tests/test_slices_cpu.py (float32 against float64
# coordinates) and tests/test_slices_kernels_gpu.py (the device against the float32 restatement).
_W2 = [["zscore", ("window", 40.0, 400.0)], [("percentile",), ("window", 300.0, 1500.0)]]
_W4 = [["zscore", ("percentile",), ("window", 40.0, 400.0), ("window", -600.0, 1500.0)]] * 4
_WARP = dict(ssr=(30.0, 1.1, 0.05, -0.03))
GATHER_CASES = {
    "identity": dict(shape=(1, 4, 12, 16), kw=dict(size=(12, 16)), z=[0, 1, 2, 3]),
    "up_5x7_to_16x16": dict(shape=(1, 4, 5, 7), kw=dict(size=(16, 16)), z=[0, 1, 2, 3]),
    "down_50x60_to_32x32": dict(shape=(1, 3, 50, 60), kw=dict(size=(32, 32)), z=[0, 1, 2]),
    "w18_scalar_stores": dict(shape=(1, 3, 21, 22), kw=dict(size=(10, 18)), z=[2, 0]),
    "d3_context2": dict(shape=(1, 3, 9, 11), kw=dict(size=(12, 12), context=2), z=[1, 0, 2]),
    "d3_context2_zero": dict(shape=(1, 3, 9, 11), kw=dict(size=(12, 12), context=2, edge="zero"), z=[1, 0, 2]),
    "stride2": dict(shape=(1, 9, 9, 11), kw=dict(size=(12, 12), stride=2), z=[0, 1, 4, 7, 8]),
    "unordered_repeats": dict(shape=(1, 9, 9, 11), kw=dict(size=(8, 12)), z=[5, 0, 5, 2, 8, 8, 1]),
    "n1": dict(shape=(1, 5, 9, 11), kw=dict(size=(8, 12)), z=[3]),
    "n9": dict(shape=(1, 5, 9, 11), kw=dict(size=(8, 12)), z=[0, 1, 2, 3, 4, 4, 3, 2, 1]),
    "c1": dict(shape=(1, 3, 9, 11), kw=dict(size=(8, 12), context=0, norm=("percentile",), clip=(1.0, 99.0)), z=[0, 2]),
    "c12": dict(shape=(2, 4, 9, 11), kw=dict(size=(8, 12), modalities=2, norm=_W2, foreground=-1000), z=[0, 3, 1]),
    "c16": dict(shape=(4, 3, 9, 11), kw=dict(size=(8, 12), modalities=4, norm=_W4, context=0), z=[2, 0]),
    "warp30_constant": dict(shape=(1, 3, 40, 48), kw=dict(size=(32, 32), border="constant", border_value=-1024, label_border=255), z=[0, 1, 2],
                            params=[dict(_WARP), dict(_WARP, flips=1), dict(ssr=(-30.0, 0.9, -0.1, 0.1), gain=0.9, bias=0.1)]),
    "both_flips": dict(shape=(1, 3, 20, 22), kw=dict(size=(16, 20)), z=[0, 1, 2, 1], params=[dict(flips=3), dict(flips=1), dict(flips=2), dict(flips=0)]),
    "gain_bias": dict(shape=(1, 3, 20, 22), kw=dict(size=(16, 20), norm=("window", 40.0, 400.0)), z=[0, 2],
                      params=[dict(gain=1.3, bias=-0.2), dict(gain=0.7, bias=0.5)]),
    "labels_int64": dict(shape=(1, 3, 20, 22), kw=dict(size=(16, 20), label_dtype="int64"), z=[1, 2]),
    "uint8_volume": dict(shape=(1, 3, 20, 22), kw=dict(size=(16, 20)), z=[1, 2], dtype="uint8"),
}


def case_params(case, size, ssr_matrix):
    """the per-sample dicts of a case in the form VolumeSlicer.batch takes (None: the plain resize)"""
    if case.get("params") is None:
        return None
    out = []
    for p in case["params"]:
        M = ssr_matrix(size[0], size[1], *p["ssr"]) if "ssr" in p else None
        out.append({"M": M, "flips": p.get("flips", 0), "gain": p.get("gain", 1.0), "bias": p.get("bias", 0.0)})
    return out


def case_data(name):
    """(volume [M, D, Hs, Ws], labels [D, Hs, Ws]) of a case: the phantom of its shape, seeded by its position in the list"""
    case = GATHER_CASES[name]
    M, D, Hs, Ws = case["shape"]
    return phantom(M, D, Hs, Ws, seed=list(GATHER_CASES).index(name), dtype=np.uint8 if case.get("dtype") == "uint8" else np.int16)

"""Float64 numpy restatement of include/tiles/lmnet_tiles.h: tile starts, padding (numpy.pad), mirrored copies, the windows and the
blend with its three averaging modes.  Written as a SCATTER over whole tiles on a padded canvas -- the kernel is a gather per pixel --
so that the two share no index arithmetic.  Importable without a GPU."""
import functools
import math

import numpy as np

FLIPS = {"h": (False, True), "v": (True, False), "hv": (True, True)}       # name -> (mirror rows, mirror columns)
EPS = 2.0 ** -24


def axis(L, t, s):
    """-> (V, p, starts): virtual length, padding before, the start of every tile in virtual coordinates"""
    V = max(L, t)
    n = int(math.ceil((V - t) / s)) + 1
    return V, (V - L) // 2, [min(i * s, V - t) for i in range(n)]


def reflect_index(i, L):
    """source index of coordinate i (any integer) under reflection without the edge sample, period 2 (L - 1)"""
    P = 2 * (L - 1)
    m = i % P
    return m if m < L else P - m


def padded(src, tile, pad):
    """src [..., H, W] -> [..., Vh, Vw]: the virtual frame the tiles are cut from"""
    H, W = src.shape[-2:]
    (Vh, ph, _), (Vw, pw, _) = axis(H, tile[0], 1), axis(W, tile[1], 1)
    widths = [(0, 0)] * (src.ndim - 2) + [(ph, Vh - H - ph), (pw, Vw - W - pw)]
    return np.pad(src, widths, mode="reflect") if pad == "reflect" else np.pad(src, widths, mode="constant", constant_values=0)


def mirror(a, flip):
    """a [..., h, w] mirrored as entry `flip` ("" or None: the identity); its own inverse"""
    if not flip:
        return a
    rows, cols = FLIPS[flip]
    a = a[..., ::-1, :] if rows else a
    return a[..., ::-1] if cols else a


def gather(src, tile, stride, pad, flips):
    """src [B, ch, H, W] -> every entry [B * n_y * n_x * F, ch, th, tw] in the order [b][ty][tx][f], the dtype of src (a copy)"""
    B, ch, H, W = src.shape
    v = padded(src, tile, pad)
    ys, xs = axis(H, tile[0], stride[0])[2], axis(W, tile[1], stride[1])[2]
    out = []
    for b in range(B):
        for y0 in ys:
            for x0 in xs:
                t = v[b, :, y0:y0 + tile[0], x0:x0 + tile[1]]
                out += [mirror(t, f) for f in ("",) + tuple(flips)]
    return np.ascontiguousarray(np.stack(out))


def window(t, kind, sigma_scale=0.125):
    """the 1-D window in float64, rounded once to fp32"""
    if kind == "constant":
        return np.ones(t, dtype=np.float32)
    i = np.arange(t, dtype=np.float64)
    return np.exp(-0.5 * ((i - (t - 1) / 2.0) / (sigma_scale * t)) ** 2).astype(np.float32)


def g_of(z, average):
    """z [C, th, tw] float64 -> the averaged quantity"""
    if average == "softmax":
        e = np.exp(z - z.max(axis=0, keepdims=True))
        return e / e.sum(axis=0, keepdims=True)
    if average == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    assert average == "logits", average
    return z


def blend(z, B, H, W, tile, stride, flips, wy, wx, average="logits"):
    """z [B * E, C, th, tw] (tile outputs in gather's order) -> float64 [B, C, H, W]:
    sum_{tiles, f} w g(un-mirrored z) / (F sum_{tiles} w), w = wy[y] wx[x] from the ROUNDED tables"""
    z = np.asarray(z, dtype=np.float64)
    C, F = z.shape[1], 1 + len(flips)
    (Vh, ph, ys), (Vw, pw, xs) = axis(H, tile[0], stride[0]), axis(W, tile[1], stride[1])
    w = np.asarray(wy, dtype=np.float64)[:, None] * np.asarray(wx, dtype=np.float64)[None, :]
    num, den = np.zeros((B, C, Vh, Vw)), np.zeros((Vh, Vw))
    for y0 in ys:
        for x0 in xs:
            den[y0:y0 + tile[0], x0:x0 + tile[1]] += w
    e = 0
    for b in range(B):
        for y0 in ys:
            for x0 in xs:
                for f in ("",) + tuple(flips):
                    num[b, :, y0:y0 + tile[0], x0:x0 + tile[1]] += w * mirror(g_of(z[e], average), f)
                    e += 1
    assert e == z.shape[0], (e, z.shape)
    return (num / (F * den))[:, :, ph:ph + H, pw:pw + W]


def top2_gap(m):
    """m [B, C, H, W], C >= 2 -> [B, H, W]: the gap between the two largest classes of every pixel"""
    s = np.sort(m, axis=1)
    return s[:, -1] - s[:, -2]


def tol(average, zmax):
    """absolute tolerance of the fp32 blend: 128 roundings of the sum at the scale of the largest tile value for "logits"; for the
    probability modes (values in [0, 1]) the softmax's own roundings on top: 256"""
    return 128 * EPS * zmax if average == "logits" else 256 * EPS


def seeded(shape, seed):
    """N(0, 1) fp32 values"""
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


# ---------------------------------------------------------------- the cases of the kernel tests (tests/test_tiles_kernels_gpu.py)
IMAGES = [(32, 32), (33, 47), (20, 70), (21, 33), (97, 64)]
TILES = [(32, 32), (32, 48)]


def strides_of(tile):
    """t, t/2, t/4 and 24 per axis"""
    return [tile, (tile[0] // 2, tile[1] // 2), (tile[0] // 4, tile[1] // 4), (24, 24)]


# one case per image x tile x stride; the other axes cycle with different periods, so that every (C, mode) pair, every F, both
# windows, both pads and both batch sizes occur (tests/test_tiles_cpu.py asserts that they do)
BLEND_CLASSES = [1, 2, 3, 5, 9, 64]
MODES = ("logits", "softmax", "sigmoid")
FLIP_SUBSETS = [(), ("h",), ("v",), ("hv",), ("h", "v"), ("v", "hv"), ("hv", "h"), ("h", "v", "hv")]


def geometries():
    return [(image, tile, stride) for image in IMAGES for tile in TILES for stride in strides_of(tile)]


def blend_cases():
    out = []
    for k, (image, tile, stride) in enumerate(geometries()):
        out.append(dict(image=image, tile=tile, stride=stride, C=BLEND_CLASSES[k % 6], average=MODES[(k // 6 + k) % 3],
                        flips=((), (("h",), ("v",), ("hv",))[k % 3], ("h", "v", "hv"))[(k // 2 + k // 18) % 3], window=("gaussian", "constant")[(k + k // 4) % 2],
                        pad=("reflect", "zero")[(k // 2) % 2], B=(1, 3)[(k // 3 + k // 6) % 2], seed=100 + k))
    return out


def gather_cases():
    return [dict(image=image, tile=tile, stride=stride, flips=FLIP_SUBSETS[k % 8], channel=(1, 3, 16)[k % 3], B=(1, 3)[(k // 8 + k) % 2],
                 seed=300 + k) for k, (image, tile, stride) in enumerate(geometries())]


def case_id(c):
    return "%dx%d-t%dx%d-s%dx%d" % (c["image"] + c["tile"] + c["stride"]) + "".join("-%s%s" % (k if len(k) == 1 else "ch" if k == "channel" else "", c[k]) for k in sorted(c) if k not in (
        "image", "tile", "stride", "seed", "flips")) + ("-" + "+".join(c["flips"]) if c.get("flips") else "")


@functools.lru_cache(maxsize=None)
def blend_case(k):
    """-> (case, z fp32 [B * E, C, th, tw], wy, wx, float64 reference [B, C, H, W]); computed once, never modified"""
    c = blend_cases()[k]
    (H, W), tile, stride, flips = c["image"], c["tile"], c["stride"], c["flips"]
    E = len(axis(H, tile[0], stride[0])[2]) * len(axis(W, tile[1], stride[1])[2]) * (1 + len(flips))
    z = seeded((c["B"] * E, c["C"]) + tile, c["seed"])
    wy, wx = window(tile[0], c["window"]), window(tile[1], c["window"])
    ref = blend(z, c["B"], H, W, tile, stride, flips, wy, wx, c["average"])
    for a in (z, wy, wx, ref):
        a.setflags(write=False)
    return c, z, wy, wx, ref

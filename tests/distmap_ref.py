"""Restatement of include/distmap/lmnet_distmap.h in numpy and float64 torch, written from the definitions:

  * sd2 / flags: the signed squared Euclidean distance of a mask, by brute force (sd2_brute) and separably (sd2_plane: a column
    scan, then min_j (x - j)^2 + g^2 over a dense [W, W] table); exact integers.  A mask that is empty or the whole image: all 0;
  * phi: Kervadec's one_hot2dist from sd2;
  * masks of label maps and of logits (float64; near_threshold counts the elements whose fp32 evaluation could fall either way);
  * loss: both terms under both heads, differentiable float64 torch, with N and the sum of magnitudes that conditions the
    boundary sum; loss_and_grad runs autograd on it;
  * seeded generators: planes() yields one mask of every kind the GPU tests name, label_batch() a label map that holds them all.

tests/test_distmap_cpu.py checks sd2_plane against scipy.ndimage.distance_transform_edt and sd2_brute, phi against Kervadec's
formula on scipy's transforms, and the gradients against finite differences."""
import numpy as np
import torch

KINDS = ("blobs", "noise", "corner", "corner_complement", "frame", "checker", "empty", "full")
VOID = 255
MARGIN = 1e-6          # |p - threshold| below this: fp32 and float64 may disagree on the mask


# ---------------------------------------------------------------------------------------------------------------- the transform
def _to_nearest(T):
    """int32 [H, W]: squared distance from every pixel OUTSIDE T to the nearest True pixel of T (T must hold one); 0 inside T.  Only
    the columns that hold a pixel of T can carry the minimum, and only the pixels outside T are asked for: sparse masks stay cheap."""
    H, W = T.shape
    big = 40000                                          # big^2 + 1023^2 < 2^31
    g = np.full((H, W), big, np.int32)
    run = np.full(W, big, np.int32)
    for y in range(H):                                   # distance to the nearest True above or at y
        run = np.where(T[y], 0, np.minimum(run + 1, big)).astype(np.int32)
        g[y] = run
    run = np.full(W, big, np.int32)
    for y in range(H - 1, -1, -1):
        run = np.where(T[y], 0, np.minimum(run + 1, big)).astype(np.int32)
        g[y] = np.minimum(g[y], run)
    cols = np.nonzero(T.any(0))[0]
    g2 = g[:, cols] ** 2
    out = np.zeros((H, W), np.int32)
    for y in range(H):
        xs = np.nonzero(~T[y])[0]
        if xs.size:
            out[y, xs] = (((xs[:, None] - cols[None, :]) ** 2).astype(np.int32) + g2[y][None, :]).min(1)
    return out


def flag_of(M):
    n = int(np.count_nonzero(M))
    return 1 if n == 0 else 2 if n == M.size else 0


def sd2_plane(M):
    """int32 [H, W] of a boolean mask."""
    M = np.asarray(M, bool)
    if flag_of(M):
        return np.zeros(M.shape, np.int32)
    return (_to_nearest(M) - _to_nearest(~M)).astype(np.int32)


def sd2_brute(M):
    """The definition, pixel by pixel (small planes only)."""
    M = np.asarray(M, bool)
    out = np.zeros(M.shape, np.int32)
    if flag_of(M):
        return out
    yy, xx = np.nonzero(M)
    yo, xo = np.nonzero(~M)
    for y in range(M.shape[0]):
        for x in range(M.shape[1]):
            if M[y, x]:
                out[y, x] = -int(((yo - y) ** 2 + (xo - x) ** 2).min())
            else:
                out[y, x] = int(((yy - y) ** 2 + (xx - x) ** 2).min())
    return out


def maps(masks):
    """(sd2 int32 [B, nk, H, W], flags int32 [B, nk]) of boolean masks [B, nk, H, W]."""
    masks = np.asarray(masks, bool)
    B, nk = masks.shape[:2]
    sd2 = np.stack([np.stack([sd2_plane(masks[b, k]) for k in range(nk)]) for b in range(B)])
    flags = np.array([[flag_of(masks[b, k]) for k in range(nk)] for b in range(B)], np.int32)
    return sd2, flags


def phi(sd2):
    """float64: sqrt(sd2) outside, -(sqrt(-sd2) - 1) inside, 0 where sd2 == 0 (a flagged plane)."""
    s = np.asarray(sd2, np.float64)
    return np.where(s > 0, np.sqrt(np.abs(s)), np.where(s < 0, 1.0 - np.sqrt(np.abs(s)), 0.0))


# ---------------------------------------------------------------------------------------------------------------- masks
def default_classes(C):
    return list(range(1, C)) if C > 1 else [0]


def masks_of_labels(y, classes):
    """bool [B, nk, H, W]: label == k (a void or out-of-range label equals no class)."""
    y = np.asarray(y).astype(np.int64)
    return np.stack([y == k for k in classes], 1)


def probabilities(lg, mode):
    z = np.asarray(lg, np.float64)
    if mode == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def masks_of_logits(lg, mode, classes, threshold=0.5):
    """(bool [B, nk, H, W], number of elements within MARGIN of the threshold).  Sigmoid at 0.5 is the exact test z > 0."""
    z = np.asarray(lg)
    if mode == "sigmoid" and threshold == 0.5:
        return z[:, classes] > 0, 0
    p = probabilities(z, mode)[:, classes]
    return p > threshold, int(np.count_nonzero(np.abs(p - threshold) < MARGIN))


# ---------------------------------------------------------------------------------------------------------------- the losses
def loss(lg, target, head, term, classes, sd2_g, sd2_p=None, alpha=2.0, scale=1.0):
    """(scale * L as a float64 tensor, N, (1 / N) sum |terms|) of float64 logits [B, C, H, W]; N = 0 gives 0, not NaN."""
    C = lg.shape[1]
    t = torch.as_tensor(np.asarray(target).astype(np.int64))
    ks = torch.as_tensor(classes)
    if head == "softmax":
        p = torch.softmax(lg, 1)[:, ks]
        valid = ((t >= 0) & (t < C))[:, None].expand_as(p)
        g = t[:, None] == ks[None, :, None, None]
    else:
        if t.dim() == 3:
            t = t[:, None]
        p = torch.sigmoid(lg)[:, ks]
        tk = t[:, ks]
        valid = (tk == 0) | (tk == 1)
        g = tk == 1
    if term == "boundary":
        f = p * torch.as_tensor(phi(sd2_g))
    else:
        w = np.abs(np.asarray(sd2_p, np.float64)) ** (alpha / 2) + np.abs(np.asarray(sd2_g, np.float64)) ** (alpha / 2)
        f = (p - g.double()) ** 2 * torch.as_tensor(w)
    n = int(valid.sum())
    if n == 0:
        return lg.sum() * 0, 0, 0.0
    f = f * valid
    return scale * f.sum() / n, n, float(f.detach().abs().sum()) / n


def prediction_maps(lg, head, classes):
    """sd2 of the prediction thresholded at 0.5, and the number of elements too near the threshold to call."""
    m, near = masks_of_logits(np.asarray(lg), head, classes)
    return maps(m)[0], near


def target_masks(target, head, classes):
    t = np.asarray(target).astype(np.int64)
    if head == "softmax":
        return masks_of_labels(t, classes)
    if t.ndim == 3:
        t = t[:, None]
    return t[:, classes] == 1


def loss_and_grad(lg, target, head, term, classes, alpha=2.0, scale=1.0, gscale=None):
    """-> (loss, d (gscale * loss) / d logits float64 numpy, N, magnitude, near) on the fp32 logits as they are."""
    l64 = torch.as_tensor(np.asarray(lg)).double().requires_grad_(True)
    sd2_g = maps(target_masks(target, head, classes))[0]
    sd2_p, near = (None, 0) if term == "boundary" else prediction_maps(lg, head, classes)
    val, n, mag = loss(l64, target, head, term, classes, sd2_g, sd2_p, alpha, scale)
    (val * (1.0 if gscale is None else gscale)).backward()
    return float(val.detach()), l64.grad.numpy(), n, abs(scale) * mag, near


# ---------------------------------------------------------------------------------------------------------------- generators
def blobs(H, W, rng, n=3):
    """Organ-like: the union of a few ellipses."""
    yy, xx = np.mgrid[:H, :W]
    M = np.zeros((H, W), bool)
    for _ in range(n):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        ry, rx = rng.uniform(1.5, max(2.0, H / 3)), rng.uniform(1.5, max(2.0, W / 3))
        M |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return M


def planes(H, W, seed=0, sparse=False):
    """{kind: bool [H, W]} with every kind of KINDS.  sparse: blobs and noise hold a handful of pixels (the long scans of the big
    planes)."""
    rng = np.random.default_rng([seed, H, W])
    corner = np.zeros((H, W), bool)
    corner[H - 1, 0] = True
    frame = np.ones((H, W), bool)
    frame[1:-1, 1:-1] = False
    yy, xx = np.mgrid[:H, :W]
    out = {"blobs": blobs(H, W, rng, 1 if sparse else 3), "noise": rng.random((H, W)) < (4.0 / (H * W) if sparse else 0.5), "corner": corner,
           "corner_complement": ~corner, "frame": frame, "checker": (yy + xx) % 2 == 0, "empty": np.zeros((H, W), bool),
           "full": np.ones((H, W), bool)}
    if H * W <= 4:                                        # 2 x 2: the frame is the whole image; keep it an ordinary mask
        out["frame"] = corner.copy()
    for kind in ("blobs", "noise"):                       # (a tiny or sparse plane may come out empty or full: make it ordinary)
        if flag_of(out[kind]):
            out[kind][0, 0], out[kind][-1, -1] = True, False
    assert tuple(out) == KINDS
    return out


def label_batch(H, W, C, classes, seed=0, sparse=False):
    """uint8 [len(KINDS) + 1, H, W]: sample b holds kind b's mask as the FIRST scored class, the rest of the image spread over the
    other classes (scored ones included) -- in stripes, not noise, when sparse -- and the last sample is void everywhere."""
    rng = np.random.default_rng([seed, H, W, C])
    k0 = classes[0]
    others = [c for c in range(C) if c != k0]
    out = []
    for kind, M in planes(H, W, seed, sparse).items():
        if not others:
            rest = np.full((H, W), VOID)
        elif sparse:
            rest = np.asarray(others)[(np.mgrid[:H, :W][0] * len(others)) // H]
        else:
            rest = np.asarray(others)[rng.integers(0, len(others), (H, W))]
        out.append(np.where(M, k0, rest))
    out.append(np.full((H, W), VOID))
    return np.stack(out).astype(np.uint8)


def logits_of_labels(y, C, mode, seed=0):
    """fp32 logits [B, C, H, W] whose thresholded masks are exactly those of the label map y: margin 6 for the labelled class; a void
    pixel has no class above the threshold (softmax at C = 2 cannot say 'none': there it goes to class 0)."""
    rng = np.random.default_rng([seed, C, 7])
    y = np.asarray(y).astype(np.int64)
    on = np.stack([y == c for c in range(C)], 1)
    if mode == "sigmoid":
        z = np.where(on, 1.0, -1.0) * (3.0 + rng.random(on.shape))
    else:
        if C == 2:
            on[:, 0] |= ~on.any(1)
        z = 6.0 * on + np.where(on.any(1, keepdims=True), 0.5 * rng.random(on.shape), 0.0)
    return z.astype(np.float32)


def loss_inputs(B, C, H, W, head, seed=0, void=False):
    """(fp32 logits [B, C, H, W], uint8 target) of a loss case: logits 2.5 * N(0, 1); organ-like labels, 20 % void on request.
    Softmax head: a label map whose classes are nested blobs; sigmoid head: one independent blob plane per class."""
    rng = np.random.default_rng([seed, B, C, H, W, 11])
    lg = (2.5 * rng.standard_normal((B, C, H, W))).astype(np.float32)
    if head == "softmax":
        y = np.zeros((B, H, W), np.int64)
        for b in range(B):
            for c in range(1, min(C, 6)):
                y[b][blobs(H, W, rng, 2)] = c
            if C > 6:                                     # the high classes in a stripe, so that every class id occurs
                y[b, :, -3:] = 6 + (np.arange(3 * H) + b).reshape(H, 3) % (C - 6)
    else:
        y = np.stack([np.stack([blobs(H, W, rng, 2) for _ in range(C)]) for _ in range(B)]).astype(np.int64)
    if void:
        y = np.where(rng.random(y.shape) < 0.2, VOID, y)
    return lg, y.astype(np.uint8)

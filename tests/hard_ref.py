"""The hard-pixel criterion of include/hard/lmnet_hard.h restated in numpy float64: the reference of the GPU tests of
lm_net_amd.loss.HardPixelLoss and hard_pixel_values.  The header's definitions, line by line: the per-element values under both heads
and the validity rule of each, the groups, the count K = min(N, max(1, floor(float32(keep) N), min_kept, Nhard)), the K-th largest value
tau with n_gt and n_eq, the term (sum_{l > tau} l + (K - n_gt) tau) / K, the tie rule of the gradient and the edge rules (N = 0: the
group contributes 0; +0 at every void and every unselected position).  tests/test_hard_cpu.py checks it against torch.topk over
F.cross_entropy / F.binary_cross_entropy_with_logits, float64 autograd, finite differences and an explicit OHEM loop.

A device record can be handed in (`device=(values, selection)`, the fp32 values and the int32 [G, 5] record of a call): the gradient
is then evaluated on the device's own selection -- every element classified by its fp32 value against the record's tau, with the
record's K, n_gt and n_eq -- and the loss at the device's K, because Nhard counts fp32 comparisons that float64 cannot restate at a
value within rounding of the cut.
"""
from types import SimpleNamespace

import numpy as np

VOID = 255
WORDS = 5
# the bar of the device's fp32 values against values(): |v - l| <= VALUES_BAR * max(1, l) per element.  8 x the largest deviation
# measured on an MI355X over the shapes of tests/test_hard_kernels_gpu.py, 5.452e-07 of max(1, l) (softmax head, 64 classes,
# 2 x 96 x 96, logits of scale 3), and not above 1e-5
VALUES_BAR = 4.36e-6


def inputs(B, C, H, W, head="softmax", seed=0, void=0.2, dtype=np.int64, scale=1.0):
    """(fp32 logits [B, C, H, W], target): a label map [B, H, W] under a softmax head, planes [B, C, H, W] in {0, 1} under a sigmoid
    head, a fraction `void` of the elements VOID."""
    rng = np.random.default_rng(seed)
    lg = (scale * rng.standard_normal((B, C, H, W))).astype(np.float32)
    if head == "softmax":
        y = rng.integers(0, C, (B, H, W))
    else:
        y = (rng.random((B, C, H, W)) < 0.4).astype(np.int64)
    y[rng.random(y.shape) < void] = VOID
    return lg, y.astype(dtype)


def cut_of(thresh):
    """float32(-log(thresh)), the logarithm in double; None passes through"""
    return None if thresh is None else np.float32(-np.log(np.float64(thresh))) + np.float32(0.0)


def count(N, keep=None, min_kept=0, nhard=0):
    """K of a group with N valid elements, in the integer / double arithmetic of the header"""
    if N == 0:
        return 0
    kkeep = 0 if keep is None else int(np.floor(np.float64(np.float32(keep)) * np.float64(N)))
    return int(min(N, max(1, kkeep, int(min_kept), int(nhard))))


def log_softmax(z):
    m = z.max(axis=1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=1, keepdims=True))


def values(lg, y, head="softmax", weight=None):
    """(l, valid, dl): the float64 value of every element in the layout of the header ([B, H, W] under a softmax head; 0 at a void
    element), its validity, and d l / d logits [B, C, H, W] (0 at a void position)"""
    z = np.asarray(lg, np.float64)
    B, C, H, W = z.shape
    y = np.asarray(y).astype(np.int64)
    w = np.ones(C) if weight is None else np.asarray(weight, np.float64)
    if head == "softmax":
        valid = (y >= 0) & (y < C)
        yc = np.where(valid, y, 0)
        lp = log_softmax(z)
        onehot = (np.arange(C)[None, :, None, None] == yc[:, None])
        wy = w[yc]
        l = np.where(valid, -wy * np.take_along_axis(lp, yc[:, None], 1)[:, 0], 0.0)
        dl = np.where(valid[:, None], wy[:, None] * (np.exp(lp) - onehot), 0.0)
    else:
        if y.ndim == 3:
            y = y[:, None]
        valid = (y == 0) | (y == 1)
        t = np.where(valid, y, 0).astype(np.float64)
        wc = w[None, :, None, None]
        sp = np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))          # softplus(z)
        l = np.where(valid, wc * (sp - t * z), 0.0)
        p = np.where(z >= 0, 1.0 / (1.0 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))))
        dl = np.where(valid, wc * (p - t), 0.0)
    return np.maximum(l, 0.0), valid, dl


def grouped(a, per_image):
    """[G, M]: the elements of every group"""
    a = np.asarray(a)
    return a.reshape(a.shape[0], -1) if per_image else a.reshape(1, -1)


def select(v, K):
    """(tau, n_gt, n_eq) of the valid values v of a group: tau the K-th largest (np.partition on the same array)"""
    if K == 0:
        return v.dtype.type(0), 0, 0
    tau = np.partition(v, v.size - K)[v.size - K]
    return tau, int((v > tau).sum()), int((v == tau).sum())


def bits(x):
    return int(np.asarray(x, np.float32).view(np.int32))


def record_of(vals32, valid, per_image, keep=None, min_kept=0, thresh=None):
    """The int32 [G, 5] record of fp32 values: N, K, n_gt, n_eq, the bits of tau -- numpy's selection on the same fp32 array."""
    out = []
    cut = cut_of(thresh)
    for v, ok in zip(grouped(vals32, per_image), grouped(valid, per_image)):
        v = np.ascontiguousarray(v[ok], np.float32)
        K = count(v.size, keep, min_kept, 0 if cut is None else int((v > cut).sum()))
        tau, n_gt, n_eq = select(v, K)
        out.append([v.size, K, n_gt, n_eq, bits(tau) if K else 0])
    return np.asarray(out, np.int32)


def loss_and_grad(lg, y, C=None, head="softmax", keep=None, min_kept=0, thresh=None, weight=None, per_image=False, scale=1.0, gscale=1.0,
                  device=None):
    """namespace(loss, terms [G], grad [B, C, H, W], values, valid, record int64 [G, 4] = N, K, n_gt, n_eq, tau [G], weights: the
    gradient weight of every element).  device: see the module docstring."""
    l, valid, dl = values(lg, y, head, weight)
    lgr, okr = grouped(l, per_image), grouped(valid, per_image)
    G = lgr.shape[0]
    cut = cut_of(thresh)
    terms, rec, taus = np.zeros(G), np.zeros((G, 4), np.int64), np.zeros(G)
    wts = np.zeros(lgr.shape)
    if device is not None:
        dv, dr = grouped(np.asarray(device[0], np.float32), per_image), np.asarray(device[1]).reshape(G, WORDS)
    for g in range(G):
        v = lgr[g][okr[g]]
        N = v.size
        if device is None:
            K = count(N, keep, min_kept, 0 if cut is None else int((v > np.float64(cut)).sum()))
        else:
            K = int(dr[g, 1])
            assert int(dr[g, 0]) == N and (N == 0) == (K == 0) and K <= N, (dr[g], N)
        tau, n_gt, n_eq = select(v, K)
        if K:
            terms[g] = (v[v > tau].sum() + (K - n_gt) * tau) / K
        rec[g], taus[g] = (N, K, n_gt, n_eq), tau
        if not K:
            continue
        if device is None:
            wts[g] = np.where(okr[g] & (lgr[g] > tau), 1.0 / K, np.where(okr[g] & (lgr[g] == tau), (K - n_gt) / (max(n_eq, 1) * K), 0.0))
        else:                                                # the device's own selection: its values against its tau
            dtau = np.asarray(dr[g, 4], np.int32).view(np.float32)
            d_gt, d_eq = int(dr[g, 2]), int(dr[g, 3])
            wts[g] = np.where(okr[g] & (dv[g] > dtau), 1.0 / K, np.where(okr[g] & (dv[g] == dtau), (K - d_gt) / (max(d_eq, 1) * K), 0.0))
    loss = scale * terms.sum() / G
    wt = wts.reshape(l.shape)
    grad = gscale * scale / G * (wt[:, None] if head == "softmax" else wt) * dl
    grad = grad + 0.0                                        # (-0 -> +0)
    return SimpleNamespace(loss=loss, terms=terms, grad=grad, values=l, valid=valid, record=rec, tau=taus, weights=wt)

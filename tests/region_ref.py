"""The region-overlap losses of include/region/lmnet_region.h restated in numpy float64: the reference of the GPU tests of
lm_net_amd.loss.RegionLoss and region_sums.  The header's definitions, line by line: the sums I, P1, P2, T, N of every (group, scored
class) over the valid elements, the ratio of the kind, the edge rules (a denominator that is exactly 0 gives R = 1; u <= 0 under
exponent != 1 gives 0 with a zero derivative), the coefficients a, b, c and the gradient through the softmax or the sigmoid.
tests/test_region_cpu.py checks it against the reference's own classes, a torch float64 autograd composition and finite differences.
"""
from types import SimpleNamespace

import numpy as np

VOID = 255


def inputs(B, C, H, W, head="softmax", seed=0, void=0.0, dtype=np.int64):
    """fp32 logits of unit scale and a target of `dtype` (a label map, or planes under a sigmoid head), a fraction `void` of it VOID."""
    rng = np.random.default_rng(seed)
    lg = rng.standard_normal((B, C, H, W)).astype(np.float32)
    if head == "softmax":
        y = rng.integers(0, C, (B, H, W))
    else:
        y = (rng.random((B, C, H, W)) < 0.4).astype(np.int64)
    if void > 0:
        y[rng.random(y.shape) < void] = VOID
    return lg, y.astype(dtype)


def class_ids(C, classes=None):
    return list(range(C)) if classes is None else sorted(int(k) for k in classes)


def probabilities(logits, head):
    z = np.asarray(logits, dtype=np.float64)
    if head == "softmax":
        e = np.exp(z - z.max(1, keepdims=True))
        return e / e.sum(1, keepdims=True)
    return np.where(z >= 0, 1.0 / (1.0 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))))


def targets(y, C, head):
    """(t, valid) as float64 / bool [B, C, H, W]"""
    y = np.asarray(y).astype(np.int64)
    if head == "softmax":
        valid = (y >= 0) & (y < C)
        t = (y[:, None] == np.arange(C)[None, :, None, None]) & valid[:, None]
        return t.astype(np.float64), np.broadcast_to(valid[:, None], t.shape)
    if y.ndim == 3:
        y = y[:, None]
    valid = (y == 0) | (y == 1)
    return ((y == 1) & valid).astype(np.float64), valid


def power(u, ex):
    """(L, dL/du) of the edge rule"""
    if ex == 1.0:
        return u, 1.0
    if u > 0.0:
        return u ** ex, ex * u ** (ex - 1.0)
    return 0.0, 0.0


def finish(S, Cn, kind, denominator, smooth, alpha, beta, exponent, scale, weight):
    """S [G, nk, 3] (I, P1, P2) and Cn [G, nk, 2] (T, N) -> (loss, per_class [G, nk], coef [G, nk, 3], u [G, nk])"""
    G, nk = S.shape[:2]
    sq = denominator == "squared"
    s, wn = float(smooth), float(scale) / (G * nk)
    w = np.ones(nk) if weight is None else np.asarray(weight, dtype=np.float64)
    per_class, coef, us = np.zeros((G, nk)), np.zeros((G, nk, 3)), np.zeros((G, nk))
    loss = 0.0
    for g in range(G):
        I, P1, P2, T = S[g, :, 0], S[g, :, 1], S[g, :, 2], Cn[g, :, 0].astype(np.float64)
        if kind == "generalized_dice":
            fin = [1.0 / (t * t) for t in T if t > 0]
            vmax = max(fin) if fin else 0.0
            v = np.array([1.0 / (t * t) if t > 0 else vmax for t in T])
            num, den = 2.0 * (v * I).sum() + s, (v * (P1 + T)).sum() + s
            if den == 0.0:
                continue
            u = 1.0 - num / den
            L, dL = power(u, exponent)
            per_class[g], us[g] = L, u
            coef[g, :, 0] = -dL * wn * nk * 2.0 * v / den
            coef[g, :, 1] = dL * wn * nk * v * num / (den * den)
            loss += wn * nk * L
            continue
        for k in range(nk):
            D = (P2[k] if sq else P1[k]) + T[k]
            if kind == "dice":
                num, den = 2.0 * I[k] + s, D + s
                rI, rP = (2.0 / den, -num / den ** 2) if den != 0.0 else (0.0, 0.0)
            elif kind == "jaccard":
                num, den = I[k] + s, D - I[k] + s
                rI, rP = (1.0 / den + num / den ** 2, -num / den ** 2) if den != 0.0 else (0.0, 0.0)
            else:
                num, den = I[k] + s, I[k] + alpha * (P1[k] - I[k]) + beta * (T[k] - I[k]) + s
                rI, rP = (1.0 / den - num * (1.0 - alpha - beta) / den ** 2, -alpha * num / den ** 2) if den != 0.0 else (0.0, 0.0)
            if den == 0.0:
                continue
            u = 1.0 - num / den
            L, dL = power(u, exponent)
            per_class[g, k], us[g, k] = L, u
            coef[g, k, 0] = -dL * w[k] * wn * rI
            coef[g, k, 2 if sq else 1] = (2.0 if sq else 1.0) * -dL * w[k] * wn * rP
            loss += w[k] * wn * L
    return loss, per_class, coef, us


def loss_and_grad(logits, y, C, kind="dice", head="softmax", classes=None, weight=None, per_image=False, denominator=None, smooth=1e-5,
                  alpha=0.5, beta=0.5, exponent=1.0, scale=1.0, gscale=1.0, p=None):
    """-> namespace(loss, grad [B, C, H, W], per_class [G, nk], sums [G, nk, 3], counts [G, nk, 2] int32, coef [G, nk, 3], u [G, nk]).
    `p`: probabilities to use instead of those of the logits (the edge cases hand in a p that is exactly 1)."""
    if denominator is None:
        denominator = "squared" if kind in ("dice", "jaccard") else "linear"
    assert denominator == "linear" or kind in ("dice", "jaccard")
    assert kind != "generalized_dice" or weight is None
    ids = class_ids(C, classes)
    nk = len(ids)
    p = probabilities(logits, head) if p is None else np.asarray(p, dtype=np.float64)
    t, valid = targets(y, C, head)
    B = p.shape[0]
    G = B if per_image else 1
    m = valid.astype(np.float64)
    red = (lambda a: a[:, ids].sum((2, 3))) if per_image else (lambda a: a[:, ids].sum((0, 2, 3))[None])
    S = np.stack([red(p * t * m), red(p * m), red(p * p * m) if denominator == "squared" else np.zeros((G, nk))], -1)
    Cn = np.stack([red(t * m), red(m)], -1)
    loss, per_class, coef, u = finish(S, Cn, kind, denominator, smooth, alpha, beta, exponent, scale, weight)
    d = np.zeros_like(p)                                 # d loss / dp, 0 for an unscored class and at a void element
    for g in range(G):
        sel = slice(g, g + 1) if per_image else slice(None)
        for kk, k in enumerate(ids):
            a, b, c = coef[g, kk]
            d[sel, k] = (a * t[sel, k] + b + c * p[sel, k]) * m[sel, k]
    if head == "softmax":
        grad = p * (d - (p * d).sum(1, keepdims=True))
    else:
        grad = p * (1.0 - p) * d
    grad = np.where(valid, grad * gscale, 0.0)           # +0 at every void position
    return SimpleNamespace(loss=loss, grad=grad, per_class=per_class, sums=S, counts=np.rint(Cn).astype(np.int32), coef=coef, u=u)

"""The restatement behind the CurveMeter tests (include/curves/lmnet_curves.h, lm_net_amd.metrics.CurveMeter): numpy, brute force.

For every threshold k and every (image, class) plane it counts `(score >= edge_k) & positive` and `(score >= edge_k) & negative`
directly -- it bins nothing and takes no suffix sums, so it is independent of both the kernel's search and the host's arithmetic.
"sigmoid" and "probability" scores are compared as np.float32 against the fp32 edge table (the comparison the kernel makes, bit for
bit); "softmax" scores are float64 softmax values compared against the float64 thresholds (the GPU test keeps its inputs away from
the edges by a margin far above fp32 rounding).  The ROC / PR / AUROC / average-precision formulas of the issue are restated in plain
loops, and `exact_auroc` is the unbinned area by rank statistics.  Importable without a GPU."""
import zlib

import numpy as np

from lm_net_amd import hip


def rng(key):
    return np.random.default_rng(zlib.crc32(key.encode()))


# ---------------------------------------------------------------- inputs
def logits(shape, key, scale=4.0):
    return (rng(key).standard_normal(shape) * scale).astype(np.float32)


def plane_targets(shape, key, void=0.2, dtype=np.int64):
    """0 / 1 planes with a `void` share of other values (2, 255 and, for int64, -1 and 300)."""
    r = rng(key)
    t = (r.random(shape) < 0.4).astype(np.int64)
    junk = np.array([2, 255, 7] if dtype == np.uint8 else [2, 255, -1, 300], dtype=np.int64)
    t = np.where(r.random(shape) < void, junk[r.integers(0, len(junk), shape)], t)
    return t.astype(dtype)


def label_targets(shape, C, key, void=0.2, dtype=np.int64):
    """label maps [B, H, W] in [0, C) with a `void` share of labels outside (C, 255 and, for int64, -1 and 1000)."""
    r = rng(key)
    t = r.integers(0, C, shape)
    junk = np.array([C, 255] if dtype == np.uint8 else [C, 255, -1, 1000], dtype=np.int64)
    t = np.where(r.random(shape) < void, junk[r.integers(0, len(junk), shape)], t)
    return t.astype(dtype)


# ---------------------------------------------------------------- brute-force counts
def classes_of(target, C, form):
    """pos, neg: bool [B, C, HW].  form "planes": target [B, C, ...], 1 / 0 / void; "labels": target [B, ...], one-vs-rest."""
    t = np.asarray(target).astype(np.int64)
    if form == "planes":
        t = t.reshape(t.shape[0], C, -1)
        return t == 1, t == 0
    t = t.reshape(t.shape[0], 1, -1)
    valid = (t >= 0) & (t < C)
    pos = t == np.arange(C).reshape(1, C, 1)
    return pos & valid, ~pos & valid


def scores_of(values, scores):
    """[B, C, HW] scores: fp32 as they are for "sigmoid" (logits) and "probability"; float64 softmax over C for "softmax"."""
    v = np.asarray(values)
    v = v.reshape(v.shape[0], v.shape[1], -1)
    if scores != "softmax":
        return v.astype(np.float32)
    z = v.astype(np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def edges_of(thresholds, scores):
    """what a score is compared with: the fp32 table of hip.curve_edges, or the float64 thresholds for "softmax" """
    if scores == "softmax":
        return hip.curve_thresholds(thresholds)
    return hip.curve_edges(thresholds, "logit" if scores == "sigmoid" else "probability")


def counts(values, target, thresholds, scores="sigmoid", form="planes"):
    """tp, fp, fn, tn as int64 [B, C, N], each counted directly at every threshold (NaN scores: predicted off)."""
    s = scores_of(values, scores)
    pos, neg = classes_of(target, s.shape[1], form)
    e = edges_of(thresholds, scores)
    out = np.zeros((4,) + s.shape[:2] + (len(e),), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for k, ek in enumerate(e):
            on = s >= ek
            out[0, :, :, k] = (on & pos).sum(-1)
            out[1, :, :, k] = (on & neg).sum(-1)
            out[2, :, :, k] = (~on & pos).sum(-1)
            out[3, :, :, k] = (~on & neg).sum(-1)
    return out[0], out[1], out[2], out[3]


def hist_from_counts(tp, fp, fn, tn):
    """The histograms [.., 2, N + 1] whose cells the kernel must produce: bin b holds the elements on at thresholds 0 .. b - 1 and off
    from b on, so cell b = on(b - 1) - on(b), with on(-1) = all and on(N) = none.  (Thresholds are non-decreasing.)"""
    def cells(on, off):
        total = on[..., :1] + off[..., :1]
        ext = np.concatenate([total, on, np.zeros_like(total)], -1)
        return ext[..., :-1] - ext[..., 1:]
    return np.stack([cells(fp, tn), cells(tp, fn)], -2)


def hist(values, target, thresholds, scores="sigmoid", form="planes"):
    return hist_from_counts(*counts(values, target, thresholds, scores, form))


# ---------------------------------------------------------------- the formulas, in loops
def _ratio(a, b):
    return float(a) / float(b) if b > 0 else float("nan")


def roc(tp, fp, fn, tn):
    """fpr, tpr [C, N] of pooled counts [C, N]"""
    C, N = tp.shape
    fpr, tpr = np.zeros((C, N)), np.zeros((C, N))
    for c in range(C):
        for k in range(N):
            fpr[c, k] = _ratio(fp[c, k], fp[c, k] + tn[c, k])
            tpr[c, k] = _ratio(tp[c, k], tp[c, k] + fn[c, k])
    return fpr, tpr


def pr(tp, fp, fn, tn):
    C, N = tp.shape
    prec, rec = np.zeros((C, N)), np.zeros((C, N))
    for c in range(C):
        for k in range(N):
            prec[c, k] = _ratio(tp[c, k], tp[c, k] + fp[c, k]) if tp[c, k] + fp[c, k] > 0 else 1.0
            rec[c, k] = _ratio(tp[c, k], tp[c, k] + fn[c, k])
    return prec, rec


def auroc(tp, fp, fn, tn):
    """[C]: trapezoid over (1, 1), the binned points in threshold order, (0, 0); NaN without a positive or a negative"""
    fpr, tpr = roc(tp, fp, fn, tn)
    out = np.zeros(tp.shape[0])
    for c in range(tp.shape[0]):
        x, y = [1.0] + list(fpr[c]) + [0.0], [1.0] + list(tpr[c]) + [0.0]
        out[c] = sum((x[i] - x[i + 1]) * (y[i] + y[i + 1]) / 2 for i in range(len(x) - 1))
    return out


def average_precision(tp, fp, fn, tn):
    """[C]: sum_k (R_k - R_{k+1}) P_k, R_N = 0; NaN without a positive"""
    prec, rec = pr(tp, fp, fn, tn)
    out = np.zeros(tp.shape[0])
    for c in range(tp.shape[0]):
        r = list(rec[c]) + [0.0]
        out[c] = sum((r[k] - r[k + 1]) * prec[c, k] for k in range(tp.shape[1]))
    return out


def nanmean(v):
    v = np.asarray(v, dtype=np.float64)
    ok = ~np.isnan(v)
    return float(v[ok].mean()) if ok.any() else float("nan")


def exact_auroc(score, positive):
    """The unbinned area: P(score of a positive > score of a negative) + P(equal) / 2, by average ranks (Mann-Whitney U)."""
    score, positive = np.asarray(score, dtype=np.float64).ravel(), np.asarray(positive, dtype=bool).ravel()
    n_pos, n_neg = int(positive.sum()), int((~positive).sum())
    if n_pos == 0 or n_neg == 0:
        return float("nan")
    order = np.argsort(score, kind="stable")
    s = score[order]
    rank = np.zeros(len(s))
    i = 0
    while i < len(s):
        j = i
        while j + 1 < len(s) and s[j + 1] == s[i]:
            j += 1
        rank[order[i:j + 1]] = (i + j) / 2 + 1                   # the average of the 1-based ranks i + 1 .. j + 1
        i = j + 1
    return float((rank[positive].sum() - n_pos * (n_pos + 1) / 2) / (n_pos * n_neg))


# ---------------------------------------------------------------- softmax inputs with a margin
def softmax_case(shape, thresholds, key, margin=1e-4, max_rounds=60):
    """fp32 logits [B, C, H, W] in [-8, 8] such that no float64 softmax probability of any pixel lies within `margin` of an edge
    k / (N - 1), k >= 1 (the edge at 0 is met by every non-NaN score): a pixel that fails is redrawn whole.  -> logits, rounds."""
    B, C, H, W = shape
    r = rng(key)
    t = hip.curve_thresholds(thresholds)[1:]
    z = np.clip(r.standard_normal((B, C, H * W)) * 3.0, -8, 8).astype(np.float32)
    for rounds in range(max_rounds):
        p = scores_of(z, "softmax")
        k = np.clip(np.searchsorted(t, p), 1, len(t) - 1)
        near = np.minimum(np.abs(p - t[k - 1]), np.abs(p - t[k])) < margin
        bad = near.any(1)                                        # [B, HW]
        if not bad.any():
            return z.reshape(shape), rounds
        b, i = np.nonzero(bad)
        z[b, :, i] = np.clip(r.standard_normal((len(b), C)) * 3.0, -8, 8).astype(np.float32)
    raise RuntimeError("softmax_case %s: no margin after %d rounds" % (key, max_rounds))

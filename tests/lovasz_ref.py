"""A numpy / float64-torch restatement of the Lovasz-Softmax loss and the Lovasz hinge (Berman, Triki, Blaschko, CVPR 2018), written
from the paper's algorithm 1 and the definitions of include/lovasz/lmnet_lovasz.h: the errors, the stable order (np.lexsort), the
gradient of the Jaccard index along the order in closed form, both heads and every reduction.  `loss_and_grad(..., order=)` evaluates
the loss and its autograd gradient in float64 on a GIVEN order: on one order the loss is linear in the errors, so the device's
arithmetic can be checked apart from which of two nearly equal errors its fp32 sort put first."""
import numpy as np
import torch


def class_ids(n_classes, head, classes):
    """(sorted scored class ids, present) as lm_net_amd.loss.LovaszLoss reads its arguments."""
    if isinstance(classes, str):
        assert classes in ("present", "all")
        return list(range(n_classes)), classes == "present" and head == "softmax"
    return sorted(int(k) for k in classes), False


def segments(x, B, nk, per_image):
    """[B, nk, HW] -> [S, P]: a segment per class over the batch, or per (image, class)."""
    hw = x.shape[-1]
    return x.reshape(B * nk, hw) if per_image else x.permute(1, 0, 2).reshape(nk, B * hw)


def errors_of(logits, target, head, ids, per_image):
    """(e, fg, valid) as float64 / bool torch tensors [S, P]; e is differentiable in `logits` (a float64 tensor [B, C, H, W])."""
    B, C, H, W = logits.shape
    t = torch.as_tensor(np.asarray(target).astype(np.int64))
    if head == "softmax":
        t = t.reshape(B, 1, H * W)
        p = torch.softmax(logits, 1).reshape(B, C, H * W)[:, ids]
        valid = ((t >= 0) & (t < C)).expand(B, len(ids), H * W)
        fg = (t == torch.tensor(ids).reshape(1, -1, 1)) & valid
        e = torch.where(fg, 1.0 - p, p)                    # |fg - p| with the subgradient -1 / +1 taken at e = 0 too
    else:
        t = t.reshape(B, C, H * W)[:, ids]
        z = logits.reshape(B, C, H * W)[:, ids]
        valid = (t == 0) | (t == 1)
        fg = t == 1
        e = 1.0 - z * (2.0 * fg.double() - 1.0)
    e = torch.where(valid, e, torch.zeros_like(e))
    nk = len(ids)
    return segments(e, B, nk, per_image), segments(fg, B, nk, per_image), segments(valid, B, nk, per_image)


def stable_order(e, valid):
    """[S, P] int64: the valid elements by e descending, ties by index ascending, the void elements after them by index."""
    e, valid = np.asarray(e, dtype=np.float64), np.asarray(valid, dtype=bool)
    idx = np.arange(e.shape[1])
    return np.stack([np.lexsort((idx, -e[s], ~valid[s])) for s in range(e.shape[0])])


def coefficients(fg_sorted, n_valid):
    """The closed form of lovasz_grad along one sorted segment: fg_sorted bool [P] in rank order, the first n_valid ranks valid."""
    fg = np.asarray(fg_sorted, dtype=bool)
    P = fg.shape[0]
    g = np.zeros(P)
    V = int(n_valid)
    G = int(fg[:V].sum())
    if V == 0:
        return g
    if G == 0:
        g[0] = 1.0
        return g
    n = np.cumsum(fg[:V]).astype(np.float64)
    m = np.arange(1, V + 1) - n
    f = fg[:V]
    with np.errstate(divide="ignore", invalid="ignore"):
        g[:V] = np.where(f, 1.0 / (G + m), (G - n) / ((G + m - 1.0) * (G + m)))
    return g


def coefficients_cumsum(fg_sorted):
    """Berman's lovasz_grad as published: 1 - intersection / union along the order, then first differences."""
    gt = np.asarray(fg_sorted, dtype=np.float64)
    gts = gt.sum()
    inter = gts - np.cumsum(gt)
    union = gts + np.cumsum(1.0 - gt)
    jac = 1.0 - inter / union
    if len(gt) > 1:
        jac[1:] = jac[1:] - jac[:-1]
    return jac


def weights(G, nk, groups, present):
    """w_s of every segment from the foreground counts G [S]: the mean over a group's (present) segments, then over the groups."""
    G = np.asarray(G).reshape(groups, nk)
    w = np.zeros((groups, nk))
    for q in range(groups):
        on = G[q] > 0 if present else np.ones(nk, dtype=bool)
        if on.any():
            w[q, on] = 1.0 / (on.sum() * groups)
    return w.reshape(-1)


def loss_and_grad(logits, target, n_classes, head="softmax", classes="present", per_image=False, scale=1.0, gscale=1.0, order=None):
    """(loss, dlogits float64 [B, C, H, W], counts int [S, 2], order [S, P]) in float64; `order` [S, P]: evaluate on this order
    instead of the restatement's own."""
    ids, present = class_ids(n_classes, head, classes)
    z = torch.tensor(np.asarray(logits), dtype=torch.float64, requires_grad=True)
    B = z.shape[0]
    e, fg, valid = errors_of(z, target, head, ids, per_image)
    S, P = e.shape
    perm = stable_order(e.detach().numpy(), valid.numpy()) if order is None else np.asarray(order).astype(np.int64)
    assert perm.shape == (S, P) and all(np.array_equal(np.sort(perm[s]), np.arange(P)) for s in range(S)), "not a permutation"
    fgn, vn = fg.numpy(), valid.numpy()
    counts = np.stack([vn.sum(1), (fgn & vn).sum(1)], 1).astype(np.int64)
    g = np.stack([coefficients(fgn[s][perm[s]], counts[s, 0]) for s in range(S)])
    w = weights(counts[:, 1], len(ids), B if per_image else 1, present)
    es = torch.gather(e, 1, torch.from_numpy(perm))
    if head == "sigmoid":
        es = torch.relu(es)
    loss = scale * (torch.from_numpy(w) * (es * torch.from_numpy(g)).sum(1)).sum()
    (loss * gscale).backward()
    return float(loss.detach()), z.grad.numpy(), counts, perm


# ---------------------------------------------------------------------------------------------------------------------- inputs
def inputs(B, C, H, W, head, seed=0, void=0.0, sat=1.0, integer=False):
    """fp32 logits [B, C, H, W] (N(0, 9) times `sat`, or small integers) and a uint8 target of the head's shape with a fraction `void`
    of void positions (255)."""
    rng = np.random.default_rng(seed)
    lg = rng.integers(-3, 4, (B, C, H, W)).astype(np.float32) if integer else (3.0 * sat * rng.standard_normal((B, C, H, W))).astype(np.float32)
    if head == "softmax":
        y = rng.integers(0, C, (B, H, W)).astype(np.uint8)
    else:
        y = rng.integers(0, 2, (B, C, H, W)).astype(np.uint8)
    if void:
        y[rng.random(y.shape) < void] = 255
    return lg, y

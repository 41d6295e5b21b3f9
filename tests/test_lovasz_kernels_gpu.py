"""GPU: the kernels of include/lovasz/lmnet_lovasz.h (lm_net_amd/csrc/lovasz.hip).

Sort: hip.lovasz_order on raw keys equals np.lexsort((index, key)) exactly, twice bit-identically, at lengths around the wave, the
block and the tile (hip.LOVASZ_TILE) and at one length with more tiles per segment than the scan block has threads, on key sets that
isolate stability, each digit and each digit boundary.
Ranks: lovasz_ranks -- errors against float64 (1e-6 absolute for the softmax head: fp32 expf and one division on values in [0, 1];
exact for the hinge on small integer logits; on continuous logits 1 - z s is one fp32 rounding of a value of size at most 1 + |z|,
half an ulp is 6e-8 (1 + |z|), so 1e-6 max(1, max |z|) is asserted), perm equal to the stable order of the device's OWN errors with void last, counts exact.
Loss and gradient: against tests/lovasz_ref.py loss_and_grad(..., order=device perm) in float64, with the bars of
tests/test_distmap_kernels_gpu.py: |L - ref| < 1e-5 |ref| (a sum of non-negative terms) and max |dlogits - ref| < 1e-4 max |ref|.
The reference is evaluated on the device's order because an fp32 and a float64 sort disagree on near-ties, and swapped ranks swap
coefficients; the order itself is pinned by the ranks tests."""
import numpy as np
import pytest
import torch

import lovasz_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


# ---------------------------------------------------------------------------------------------------------------------- the sort
def _key_sets(S, P, rng, full):
    idx = np.arange(P, dtype=np.uint64)
    one = lambda a: np.broadcast_to(np.asarray(a, dtype=np.uint64), (S, P))
    sets = {"equal": one(7), "full": rng.integers(0, 1 << 32, (S, P), dtype=np.uint64)}
    if full:
        sets["descending"] = one((P - 1 - idx) * 3 + 1)
        sets["two"] = np.where(rng.random((S, P)) < 0.5, 5, 0xF0000005).astype(np.uint64)
        for b in range(4):
            sets["byte%d" % b] = (rng.integers(0, 256, (S, P), dtype=np.uint64) << (8 * b)) | (0x01010101 & ~(0xFF << (8 * b)))
        for b in (6, 14, 22):
            sets["straddle%d" % b] = rng.integers(0, 16, (S, P), dtype=np.uint64) << b
    return {k: np.ascontiguousarray(v).astype(np.uint32) for k, v in sets.items()}


def _sort_lengths():
    from lm_net_amd import hip
    T = hip.LOVASZ_TILE
    return [1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17]


def _check_order(keys):
    from lm_net_amd import hip
    S, P = keys.shape
    k = torch.from_numpy(keys.view(np.int32)).to(DEV)
    ws = torch.empty(hip.lovasz_workspace(S, P), dtype=torch.uint8, device=DEV)
    out = []
    for _ in range(2):
        perm = torch.full((S, P), -1, dtype=torch.int32, device=DEV)
        hip.lovasz_order(k, ws, perm)
        out.append(perm)
    assert torch.equal(out[0], out[1])
    assert np.array_equal(k.cpu().numpy(), keys.view(np.int32))                  # keys is not modified
    idx = np.arange(P)
    want = np.stack([np.lexsort((idx, keys[s])) for s in range(S)])
    got = out[0].cpu().numpy()
    assert np.array_equal(got, want), "first difference at %s" % (np.argwhere(got != want)[:1].tolist(),)


@pytest.mark.parametrize("S", [1, 3, 17])
def test_order_equals_lexsort(S):
    rng = np.random.default_rng(S)
    for P in _sort_lengths():
        for name, keys in _key_sets(S, P, rng, full=True).items():
            try:
                _check_order(keys)
            except AssertionError as e:
                raise AssertionError("S=%d P=%d keys=%s: %s" % (S, P, name, e))


def test_order_more_tiles_than_scan_threads():
    """More tiles per segment than the scan block has threads (hip.LOVASZ_SCAN_THREADS): the wave walks its digit row in more than
    one chunk and carries the sum across; at 257 tiles the coefficient pass also sums more tile counts than its block has threads
    (test_more_tiles_than_coef_threads)."""
    from lm_net_amd import hip
    for nb in (hip.LOVASZ_SCAN_THREADS + 1, 2 * hip.LOVASZ_SCAN_THREADS + 2):
        P = (nb - 1) * hip.LOVASZ_TILE + 5
        assert (P + hip.LOVASZ_TILE - 1) // hip.LOVASZ_TILE == nb > hip.LOVASZ_SCAN_THREADS
        for name, keys in _key_sets(2, P, np.random.default_rng(nb), full=False).items():
            _check_order(keys)


# --------------------------------------------------------------------------------------------------------- ranks, loss, gradient
def _special(y, C, head, special):
    y = y.copy()
    if special == "void_image":
        y[0] = 255
    elif special == "absent":                              # class 1 / plane 1 has no foreground anywhere
        if head == "softmax":
            y[y == 1] = 0
        else:
            y[:, min(1, C - 1)][y[:, min(1, C - 1)] == 1] = 0
    elif special == "whole":                               # class 1 is the whole of image 0 / plane 0 is all foreground
        if head == "softmax":
            y[0] = 1
        else:
            y[0, 0] = 1
    return y


def _check(B, C, H, W, head, classes, per_image, void=0.2, special=None, sat=1.0, seed=1):
    from lm_net_amd import LovaszLoss, lovasz_ranks
    lg, y = R.inputs(B, C, H, W, head, seed=seed, void=void, sat=sat)
    y = _special(y, C, head, special)
    ids, present = R.class_ids(C, head, classes)
    zl, yt = torch.from_numpy(lg).to(DEV), torch.from_numpy(y).to(DEV)
    errors, perm, counts = lovasz_ranks(zl, yt, C, head, classes, per_image)
    e64, fg, valid = R.errors_of(torch.from_numpy(lg).double(), y, head, ids, per_image)
    e_dev = errors.cpu().numpy()
    assert e_dev.shape == tuple(e64.shape)
    print("max |errors - float64| = %.3e" % np.abs(e_dev - e64.numpy()).max())
    assert np.abs(e_dev - e64.numpy()).max() < (1e-6 if head == "softmax" else 1e-6 * max(1.0, float(np.abs(lg).max())))
    assert not e_dev[~valid.numpy()].any()
    assert np.array_equal(perm.cpu().numpy(), R.stable_order(e_dev, valid.numpy()))
    crit = LovaszLoss(C, head=head, classes=classes, per_image=per_image, scale=0.5)
    z = zl.clone().requires_grad_(True)
    loss = crit(z, yt)
    loss.backward()
    order = crit.ranks[1].cpu().numpy()
    assert np.array_equal(order, perm.cpu().numpy())
    want, wgrad, wcounts, _ = R.loss_and_grad(lg, y, C, head, classes, per_image, scale=0.5, order=order)
    assert np.array_equal(counts.cpu().numpy(), wcounts) and np.array_equal(crit.ranks[2].cpu().numpy(), wcounts)
    got, d = float(loss.detach()), z.grad.cpu().numpy().astype(np.float64)
    print("loss %.9g ref %.9g rel %.3e; grad max err %.3e of %.3e" % (got, want, abs(got - want) / max(abs(want), 1e-300),
                                                                      np.abs(d - wgrad).max(), np.abs(wgrad).max()))
    assert want > 0 and abs(got - want) < 1e-5 * abs(want)
    assert np.abs(d - wgrad).max() < 1e-4 * np.abs(wgrad).max()
    void_at = np.broadcast_to((y >= C)[:, None] if head == "softmax" else (y > 1), d.shape)
    g32 = z.grad.cpu().numpy().view(np.int32)
    assert not g32[void_at].any()                          # +0, no bit set, at every void position
    return wcounts


SHAPES = [(1, 2, 2, 2), (2, 3, 24, 40), (3, 9, 16, 17), (2, 2, 64, 96), (8, 2, 64, 96), (2, 3, 352, 352)]
CLASSES = ["present", "all", [1]]


@pytest.mark.parametrize("per_image", [False, True], ids=["batch", "image"])
@pytest.mark.parametrize("head", ["softmax", "sigmoid"])
@pytest.mark.parametrize("n,shape", list(enumerate(SHAPES)), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_loss_and_gradient(n, shape, head, per_image):
    B, C, H, W = shape
    _check(B, C, H, W, head, CLASSES[(n + per_image) % 3], per_image, seed=n)


def test_more_tiles_than_coef_threads():
    """8 x 1 x 256 x 257 per batch: one segment of 257 tiles, so a block of the coefficient pass (256 threads) sums the foreground
    counts of the tiles before it in more than one step per thread."""
    from lm_net_amd import hip
    assert (8 * 256 * 257 + hip.LOVASZ_TILE - 1) // hip.LOVASZ_TILE == 257
    _check(8, 1, 256, 257, "sigmoid", "all", False)


@pytest.mark.parametrize("per_image", [False, True], ids=["batch", "image"])
def test_one_logit_sigmoid(per_image):
    _check(2, 1, 24, 40, "sigmoid", "all", per_image)
    _check(1, 1, 2, 2, "sigmoid", "all", per_image, void=0.0)


@pytest.mark.parametrize("per_image", [False, True], ids=["batch", "image"])
@pytest.mark.parametrize("head", ["softmax", "sigmoid"])
@pytest.mark.parametrize("classes", ["present", "all"])
@pytest.mark.parametrize("special", ["void_image", "absent", "whole"])
def test_special_targets(special, classes, head, per_image):
    counts = _check(2, 3, 24, 40, head, classes, per_image, special=special)
    if special == "void_image" and per_image:
        assert not counts[:3].any()
    if special == "absent":
        assert (counts[:, 1] == 0).any()
    if special == "whole" and per_image:
        assert (counts[:, 0] == counts[:, 1]).any()


@pytest.mark.parametrize("head", ["softmax", "sigmoid"])
def test_saturated_logits(head):
    """Logits times 60: the softmax errors are 0 or 1 at most pixels, so the order is decided by the stability rule."""
    _check(2, 3, 24, 40, head, "present", False, sat=60.0)
    _check(2, 3, 24, 40, head, "all", True, sat=60.0)


def test_hinge_errors_exact_on_integer_logits():
    from lm_net_amd import lovasz_ranks
    lg, y = R.inputs(2, 3, 24, 40, "sigmoid", seed=2, void=0.2, integer=True)
    errors, perm, counts = lovasz_ranks(torch.from_numpy(lg).to(DEV), torch.from_numpy(y).to(DEV), 3, "sigmoid", "all", False)
    e64, fg, valid = R.errors_of(torch.from_numpy(lg).double(), y, "sigmoid", [0, 1, 2], False)
    assert np.array_equal(errors.cpu().numpy().astype(np.float64), e64.numpy())
    assert np.array_equal(perm.cpu().numpy(), R.stable_order(e64.numpy(), valid.numpy()))          # seven distinct errors: ties everywhere
    assert np.array_equal(counts.cpu().numpy(), np.stack([valid.numpy().sum(1), fg.numpy().sum(1)], 1))


def _run(crit, lg, y, gscale=None):
    z = torch.from_numpy(lg).to(DEV).requires_grad_(True)
    loss = crit(z, torch.from_numpy(y).to(DEV))
    if gscale is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(gscale, device=DEV))
    return loss.detach().clone(), z.grad.clone()


@pytest.mark.parametrize("head", ["softmax", "sigmoid"])
def test_bit_identical_in_both_deterministic_modes(head):
    from lm_net_amd import LovaszLoss, hip
    lg, y = R.inputs(2, 3, 64, 96, head, seed=4, void=0.2)
    crit = LovaszLoss(3, head=head, per_image=True)
    out = []
    try:
        for det in (False, True, False, True):
            hip.set_deterministic(det)
            out.append(_run(crit, lg, y))
    finally:
        hip.set_deterministic(False)
    for loss, grad in out[1:]:
        assert torch.equal(loss.view(torch.int32), out[0][0].view(torch.int32)) and torch.equal(grad.view(torch.int32), out[0][1].view(torch.int32))


@pytest.mark.parametrize("head", ["softmax", "sigmoid"])
def test_scale_and_gscale_by_powers_of_two_are_exact(head):
    from lm_net_amd import LovaszLoss
    lg, y = R.inputs(2, 3, 24, 40, head, seed=6, void=0.2)
    crit = LovaszLoss(3, head=head)
    l1, g1 = _run(crit, lg, y)
    crit.scale = 4.0                                       # a plain attribute read at every call
    l4, g4 = _run(crit, lg, y, gscale=0.5)
    assert float(l1) > 0 and torch.equal(l4, 4.0 * l1) and torch.equal(g4, 2.0 * g1)


@pytest.mark.parametrize("head,classes,per_image", [("softmax", "present", False), ("softmax", "all", True), ("sigmoid", "all", False)])
def test_zero_valid_is_exactly_zero(head, classes, per_image):
    from lm_net_amd import LovaszLoss
    lg, y = R.inputs(2, 3, 24, 40, head, seed=8)
    y[:] = 255
    loss, grad = _run(LovaszLoss(3, head=head, classes=classes, per_image=per_image), lg, y)
    assert loss.view(torch.int32).item() == 0 and not grad.view(torch.int32).any()

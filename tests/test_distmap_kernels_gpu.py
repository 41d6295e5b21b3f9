"""GPU: lmn_dist_map and the two losses on it (include/distmap/lmnet_distmap.h) against the restatement tests/distmap_ref.py.

The maps: sd2 and flags equal the restatement element for element, from labels (int64 and uint8) and from logits in both modes, at
37 x 45 and 36 x 44 (odd and even tails, W < 64), 130 x 67 (three 64-row groups, two column blocks), 2 x 2, and 1024 x 66 / 66 x 1024
(the side limit on each axis, sparse masks: the longest scans).  Every batch holds organ-like blobs, noise, a single corner pixel and
its complement, a one-pixel frame, a checkerboard, an empty plane, a full plane and a sample that is void everywhere
(distmap_ref.label_batch), at C = 2, 5 and 64 with a subset of the classes; two calls are bit-identical.

The losses: both terms under both heads against float64 on the same fp32 inputs, C in {1 (sigmoid), 2, 3, 5, 64}, with and without
20 % void labels, alpha in {2, 1, 2.5}, gradient scalars None and 0.37.  Tolerances -- those of tests/test_sigmoid_loss_gpu.py with
one derived change:
    max |dlogits - ref| < 1e-4 max |ref|;
    the Hausdorff term is a sum of non-negative terms: |L - ref| < 1e-5 |ref|;
    the boundary term is a signed sum that can cancel to near 0: |L - ref| < 1e-5 (1 / N) sum |p_k phi_k|, the same factor on the sum
    of magnitudes (the conditioning of the sum, from the restatement);
    a reference of exactly 0 must give exactly 0.
The gradient is bitwise +0 at void pixels; deterministic mode is bit-identical over two runs; precomputed maps= give the same bits."""
import functools

import numpy as np
import pytest
import torch

import distmap_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

SMALL = [(37, 45), (36, 44), (130, 67), (2, 2)]
BIG = [(1024, 66), (66, 1024)]
CLASSES = {2: [1], 5: [1, 3], 64: [1, 17, 63]}
MAP_CASES = [(s, C) for s in SMALL for C in (2, 5, 64)] + [(s, 2) for s in BIG]


@functools.lru_cache(maxsize=None)
def _map_case(shape, C):
    """(label map uint8, sd2, flags) of the restatement: computed once, shared by the four sources, never written."""
    y = R.label_batch(*shape, C, CLASSES[C], seed=C, sparse=shape in BIG)
    sd2, flags = R.maps(R.masks_of_labels(y, CLASSES[C]))
    for a in (y, sd2, flags):
        a.setflags(write=False)
    return y, sd2, flags


@pytest.mark.parametrize("source", ["int64", "uint8", "softmax", "sigmoid"])
@pytest.mark.parametrize("shape,C", MAP_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "C%d" % v)
def test_maps_equal_the_restatement(shape, C, source):
    from lm_net_amd import distance_maps
    y, want_sd2, want_flags = _map_case(shape, C)
    assert sorted(set(want_flags.ravel().tolist())) == [0, 1, 2] and want_flags[-1].tolist() == [1] * len(CLASSES[C])
    if source in ("int64", "uint8"):
        src = torch.from_numpy(y.astype(np.int64 if source == "int64" else np.uint8)).to(DEV)
        run = lambda: distance_maps(src, C, CLASSES[C])
    else:
        lg = R.logits_of_labels(y, C, source, seed=1)
        m, near = R.masks_of_logits(lg, source, CLASSES[C])
        assert near == 0 and np.array_equal(m, R.masks_of_labels(y, CLASSES[C]))       # (the inputs say what the labels say)
        src = torch.from_numpy(lg).to(DEV)
        run = lambda: distance_maps(src, C, CLASSES[C], mode=source)
    sd2, flags = run()
    again = run()
    torch.cuda.synchronize()
    assert sd2.dtype == torch.int32 and tuple(sd2.shape) == want_sd2.shape and tuple(flags.shape) == want_flags.shape
    assert np.array_equal(flags.cpu().numpy(), want_flags)
    got = sd2.cpu().numpy()
    bad = np.argwhere(got != want_sd2)
    assert bad.size == 0, (len(bad), bad[:5].tolist(), [int(got[tuple(i)]) for i in bad[:5]], [int(want_sd2[tuple(i)]) for i in bad[:5]])
    assert torch.equal(sd2, again[0]) and torch.equal(flags, again[1])                # two calls: the same bits


def test_default_classes_thresholds_and_the_channel_form():
    """classes=None is 1 .. C - 1; [B, 1, H, W] labels are accepted; a threshold other than 0.5 moves the mask."""
    from lm_net_amd import distance_maps
    y = R.label_batch(9, 13, 4, [1], seed=3)
    yt = torch.from_numpy(y).to(DEV)
    sd2, flags = distance_maps(yt[:, None], 4)
    want = R.maps(R.masks_of_labels(y, [1, 2, 3]))
    assert np.array_equal(sd2.cpu().numpy(), want[0]) and np.array_equal(flags.cpu().numpy(), want[1])
    rng = np.random.default_rng(0)
    lg = rng.standard_normal((2, 3, 9, 13)).astype(np.float32) * 2
    for mode in ("softmax", "sigmoid"):
        for thr in (0.3, 0.5, 0.8):
            m, near = R.masks_of_logits(lg, mode, [0, 2], thr)
            assert near == 0
            got = distance_maps(torch.from_numpy(lg).to(DEV), 3, [0, 2], mode=mode, threshold=thr)
            assert np.array_equal(got[0].cpu().numpy(), R.maps(m)[0]), (mode, thr)


# ---------------------------------------------------------------- the losses
HEADS = [("sigmoid", 1), ("softmax", 2), ("softmax", 3), ("sigmoid", 3), ("softmax", 5), ("softmax", 64)]
TERMS = [("boundary", 2.0), ("hausdorff", 2.0), ("hausdorff", 1.0), ("hausdorff", 2.5)]
B, H, W = 2, 37, 45


def _classes(C):
    return [1, 17, 63] if C == 64 else R.default_classes(C)


def _crit(head, C, term, alpha, scale=1.0):
    from lm_net_amd import BoundaryLoss, HausdorffDTLoss
    if term == "boundary":
        return BoundaryLoss(C, _classes(C), head=head, scale=scale)
    return HausdorffDTLoss(C, _classes(C), head=head, alpha=alpha, scale=scale)


def _run(crit, lg, y, gs, maps=None):
    """(loss fp32 tensor, dlogits) of one forward and backward through autograd."""
    z = lg.clone().requires_grad_(True)
    loss = crit(z, y, maps=maps)
    (loss if gs is None else loss * gs).backward()
    torch.cuda.synchronize()
    return loss.detach(), z.grad


def _check(loss, d, want, wgrad, mag, term):
    loss = float(loss)
    print("loss %.9g ref %.9g magnitude %.6g  max|d - ref| %.3g of max|ref| %.3g"
          % (loss, want, mag, np.abs(d - wgrad).max(), np.abs(wgrad).max()))
    if want == 0.0:
        assert loss == 0.0
    elif term == "boundary":
        assert abs(loss - want) < 1e-5 * mag, (loss, want, mag)
    else:
        assert abs(loss - want) < 1e-5 * abs(want), (loss, want)
    if not wgrad.any():
        assert not d.any()
    else:
        assert np.abs(d - wgrad).max() < 1e-4 * np.abs(wgrad).max()


@pytest.mark.parametrize("gs", [None, 0.37])
@pytest.mark.parametrize("term,alpha", TERMS, ids=lambda v: str(v))
@pytest.mark.parametrize("void", [False, True], ids=["dense", "void"])
@pytest.mark.parametrize("head,C", HEADS, ids=lambda v: str(v))
def test_losses_against_float64(head, C, void, term, alpha, gs):
    from lm_net_amd import hip
    lg_np, y_np = R.loss_inputs(B, C, H, W, head, seed=C, void=void)
    want, wgrad, n, mag, near = R.loss_and_grad(lg_np, y_np, head, term, _classes(C), alpha=alpha, scale=1.7, gscale=gs)
    assert near == 0 and n > 0 and (not void or n < B * len(_classes(C)) * H * W)
    lg, y = torch.from_numpy(lg_np).to(DEV), torch.from_numpy(y_np).to(DEV)
    crit = _crit(head, C, term, alpha, scale=1.7)
    loss, grad = _run(crit, lg, y, gs)                                  # ordinary mode: within the tolerances
    d = grad.cpu().numpy().astype(np.float64)
    _check(loss, d, want, wgrad, mag, term)
    assert tuple(crit.maps.shape) == (B, len(_classes(C)), H, W) and crit.maps.dtype == torch.int32
    assert np.array_equal(crit.maps.cpu().numpy(), R.maps(R.target_masks(y_np, head, _classes(C)))[0])
    # bitwise +0 at every void pixel / element (and in the planes of a sigmoid head that are not scored)
    bits = grad.view(torch.int32).cpu().numpy()
    if head == "softmax":
        dead = np.broadcast_to((y_np == R.VOID)[:, None], bits.shape)
    else:
        dead = (y_np.reshape(bits.shape) == R.VOID) | ~np.isin(np.arange(C), _classes(C))[None, :, None, None]
    assert (dead.any() or not void) and not bits[dead].any()
    # deterministic mode: the same bits over two runs, with precomputed maps too, and within the tolerances
    hip.set_deterministic(True)
    try:
        a = _run(crit, lg, y, gs)
        b = _run(crit, lg, y, gs)
        c = _run(crit, lg, y.long(), gs, maps=crit.target_maps(y))
    finally:
        hip.set_deterministic(False)
    for other in (b, c):
        assert torch.equal(a[0].view(torch.int32), other[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), other[1].view(torch.int32))
    _check(a[0], a[1].cpu().numpy().astype(np.float64), want, wgrad, mag, term)


@pytest.mark.parametrize("head,C", [("softmax", 3), ("softmax", 5), ("sigmoid", 3)], ids=lambda v: str(v))
def test_zero_references_give_exact_zeros(head, C):
    """No valid pixel: loss 0 and a gradient of +0 bits in both terms, never NaN.  Every target plane flagged: the boundary term is
    exactly 0 with a zero gradient (phi = 0 everywhere)."""
    lg_np, y_np = R.loss_inputs(B, C, H, W, head, seed=1)
    lg = torch.from_numpy(lg_np).to(DEV)
    void = torch.full(y_np.shape, R.VOID, dtype=torch.uint8, device=DEV)
    for term, alpha in TERMS[:3]:
        loss, grad = _run(_crit(head, C, term, alpha), lg, void, 0.37)
        assert float(loss) == 0.0 and not grad.view(torch.int32).any()
    for fill in (0, 1) if head == "sigmoid" else (0,):                 # empty planes; full planes under a sigmoid head
        flat = torch.full(y_np.shape, fill, dtype=torch.uint8, device=DEV)
        crit = _crit(head, C, "boundary", 2.0)
        loss, grad = _run(crit, lg, flat, None)
        want = R.loss_and_grad(lg_np, flat.cpu().numpy(), head, "boundary", _classes(C))
        assert want[0] == 0.0 and want[2] > 0 and float(loss) == 0.0 and not grad.any() and not crit.maps.any()


def test_direct_entries_gscale_none_and_scale_zero():
    """The wrapper's gscale=None is the factor 1 (the bits of autograd's ones); scale is a plain attribute read at every call."""
    from lm_net_amd import hip
    head, C, term = "softmax", 3, "hausdorff"
    lg_np, y_np = R.loss_inputs(B, C, H, W, head, seed=2, void=True)
    lg, y = torch.from_numpy(lg_np).to(DEV), torch.from_numpy(y_np).to(DEV)
    crit = _crit(head, C, term, 2.0)
    hip.set_deterministic(True)
    try:
        loss, grad = _run(crit, lg, y, None)
        sums = torch.empty(hip.DISTMAP_SUMS_WORDS, dtype=torch.int32, device=DEV)
        out = torch.empty(1, device=DEV)
        d = torch.empty_like(lg)
        hip.dist_loss_fwd(lg, y, hip.DISTMAP_SOFTMAX, hip.DISTMAP_HAUSDORFF, 2.0, 1.0, crit.class_mask, crit.maps, crit.pred_maps, sums, out)
        hip.dist_loss_bwd(lg, y, hip.DISTMAP_SOFTMAX, hip.DISTMAP_HAUSDORFF, 2.0, crit.class_mask, crit.maps, crit.pred_maps, sums, None, d)
        torch.cuda.synchronize()
        assert torch.equal(out[0].view(torch.int32), loss.view(torch.int32)) and torch.equal(d.view(torch.int32), grad.view(torch.int32))
        crit.scale = 0.25
        quarter, gq = _run(crit, lg, y, None)
        assert float(quarter) == 0.25 * float(loss) and torch.equal(gq * 4, grad)          # (a power of two: exact)
        crit.scale = 0.0
        zero, gz = _run(crit, lg, y, None)
        assert float(zero) == 0.0 and not gz.any()
    finally:
        hip.set_deterministic(False)
    assert np.array_equal(crit.pred_maps.cpu().numpy(), R.prediction_maps(lg_np, head, _classes(C))[0])

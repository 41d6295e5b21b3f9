"""CPU: the host side of the distance maps and their losses (include/distmap/lmnet_distmap.h; lm_net_amd.loss.distance_maps,
BoundaryLoss, HausdorffDTLoss): registry and header agree, the argument checks of the C
entries (rejected before any HIP call, with fake device pointers), the workspace formula, the classes' ValueErrors, the restatement
tests/distmap_ref.py against scipy.ndimage.distance_transform_edt, brute force and hand-computed planes, its gradients against
finite differences, and the conditions the GPU tests rest on.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import distmap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_ENTRIES = ["lmn_dist_map", "lmn_dist_loss_fwd", "lmn_dist_loss_bwd"]


# ---------------------------------------------------------------- ABI
def test_registry_and_header_agree():
    """The feature's own part of the registry: the literal list, its place in hip.HEADERS, the number of #defines, the header's
    citations and the package's exports.  (Header / export / layout / return-type / constants checks: tests/test_host_cpu.py.)"""
    from lm_net_amd import hip
    assert hip.SYMBOLS_DISTMAP == ["lmn_dist_workspace"] + DEVICE_ENTRIES
    assert hip.HEADERS["distmap/lmnet_distmap.h"] is hip.SYMBOLS_DISTMAP
    header = open(os.path.join(ROOT, "include", "distmap", "lmnet_distmap.h")).read()
    assert len(re.findall(r"^#define LMN_DISTMAP_\w+ \d+\b", header, re.M)) == 10
    assert (hip.DISTMAP_MAX_SIDE, hip.DISTMAP_FLAG_EMPTY, hip.DISTMAP_FLAG_FULL, hip.DISTMAP_SUMS_WORDS) == (1024, 1, 2, 4)
    for cite in ("SIGNED SQUARED", "THE PLANE IS ALL 0", "posmask.any()", "one_hot2dist", "rint((edt(M) + edt(~M))^2) == |sd2|",
                 "never NaN", "is not pinned", "dist_map: ", "dist_loss_fwd: ", "dist_loss_bwd: ", "at most W - 1 steps"):
        assert cite in header, cite
    import lm_net_amd
    from lm_net_amd import loss
    for name in ("BoundaryLoss", "HausdorffDTLoss", "distance_maps"):
        assert getattr(lm_net_amd, name) is getattr(loss, name) and name in lm_net_amd.__all__
    for doc in (loss.BoundaryLoss.__doc__, loss.distance_maps.__doc__):
        assert "Deliberate difference" in doc


# ---------------------------------------------------------------- argument checks
FAKE = ctypes.c_void_p(0x1000)


def _map(null=(), logits=False, **kw):
    """lmn_dist_map with fake device pointers: every case here must be rejected before any HIP call."""
    from lm_net_amd import hip
    lib = hip.load()
    a = dict(logits=FAKE if logits else None, labels=None if logits else FAKE, workspace=FAKE, sd2=FAKE, flags=FAKE)
    for k in null:
        a[k] = None
    g = dict(dict(kind=1, thr=0.5, mode=0, B=3, C=4, H=33, W=65, class_mask=0b1110, ws_bytes=1 << 40), **kw)
    rc = lib.lmn_dist_map(a["logits"], a["labels"], g["kind"], ctypes.c_float(g["thr"]), g["mode"], g["B"], g["C"], g["H"], g["W"],
                          ctypes.c_uint64(g["class_mask"]), a["workspace"], ctypes.c_int64(g["ws_bytes"]), a["sd2"], a["flags"], None)
    return rc, lib.lmn_last_error().decode()


def test_dist_map_rejects_bad_arguments():
    from lm_net_amd import hip
    for name in ("workspace", "sd2", "flags"):
        rc, err = _map(null=(name,))
        assert rc == -1 and err == "dist_map: null pointer", (name, err)
    rc, err = _map(null=("labels",))                                  # neither source
    assert rc == -1 and err == "dist_map: exactly one of logits, labels required", err
    lib = hip.load()
    rc = lib.lmn_dist_map(FAKE, FAKE, 1, ctypes.c_float(0.5), 0, 3, 4, 33, 65, ctypes.c_uint64(2), FAKE, ctypes.c_int64(1 << 40), FAKE, FAKE, None)
    assert rc == -1 and lib.lmn_last_error().decode() == "dist_map: exactly one of logits, labels required"          # both
    for kw, msg in ((dict(B=0), "B=0 < 1"), (dict(C=0, class_mask=1), "C=0 not in [1, 64]"), (dict(C=65), "C=65"),
                    (dict(H=1), "size 1x65 outside [2, 1024]"), (dict(H=1025), "size 1025x65"), (dict(W=1), "size 33x1 outside"),
                    (dict(W=1025), "size 33x1025"), (dict(class_mask=0), "class_mask is empty"), (dict(class_mask=0b10010), "a class >= C=4"),
                    (dict(kind=2), "unknown label kind 2"), (dict(B=2048, H=1024, W=1024, class_mask=2), "not below 2^31"),
                    (dict(ws_bytes=1000), "workspace of 1000 bytes too small")):
        rc, err = _map(**kw)
        assert rc == -1 and msg in err and err.startswith("dist_map: "), (kw, err)
    for kw, msg in ((dict(mode=2), "unknown mode 2"), (dict(thr=float("nan")), "threshold is NaN"),
                    (dict(C=1, class_mask=1, mode=hip.DISTMAP_SOFTMAX), "C=1 needs a sigmoid head")):
        rc, err = _map(logits=True, **kw)
        assert rc == -1 and msg in err and err.startswith("dist_map: "), (kw, err)
    # the bounds themselves pass: the last check, of the workspace, is reached (C = 1 is fine from labels and under a sigmoid)
    for kw in (dict(B=2047, C=64, H=1024, W=1024, class_mask=1 << 63), dict(B=1, C=1, H=2, W=2, class_mask=1),
               dict(B=1, C=1, H=2, W=2, class_mask=1, logits=True, mode=hip.DISTMAP_SIGMOID)):
        need = hip.dist_workspace(kw["B"], 1, kw["H"], kw["W"])
        rc, err = _map(ws_bytes=need - 1, **kw)
        assert rc == -1 and "workspace of %d bytes too small, %d needed" % (need - 1, need) in err, err


LOSS_POINTERS = ("logits", "target", "sd2_g", "sd2_p", "sums", "out")


def _loss(which, null=(), **kw):
    """lmn_dist_loss_fwd / _bwd with fake device pointers."""
    from lm_net_amd import hip
    lib = hip.load()
    a = {k: FAKE for k in LOSS_POINTERS}
    g = dict(dict(kind=1, head=0, term=1, alpha=2.0, scale=1.0, B=3, C=4, H=33, W=65, class_mask=0b1110), **kw)
    if g["term"] == 0:
        a["sd2_p"] = None
    for k in null:
        a[k] = None if a[k] is not None else FAKE
    cm = ctypes.c_uint64(g["class_mask"])
    if which == "fwd":
        rc = lib.lmn_dist_loss_fwd(a["logits"], a["target"], g["kind"], g["head"], g["term"], ctypes.c_float(g["alpha"]),
                                   ctypes.c_float(g["scale"]), g["B"], g["C"], g["H"], g["W"], cm, a["sd2_g"], a["sd2_p"], a["sums"], a["out"], None)
    else:
        rc = lib.lmn_dist_loss_bwd(a["logits"], a["target"], g["kind"], g["head"], g["term"], ctypes.c_float(g["alpha"]), g["B"], g["C"],
                                   g["H"], g["W"], cm, a["sd2_g"], a["sd2_p"], a["sums"], None, a["out"], None)
    return rc, lib.lmn_last_error().decode()


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_loss_entries_reject_bad_arguments(which):
    pre = "dist_loss_%s: " % which
    for name in ("logits", "target", "sd2_g", "sums", "out"):
        rc, err = _loss(which, null=(name,))
        assert rc == -1 and err == pre + "null pointer", (name, err)
    for term in (0, 1):                                               # sd2_p with the boundary term, none with the Hausdorff term
        rc, err = _loss(which, null=("sd2_p",), term=term)
        assert rc == -1 and err == pre + "sd2_p goes with the Hausdorff term and only with it", err
    cases = [(dict(head=2), "unknown head 2"), (dict(term=2), "unknown term 2"), (dict(B=0), "B=0 < 1"), (dict(C=65), "C=65 not in [1, 64]"),
             (dict(C=1, class_mask=1), "C=1 needs a sigmoid head"), (dict(H=1), "size 1x65"), (dict(W=1025), "size 33x1025"),
             (dict(class_mask=0), "class_mask is empty"), (dict(class_mask=1 << 4), "a class >= C=4"), (dict(kind=7), "unknown label kind 7"),
             (dict(B=600, C=4, H=1024, W=1024, class_mask=2), "B * C * H * W"), (dict(alpha=0.0), "alpha=0 not in (0, 8]"),
             (dict(alpha=-1.0), "alpha=-1"), (dict(alpha=9.0), "alpha=9"), (dict(alpha=float("nan")), "alpha=nan")]
    if which == "fwd":
        cases += [(dict(scale=float("inf")), "scale=inf is not finite"), (dict(scale=float("nan")), "is not finite")]
    for kw, msg in cases:
        rc, err = _loss(which, **kw)
        assert rc == -1 and msg in err and err.startswith(pre), (kw, err)
    rc, err = _loss(which, term=0, alpha=-5.0, head=2)                # (alpha is not read by the boundary term: the head is what fails)
    assert "unknown head" in err


def test_workspace_is_host_arithmetic():
    from lm_net_amd import hip
    up = lambda v: (v + 255) // 256 * 256
    for B, nk, H, W in ((1, 1, 2, 2), (2, 3, 37, 45), (8, 1, 352, 352), (8, 8, 352, 352), (1, 64, 1024, 1024), (2047, 1, 1024, 1024)):
        n = B * nk
        assert hip.dist_workspace(B, nk, H, W) == up(n * H * W) + up(2 * n * H * W) + up(4 * n)
    assert hip.dist_workspace(1, 1, 2, 2) == 768
    for args, msg in (((0, 1, 8, 8), "B=0"), ((1, 0, 8, 8), "nk=0"), ((1, 65, 8, 8), "nk=65"), ((1, 1, 1, 8), "1x8"), ((1, 1, 8, 1025), "8x1025"),
                      ((2048, 1, 1024, 1024), "B=2048")):
        with pytest.raises(ValueError, match="dist_workspace"):
            hip.dist_workspace(*args)
        assert msg in hip.load().lmn_last_error().decode()


def test_python_refuses_what_it_cannot_run():
    """The family's own rules; what it shares with the other criteria (class count, class list, head, logits, target, scale, "no CPU
    fallback") is in tests/test_criteria_cpu.py."""
    from lm_net_amd import BoundaryLoss, HausdorffDTLoss, distance_maps
    y = torch.zeros(2, 8, 9, dtype=torch.int64)
    z = torch.zeros(2, 3, 8, 9)
    for args, kw, msg in (((y, 3), dict(mode="argmax"), "mode"), ((y.float(), 3), {}, "label map"), ((y[0], 3), {}, "label map"),
                          ((z, 3), dict(mode="softmax", threshold=1.0), "threshold"), ((z, 4), dict(mode="softmax"), "logits"),
                          ((y, 3), dict(mode="sigmoid"), "logits"), ((z[:, :1], 1), dict(mode="softmax"), "n_classes >= 2"),
                          ((torch.zeros(2, 1, 9, dtype=torch.int64), 3), {}, "2 <= H, W <= 1024"),
                          ((torch.zeros(1, 4, 1025, dtype=torch.uint8), 3), {}, "2 <= H, W <= 1024")):
        with pytest.raises(ValueError, match=msg):
            distance_maps(*args, **kw)
    for cls in (BoundaryLoss, HausdorffDTLoss):
        c = cls(3)
        assert c.classes == [1, 2] and c.class_mask == 0b110 and c.scale == 1.0 and c.maps is None
        assert cls(1, head="sigmoid").classes == [0] and cls(9, classes=[5, 2]).classes == [2, 5]
        with pytest.raises(ValueError, match="2 <= H, W <= 1024"):
            c(torch.zeros(2, 3, 1, 9), torch.zeros(2, 1, 9, dtype=torch.int64))
    for alpha in (0.0, -2.0, 8.5):
        with pytest.raises(ValueError, match=r"alpha = .* outside the limit \(0, 8\]"):
            HausdorffDTLoss(3, alpha=alpha)
    assert HausdorffDTLoss(3, alpha=1).alpha == 1.0 and HausdorffDTLoss(2).alpha == 2.0


# ---------------------------------------------------------------- the restatement
SHAPES = [(2, 2), (9, 13), (37, 45), (36, 44)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_against_scipy(shape):
    """On ordinary masks rint((edt(M) + edt(~M))^2) == |sd2| with the sign of the membership, and phi is Kervadec's one_hot2dist on
    scipy's transforms, exactly."""
    ndi = pytest.importorskip("scipy.ndimage")
    seen = 0
    for seed in (0, 1):
        for kind, M in R.planes(*shape, seed=seed).items():
            if R.flag_of(M):
                continue
            pos, neg = ndi.distance_transform_edt(M), ndi.distance_transform_edt(~M)
            sd2 = R.sd2_plane(M)
            assert np.array_equal(np.rint((pos + neg) ** 2).astype(np.int64), np.abs(sd2)), kind
            assert np.array_equal(sd2 < 0, M) and not (sd2 == 0).any(), kind
            assert np.array_equal(R.phi(sd2), neg * ~M - (pos - 1) * M), kind         # one_hot2dist
            seen += 1
    assert seen == 2 * (len(R.KINDS) - 2)


def test_restatement_against_brute_force_and_by_hand():
    for shape in ((2, 2), (5, 7), (9, 13)):
        for kind, M in R.planes(*shape, seed=3).items():
            assert np.array_equal(R.sd2_plane(M), R.sd2_brute(M)), (shape, kind)
    # the flagged-plane rule
    for M, f in ((np.zeros((4, 5), bool), 1), (np.ones((4, 5), bool), 2)):
        assert R.flag_of(M) == f and not R.sd2_plane(M).any() and not R.phi(R.sd2_plane(M)).any()
    # by hand: one pixel at (1, 1) of 3 x 4
    M = np.zeros((3, 4), bool)
    M[1, 1] = True
    assert R.sd2_plane(M).tolist() == [[2, 1, 2, 5], [1, -1, 1, 4], [2, 1, 2, 5]]
    assert R.phi(R.sd2_plane(M))[1].tolist() == [1.0, 0.0, 1.0, 2.0]                  # -(sqrt(1) - 1) = 0 on the border of the mask
    # its complement: the mask pixels look at the one hole
    assert R.sd2_plane(~M).tolist() == [[-2, -1, -2, -5], [-1, 1, -1, -4], [-2, -1, -2, -5]]
    sd2, flags = R.maps(np.stack([M, ~M, np.zeros_like(M), np.ones_like(M)])[None])
    assert flags.tolist() == [[0, 0, 1, 2]] and sd2.shape == (1, 4, 3, 4) and sd2.dtype == np.int32
    # the largest value the format has to hold: the corner pixel of a 1024 x 1024 plane
    assert 2 * 1023 ** 2 < 2 ** 24 and np.float32(2 * 1023 ** 2) == 2 * 1023 ** 2


def test_masks_of_labels_and_logits():
    y = R.label_batch(9, 13, 5, [1, 3], seed=0)
    m = R.masks_of_labels(y, [1, 3])
    assert m.shape == (len(R.KINDS) + 1, 2, 9, 13) and not m[-1].any()               # the void sample belongs to no class
    for b, (kind, M) in enumerate(R.planes(9, 13, seed=0).items()):
        assert np.array_equal(m[b, 0], M), kind                                       # every kind, as the first scored class
    for C, classes in ((2, [1]), (5, [1, 3]), (64, [1, 17, 63])):
        y = R.label_batch(9, 13, C, classes, seed=1)
        want = R.masks_of_labels(y, classes)
        for mode in ("softmax", "sigmoid"):
            got, near = R.masks_of_logits(R.logits_of_labels(y, C, mode), mode, classes)
            assert near == 0 and np.array_equal(got, want), (C, mode)
    # the threshold and the margin counter
    z = np.zeros((1, 2, 2, 2), np.float32)
    assert R.masks_of_logits(z, "softmax", [1])[1] == 4 and not R.masks_of_logits(z, "softmax", [1])[0].any()
    assert not R.masks_of_logits(z, "sigmoid", [1])[0].any()                          # z > 0 is strict


GRAD_CASES = [("softmax", "boundary", 3, [1, 2], 2.0), ("softmax", "hausdorff", 3, [2], 2.0), ("softmax", "hausdorff", 5, [1, 3], 1.0),
              ("sigmoid", "boundary", 1, [0], 2.0), ("sigmoid", "hausdorff", 3, [0, 2], 2.5)]


@pytest.mark.parametrize("head,term,C,classes,alpha", GRAD_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_restatement_gradients_against_finite_differences(head, term, C, classes, alpha):
    lg, y = R.loss_inputs(2, C, 6, 7, head, seed=4, void=True)
    val, grad, n, mag, near = R.loss_and_grad(lg, y, head, term, classes, alpha=alpha, scale=0.7, gscale=0.37)
    assert near == 0 and n > 0 and mag > 0 and grad.shape == lg.shape
    sd2_g = R.maps(R.target_masks(y, head, classes))[0]
    sd2_p = None if term == "boundary" else R.prediction_maps(lg, head, classes)[0]

    def f(z):
        return float(R.loss(torch.as_tensor(z), y, head, term, classes, sd2_g, sd2_p, alpha, 0.7)[0])
    z0 = lg.astype(np.float64)
    assert abs(f(z0) - val) < 1e-15
    rng = np.random.default_rng(0)
    h = 1e-6
    for _ in range(12):
        i = tuple(rng.integers(0, s) for s in lg.shape)
        zp, zm = z0.copy(), z0.copy()
        zp[i] += h
        zm[i] -= h
        fd = 0.37 * (f(zp) - f(zm)) / (2 * h)
        assert abs(fd - grad[i]) < 1e-7 * max(1.0, np.abs(grad).max()), (i, fd, grad[i])
    # void pixels / elements carry no gradient
    if head == "softmax":
        assert not grad[np.broadcast_to((y == R.VOID)[:, None], grad.shape)].any()
    else:
        assert not grad[y == R.VOID].any()


def test_restatement_edge_cases():
    """No valid pixel: 0, gradient 0.  Every plane flagged: the boundary term is exactly 0."""
    lg, y = R.loss_inputs(2, 3, 6, 7, "softmax", seed=1)
    void = np.full_like(y, R.VOID)
    for term in ("boundary", "hausdorff"):
        val, grad, n, mag, near = R.loss_and_grad(lg, void, "softmax", term, [1, 2])
        assert val == 0.0 and n == 0 and not grad.any()
    val, grad, n, mag, near = R.loss_and_grad(lg, np.zeros_like(y), "softmax", "boundary", [1, 2])       # both target planes empty
    assert val == 0.0 and n == 2 * y.size and not grad.any()
    # the scale is a factor, gscale another
    a = R.loss_and_grad(lg, y, "softmax", "hausdorff", [1], scale=1.0)
    b = R.loss_and_grad(lg, y, "softmax", "hausdorff", [1], scale=3.0, gscale=0.5)
    assert abs(b[0] - 3 * a[0]) < 1e-12 * abs(a[0]) and np.allclose(b[1], 1.5 * a[1], rtol=1e-12, atol=0)


def test_generators_hold_what_the_gpu_tests_name():
    for shape, sparse in (((37, 45), False), ((2, 2), False), ((130, 67), False), ((66, 1024), True)):
        p = R.planes(*shape, seed=0, sparse=sparse)
        assert tuple(p) == R.KINDS
        assert [R.flag_of(m) for m in p.values()] == [0, 0, 0, 0, 0, 0, 1, 2], shape
        assert p["corner"].sum() == 1 and (~p["corner_complement"]).sum() == 1
        if min(shape) > 2:
            assert p["frame"].sum() == 2 * sum(shape) - 4 and p["frame"][0].all() and p["frame"][:, -1].all()
        if sparse:
            assert 1 <= p["noise"].sum() <= 64
    lg, y = R.loss_inputs(2, 64, 37, 45, "softmax", seed=0, void=True)
    assert set(range(64)) <= set(np.unique(y).tolist()) and 0.15 < (y == R.VOID).mean() < 0.25
    lg, y = R.loss_inputs(2, 3, 37, 45, "sigmoid", seed=0, void=True)
    assert y.shape == (2, 3, 37, 45) and set(np.unique(y).tolist()) == {0, 1, R.VOID}

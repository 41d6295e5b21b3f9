"""The subjects of the busy-stream tests (tests/busy.py): for every public class or function under test three valid, in-range inputs
A, B, C of one geometry and the float64 / integer reference of each, from the families' own restatements (tests/*_ref.py).
Importable without a GPU: tests/test_busy_cpu.py asserts on these alone that the three references of every compared output differ
by 100 tolerances (exact outputs: in at least half of their elements), the precondition of the stream-order assertion.

The bounds are the ones the families' kernel tests hold the same outputs to.  Those tests write them as literals, so they are named
here once, each with the line it restates:
  LOSS_BAR  1e-5  |L - ref| < 1e-5 |ref|            test_void_loss_gpu, test_sigmoid_loss_gpu, test_distmap_kernels_gpu (boundary:
                                                    of the magnitude (1 / N) sum |terms|), test_lovasz_kernels_gpu, test_region_kernels_gpu
  GRAD_BAR  1e-4  max |d - ref| < 1e-4 max |ref|    the same five files
  SUMS_BAR  1e-5  of max |ref|                      test_region_kernels_gpu (region_sums)
  ERR_BAR   1e-6  (times max(1, max |z|), hinge)    test_lovasz_kernels_gpu (errors)
  F64_BAR   1e-9  times max(1, |ref|), per element  test_surface_gpu, test_volume_kernels_gpu (the float64 sums)
Everything else is integer arithmetic and must be EQUAL.  The geometries are the smallest the kernel tests use that still span more
than one block and more than one launch: B = 2, 4 classes, 48 x 64 for the 2D criteria and meters, 8 x 16 x 24 for the 3D ones."""
import functools

import numpy as np
import torch

from busy import Subject

LOSS_BAR, GRAD_BAR, SUMS_BAR, ERR_BAR, F64_BAR = 1e-5, 1e-4, 1e-5, 1e-6, 1e-9
B, C, H, W = 2, 4, 48, 64
D3, H3, W3 = 8, 16, 24
VOID = 255
CASES = ("A", "B", "C")
_SEED = {"A": 11, "B": 22, "C": 33}
_SCALE = {"A": 1.0, "B": 2.0, "C": 3.5}                          # logits of three scales: losses and gradients far apart
_PROBS = {"A": (1, 1, 1, 1), "B": (1, 2, 3, 6), "C": (6, 1, 3, 2)}   # class frequencies: every integer count differs
_VOID = {"A": 0.1, "B": 0.2, "C": 0.3}


def _rng(case, salt):
    return np.random.default_rng([_SEED[case], salt])


def logits(case, n=C, shape=None):
    return (_SCALE[case] * _rng(case, 1).standard_normal(shape or (B, n, H, W))).astype(np.float32)


def label_map(case, void=False, dtype=np.int64, shape=(B, H, W), n=C):
    rng = _rng(case, 2)
    p = np.asarray(_PROBS[case][:n], np.float64)
    y = rng.choice(n, size=shape, p=p / p.sum())
    if void:
        y[rng.random(shape) < _VOID[case]] = VOID
    return y.astype(dtype)


def planes(case, void=False, dtype=np.uint8, n=C):
    """sigmoid-head target planes [B, n, H, W] in {0, 1} (255: void)"""
    rng = _rng(case, 3)
    y = (rng.random((B, n, H, W)) < 0.2 + 0.1 * _PROBS[case][0]).astype(np.int64)
    if void:
        y[rng.random(y.shape) < _VOID[case]] = VOID
    return y.astype(dtype)


def _abs(a):
    return float(np.abs(np.asarray(a, np.float64)).max())


def _loss_grad(loss, grad, loss_scale=None):
    grad = np.asarray(grad, np.float64)
    return [("loss", np.float64(loss), LOSS_BAR * (abs(loss) if loss_scale is None else loss_scale)), ("dlogits", grad, GRAD_BAR * _abs(grad))]


def _subject(name, make, ref, **kw):
    return Subject(name, {k: make(k) for k in CASES}, ref, **kw)


# ------------------------------------------------------------------------------------------------------------------------ criteria
W_CE, W_DICE = (1.0, 2.0, 0.5, 1.5), (1.0, 0.5, 2.0, 1.5)
SEG_EXT = dict(ignore_index=VOID, focal_scale=0.5, focal_gamma=1.5, label_smoothing=1e-3)


def _seg_ref(wce, wdice, **kw):
    import void_ref as V

    def ref(arrays, got=None):
        lg, y = arrays
        terms, grad = V.loss_and_grad(torch.from_numpy(lg), torch.from_numpy(y), torch.tensor(wce), torch.tensor(wdice), **kw)
        return _loss_grad(terms[0], grad.numpy())
    return ref


def seg_default():
    return _subject("SegLoss", lambda k: [logits(k), label_map(k)], _seg_ref(W_CE, W_DICE))


def seg_extended():
    return _subject("SegLoss-extended", lambda k: [logits(k), label_map(k, void=True)],
                    _seg_ref(W_CE, W_DICE, eps=1e-3, ignore_index=VOID, focal_scale=0.5, gamma=1.5))


def focal():
    return _subject("FocalLoss", lambda k: [logits(k), label_map(k, void=True)],
                    _seg_ref((1.0,) * C, (1.0,) * C, ignore_index=VOID, ce_scale=0.0, dice_scale=0.0, focal_scale=1.0))


def sigmoid_seg():
    import sigmoid_ref as S

    def ref(arrays, got=None):
        lg, t = arrays
        terms, grad = S.loss_and_grad(torch.from_numpy(lg), torch.from_numpy(t.astype(np.int64)))
        return _loss_grad(terms[0], grad.numpy())
    return _subject("SigmoidSegLoss", lambda k: [logits(k), planes(k, void=True)], ref)


DIST_CLASSES = [1, 2, 3]


def dist_loss(term):
    """BoundaryLoss / HausdorffDTLoss(alpha=2) under a softmax head, the maps from target_maps"""
    import distmap_ref as D

    def ref(arrays, got=None):
        lg, y = arrays
        loss, grad, n, mag, near = D.loss_and_grad(lg, y, "softmax", term, DIST_CLASSES)
        assert near == 0 and n > 0, "a prediction within 1e-6 of the threshold: choose another seed"
        return _loss_grad(loss, grad, mag if term == "boundary" else None)
    return _subject({"boundary": "BoundaryLoss", "hausdorff": "HausdorffDTLoss"}[term], lambda k: [logits(k), label_map(k, void=True, dtype=np.uint8)], ref)


# which classes occur in which image: every (image, class) plane is ordinary (O) or empty (E); between any two cases at least three of
# the six planes change kind, so flags differ in half of its elements and sd2 (all 0 on an empty plane) in more
_DIST_SETS = {"A": ((0, 1, 2, 3), (0, 1, 2)), "B": ((0, 1, 3), (0, 2, 3)), "C": ((0, 2), (0, 1, 3))}


def distance_maps():
    import distmap_ref as D

    def make(k):
        rng = _rng(k, 4)
        return [np.stack([np.asarray(s)[rng.integers(0, len(s), (H, W))] for s in _DIST_SETS[k]]).astype(np.uint8)]

    def ref(arrays, got=None):
        sd2, flags = D.maps(D.masks_of_labels(arrays[0], DIST_CLASSES))
        return [("sd2", sd2.astype(np.int32), None), ("flags", flags.astype(np.int32), None)]
    return _subject("distance_maps", make, ref, exact=True)


def lovasz(head, per_image, ranks_only=False):
    """LovaszLoss: loss, dlogits, errors, perm.  The loss is linear in the errors on ONE order, so the reference is evaluated on the
    device's own order (tests/lovasz_ref.py), and that order is held to the stable order of the device's errors.  lovasz_ranks:
    errors, perm, counts."""
    import lovasz_ref as R

    def make(k):
        return [logits(k), label_map(k, void=True, dtype=np.uint8) if head == "softmax" else planes(k, void=True)]

    def ref(arrays, got=None):
        lg, y = arrays
        ids, _ = R.class_ids(C, head, "present")
        e64, _, valid = R.errors_of(torch.from_numpy(lg).double(), y, head, ids, per_image)
        e64, valid = e64.numpy(), valid.numpy()
        e_bar = ERR_BAR * (1.0 if head == "softmax" else max(1.0, _abs(lg)))
        if ranks_only:
            order = R.stable_order(e64 if got is None else got[0], valid)
            counts = R.loss_and_grad(lg, y, C, head, "present", per_image, order=order)[2]
            return [("errors", e64, e_bar), ("perm", order.astype(np.int32), None), ("counts", counts.astype(np.int32), None)]
        order = R.stable_order(e64 if got is None else got[2], valid)
        loss, grad, _, _ = R.loss_and_grad(lg, y, C, head, "present", per_image, scale=0.5, order=order if got is None else got[3])
        return _loss_grad(loss, grad) + [("errors", e64, e_bar), ("perm", order.astype(np.int32), None)]
    name = "%s-%s%s" % ("lovasz_ranks" if ranks_only else "LovaszLoss", head, "-per_image" if per_image else "")
    return _subject(name, make, ref, exact=True, no_growth=not ranks_only)


REGION_KINDS = {"dice": {}, "jaccard": {"denominator": "linear"}, "tversky": {"alpha": 0.3, "beta": 0.7, "exponent": 0.75},
                "generalized_dice": {}}


def region(kind, per_image):
    import region_ref as R
    kw = dict(kind=kind, per_image=per_image, **REGION_KINDS[kind])

    def ref(arrays, got=None):
        r = R.loss_and_grad(arrays[0], arrays[1], C, **kw)
        return _loss_grad(r.loss, r.grad)
    return _subject("RegionLoss-%s%s" % (kind, "-per_image" if per_image else ""), lambda k: [logits(k), label_map(k, void=True, dtype=np.uint8)],
                    ref, no_growth=True)


def region_sums():
    import region_ref as R

    def ref(arrays, got=None):
        r = R.loss_and_grad(arrays[0], arrays[1], C, per_image=True)
        return [("sums", r.sums, SUMS_BAR * _abs(r.sums)), ("counts", r.counts, None)]
    return _subject("region_sums", lambda k: [logits(k), label_map(k, void=True, dtype=np.uint8)], ref)


def loss_subjects():
    out = [seg_default(), seg_extended(), focal(), sigmoid_seg(), dist_loss("boundary"), dist_loss("hausdorff"), distance_maps()]
    out += [lovasz(h, p) for h in ("softmax", "sigmoid") for p in (False, True)]
    out += [region(k, p) for k in REGION_KINDS for p in (False, True)]
    out += [lovasz("softmax", True, ranks_only=True), region_sums()]
    return out


LOSS_NAMES = ["SegLoss", "SegLoss-extended", "FocalLoss", "SigmoidSegLoss", "BoundaryLoss", "HausdorffDTLoss", "distance_maps",
              "LovaszLoss-softmax", "LovaszLoss-softmax-per_image", "LovaszLoss-sigmoid", "LovaszLoss-sigmoid-per_image",
              "RegionLoss-dice", "RegionLoss-dice-per_image", "RegionLoss-jaccard", "RegionLoss-jaccard-per_image", "RegionLoss-tversky",
              "RegionLoss-tversky-per_image", "RegionLoss-generalized_dice", "RegionLoss-generalized_dice-per_image",
              "lovasz_ranks-softmax-per_image", "region_sums"]


# ------------------------------------------------------------------------------------------------------------------------ meters
def organ_map(case, salt, shape=(B, H, W)):
    """int64 label maps: one random ellipse per class 1 .. C - 1 and image, so that areas, borders and distances differ from case
    to case"""
    rng = _rng(case, salt)
    n, h, w = shape
    yy, xx = np.mgrid[:h, :w]
    out = np.zeros(shape, np.int64)
    for b in range(n):
        for k in range(1, C):
            cy, cx = rng.uniform(0.2, 0.8) * h, rng.uniform(0.2, 0.8) * w
            ry, rx = rng.uniform(0.1, 0.3) * h, rng.uniform(0.1, 0.3) * w
            out[b][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = k
    return out


def box_volumes(case):
    """(pred, target) uint8 [D3, H3, W3]: in every 4 x 4 x 4 cell of a case-specific choice one box of 1 .. 3 voxels a side at a random
    offset that stays clear of the cell's far faces (so no two boxes touch under any connectivity), of one class on both sides;
    the two sides draw their boxes independently, so lesions of every size 1 .. 27 and overlaps of every count occur"""
    rng = _rng(case, 5)
    out = [np.zeros((D3, H3, W3), np.uint8) for _ in range(2)]
    for z in range(0, D3, 4):
        for y in range(0, H3, 4):
            for x in range(0, W3, 4):
                k = int(rng.integers(1, C))
                for L in out:
                    if rng.random() < 0.9:
                        e = rng.integers(1, 4, 3)
                        o = [int(rng.integers(0, 4 - v)) for v in e]
                        L[z + o[0]:z + o[0] + e[0], y + o[1]:y + o[1] + e[1], x + o[2]:x + o[2] + e[2]] = k
    return out


def confusion(with_logits):
    def ref(arrays, got=None):
        p, t = arrays
        pred = p.argmax(1) if with_logits else p.astype(np.int64)
        return [("total", np.bincount((C * t + pred).ravel(), minlength=C * C).reshape(C, C).astype(np.float64), None)]
    make = lambda k: [logits(k) if with_logits else label_map(k, dtype=np.uint8)[:, ::-1].copy(), label_map(k)]
    return _subject("ConfusionMeter-%s" % ("logits" if with_logits else "labels"), make, ref, exact=True)


def image_stats():
    import void_ref as V
    ref = lambda arrays, got=None: [("stats", V.image_stats(V.argmax_first(arrays[0]), arrays[1], C), None)]
    return _subject("ImageStatsMeter", lambda k: [logits(k), label_map(k, void=True)], ref, exact=True)


def sign_logits(case):
    """logits well away from the threshold whose signs follow the element index mod 3 -- (+ + -), (+ - +), (- + +) in cases A, B, C --
    so that the thresholded maps of any two cases differ in two thirds of their elements (three binary maps cannot do better)"""
    pattern = {"A": (1, 1, -1), "B": (1, -1, 1), "C": (-1, 1, 1)}[case]
    z = 1.0 + np.abs(logits(case).astype(np.float64))
    sign = np.asarray(pattern, np.float64)[np.arange(z.size) % 3].reshape(z.shape)
    return (sign * z).astype(np.float32)


def sigmoid_stats():
    import sigmoid_ref as S
    ref = lambda arrays, got=None: [("stats", S.stats(arrays[0], arrays[1], 0.3), None), ("labels", S.labels(arrays[0], 0.3), None)]
    return _subject("SigmoidStatsMeter", lambda k: [sign_logits(k), planes(k, void=True)], ref, exact=True)


CURVE_THRESHOLDS = 11


def curve():
    import curves_ref as Cv
    ref = lambda arrays, got=None: [("hist", Cv.hist(arrays[0], arrays[1], CURVE_THRESHOLDS, "sigmoid", "planes"), None)]
    return _subject("CurveMeter", lambda k: [logits(k), planes(k, void=True)], ref, exact=True)


def _f64_bar(a):
    return F64_BAR * np.maximum(1.0, np.abs(a))


def surface():
    import surface_ref as S

    def ref(arrays, got=None):
        si, sf, _ = S.batch_stats(arrays[0], arrays[1], list(range(1, C)))
        return [("stats_i", si, None), ("stats_f", sf, _f64_bar(sf))]
    return _subject("SurfaceDistanceMeter", lambda k: [organ_map(k, 6), organ_map(k, 7)], ref, exact=True)


def volume_surface():
    import volume_ref as VR

    def ref(arrays, got=None):
        si, sf, _ = VR.cases_stats([(arrays[0], arrays[1])], list(range(1, C)), (2, 1, 1))
        return [("stats_i", si, None), ("stats_f", sf, _f64_bar(sf))]
    return _subject("VolumeSurfaceMeter", box_volumes, ref, exact=True)


LESION_CAP = dict(max_components=128, max_pairs=64)
LESION_HEAD = (64, 64, 16, 16, 4)            # the compared head of every record: the tables are never more than half full by design


def lesion():
    import lesion_ref as LR

    def ref(arrays, got=None):
        rec = LR.records(arrays[0], arrays[1], C, 26)
        assert rec[0].size >= LESION_HEAD[0] and rec[2].size >= LESION_HEAD[2] and rec[0].size <= LESION_CAP["max_components"]
        rec = [r.astype(t) for r, t in zip(rec, (np.int64, np.int32, np.int64, np.int32, np.int32))]
        return [(n, r[:h][None], None) for n, r, h in zip(("comp_keys", "comp_sizes", "pair_keys", "pair_counts", "ctrl"), rec, LESION_HEAD)]
    return _subject("LesionMeter", box_volumes, ref, exact=True)


def lesion_finish(outs):
    return [o[:, :h] for o, h in zip(outs, LESION_HEAD)]


def meter_subjects():
    return [confusion(False), confusion(True), image_stats(), sigmoid_stats(), curve(), surface(), volume_surface(), lesion()]


METER_NAMES = ["ConfusionMeter-labels", "ConfusionMeter-logits", "ImageStatsMeter", "SigmoidStatsMeter", "CurveMeter",
               "SurfaceDistanceMeter", "VolumeSurfaceMeter", "LesionMeter"]


# ------------------------------------------------------------------------------------------------------------------------ data
HS, WS = 60, 80                                # source frames; the network size is H x W
MEAN3, STD3 = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def frames(case):
    rng = _rng(case, 8)
    img = rng.integers(0, 256, (B, HS, WS, 3), dtype=np.uint8)
    img[:, :HS // 3] //= 3                                          # structure, so that contrast and hue see non-uniform frames
    return img, rng.integers(0, 64, (B, HS, WS), dtype=np.uint8)


def preprocess():
    from oracle import preprocess_ref as P

    def make(k):
        img, mask = frames(k)
        return [img, mask, np.array({"A": [0, 1], "B": [3, 2], "C": [1, 3]}[k], np.uint8)]

    def ref(arrays, got=None):
        img, mask, flips = arrays
        x, _ = P.preprocess(img, mask, (H, W), flips=flips)
        y = []
        for b in range(B):                                           # mask_mode="labels": P.preprocess's mask path without the threshold
            mk = P.resize_nearest(mask[b], H, W)
            mk = mk[:, ::-1] if flips[b] & 1 else mk
            y.append((mk[::-1] if flips[b] & 2 else mk).astype(np.int64))
        return [("x", x, None), ("labels", np.stack(y), None)]
    return _subject("DevicePreprocess", make, ref, exact=True)


def augment_params(case, one_of):
    """the host side of a DeviceAugment call: per-sample dicts that differ from case to case (a parameter copy that reads another
    call's host memory then shows in the result)"""
    from lm_net_amd.data import ssr_matrix
    k = CASES.index(case)
    p = [{"crop": (2 + k, 3, HS - 8, WS - 10 - k), "M": ssr_matrix(H, W, 20.0 - 15.0 * k, 1.0 + 0.05 * k, 0.05, -0.02 * k), "flips": k + 1,
          "cj": [1.1 - 0.1 * k, 0.9 + 0.1 * k, 1.2, 0.1 * (k - 1)], "order": [k, 3, (k + 1) % 3, (k + 2) % 3]},
         {"crop": (0, k, HS - k, WS - 2 * k), "flips": (k + 2) % 4, "cj": [0.9, 1.2 - 0.1 * k, 0.8 + 0.1 * k, 0.05], "order": [3, 2, 1, 0]}]
    if one_of:
        g = np.random.default_rng(40 + k)
        p[0]["oneof"] = {"op": "grid_distortion", "num_steps": 5, "xsteps": list(1 + g.uniform(-0.3, 0.3, 6)), "ysteps": list(1 + g.uniform(-0.3, 0.3, 6))}
        p[1]["oneof"] = {"op": "elastic", "seed": 11 + k, "alpha": 30.0 + 5 * k, "sigma": 3.0}
    return p


def augment(one_of):
    def ref(arrays, got=None, host=None):
        import augment_ref as A
        import oneof_ref as O
        x, y, g = (O if one_of else A).augment(arrays[0], arrays[1], host, (H, W), MEAN3, STD3, 1)
        return [("x", np.asarray(x), None), ("labels", np.asarray(y), None), ("gray_sum", np.asarray(g, np.int64), None)]
    s = _subject("DeviceAugment-%s" % ("oneof" if one_of else "plain"), lambda k: list(frames(k)), ref, exact=True)
    s.host = {k: augment_params(k, one_of) for k in CASES}
    return s


SLICER = dict(size=(32, 48), norm=[["zscore", ("window", 40.0, 400.0)]], context=1, foreground=-1000, clip=(0.5, 99.5))
SLICER_SRC = (8, 40, 50)                        # D, Hs, Ws
SLICER_Z = [1, 5, 7, 2]


def slicer_params(case):
    from lm_net_amd.data import ssr_matrix
    k = CASES.index(case)
    h, w = SLICER["size"]
    return [{"M": ssr_matrix(h, w, 10.0 + 10 * k, 1.05, 0.03 * k, -0.02), "flips": k, "gain": 1.0 + 0.05 * k, "bias": 0.02 * k},
            {"M": None, "flips": 3 - k, "gain": 0.95, "bias": -0.03 * k}, {"M": None, "flips": 0}, {"M": ssr_matrix(h, w, -25.0, 0.9 + 0.05 * k, 0.0, 0.05), "flips": 1}]


def slicer():
    """VolumeSlicer: open_case (record EQUAL, table to 1e-6), batch (labels EQUAL, images within slices_ref.tol on the device's own
    table, as tests/test_slices_kernels_gpu.py compares them) and restore (EQUAL)"""
    import slices_ref as R

    def make(k):
        rng = _rng(k, 9)
        lo, hi = {"A": (-900, 600), "B": (-500, 1500), "C": (-990, 3000)}[k]
        vol = rng.integers(lo, hi, (1,) + SLICER_SRC).astype(np.int16)
        vol[rng.random(vol.shape) < 0.2 + 0.1 * CASES.index(k)] = -1024
        lab = label_map(k, dtype=np.uint8, shape=SLICER_SRC)
        return [vol, lab, label_map(k, dtype=np.uint8, shape=(len(SLICER_Z),) + SLICER["size"])[:, ::-1].copy()]

    def ref(arrays, got=None, host=None):
        from lm_net_amd import VolumeSlicer
        vol, lab, net = arrays
        s = VolumeSlicer(**SLICER)
        rec = R.record(vol, s.foreground, s.q_ppm)
        tab = R.table(rec, s.specs)
        tab_bar = np.where(tab != 0, 1e-6 * np.abs(tab), 1e-6)
        n, (h, w), src = len(SLICER_Z), s.size, SLICER_SRC[1:]
        rows = s.rows(n, host, s.size, src)
        used = tab if got is None else got[1].astype(np.float64)
        x, y, _ = R.gather(vol, lab, SLICER_Z, rows, used, [m for m, _, _, _ in s.specs], s.context, s.stride, s.size, edge=s.edge, border=s.border,
                           border_value=s.border_value, label_border=s.label_border, coord_dtype=np.float32)
        tol = R.tol(x, rows, used, 2 * s.context + 1, R.vmax(vol, s.border_value, used))
        _, back, _ = R.gather(None, net, list(range(n)), s.rows(n, None, src, (h, w)), None, None, 0, 1, src, coord_dtype=np.float32)
        return [("stats", np.asarray(rec, np.int64), None), ("table", tab, tab_bar), ("x", x, np.broadcast_to(tol, x.shape)),
                ("y", y.astype(np.uint8), None), ("restored", back.astype(np.uint8), None)]
    s = _subject("VolumeSlicer", make, ref, exact=True, no_growth=True)
    s.host = {k: slicer_params(k) for k in CASES}
    return s


POST_CLEAN = dict(keep_largest=False, min_area=3, fill_holes=True)
POST_TOP = 32                                   # components() is compared through roots and the POST_TOP largest areas / sizes
VOLPOST_CLEAN = dict(keep_largest=False, min_volume=2, fill_holes=True)


def _top(a, n=POST_TOP):
    return np.sort(np.asarray(a).reshape(-1))[::-1][:n].copy()


VOLPOST_TOP = 8


def post_finish(outs, n=POST_TOP):
    """roots as they are; areas (0 away from the root pixels: two cases agree in most elements) as their n largest values"""
    return list(outs[:-1]) + [_top(outs[-1], n)]


def volpost_finish(outs):
    return post_finish(outs, VOLPOST_TOP)


POST_FRAME = (70, 90)                           # the padded frame buffer; POST_HW: each sample's valid size inside it
POST_HW = [[70, 88], [55, 90]]


def postprocess():
    """DevicePostprocess: cleaning, the labels resized back into ragged frames, contour overlays at alpha 0.4, and components()"""
    import post_ref as PR
    import volpost_ref as VP

    def make(k):
        return [np.stack([VP.blob_labels((1, H, W), C, seed=_SEED[k] + b)[0] for b in range(B)]).clip(0, C - 1).astype(np.uint8),
                _rng(k, 10).integers(0, 256, (B,) + POST_FRAME + (3,), dtype=np.uint8)]

    def ref(arrays, got=None):
        net, stats, _, _ = PR.clean(arrays[0], C, connectivity=8, **POST_CLEAN)
        labels = PR.resize_back(net, POST_HW, *POST_FRAME)
        over = PR.overlay(labels, arrays[1], POST_HW, PR.default_palette(C), 0.4, "contour")
        roots, areas = PR.batch_components(arrays[0], C, 8)
        return [("labels_net", net, None), ("stats", stats, None), ("labels", labels, None), ("overlay", over, None), ("roots", roots, None),
                ("areas", _top(areas), None)]
    return _subject("DevicePostprocess", make, ref, exact=True)


def volpost():
    import volpost_ref as VP

    def ref(arrays, got=None):
        lab, stats, _ = VP.clean(arrays[0], C, connectivity=26, **VOLPOST_CLEAN)
        roots, sizes = VP.components(VP.label_volume(arrays[0], C), 26)
        return [("labels", lab, None), ("stats", stats, None), ("roots", roots.astype(np.int32), None), ("sizes", _top(sizes, VOLPOST_TOP).astype(np.int32), None)]
    return _subject("VolumePostprocess", lambda k: [VP.blob_labels((D3, H3, W3), C, seed=_SEED[k]).clip(0, C - 1).astype(np.uint8)], ref, exact=True)


def data_subjects():
    return [preprocess(), slicer(), postprocess(), volpost(), augment(False), augment(True)]


DATA_NAMES = ["DevicePreprocess", "VolumeSlicer", "DevicePostprocess", "VolumePostprocess", "DeviceAugment-plain", "DeviceAugment-oneof"]


@functools.lru_cache(maxsize=None)
def subjects():
    """{name: Subject} of every file's subjects, built once per process"""
    out = {}
    for s in loss_subjects() + meter_subjects() + data_subjects():
        assert s.name not in out
        out[s.name] = s
    return out

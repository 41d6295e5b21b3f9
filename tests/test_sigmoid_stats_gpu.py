"""GPU: lmn_sigmoid_stats (include/lmnet_sigmoid.h), lm_net_amd.metrics.SigmoidStatsMeter and sigmoid_labels against the numpy
restatement of tests/sigmoid_ref.py.  Integer arithmetic throughout: statistics and label maps must be EQUAL, element for element,
and two calls bit-identical; the meter's scores equal tests/void_ref.py::score on the same statistics to 1e-12 (a handful of float64
operations on exact integers)."""
import numpy as np
import pytest
import torch

import post_ref
import sigmoid_ref as S
import surface_ref
from tools import metrics_ref

pytestmark = pytest.mark.gpu


def _close(a, b, tol):
    return (np.isnan(a) and np.isnan(b)) or a == b or abs(a - b) <= tol * max(abs(b), 1e-300)


def _call(lg, t, thr, stats=True, labels=True):
    from lm_net_amd import hip
    B, C = lg.shape[:2]
    st = torch.full((B, C, 4), -7, device="cuda", dtype=torch.int64) if stats else None      # (overwritten, not added to)
    lab = torch.full(lg.shape, 9, device="cuda", dtype=torch.uint8) if labels else None
    hip.sigmoid_stats(lg, t, hip.sig_logit_threshold(thr), st, lab)
    torch.cuda.synchronize()
    return st, lab


@pytest.mark.parametrize("H, W", [(37, 45), (36, 44)])
@pytest.mark.parametrize("C", S.STATS_C)
def test_stats_and_labels_equal_the_restatement(C, H, W):
    """37x45 runs one element per lane (HW odd), 36x44 four; both with a tail."""
    B = 3
    key = "sig_stats_gpu/%d/%dx%d" % (C, H, W)
    lg = S.logits((B, C, H, W), key + "/lg")
    lgd = lg.cuda()
    for void in (False, True):
        t = S.targets((B, C, H, W), key + "/t", key + "/v" if void else None)
        n_valid = ((t == 0) | (t == 1)).flatten(2).sum(2)
        for dtype in (torch.int64, torch.uint8):
            td = t.to(dtype).cuda()
            for thr in S.STATS_THR:
                want_s, want_l = S.stats(lg.numpy(), t.numpy(), thr), S.labels(lg.numpy(), thr)
                st, lab = _call(lgd, td, thr)
                tag = (C, H, W, void, dtype, thr)
                assert np.array_equal(st.cpu().numpy(), want_s), tag
                assert np.array_equal(lab.cpu().numpy(), want_l), tag
                assert torch.equal(st.cpu().sum(-1), n_valid), tag
                st2, lab2 = _call(lgd, td, thr)                   # identical from call to call
                assert torch.equal(st, st2) and torch.equal(lab, lab2), tag
                only_s, none = _call(lgd, td, thr, labels=False)
                none2, only_l = _call(lgd, None, thr, stats=False)
                assert none is None and none2 is None and torch.equal(only_s, st) and torch.equal(only_l, lab), tag


def test_threshold_ties_less_than_one_wave_and_one_element():
    """z == logit_threshold is predicted on (fp32 compare); HW = 35 and HW = 1 with B = 1."""
    from lm_net_amd import hip
    lt = hip.sig_logit_threshold(0.3)
    for hw in (35, 1):
        z = S.logits((1, 2, 1, hw), "sig_stats_gpu/tie/%d" % hw)
        z[0, 0, 0, 0] = lt
        z[0, 1, 0, 0] = float(np.nextafter(np.float32(lt), np.float32(-10)))
        t = S.targets((1, 2, 1, hw), "sig_stats_gpu/tie/t", "sig_stats_gpu/tie/v")
        t[:, :, 0, 0] = 1
        st, lab = _call(z.cuda(), t.cuda(), 0.3)
        assert int(lab[0, 0, 0, 0]) == 1 and int(lab[0, 1, 0, 0]) == 0
        assert np.array_equal(st.cpu().numpy(), S.stats(z.numpy(), t.numpy(), 0.3))
        assert np.array_equal(lab.cpu().numpy(), S.labels(z.numpy(), 0.3))


def test_many_blocks_per_plane():
    """B = 1, C = 2 at 352x352: 123904 elements per plane = 121 trips of 256 quads over 121 blocks (the cap is 1024 / 2 per plane);
    B = 2, C = 64 at 149x221 (odd): 129 trips of 256 lanes over 1024 / 128 = 8 blocks per plane, 16-17 trips each."""
    for B, C, H, W in ((1, 2, 352, 352), (2, 64, 149, 221)):
        key = "sig_stats_gpu/big/%d" % C
        lg = S.logits((B, C, H, W), key + "/lg")
        t = S.targets((B, C, H, W), key + "/t", key + "/v")
        st, lab = _call(lg.cuda(), t.cuda(), 0.5)
        assert np.array_equal(st.cpu().numpy(), S.stats(lg.numpy(), t.numpy(), 0.5))
        assert np.array_equal(lab.cpu().numpy(), S.labels(lg.numpy(), 0.5))


@pytest.mark.parametrize("C", [1, 5])
def test_meter_scores(C):
    from lm_net_amd import SigmoidStatsMeter
    from lm_net_amd.metrics import sigmoid_labels
    lg, t = S.stats_case(C, void=True)
    cw = S.stats_class_weights(C)
    for thr in S.STATS_THR:
        m = SigmoidStatsMeter(C, threshold=thr)
        m.update(lg[:2].cuda(), t[:2].cuda())
        if C == 1:                                                # the [B, H, W] mask of a binary pipeline; bool is taken as uint8
            m.update(lg[2:].cuda(), (t[2:, 0] == 1).cuda())
            want = np.concatenate([S.stats(lg[:2].numpy(), t[:2].numpy(), thr), S.stats(lg[2:].numpy(), (t[2:] == 1).numpy(), thr)])
        else:
            m.update(lg[2:].cuda(), t[2:].to(torch.uint8).cuda())
            want = S.stats(lg.numpy(), t.numpy(), thr)
        assert m.raw().is_cuda and np.array_equal(m.raw().cpu().numpy(), want)
        for mname in S.METRICS:
            pname, pkw = S.PRODUCT_NAMES.get(mname, (mname, {}))
            for r in S.REDUCTIONS:
                w = cw if "weighted" in r else None
                assert _close(m.score(pname, r, w, **pkw), S.score(want, mname, r, w), 1e-12), (thr, mname, r)
        assert m.per_image("iou").shape == (3, C)
        lab = m.labels(lg.cuda())
        assert lab.dtype == torch.uint8 and np.array_equal(lab.cpu().numpy(), S.labels(lg.numpy(), thr))
        assert torch.equal(sigmoid_labels(lg.cuda(), thr), lab)


def test_label_maps_feed_the_two_class_meters_and_the_postprocess():
    """labels(logits).view(B * C, H, W) and the target planes viewed likewise are ordinary two-class label maps (void: 255)."""
    from lm_net_amd import SigmoidStatsMeter
    from lm_net_amd.metrics import ConfusionMeter, SurfaceDistanceMeter
    from lm_net_amd.post import DevicePostprocess
    B, C, H, W = 2, 3, 37, 45
    lg, t = S.stats_case(C, void=True)
    lg, t = lg[:B], t[:B]
    # smooth the noise a little so that the maps have components larger than a pixel
    lg = torch.nn.functional.avg_pool2d(lg, 5, 1, 2) * 3
    m = SigmoidStatsMeter(C)
    maps = m.labels(lg.cuda()).view(B * C, H, W)
    tgt = t.cuda().view(B * C, H, W)
    host = S.labels(lg.numpy()).reshape(B * C, H, W)
    th = t.numpy().reshape(B * C, H, W)
    assert np.array_equal(maps.cpu().numpy(), host)
    cm = ConfusionMeter(2)
    cm.update(maps, tgt)
    valid = th <= 1
    tp, fp, fn, tn = metrics_ref.confusion(torch.from_numpy(host[valid]), torch.from_numpy(th[valid]))
    assert cm.compute()["confusion"] == [[tn, fp], [fn, tp]]
    m.update(lg.cuda(), t.cuda())
    assert m.raw().sum((0, 1)).tolist() == [tp, fp, fn, tn]      # the same four numbers from the sigmoid statistics
    sm = SurfaceDistanceMeter(2)
    tb = (th == 1).astype(np.int64)                               # (the surface meter has no void label: foreground planes)
    sm.update(maps, torch.from_numpy(tb).cuda())
    si_r, sf_r, _ = surface_ref.batch_stats(host, tb, sm.classes)
    si, sf = (a.cpu().numpy() for a in sm.raw())
    assert np.array_equal(si, si_r) and bool((np.abs(sf - sf_r) <= 1e-9 * np.maximum(1, np.abs(sf_r))).all())
    kw = dict(keep_largest=True, min_area=4, fill_holes=True)
    out = DevicePostprocess(2, **kw)(maps)
    want_net, want_stats, removed, _ = post_ref.clean(host, 2, connectivity=8, **kw)
    assert removed > 0
    assert np.array_equal(out.labels_net.cpu().numpy(), want_net) and np.array_equal(out.stats.cpu().numpy(), want_stats)

"""CPU: the host side of the threshold sweeps (include/curves/lmnet_curves.h, lm_net_amd.metrics.CurveMeter): registry and header
agree, the edge tables of hip.curve_edges, the argument checks of the C entries (rejected before
any HIP call, with fake device pointers), the meter's float64 arithmetic against the brute-force restatement tests/curves_ref.py, and
that restatement against scikit-learn on scores for which binning loses nothing.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import curves_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- ABI
def test_registry_and_header_agree():
    """The feature's own part of the registry: the literal list, its place in hip.HEADERS, the number and values of its #defines and
    the header's citations.  (Header / export / layout / return-type / constants checks: tests/test_host_cpu.py.)"""
    from lm_net_amd import hip
    assert hip.SYMBOLS_CURVES == ["lmn_curve_workspace", "lmn_curve_hist"]
    assert hip.HEADERS["curves/lmnet_curves.h"] is hip.SYMBOLS_CURVES
    header = open(os.path.join(ROOT, "include", "curves", "lmnet_curves.h")).read()
    assert len(re.findall(r"^#define LMN_CURVE_\w+ \d+\b", header, re.M)) == 8
    assert (hip.CURVE_MAX_EDGES, hip.CURVE_MAX_CLASSES) == (1024, 64)
    assert (hip.CURVE_T_U8, hip.CURVE_T_I64) == (hip.SIG_T_U8, hip.SIG_T_I64)    # hip.sig_target_kind serves both
    assert "train.py:29" in header and "BIN RULE" in header


# ---------------------------------------------------------------- edge tables
def test_curve_edges():
    from lm_net_amd import hip
    for n in (2, 101, 1024):
        for kind in ("logit", "probability"):
            e = hip.curve_edges(n, kind)
            assert e.dtype == np.float32 and e.shape == (n,) and bool(np.all(np.diff(e) >= 0)), (n, kind)
        t = hip.curve_thresholds(n)
        assert t.dtype == np.float64 and t[0] == 0.0 and t[-1] == 1.0 and np.array_equal(t, np.arange(n) / (n - 1))
        assert np.array_equal(hip.curve_edges(n, "probability"), t.astype(np.float32))
        lg = hip.curve_edges(n, "logit")
        assert lg[0] == -np.inf and lg[-1] == np.inf and bool(np.isfinite(lg[1:-1]).all())
    for bad in (1, 1025, 0, -3, [0.7, 0.3], [0.1, 1.5], [-0.1, 0.5], [float("nan")], [], [0.0] * 1025, "abc", None, 0.5, True):
        with pytest.raises(ValueError, match="curve_edges"):
            hip.curve_edges(bad, "logit")
    with pytest.raises(ValueError, match="kind"):
        hip.curve_edges(5, "logits")
    e = hip.curve_edges([0.5], "logit")
    assert e.shape == (1,) and e[0] == 0.0 and not np.signbit(e[0]) and float(e[0]) == hip.sig_logit_threshold(0.5)
    for thr in (0.1, 0.25, 0.3, 0.5, 0.731, 0.999):                               # the arithmetic of sig_logit_threshold, bit for bit
        assert float(hip.curve_edges([thr], "logit")[0]) == hip.sig_logit_threshold(thr)
    assert hip.curve_edges(101, "logit")[50] == 0.0
    assert np.array_equal(hip.curve_edges([0.2, 0.2, 0.9], "probability"), np.array([0.2, 0.2, 0.9], dtype=np.float32))   # ties pass
    for bad in (0.0, 1.0):                                                       # sig_logit_threshold itself stays as it is
        with pytest.raises(ValueError, match="outside"):
            hip.sig_logit_threshold(bad)


# ---------------------------------------------------------------- argument checks
GOOD = dict(target_kind=1, target_form=0, score_kind=0, n_edges=101, B=2, C=3, HW=391)


def _entry(null=None, **kw):
    """lmn_curve_hist with fake device pointers: every case here must be rejected before any HIP call."""
    from lm_net_amd import hip
    lib = hip.load()
    fake = ctypes.c_void_p(0x1000)
    a = dict(values=fake, target=fake, edges=fake, workspace=fake, hist=fake)
    if null:
        a[null] = None
    g = dict(GOOD, **kw)
    rc = lib.lmn_curve_hist(a["values"], a["target"], g["target_kind"], g["target_form"], g["score_kind"], a["edges"], g["n_edges"],
                            g["B"], g["C"], ctypes.c_int64(g["HW"]), a["workspace"], a["hist"], None)
    return rc, lib.lmn_last_error().decode()


def test_entry_rejects_bad_arguments():
    for name in ("values", "target", "edges", "hist"):
        rc, err = _entry(null=name)
        assert rc == -1 and err == "curve_hist: null pointer", (name, err)
    rc, err = _entry(null="workspace", score_kind=1)
    assert rc == -1 and "needs its workspace" in err, err
    for kw, msg in ((dict(target_kind=2), "unknown target_kind 2"), (dict(target_kind=-1), "unknown target_kind -1"),
                    (dict(target_form=2), "unknown target_form 2"), (dict(target_form=-1), "unknown target_form -1"),
                    (dict(score_kind=2), "unknown score_kind 2"), (dict(score_kind=-1), "unknown score_kind -1"),
                    (dict(n_edges=0), "n_edges=0 not in [1, 1024]"), (dict(n_edges=1025), "n_edges=1025 not in [1, 1024]"),
                    (dict(n_edges=-1), "n_edges=-1"), (dict(C=0), "C=0 not in [1, 64]"), (dict(C=65), "C=65 not in [1, 64]"),
                    (dict(C=1, score_kind=1), "C=1 not in [2, 64]"), (dict(C=65, score_kind=1), "C=65 not in [2, 64]"),
                    (dict(B=0), "B=0"), (dict(B=-1), "B=-1"), (dict(HW=0), "HW=0"), (dict(HW=-5), "HW=-5"), (dict(HW=2 ** 31), "2^31"),
                    (dict(B=4, HW=2 ** 29), "B * HW < 2^31"), (dict(B=1024, C=64), "B * C = 65536 above 65535")):
        rc, err = _entry(**kw)
        assert rc == -1 and msg in err and err.startswith("curve_hist: "), (kw, err)


def test_workspace_is_host_arithmetic():
    from lm_net_amd import hip
    assert hip.curve_workspace(hip.CURVE_RAW, 8, 352 * 352) == 0
    assert hip.curve_workspace(hip.CURVE_SOFTMAX, 8, 352 * 352) == 4 * 8 * 352 * 352
    assert hip.curve_workspace(hip.CURVE_SOFTMAX, 1, 1) == 4
    for args, msg in (((2, 1, 10), "unknown score_kind 2"), ((1, 0, 10), "B=0"), ((1, 4, 2 ** 29), "B * HW < 2^31"), ((0, 1, 0), "HW=0")):
        with pytest.raises(ValueError, match="curve_workspace"):
            hip.curve_workspace(*args)
        assert msg in hip.load().lmn_last_error().decode()


def test_python_wrapper_checks_sizes_before_the_library():
    from lm_net_amd import hip
    v, t = torch.zeros(2, 3, 5, 7), torch.zeros(2, 3, 5, 7, dtype=torch.int64)
    e, h = torch.zeros(4), torch.zeros(2, 3, 2, 5, dtype=torch.int64)
    for args, msg in (((v, t, 2, 0, e, h), "unknown target_form"), ((v, t, 0, 3, e, h), "unknown target_form"),
                      ((v, t, 0, 0, e, h), "target .* does not match"),                # a CPU target
                      ((v, t, 0, 0, torch.zeros(0), h), "0 edges"), ((v, t, 0, 0, torch.zeros(1025), h), "1025 edges")):
        with pytest.raises(ValueError, match=msg):
            hip.curve_hist(*args)
    with pytest.raises(ValueError, match="contiguous"):
        hip.curve_hist(v.transpose(2, 3), t, 0, 0, e, h)


def test_meter_refuses_what_it_cannot_run():
    from lm_net_amd import CurveMeter
    for kw, msg in ((dict(n_classes=0), "outside"), (dict(n_classes=65), "outside"), (dict(n_classes=1, scores="softmax"), r"outside \[2, 64\]"),
                    (dict(n_classes=2, scores="logits"), "scores="), (dict(n_classes=2, thresholds=1), "curve_edges"),
                    (dict(n_classes=2, thresholds=[0.9, 0.1]), "non-decreasing")):
        with pytest.raises(ValueError, match=msg):
            CurveMeter(device="cpu", **kw)
    m = CurveMeter(3, "sigmoid", 11, device="cpu")
    assert m.thresholds.shape == (11,) and m.edges.dtype == np.float32 and tuple(m.raw().shape) == (0, 3, 2, 12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.update(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.update(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))      # a label map
    with pytest.raises(ValueError, match="n_classes"):
        m.update(torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="add_raw"):
        m.add_raw(torch.zeros(1, 3, 2, 11, dtype=torch.int64))
    with pytest.raises(ValueError, match="average"):
        m.auroc(average="micro")


# ---------------------------------------------------------------- host arithmetic
def _fed_meter(C, thresholds, scores, key, B=3, hw=(9, 11), form="planes"):
    """A CPU-side CurveMeter fed, through add_raw, with the histograms of the restatement -> meter, the restatement's counts."""
    from lm_net_amd import CurveMeter
    z = R.logits((B, C) + hw, key + "/z", 2.0)
    if scores == "probability":
        z = (1 / (1 + np.exp(-z.astype(np.float64)))).astype(np.float32)
    t = R.plane_targets((B, C) + hw, key + "/t") if form == "planes" else R.label_targets((B,) + hw, C, key + "/t")
    cnt = R.counts(z, t, thresholds, scores, form)
    m = CurveMeter(C, scores, thresholds, device="cpu")
    h = torch.from_numpy(R.hist_from_counts(*cnt))
    m.add_raw(h[:1])
    m.add_raw(h[1:])
    return m, cnt


@pytest.mark.parametrize("C,thresholds,scores,form", [(1, 101, "sigmoid", "planes"), (3, 17, "sigmoid", "labels"), (4, 33, "softmax", "labels"),
                                                      (2, [0.0, 0.2, 0.2, 0.5, 0.9, 1.0], "probability", "planes"), (2, [0.5], "sigmoid", "planes")],
                         ids=["binary", "labels", "softmax", "list", "one"])
def test_meter_arithmetic_equals_the_restatement(C, thresholds, scores, form):
    m, cnt = _fed_meter(C, thresholds, scores, "host/%s/%d" % (scores, C), form=form)
    got = m.counts(per_image=True)
    for a, b in zip(got, cnt):
        assert a.dtype == np.int64 and np.array_equal(a, b)
    pooled = tuple(a.sum(0) for a in cnt)
    for a, b in zip(m.counts(), pooled):
        assert np.array_equal(a, b) and a.shape == (C, len(m.thresholds))
    close = lambda a, b: np.allclose(a, b, rtol=0, atol=1e-12, equal_nan=True) and np.array_equal(np.isnan(a), np.isnan(b))
    fpr, tpr, thr = m.roc()
    assert close(fpr, R.roc(*pooled)[0]) and close(tpr, R.roc(*pooled)[1]) and np.array_equal(thr, R.hip.curve_thresholds(thresholds))
    prec, rec, _ = m.pr()
    assert close(prec, R.pr(*pooled)[0]) and close(rec, R.pr(*pooled)[1])
    assert close(m.auroc(), R.auroc(*pooled)) and close(m.average_precision(), R.average_precision(*pooled))
    assert close(m.auroc("macro"), R.nanmean(R.auroc(*pooled))) and close(m.average_precision("macro"), R.nanmean(R.average_precision(*pooled)))
    per = m.auroc(per_image=True)
    assert per.shape == (3, C)
    for i in range(3):
        assert close(per[i], R.auroc(*(a[i] for a in cnt)))
        assert close(m.average_precision(per_image=True)[i], R.average_precision(*(a[i] for a in cnt)))
        assert close(m.auroc("macro", per_image=True)[i], R.nanmean(R.auroc(*(a[i] for a in cnt))))
    from lm_net_amd.metrics import STATS_METRICS
    tp, fp, fn, tn = (a.astype(np.float64) for a in pooled)
    for name in STATS_METRICS:
        s = m.score(name, zero_division=0.25, beta=2.0)
        assert s.shape == tp.shape
        with np.errstate(divide="ignore", invalid="ignore"):
            want = STATS_METRICS[name](tp, fp, fn, tn, beta=2.0) if name == "fbeta" else STATS_METRICS[name](tp, fp, fn, tn)
        assert close(s, np.where(np.isnan(want), 0.25, want)), name
    with np.errstate(divide="ignore", invalid="ignore"):
        f1 = np.where(2 * tp + fp + fn > 0, 2 * tp / (2 * tp + fp + fn), 1.0)
    best_t, best_s = m.best_threshold("f1")
    for c in range(C):
        k = min(k for k in range(f1.shape[1]) if f1[c, k] == f1[c].max())
        assert best_t[c] == m.thresholds[k] and abs(best_s[c] - f1[c, k]) <= 1e-12


def test_nan_rule_and_tie_breaking():
    from lm_net_amd import CurveMeter
    m = CurveMeter(3, "probability", [0.1, 0.3, 0.5, 0.7, 0.9], device="cpu")
    h = torch.zeros(2, 3, 2, 6, dtype=torch.int64)
    # class 0: two positives in bin 3 and two negatives in bin 1 -- thresholds 0.3 and 0.5 both separate them perfectly
    h[0, 0, 1, 3], h[0, 0, 0, 1] = 2, 2
    # class 1: negatives only; class 2: positives only
    h[0, 1, 0, 2], h[1, 1, 0, 4] = 5, 1
    h[1, 2, 1, 5], h[0, 2, 1, 0] = 3, 1
    m.add_raw(h)
    au, ap = m.auroc(), m.average_precision()
    assert au[0] == 1.0 and np.isnan(au[1]) and np.isnan(au[2])
    assert ap[0] == 1.0 and np.isnan(ap[1]) and ap[2] == 0.75                     # AP needs a positive only; one of four is never on
    assert m.auroc("macro") == 1.0 and m.average_precision("macro") == 0.875
    per = m.auroc(per_image=True)
    assert per.shape == (2, 3) and per[0, 0] == 1.0 and bool(np.isnan(per[1]).all()) and np.isnan(m.auroc("macro", per_image=True)[1])
    fpr, tpr, _ = m.roc()
    assert bool(np.isnan(tpr[1]).all()) and bool(np.isnan(fpr[2]).all()) and not np.isnan(fpr[1]).any()
    prec, rec, _ = m.pr()
    assert prec[0].tolist() == [0.5, 1.0, 1.0, 1.0, 1.0] and rec[0].tolist() == [1.0, 1.0, 1.0, 0.0, 0.0]
    t, s = m.best_threshold("f1")
    assert t[0] == 0.3 and s[0] == 1.0                                             # the LOWEST threshold of the highest score
    assert t[1] == 0.9 and s[1] == 1.0                                             # nothing on, nothing labelled: 0/0 -> zero_division
    t, s = m.best_threshold("iou", zero_division=0.0)
    assert t[0] == 0.3 and t[2] == 0.1 and s[2] == 0.75
    m.reset()
    assert tuple(m.raw().shape) == (0, 3, 2, 6) and tuple(m.counts()[0].shape) == (3, 5) and bool(np.isnan(m.auroc()).all())


# ---------------------------------------------------------------- the restatement against scikit-learn
def test_restatement_against_sklearn():
    """Scores quantised to k / 64, k = 1 .. 63, thresholds N = 65: every ROC vertex is a bin edge, so the binned AUROC and AP lose
    nothing and must equal roc_auc_score / average_precision_score; the rank-statistic AUROC equals it too."""
    metrics = pytest.importorskip("sklearn.metrics")
    r = R.rng("sklearn")
    B, C, H, W = 2, 3, 13, 17
    t = (r.random((B, C, H, W)) < 0.35).astype(np.int64)
    q = np.clip(np.rint(32 + 14 * r.standard_normal((B, C, H, W)) + 12 * (2 * t - 1)), 1, 63)
    p = (q / 64.0).astype(np.float32)
    assert np.array_equal(p.astype(np.float64) * 64, q)
    cnt = tuple(a.sum(0) for a in R.counts(p, t, 65, "probability"))
    au, ap = R.auroc(*cnt), R.average_precision(*cnt)
    for c in range(C):
        y, s = t[:, c].ravel(), p[:, c].ravel().astype(np.float64)
        assert abs(au[c] - metrics.roc_auc_score(y, s)) <= 1e-12, c
        assert abs(ap[c] - metrics.average_precision_score(y, s)) <= 1e-12, c
        assert abs(R.exact_auroc(s, y == 1) - metrics.roc_auc_score(y, s)) <= 1e-12, c

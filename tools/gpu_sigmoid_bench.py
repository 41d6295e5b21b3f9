"""Cost of the sigmoid-head entries (include/lmnet_sigmoid.h), batch 8 at 352x352.  Median over --rounds of device-event timings of
--iters calls each, after warm-up, the variants alternating inside every round of one process:

  loss (forward + backward pairs, us per pair)
    sig_c1_a, sig_c1_b   lmn_sigloss_fwd + _bwd at C = 1, int64 targets, no void, default terms, timed twice:
                         |a - b| / a is the A/A spread of this run;
    sig_c1_void20        the same with 20 % void elements;      sig_c1_u8: uint8 targets;      sig_c1_all_terms: 20 % void, scales
                         (0.7, 1.3, 0.5), focal on (gamma 1.5);
    sig_c9, sig_c9_void20, sig_c9_all_terms   the same at C = 9 (nine overlapping planes);
    segloss_c2, segloss_c9   lmn_segloss_fwd + _bwd on the same batch: the softmax route a binary user takes today;
    segloss_ex_c2, segloss_ex_c9   lmn_segloss_ex_fwd + _bwd (void labels) on the same batch;
    eager_c1, eager_c9   the eager torch composition of BCE + Dice (the default terms) with autograd;
    eager_c1_all_terms, eager_c9_all_terms   the eager composition of all three terms with a void mask;
  statistics (us per call)
    sigmoid_stats_c2 / _c9 (stats and label maps), sigmoid_stats_only_c2 / _c9, image_stats_c2 / _c9 (lmn_image_stats on logits).

`bar`: sig_c1 <= segloss_c2 * (1 + spread): the one-logit loss reads 12 bytes per pixel and pass where the two-class softmax loss
reads 16, so it should not be slower beyond the A/A spread of the run; the tool exits non-zero when it is.  Everything else is reported, not barred.
Prints one JSON line; --out writes it to a file as well (profiles/sigmoid_bench.json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lm_net_amd import hip  # noqa: E402
from tools.detweights import det_input, uniform  # noqa: E402


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters   # us per call


def eager(lg, t, valid, all_terms):
    """The same terms composed from torch operators (what a user writes today), forward + backward."""
    z = lg.detach().requires_grad_(True)
    tf = (t == 1).float()

    def f():
        z.grad = None
        v = valid.float() if valid is not None else None
        n = v.sum().clamp_min(1) if v is not None else float(z.numel())
        elem = torch.nn.functional.binary_cross_entropy_with_logits(z, tf, reduction="none")
        bce = (elem * v).sum() / n if v is not None else elem.mean()
        p = torch.sigmoid(z)
        pv, tv = (p * v, tf * v) if v is not None else (p, tf)
        i_c, z_c, y_c = (pv * tf).sum((0, 2, 3)), (pv * p).sum((0, 2, 3)), tv.sum((0, 2, 3))
        dice = (1 - (2 * i_c + 1e-5) / (z_c + y_c + 1e-5)).mean()
        loss = bce + dice
        if all_terms:
            p_t = p * tf + (1 - p) * (1 - tf)
            foc = elem * (1 - p_t) ** 1.5 * (0.25 * tf + 0.75 * (1 - tf))
            nc = v.sum((0, 2, 3)).clamp_min(1) if v is not None else float(z.numel() // z.shape[1])
            loss = 0.7 * bce + 1.3 * dice + 0.5 * (((foc * v) if v is not None else foc).sum((0, 2, 3)) / nc).sum()
        loss.backward()
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, H, W = 8, 352, 352
    variants, meters = {}, {}
    keep = []
    for C in (1, 9):
        lg = (det_input((B, C, H, W), "sig_bench/%d" % C) * 2.5).cuda()
        n = B * C * H * W
        t = torch.from_numpy((uniform("sig_bench/t%d" % C, n) < 0.3).astype(np.int64)).reshape(B, C, H, W).cuda()
        void = torch.from_numpy(uniform("sig_bench/v%d" % C, n) < 0.2).reshape(B, C, H, W).cuda()
        tv = torch.where(void, torch.full_like(t, 255), t)
        ones = torch.ones(C, device="cuda")
        d = torch.empty_like(lg)
        sums = torch.empty(hip.sig_sums_words(C), device="cuda", dtype=torch.int32)
        coef, loss4 = torch.empty(hip.sig_coef_floats(C), device="cuda"), torch.empty(4, device="cuda")

        def sig(target, par, lg=lg, ones=ones, sums=sums, coef=coef, loss4=loss4, d=d):
            def f():
                hip.sigloss_fwd(lg, target, ones, ones, ones, par, sums, coef, loss4)
                hip.sigloss_bwd(lg, target, ones, coef, None, par, d)
            return f
        default = hip.sig_param()
        every = hip.sig_param(1e-5, 0.7, 1.3, 0.5, 1.5, 0.25)
        if C == 1:
            variants["sig_c1_a"] = sig(t, default)
            variants["sig_c1_b"] = sig(t, default)
            variants["sig_c1_u8"] = sig(t.to(torch.uint8), hip.sig_param(target_kind=hip.SIG_T_U8))
        else:
            variants["sig_c9"] = sig(t, default)
        variants["sig_c%d_void20" % C] = sig(tv, default)
        variants["sig_c%d_all_terms" % C] = sig(tv, every)
        variants["eager_c%d" % C] = eager(lg, t, None, False)
        variants["eager_c%d_all_terms" % C] = eager(lg, tv, ~void, True)
        keep.append((lg, t, tv, void))
    for C in (2, 9):
        lg = (det_input((B, C, H, W), "sig_bench/soft%d" % C) * 2.5).cuda()
        u = uniform("sig_bench/y%d" % C, B * H * W)
        y = torch.from_numpy(np.minimum((u * C).astype(np.int64), C - 1).reshape(B, H, W)).cuda()
        w = torch.ones(C, device="cuda")
        d = torch.empty_like(lg)
        so, co, lo = torch.empty(3 + 3 * C, device="cuda"), torch.empty(3 + 2 * C, device="cuda"), torch.empty(1, device="cuda")
        sx, cx, l4 = (torch.empty(hip.loss_sums_floats(C), device="cuda"), torch.empty(hip.loss_coef_floats(C), device="cuda"),
                      torch.empty(4, device="cuda"))
        par = hip.loss_param(255)

        def old(lg=lg, y=y, w=w, so=so, co=co, lo=lo, d=d):
            hip.segloss_fwd(lg, y, w, w, 0.0, 1e-5, so, co, lo)
            hip.segloss_bwd(lg, y, w, co, None, d)

        def ex(lg=lg, y=y, w=w, sx=sx, cx=cx, l4=l4, d=d, par=par):
            hip.segloss_ex_fwd(lg, y, w, w, par, sx, cx, l4)
            hip.segloss_ex_bwd(lg, y, w, cx, None, par, d)
        variants["segloss_c%d" % C] = old
        variants["segloss_ex_c%d" % C] = ex
        # statistics: C sigmoid planes against the C-class arg-max statistics on the same logits
        t = torch.from_numpy((uniform("sig_bench/st%d" % C, B * C * H * W) < 0.3).astype(np.int64)).reshape(B, C, H, W).cuda()
        st = torch.empty(B, C, 4, device="cuda", dtype=torch.int64)
        lab = torch.empty(B, C, H, W, device="cuda", dtype=torch.uint8)
        meters["sigmoid_stats_c%d" % C] = lambda lg=lg, t=t, st=st, lab=lab: hip.sigmoid_stats(lg, t, 0.0, st, lab)
        meters["sigmoid_stats_only_c%d" % C] = lambda lg=lg, t=t, st=st: hip.sigmoid_stats(lg, t, 0.0, st, None)
        meters["image_stats_c%d" % C] = lambda lg=lg, y=y, st=st, C=C: hip.image_stats(lg, y, C, 255, st)
    out = {"what": "B=8 352x352, us per call (median of %d rounds x %d calls, variants alternating); loss variants are forward + backward"
                   % (a.rounds, a.iters)}
    for name, group in (("loss", variants), ("stats", meters)):
        for f in group.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        us = {k: [] for k in group}
        for _ in range(a.rounds):
            for k, f in group.items():
                us[k].append(timed(f, a.iters))
        out[name] = {k: round(statistics.median(v), 2) for k, v in us.items()}
    r = out["loss"]
    sig = min(r["sig_c1_a"], r["sig_c1_b"])
    out["aa_spread"] = round(abs(r["sig_c1_a"] - r["sig_c1_b"]) / r["sig_c1_a"], 4)
    out["sig_c1_over_segloss_c2"] = round(sig / r["segloss_c2"], 4)
    out["sig_c9_over_segloss_c9"] = round(r["sig_c9"] / r["segloss_c9"], 4)
    out["bar"] = bool(sig <= r["segloss_c2"] * (1 + out["aa_spread"]))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not out["bar"]:
        sys.exit("gpu_sigmoid_bench: the one-logit sigmoid loss is slower than the two-class softmax loss beyond the bar")


if __name__ == "__main__":
    main()

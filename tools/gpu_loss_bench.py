"""Cost of the loss entries with void labels (include/lmnet_loss.h) against the entries they extend, batch 8 at 352x352, C = 2 and 9.
Per class count the median over --rounds of device-event timings of --iters forward + backward pairs each, after warm-up, the
variants alternating inside every round of one process:
  old_a, old_b   lmn_segloss_fwd + lmn_segloss_bwd, timed twice: |old_a - old_b| / old_a is the A/A spread of this run;
  new_plain      lmn_segloss_ex_fwd + _bwd, no void label, focal off, unit scales  (same traffic; one compare and one count more);
  new_void20     the same with 20 % void labels;
  new_all_terms  20 % void, scales (0.7, 1.3, 0.5), focal on (gamma 1.5).
`bar`: new_plain <= old * (1 + max(0.10, 2 * spread)), old = the smaller of old_a and old_b's medians; the tool exits non-zero when
it is false.  new_void20 and new_all_terms are reported, not barred.  Also lmn_image_stats against lmn_confusion on the same batch
(logits in both).  Prints one JSON line; --out writes it to a file as well."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, H, W = 8, 352, 352
    out = {"what": "loss forward + backward, B=8 352x352, us per pair (median of %d rounds x %d pairs, variants alternating)" % (a.rounds, a.iters)}
    ok = True
    for C in (2, 9):
        lg = (det_input((B, C, H, W), "loss_bench/%d" % C) * 2.5).cuda()
        u = uniform("loss_bench/y%d" % C, B * H * W)
        y = torch.from_numpy(np.minimum((u * C).astype(np.int64), C - 1).reshape(B, H, W)).cuda()
        yv = torch.where(torch.from_numpy(uniform("loss_bench/v%d" % C, B * H * W) < 0.2).reshape(B, H, W).cuda(), torch.full_like(y, 255), y)
        w = torch.ones(C, device="cuda")
        d = torch.empty_like(lg)
        sums_o, coef_o, loss_o = torch.empty(3 + 3 * C, device="cuda"), torch.empty(3 + 2 * C, device="cuda"), torch.empty(1, device="cuda")
        sums, coef, loss4 = (torch.empty(hip.loss_sums_floats(C), device="cuda"), torch.empty(hip.loss_coef_floats(C), device="cuda"),
                             torch.empty(4, device="cuda"))

        def old():
            hip.segloss_fwd(lg, y, w, w, 1e-3, 1e-5, sums_o, coef_o, loss_o)
            hip.segloss_bwd(lg, y, w, coef_o, None, d)

        def new(labels, par):
            def f():
                hip.segloss_ex_fwd(lg, labels, w, w, par, sums, coef, loss4)
                hip.segloss_ex_bwd(lg, labels, w, coef, None, par, d)
            return f
        variants = {"old_a": old, "old_b": old,
                    "new_plain": new(y, hip.loss_param(None, 1e-3)),
                    "new_void20": new(yv, hip.loss_param(255, 1e-3)),
                    "new_all_terms": new(yv, hip.loss_param(255, 1e-3, 1e-5, 0.7, 1.3, 0.5, 1.5, 0.25))}
        for f in variants.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        us = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, f in variants.items():
                us[k].append(timed(f, a.iters))
        r = {k: round(statistics.median(v), 2) for k, v in us.items()}
        base = min(r["old_a"], r["old_b"])
        r["aa_spread"] = round(abs(r["old_a"] - r["old_b"]) / r["old_a"], 4)
        r["new_plain_over_old"] = round(r["new_plain"] / base, 4)
        r["bar"] = bool(r["new_plain"] <= base * (1 + max(0.10, 2 * r["aa_spread"])))
        ok = ok and r["bar"]
        counts = torch.zeros(C, C, device="cuda")
        stats = torch.empty(B, C, 4, device="cuda", dtype=torch.int64)
        meters = {"confusion_us": lambda: hip.confusion(lg, yv, counts), "image_stats_us": lambda: hip.image_stats(lg, yv, C, 255, stats)}
        for f in meters.values():
            for _ in range(a.warmup):
                f()
        mu = {k: [] for k in meters}
        for _ in range(a.rounds):
            for k, f in meters.items():
                mu[k].append(timed(f, a.iters))
        r.update({k: round(statistics.median(v), 2) for k, v in mu.items()})
        out["classes_%d" % C] = r
    out["bar"] = ok
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        sys.exit("gpu_loss_bench: the new entries without void labels are slower than the old ones beyond the bar")


if __name__ == "__main__":
    main()

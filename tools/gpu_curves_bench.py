"""Cost of the threshold-sweep entry (include/curves/lmnet_curves.h), batch 8 at 352x352.  Median over --rounds of device-event timings
of --iters calls each, after warm-up, the variants alternating inside every round of one process (us per call):

  curve_<scores>_c<C>_<map>_n<N>_<kind>   lmn_curve_hist: scores sig (logits against logit edges, target planes) or softmax (C = 9,
                         an int64 label map); C = 1 and 9; N = 101 and 1024 thresholds (1024 is LMN_CURVE_MAX_EDGES); targets int64 (and
                         uint8 at N = 101); maps:
                           organ   one disc per plane, logits +-12 across a soft boundary plus noise: mostly saturated scores, which
                                   the kernel counts by wave ballots;
                           noise   sigmoid(z) uniform over (0, 1) (softmax: N(0, 2^2) logits): every element takes an LDS atomic;
  curve_sig_c1_organ_n101_i64_b   the first variant timed twice: |a - b| / a is the A/A spread of this run;
  stats_c<C>_<map>       lmn_sigmoid_stats (statistics only) at ONE threshold on the same tensors: it reads the same bytes, so the
                         histogram costs the extra over it;
  eager_c<C>_<map>_n101  the eager torch composition, torch.bucketize + torch.bincount per (image, class) plane.

Reported, not barred: `over_stats` (curve / stats per pair) and `organ_over_noise`; `ballot_route_ok` is False when an organ map is
slower than its noise map by more than the A/A spread -- then the ballot route is not doing its job.
Prints one JSON line; --out writes it to a file as well (profiles/curves_bench.json)."""
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


def discs(B, C, H, W, key):
    """signed distance (pixels, positive inside) to one disc per (image, class) plane: float64 [B, C, H, W]"""
    yy, xx = np.mgrid[0:H, 0:W]
    u = uniform(key, B * C * 3).reshape(B, C, 3)
    cy, cx, r = (0.3 + 0.4 * u[..., 0]) * H, (0.3 + 0.4 * u[..., 1]) * W, (0.12 + 0.2 * u[..., 2]) * min(H, W)
    return r[..., None, None] - np.sqrt((yy - cy[..., None, None]) ** 2 + (xx - cx[..., None, None]) ** 2)


def eager(z, t, edges):
    """what a user writes today: per plane, bucketize the scores and count (bin, class) pairs of the valid elements"""
    nb = edges.numel() + 1
    B, C = z.shape[:2]

    def f():
        out = torch.empty(B, C, 2, nb, device=z.device, dtype=torch.int64)
        for b in range(B):
            for c in range(C):
                zp, tp = z[b, c].reshape(-1), t[b, c].reshape(-1)
                valid = (tp == 0) | (tp == 1)
                idx = torch.bucketize(zp, edges, right=True) + nb * tp.clamp(0, 1)
                out[b, c] = torch.bincount(idx[valid], minlength=2 * nb).view(2, nb)
        return out
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, H, W = 8, 352, 352
    dev = "cuda"
    edges = {n: {k: torch.from_numpy(hip.curve_edges(n, k)).to(dev) for k in ("logit", "probability")} for n in (101, 1024)}
    variants, slow, keep = {}, set(), []

    def curve(z, t, form, kind, e, ws=None):
        hist = torch.empty(z.shape[0], z.shape[1], 2, e.numel() + 1, device=dev, dtype=torch.int64)
        return lambda: hip.curve_hist(z, t, form, kind, e, hist, ws)

    for C in (1, 9):
        d = discs(B, C, H, W, "curves_bench/discs%d" % C)
        noise = det_input((B, C, H, W), "curves_bench/n%d" % C).numpy().astype(np.float64)
        u = uniform("curves_bench/u%d" % C, B * C * H * W).reshape(B, C, H, W).clip(1e-7, 1 - 1e-7)
        maps = {"organ": (np.clip(d * 1.5, -12, 12) + noise, d > 0), "noise": (np.log(u / (1 - u)), None)}
        for name, (zz, inside) in maps.items():
            z = torch.from_numpy(zz.astype(np.float32)).to(dev)
            if inside is None:
                inside = uniform("curves_bench/t%d" % C, B * C * H * W).reshape(B, C, H, W) < 0.3
            t = torch.from_numpy(inside.astype(np.int64)).to(dev)
            t8 = t.to(torch.uint8)
            st = torch.empty(B, C, 4, device=dev, dtype=torch.int64)
            for n in (101, 1024):
                variants["curve_sig_c%d_%s_n%d_i64" % (C, name, n)] = curve(z, t, hip.CURVE_PLANES, hip.CURVE_RAW, edges[n]["logit"])
            variants["curve_sig_c%d_%s_n101_u8" % (C, name)] = curve(z, t8, hip.CURVE_PLANES, hip.CURVE_RAW, edges[101]["logit"])
            if C == 1 and name == "organ":
                variants["curve_sig_c1_organ_n101_i64_b"] = curve(z, t, hip.CURVE_PLANES, hip.CURVE_RAW, edges[101]["logit"])
            variants["stats_c%d_%s" % (C, name)] = lambda z=z, t=t, st=st: hip.sigmoid_stats(z, t, 0.0, st, None)
            variants["eager_c%d_%s_n101" % (C, name)] = eager(z, t, edges[101]["logit"])
            slow.add("eager_c%d_%s_n101" % (C, name))
            keep.append((z, t, t8, st))
    # softmax scores at C = 9 against an int64 label map: the organs are the discs, class 0 the background
    C = 9
    d = discs(B, C, H, W, "curves_bench/sdiscs")
    d[:, 0] = 4.0
    lab = torch.from_numpy(np.argmax(d, 1).astype(np.int64)).to(dev)
    ws = torch.empty(hip.curve_workspace(hip.CURVE_SOFTMAX, B, H * W), device=dev, dtype=torch.uint8)
    noise = det_input((B, C, H, W), "curves_bench/sn").numpy().astype(np.float64)
    for name, zz in (("organ", np.clip(d * 1.5, -12, 12) + noise), ("noise", 2.0 * noise)):
        z = torch.from_numpy(zz.astype(np.float32)).to(dev)
        for n in (101, 1024):
            variants["curve_softmax_c9_%s_n%d_i64" % (name, n)] = curve(z, lab, hip.CURVE_LABELS, hip.CURVE_SOFTMAX, edges[n]["probability"], ws)
        keep.append(z)

    out = {"what": "B=8 352x352, us per call (median of %d rounds x %d calls, variants alternating; eager: %d calls)"
                   % (a.rounds, a.iters, max(1, a.iters // 10))}
    iters = {k: max(1, a.iters // 10) if k in slow else a.iters for k in variants}
    for k, f in variants.items():
        for _ in range(1 if k in slow else a.warmup):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, f in variants.items():
            us[k].append(timed(f, iters[k]))
    r = {k: round(statistics.median(v), 2) for k, v in us.items()}
    out["us"] = r
    aa = abs(r["curve_sig_c1_organ_n101_i64"] - r["curve_sig_c1_organ_n101_i64_b"]) / r["curve_sig_c1_organ_n101_i64"]
    out["aa_spread"] = round(aa, 4)
    out["over_stats"] = {k: round(v / r["stats_c%s_%s" % (k.split("_")[2][1:], k.split("_")[3])], 3) for k, v in r.items() if k.startswith("curve_sig") and not k.endswith("_b")}
    pairs = {k: round(v / r[k.replace("_organ_", "_noise_")], 3) for k, v in r.items() if "_organ_" in k and k.startswith("curve") and not k.endswith("_b")}
    out["organ_over_noise"] = pairs
    out["ballot_route_ok"] = bool(all(v <= 1 + aa for v in pairs.values()))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""VolumeSurfaceMeter.update() cost on one case of 128 x 352 x 352: the ellipsoid organs of tests/volume_ref.py at 2 and 9 classes, at
spacing (1, 1, 1) and at the thick slices (4, 1, 1).  Per variant the median over --rounds of device-event timings of --iters calls
each (the uint8 narrowing, workspace and statistics allocation and all four kernels included; the variants alternate inside a round,
so drift of the clocks lands on all of them), an A/A spread -- the first variant timed a second time in the same rounds, relative
difference of the two medians -- and one host run per variant of the numpy restatement (tests/volume_ref.py case_stats, which already
crops every class to its bounding box) on the same case for context.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/gpu_volume_bench.py`.  Prints one JSON line; --out writes it to a file as well
(profiles/volume_bench.json)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import volume_ref as R  # noqa: E402
from lm_net_amd.metrics import VolumeSurfaceMeter  # noqa: E402


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
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 352, 352), metavar=("D", "H", "W"))
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement timing")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    D, H, W = a.shape
    steps = {}
    for C in (2, 9):
        pred, target = R.ellipsoid_case(D, H, W, C)
        p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda()
        for spacing in ((1, 1, 1), (4, 1, 1)):
            m = VolumeSurfaceMeter(C, spacing=spacing, workspace_mb=4096)

            def step(m=m, p=p, t=t):
                m.update(p, t)
                m.reset()
            steps["ellipsoids_%d_classes_spacing_%d%d%d" % ((C,) + spacing)] = (step, pred, target, m)
    names = list(steps)
    order = names + [names[0] + "_again"]                          # the A/A pair
    for name in names:
        for _ in range(a.warmup):
            steps[name][0]()
    torch.cuda.synchronize()
    us = {name: [] for name in order}
    for _ in range(a.rounds):
        for name in order:
            us[name].append(timed(steps[name.replace("_again", "")][0], a.iters))
    med = {name: statistics.median(v) for name, v in us.items()}
    out = {"what": "VolumeSurfaceMeter.update, one case of %dx%dx%d, us per call (median of %d rounds x %d calls, variants alternating)"
                   % (D, H, W, a.rounds, a.iters),
           "us": {name: round(med[name], 1) for name in names}, "us_min": {name: round(min(us[name]), 1) for name in names},
           "aa_spread": round(abs(med[order[-1]] - med[names[0]]) / med[names[0]], 4)}
    if not a.no_host:
        out["numpy_restatement_host_us"] = {}
        for name in names:
            _, pred, target, m = steps[name]
            t0 = time.perf_counter()
            R.case_stats(pred, target, m.classes, m.spacing)
            out["numpy_restatement_host_us"][name] = round((time.perf_counter() - t0) * 1e6, 1)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

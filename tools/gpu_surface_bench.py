"""SurfaceDistanceMeter.update() cost at batch 8, 352x352: the ellipse masks of tests/surface_ref.py at 2 and 9 classes and 50 %
noise at 2 classes.  Per case the median over --rounds of device-event timings of --iters calls each (workspace and statistics
allocation and all four kernels included), and the host time of the numpy restatement (tests/surface_ref.py batch_stats) on the same
batch -- the per-batch CPU work the meter replaces -- and, as the second yardstick, the eval-mode forward of LM_Net(3, C) on the same
batch size (eager, fp32, device events).  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/gpu_surface_bench.py`.  Prints one JSON line."""
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

import surface_ref as S  # noqa: E402
from lm_net_amd.metrics import SurfaceDistanceMeter  # noqa: E402


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
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy reference timing")
    ap.add_argument("--no-forward", action="store_true", help="skip the eval forward timing")
    a = ap.parse_args()
    B, H, W = 8, 352, 352
    rng = np.random.default_rng(0)
    noise = tuple((rng.random((B, H, W)) < 0.5).astype(np.int64) for _ in range(2))
    out = {"what": "SurfaceDistanceMeter.update B=8 352x352, us per call (median of %d rounds x %d calls)" % (a.rounds, a.iters)}
    for name, C, (pred, target) in (("ellipses_2_classes", 2, S.ellipse_case(B, H, W, 2)), ("ellipses_9_classes", 9, S.ellipse_case(B, H, W, 9)),
                                    ("noise_2_classes", 2, noise)):
        m = SurfaceDistanceMeter(C)
        p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda()

        def step():
            m.update(p, t)
            m.reset()
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        us = [timed(step, a.iters) for _ in range(a.rounds)]
        out[name] = {"update_us_median": round(statistics.median(us), 1), "update_us_min": round(min(us), 1)}
        if not a.no_host:
            t0 = time.perf_counter()
            S.batch_stats(pred, target, m.classes)
            out[name]["numpy_reference_host_us"] = round((time.perf_counter() - t0) * 1e6, 1)
    if not a.no_forward:
        from lm_net_amd import LM_Net
        x = torch.randn(B, 3, H, W, device="cuda")
        for C in (2, 9):
            net = LM_Net(3, C).cuda().eval()
            with torch.no_grad():
                for _ in range(a.warmup):
                    net(x)
                torch.cuda.synchronize()
                us = [timed(lambda: net(x), a.iters) for _ in range(a.rounds)]
            out["eval_forward_%d_classes_us_median" % C] = round(statistics.median(us), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""DevicePostprocess cost at batch 8, 352x352: the organ-like maps of tests/post_ref.py (punched ellipses) at 2 and 9 classes and
50 % noise at 2 classes.  Per case the median over --rounds of device-event timings of --iters calls each, after warm-up:
  clean_us     post(pred) with keep_largest, min_area = 12 and hole filling on (allocations and all launches included),
  render_us    the render alone (lmn_post_render: labels and a fill overlay at alpha 0.4 on 704 x 704 frames),
  total_us     post(pred, frames=frames): cleaning plus render in one call,
  numpy_reference_host_us   the numpy restatement (tests/post_ref.py: clean, resize_back, overlay) of the same batch on the host, ONE
                            thread of the CPU (numpy is not threaded here, whatever the machine offers),
and, as the yardstick, the eval-mode forward of LM_Net(3, C) on the same batch (eager, fp32, device events) in the same run.
`forward_bound` = total_us < the forward of the same class count, on the organ-like maps (the noise map is reported, not gated); the
tool exits non-zero when it is false.
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/gpu_post_bench.py --no-host`.  Prints one JSON line."""
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

import post_ref as R  # noqa: E402
from lm_net_amd import hip  # noqa: E402
from lm_net_amd.post import DevicePostprocess  # noqa: E402


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
    ap.add_argument("--host-repeats", type=int, default=3, help="timed runs of the numpy reference per case (after one warm-up)")
    ap.add_argument("--no-forward", action="store_true", help="skip the eval forward timing")
    a = ap.parse_args()
    B, H, W, Hs, Ws = 8, 352, 352, 704, 704
    kw = dict(keep_largest=True, min_area=12, fill_holes=True)
    frames_h = np.random.default_rng(1).integers(0, 256, (B, Hs, Ws, 3)).astype(np.uint8)
    frames = torch.from_numpy(frames_h).cuda()
    out = {"what": "DevicePostprocess B=8 352x352 -> 704x704, us per call (median of %d rounds x %d calls)" % (a.rounds, a.iters),
           "tile": "32x64", "lds_bytes_per_block": 10240}

    def median(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        us = [timed(fn, a.iters) for _ in range(a.rounds)]
        return round(statistics.median(us), 1), round(min(us), 1)

    cases = (("organs_2_classes", 2, R.punched_ellipses(B, H, W, 2)), ("organs_9_classes", 9, R.punched_ellipses(B, H, W, 9)),
             ("noise_2_classes", 2, R.noise_case(B, H, W)))
    for name, C, pred in cases:
        post = DevicePostprocess(C, alpha=0.4, **kw)
        p = torch.from_numpy(pred).cuda()
        res = post(p, frames=frames)
        labels, overlay = torch.empty_like(res.labels), torch.empty_like(res.overlay)
        r = {}
        r["clean_us"], r["clean_us_min"] = median(lambda: post(p))
        r["render_us"], _ = median(lambda: hip.post_render(res.labels_net, None, Hs, Ws, frames, post.palette, C, post.alpha256, post.mode,
                                                         labels, overlay))
        r["total_us"], r["total_us_min"] = median(lambda: post(p, frames=frames))
        if not a.no_host:
            tc, tr = [], []
            for rep in range(1 + a.host_repeats):                    # one warm-up run, then the median of the repeats
                t0 = time.perf_counter()
                net = R.clean(pred, C, connectivity=8, **kw)[0]
                t1 = time.perf_counter()
                lab = R.resize_back(net, [(Hs, Ws)] * B, Hs, Ws)
                R.overlay(lab, frames_h, [(Hs, Ws)] * B, post.palette, 0.4, "fill")
                t2 = time.perf_counter()
                if rep:
                    tc.append((t1 - t0) * 1e6)
                    tr.append((t2 - t1) * 1e6)
            r["numpy_reference_host_us"] = {"clean": round(statistics.median(tc), 1), "render": round(statistics.median(tr), 1),
                                            "threads": 1, "repeats": a.host_repeats}
        out[name] = r
    if not a.no_forward:
        from lm_net_amd import LM_Net
        x = torch.randn(B, 3, H, W, device="cuda")
        for C in (2, 9):
            net = LM_Net(3, C).cuda().eval()
            with torch.no_grad():
                out["eval_forward_%d_classes_us" % C], _ = median(lambda: net(x))
        out["forward_bound"] = bool(out["organs_2_classes"]["total_us"] < out["eval_forward_2_classes_us"]
                                    and out["organs_9_classes"]["total_us"] < out["eval_forward_9_classes_us"])
    print(json.dumps(out))
    if out.get("forward_bound") is False:
        sys.exit("gpu_post_bench: cleaning plus render is NOT cheaper than the eval forward on the organ-like maps")


if __name__ == "__main__":
    main()

"""VolumePostprocess cost on one case of 128 x 352 x 352: ellipsoid organs with debris and cavities (tests/volpost_ref.py bench_case)
at 2 and 9 classes and at connectivity 6 and 26, with keep_largest, min_volume and fill_holes (both labellings, one selection pass, the
hole filling; the uint8 narrowing and the workspace allocation included).  Per variant the median over --rounds of device-event timings
of --iters calls each; the variants alternate inside a round, so drift of the clocks lands on all of them, and the first variant is
timed a second time in the same rounds (the A/A pair: relative difference of the two medians).  Four yardsticks in the same process and
the same rounds: DevicePostprocess over the same slices in batches of 8 (it reads the same bytes and does the 2D work),
VolumeSurfaceMeter.update on the same case, the eval forward of LM_Net(3, C) over the same number of slices in batches of 8, and -- on
the host, once -- the numpy restatement and, where scipy is installed, ndimage.label + binary_fill_holes per class.  Kernel times: run
it under `rocprofv3 --kernel-trace --stats -- python tools/gpu_volpost_bench.py`.  Prints one JSON line; --out writes it to a file as
well (profiles/volpost_bench.json)."""
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

import volpost_ref as R  # noqa: E402
import volume_ref as VR  # noqa: E402
from lm_net_amd import LM_Net, VolumePostprocess, VolumeSurfaceMeter  # noqa: E402
from lm_net_amd.post import DevicePostprocess  # noqa: E402

MIN_VOLUME = 20


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters   # us per call


def scipy_clean(L0, C, connectivity):
    """The host route this class replaces: per class ndimage.label, the largest component above MIN_VOLUME, then binary_fill_holes."""
    from scipy import ndimage as ndi
    st = ndi.generate_binary_structure(3, R.ORDER[connectivity])
    out = np.zeros_like(L0)
    for k in range(1, C):
        lab, n = ndi.label(L0 == k, structure=st)
        if n:
            sizes = np.bincount(lab.ravel())[1:]
            if sizes.max() >= MIN_VOLUME:
                out[lab == 1 + int(sizes.argmax())] = k
    filled = ndi.binary_fill_holes(out > 0, structure=ndi.generate_binary_structure(3, R.ORDER[R.DUAL[connectivity]]))
    return out, filled


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 352, 352), metavar=("D", "H", "W"))
    ap.add_argument("--no-host", action="store_true", help="skip the host timings (numpy restatement, scipy)")
    ap.add_argument("--no-forward", action="store_true", help="skip the eval forward")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    D, H, W = a.shape
    steps, host = {}, {}
    for C in (2, 9):
        pred = R.bench_case(D, H, W, C)
        _, target = VR.ellipsoid_case(D, H, W, C)
        p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda()
        for conn in (6, 26):
            post = VolumePostprocess(C, connectivity=conn, keep_largest=True, min_volume=MIN_VOLUME, fill_holes=True)
            steps["volpost_%d_classes_conn_%d" % (C, conn)] = lambda post=post, p=p: post(p)
            host["volpost_%d_classes_conn_%d" % (C, conn)] = (pred, C, conn)
        post2d = DevicePostprocess(C, connectivity=8, keep_largest=True, min_area=MIN_VOLUME, fill_holes=True)

        def slices(post2d=post2d, p=p):
            for z in range(0, D, 8):
                post2d(p[z:z + 8])
        steps["post2d_slices_of_8_%d_classes" % C] = slices
        meter = VolumeSurfaceMeter(C, workspace_mb=4096)

        def score(meter=meter, p=p, t=t):
            meter.update(p, t)
            meter.reset()
        steps["volume_meter_%d_classes" % C] = score
        if not a.no_forward:
            net = LM_Net(3, C).cuda().eval()
            x = torch.randn(8, 3, H, W, device="cuda")

            def forward(net=net, x=x):
                with torch.no_grad():
                    for _ in range(0, D, 8):
                        net(x)
            steps["eval_forward_%d_classes" % C] = forward
    names = list(steps)
    order = names + [names[0] + "_again"]                          # the A/A pair
    for name in names:
        for _ in range(a.warmup):
            steps[name]()
    torch.cuda.synchronize()
    us = {name: [] for name in order}
    for _ in range(a.rounds):
        for name in order:
            us[name].append(timed(steps[name.replace("_again", "")], a.iters))
    med = {name: statistics.median(v) for name, v in us.items()}
    out = {"what": "one case of %dx%dx%d, us per case (median of %d rounds x %d calls, variants alternating): VolumePostprocess (keep_largest, "
                   "min_volume=%d, fill_holes) and its yardsticks on the same slices" % (D, H, W, a.rounds, a.iters, MIN_VOLUME),
           "device": torch.cuda.get_device_name(0),
           "us": {name: round(med[name], 1) for name in names}, "us_min": {name: round(min(us[name]), 1) for name in names},
           "aa_spread": round(abs(med[order[-1]] - med[names[0]]) / med[names[0]], 4)}
    if not a.no_host:
        out["numpy_restatement_host_us"], out["scipy_host_us"] = {}, {}
        for name, (pred, C, conn) in host.items():
            t0 = time.perf_counter()
            L2, stats, info = R.clean(pred, C, conn, keep_largest=True, min_volume=MIN_VOLUME, fill_holes=True)
            out["numpy_restatement_host_us"][name] = round((time.perf_counter() - t0) * 1e6, 1)
            got = steps[name]()
            if not (np.array_equal(got.labels.cpu().numpy(), L2) and np.array_equal(got.stats.cpu().numpy(), stats)):
                sys.exit("gpu_volpost_bench: %s differs from the restatement" % name)
            out.setdefault("removed_components", {})[name] = int((stats[1:, 0] - stats[1:, 1]).sum())
            out.setdefault("holes_filled", {})[name] = int(stats[0, 3])
            try:
                import scipy.ndimage  # noqa: F401
            except ImportError:
                out["scipy_host_us"][name] = None
                continue
            t0 = time.perf_counter()
            _, filled = scipy_clean(info["L0"], C, conn)
            out["scipy_host_us"][name] = round((time.perf_counter() - t0) * 1e6, 1)
            if not np.array_equal(filled, L2 > 0):
                sys.exit("gpu_volpost_bench: %s differs from scipy" % name)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""LesionMeter cost on one case of 128 x 352 x 352: ellipsoid organs with debris and cavities (tests/volpost_ref.py bench_case)
against a perturbed copy (shifted by one voxel along x, 0.1 % of the voxels cleared) at 2 and 9 classes, and two identical full masks
-- one pair that holds every voxel, the single-hot-key case of the pair table.  LesionMeter.update includes the uint8 narrowing, both
labellings, the match pass, the two sorts and the allocations.  Per variant the median over --rounds of device-event timings of
--iters calls each; the variants alternate inside a round, so drift of the clocks lands on all of them, and the first variant is timed
a second time in the same rounds (the A/A pair: relative difference of the two medians).  Yardsticks in the same process and the same
rounds: VolumePostprocess and VolumeSurfaceMeter.update on the same case; on the host, once, the numpy restatement (whose records must
equal the device's) and, where scipy is installed, ndimage.label of both volumes per class plus the join by np.unique -- the route
this class replaces.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/gpu_lesion_bench.py`.  Prints one
JSON line; --out writes it to a file as well (profiles/lesion_bench.json)."""
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

import lesion_ref as LR  # noqa: E402
import volpost_ref as R  # noqa: E402
from lm_net_amd import LesionMeter, VolumePostprocess, VolumeSurfaceMeter  # noqa: E402

CONNECTIVITY = 26
CAP = dict(max_components=1 << 16, max_pairs=1 << 15)


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters   # us per call


def perturbed(pred, seed=7):
    target = np.roll(pred, 1, axis=2)
    target[:, :, 0] = 0
    target[np.random.default_rng(seed).random(pred.shape) < 0.001] = 0
    return target


def scipy_join(Lp, Lt, C):
    """The host route: per class ndimage.label of both volumes, then the pairs and their counts by np.unique over the stacked ids."""
    from scipy import ndimage as ndi
    st = ndi.generate_binary_structure(3, R.ORDER[CONNECTIVITY])
    lesions = pairs = 0
    for k in range(1, C):
        lp, n_p = ndi.label(Lp == k, structure=st)
        lt, n_t = ndi.label(Lt == k, structure=st)
        both = (lp > 0) & (lt > 0)
        pairs += np.unique(lp[both].astype(np.int64) << 32 | lt[both]).size
        lesions += n_p + n_t
    return lesions, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 352, 352), metavar=("D", "H", "W"))
    ap.add_argument("--no-host", action="store_true", help="skip the host timings (numpy restatement, scipy)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    D, H, W = a.shape
    steps, host = {}, {}

    def lesion(C, p, t):
        meter = LesionMeter(C, connectivity=CONNECTIVITY, workspace_mb=4096, **CAP)

        def run():
            meter.reset()
            meter.update(p, t)
            return meter
        return run

    for C in (2, 9):
        pred = R.bench_case(D, H, W, C)
        target = perturbed(pred)
        p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda()
        steps["lesion_%d_classes" % C] = lesion(C, p, t)
        host["lesion_%d_classes" % C] = (pred, target, C)
        post = VolumePostprocess(C, connectivity=CONNECTIVITY, keep_largest=True, min_volume=20, fill_holes=True)
        steps["volpost_%d_classes" % C] = lambda post=post, p=p: post(p)
        vmeter = VolumeSurfaceMeter(C, workspace_mb=4096)

        def score(vmeter=vmeter, p=p, t=t):
            vmeter.update(p, t)
            vmeter.reset()
        steps["volume_meter_%d_classes" % C] = score
    ones = torch.ones(D, H, W, dtype=torch.int64, device="cuda")
    steps["lesion_two_full_masks"] = lesion(2, ones, ones)
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
    out = {"what": "one case of %dx%dx%d, us per case (median of %d rounds x %d calls, variants alternating): LesionMeter.update "
                   "(connectivity %d) and its yardsticks on the same case" % (D, H, W, a.rounds, a.iters, CONNECTIVITY),
           "device": torch.cuda.get_device_name(0),
           "us": {name: round(med[name], 1) for name in names}, "us_min": {name: round(min(us[name]), 1) for name in names},
           "aa_spread": round(abs(med[order[-1]] - med[names[0]]) / med[names[0]], 4)}
    full = [int(v) for v in steps["lesion_two_full_masks"]().raw()[4][0].tolist()]
    if full != [2, 1, 0, 0]:
        sys.exit("gpu_lesion_bench: two full masks gave ctrl %r" % (full,))
    if not a.no_host:
        out["numpy_restatement_host_us"], out["scipy_host_us"], out["lesions"], out["pairs"] = {}, {}, {}, {}
        for name, (pred, target, C) in host.items():
            meter = steps[name]()
            t0 = time.perf_counter()
            want = LR.records(pred, target, C, CONNECTIVITY, None, meter.max_components, meter.pair_slots)
            out["numpy_restatement_host_us"][name] = round((time.perf_counter() - t0) * 1e6, 1)
            if not all(np.array_equal(g[0].cpu().numpy(), w) for g, w in zip(meter.raw(), want)):
                sys.exit("gpu_lesion_bench: %s differs from the restatement" % name)
            out["lesions"][name], out["pairs"][name] = int(want[4][0]), int(want[4][1])
            try:
                import scipy.ndimage  # noqa: F401
            except ImportError:
                out["scipy_host_us"][name] = None
                continue
            t0 = time.perf_counter()
            got = scipy_join(LR.clamp(pred, C), LR.clamp(target, C), C)
            out["scipy_host_us"][name] = round((time.perf_counter() - t0) * 1e6, 1)
            if got != (int(want[4][0]), int(want[4][1])):
                sys.exit("gpu_lesion_bench: %s: scipy counts %r lesions and pairs" % (name, got))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

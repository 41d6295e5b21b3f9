"""Cost of the distance maps and their losses at batch 8, 352 x 352, C = 2 and 9 (classes 1 .. C - 1): lmn_dist_map from labels and
from logits on organ-like masks, on noise labels (50 % per plane at C = 2) and on ONE mask pixel per plane -- the worst case of the
row pass's outward scan, O(W) steps for every pixel; BoundaryLoss and HausdorffDTLoss forward plus backward (their maps included);
and the yardsticks on the same batch: SegLoss forward plus backward, lmn_surface_dist, the eval forward of LM_Net(3, C).  Per variant
the median over --rounds of device-event timings of --iters calls each; the variants alternate inside a round, so drift of the clocks
lands on all of them, and the first variant is timed a second time in the same rounds (the A/A pair: relative difference of the two
medians).  On the host, once, where scipy is installed: scipy.ndimage.distance_transform_edt of the mask and of its complement over
the same planes -- the route these entries replace -- whose squares must equal the device's maps.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/gpu_distmap_bench.py`.  Prints one JSON line; --out writes it to a file as well
(profiles/distmap_bench.json)."""
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

import distmap_ref as R  # noqa: E402
from lm_net_amd import LM_Net, BoundaryLoss, HausdorffDTLoss, SegLoss, distance_maps, hip  # noqa: E402


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters   # us per call


def label_maps(B, H, W, C, seed=0):
    """{kind: int64 [B, H, W]}: nested blobs, uniform noise over the classes, one pixel per scored class."""
    rng = np.random.default_rng([seed, C])
    organ = np.zeros((B, H, W), np.int64)
    for b in range(B):
        for c in range(1, C):
            organ[b][R.blobs(H, W, rng, 2)] = c
    one = np.zeros((B, H, W), np.int64)
    for c in range(1, C):
        one[:, (37 * c) % H, (91 * c) % W] = c
    return {"organ": organ, "noise": rng.integers(0, C, (B, H, W)), "one_pixel": one}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=(352, 352), metavar=("H", "W"))
    ap.add_argument("--no-host", action="store_true", help="skip the scipy timing")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    B, (H, W) = a.batch, a.size
    steps, host = {}, {}
    for C in (2, 9):
        classes = list(range(1, C))
        for kind, y_np in label_maps(B, H, W, C).items():
            y = torch.from_numpy(y_np).cuda()
            lg = torch.from_numpy(R.logits_of_labels(y_np, C, "softmax")).cuda()
            steps["map_labels_%s_%d" % (kind, C)] = lambda y=y, C=C: distance_maps(y, C)
            steps["map_logits_%s_%d" % (kind, C)] = lambda lg=lg, C=C: distance_maps(lg, C, mode="softmax")
            if kind == "organ":
                host[C] = (y_np, classes)
                z = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(C)).mul_(2.5).cuda()

                def train(crit, z=z, y=y):
                    def run():
                        zz = z.detach().requires_grad_(True)
                        crit(zz, y).backward()
                    return run
                steps["boundary_loss_%d" % C] = train(BoundaryLoss(C))
                steps["hausdorff_loss_%d" % C] = train(HausdorffDTLoss(C))
                steps["seg_loss_%d" % C] = train(SegLoss(ce_weight=None, dice_weight=None).cuda())
                ws = torch.empty(hip.surface_workspace(B, C - 1, H, W), dtype=torch.uint8, device="cuda")
                si = torch.empty(B, C - 1, 8, dtype=torch.int64, device="cuda")
                sf = torch.empty(B, C - 1, 2, dtype=torch.float64, device="cuda")
                steps["surface_dist_%d" % C] = lambda z=z, y=y, C=C, classes=classes, ws=ws, si=si, sf=sf: hip.surface_dist(z, y, C, classes, ws, si, sf)
                net = LM_Net(3, C).cuda().eval()
                x = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(1)).cuda()

                def forward(net=net, x=x):
                    with torch.no_grad():
                        net(x)
                steps["model_eval_forward_%d" % C] = forward
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
    out = {"what": "batch %d of %dx%d, us per call (median of %d rounds x %d calls, variants alternating): lmn_dist_map, the two "
                   "losses forward + backward with their maps, and their yardsticks on the same batch" % (B, H, W, a.rounds, a.iters),
           "device": torch.cuda.get_device_name(0),
           "us": {name: round(med[name], 1) for name in names}, "us_min": {name: round(min(us[name]), 1) for name in names},
           "aa_spread": round(abs(med[order[-1]] - med[names[0]]) / med[names[0]], 4)}
    if not a.no_host:
        out["scipy_edt_host_us"] = {}
        for C, (y_np, classes) in host.items():
            try:
                from scipy import ndimage as ndi
            except ImportError:
                out["scipy_edt_host_us"]["organ_%d" % C] = None
                continue
            got = distance_maps(torch.from_numpy(y_np).cuda(), C)[0].cpu().numpy()
            masks = R.masks_of_labels(y_np, classes)
            t0 = time.perf_counter()
            both = [[ndi.distance_transform_edt(m) + ndi.distance_transform_edt(~m) for m in sample] for sample in masks]
            out["scipy_edt_host_us"]["organ_%d" % C] = round((time.perf_counter() - t0) * 1e6, 1)
            for b, sample in enumerate(masks):
                for k, m in enumerate(sample):
                    if 0 < m.sum() < m.size and not np.array_equal(np.rint(both[b][k] ** 2).astype(np.int64), np.abs(got[b, k])):
                        sys.exit("gpu_distmap_bench: sample %d class %d differs from scipy" % (b, classes[k]))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

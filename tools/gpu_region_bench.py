"""Cost of the region-overlap losses at batch 8, 352 x 352, C = 2 and 9: RegionLoss forward plus backward for each kind, per batch and
per image, under a softmax head (and the Dice under a sigmoid head); and the yardsticks on the same batch: SegLoss(ce_scale=0)
forward plus backward, which reads the same bytes, and the eager torch composition of the same loss (softmax, one-hot, masked sums, the
ratio, through autograd).  Per variant the median over --rounds of device-event timings of --iters calls each; the variants alternate
inside a round, so drift of the clocks lands on all of them, and the first variant is timed a second time in the same rounds (the A/A
pair: relative difference of the two medians).  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/gpu_region_bench.py`.  Prints one JSON line; --out writes it to a file as well
(profiles/region_bench.json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from lm_net_amd import RegionLoss, SegLoss  # noqa: E402

KINDS = ("dice", "jaccard", "tversky", "generalized_dice")


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters   # us per call


def eager_region(logits, labels, kind, per_image, smooth=1e-5, alpha=0.5, beta=0.5):
    """The usual composition (no void, all classes): what these entries replace."""
    C = logits.shape[1]
    p = torch.softmax(logits, 1)
    t = torch.nn.functional.one_hot(labels, C).permute(0, 3, 1, 2).float()
    dims = (2, 3) if per_image else (0, 2, 3)
    I, P1, T = (p * t).sum(dims), p.sum(dims), t.sum(dims)
    if kind == "dice":
        R = (2 * I + smooth) / ((p * p).sum(dims) + T + smooth)
    elif kind == "jaccard":
        R = (I + smooth) / ((p * p).sum(dims) + T - I + smooth)
    elif kind == "tversky":
        R = (I + smooth) / (I + alpha * (P1 - I) + beta * (T - I) + smooth)
    else:
        v = 1.0 / (T * T).clamp_min(1.0)
        R = (2 * (v * I).sum(-1) + smooth) / ((v * (P1 + T)).sum(-1) + smooth)
    return (1 - R).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=(352, 352), metavar=("H", "W"))
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    B, (H, W) = a.batch, a.size
    steps = {}
    for C in (2, 9):
        gen = torch.Generator().manual_seed(C)
        z = torch.randn(B, C, H, W, generator=gen).mul_(2.5).cuda()
        y = torch.randint(0, C, (B, H, W), generator=gen).cuda()
        t = torch.randint(0, 2, (B, C, H, W), generator=gen, dtype=torch.uint8).cuda()

        def train(crit, target, z=z):
            def run():
                zz = z.detach().requires_grad_(True)
                crit(zz, target).backward()
            return run
        steps["seg_loss_dice_only_%d" % C] = train(SegLoss(ce_weight=None, dice_weight=None, ce_scale=0.0).cuda(), y)
        for per_image in (False, True):
            tag = "image" if per_image else "batch"
            for kind in KINDS:
                steps["%s_softmax_%s_%d" % (kind, tag, C)] = train(RegionLoss(C, kind=kind, per_image=per_image), y)

                def eager(z=z, y=y, kind=kind, per_image=per_image):
                    zz = z.detach().requires_grad_(True)
                    eager_region(zz, y, kind, per_image).backward()
                steps["eager_torch_%s_%s_%d" % (kind, tag, C)] = eager
            steps["dice_sigmoid_%s_%d" % (tag, C)] = train(RegionLoss(C, head="sigmoid", per_image=per_image), t)
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
    out = {"what": "batch %d of %dx%d, us per call (median of %d rounds x %d calls, variants alternating): RegionLoss forward + backward, "
                   "SegLoss(ce_scale=0) and the eager torch composition on the same batch" % (B, H, W, a.rounds, a.iters),
           "device": torch.cuda.get_device_name(0),
           "us": {name: round(med[name], 1) for name in names}, "us_min": {name: round(min(us[name]), 1) for name in names},
           "aa_spread": round(abs(med[order[-1]] - med[names[0]]) / med[names[0]], 4)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

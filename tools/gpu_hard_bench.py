"""Cost of the hard-pixel criterion at batch 8, 352 x 352: HardPixelLoss forward plus backward under a softmax head at 2 and 9 classes
and under a sigmoid head at 1 and 9 planes, in its top-k form (keep=0.1) and its OHEM form (thresh=0.7, min_kept=100000), on two kinds
of logits -- ORGAN-LIKE maps (ellipses per class, confident logits with a noisy rim: most values fall into a few exponent bins of the
level-1 histogram, the case of a trained network) and NOISE (Gaussian logits against random labels: the values spread over many
bins) -- and the yardsticks on the same batch: SegLoss forward plus backward and the eager composition that the criterion replaces,
F.cross_entropy(reduction="none") + torch.topk (with the .item() that a data-dependent K needs in its OHEM form).  The forward alone
(hard_pixel_values) is timed on both kinds of logits too: the organ / noise ratio of it is the cost of colliding LDS atomics in the
values pass.  Per variant the median over --rounds of device-event timings of --iters calls each; the variants alternate
inside a round, so drift of the clocks lands on all of them, and the first variant is timed a second time in the same rounds (the A/A
pair: relative difference of the two medians).  Afterwards the top-k variants run once more under the in-library kernel timer
(hip.prof_begin / prof_end: HIP events around every launch): "kernel_us" holds the mean device time per launch of every kernel of the
family, forward and backward, for each head, class count and kind of logits.  Prints one JSON line; --out writes it to a file as well
(profiles/hard_bench.json)."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from lm_net_amd import HardPixelLoss, SegLoss, hard_pixel_values, hip  # noqa: E402

MODES = {"topk": dict(keep=0.1), "ohem": dict(thresh=0.7, min_kept=100000)}


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters   # us per call


def organ_labels(B, C, H, W, gen):
    """int64 label maps: one ellipse per class 1 .. C - 1 and image on background 0"""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    y = torch.zeros(B, H, W, dtype=torch.int64)
    for b in range(B):
        for k in range(1, max(C, 2)):
            cy, cx, ry, rx = (float(v) for v in torch.rand(4, generator=gen))
            inside = ((yy - (0.2 + 0.6 * cy) * H) / ((0.05 + 0.15 * ry) * H)) ** 2 + ((xx - (0.2 + 0.6 * cx) * W) / ((0.05 + 0.15 * rx) * W)) ** 2 <= 1.0
            y[b][inside] = k
    return y


def organ_logits(y, C, gen, sigmoid):
    """confident logits of the label map: +-6 with unit noise, and a wrong answer on 3 % of the pixels"""
    B, H, W = y.shape
    wrong = torch.rand(B, H, W, generator=gen) < 0.03
    said = torch.where(wrong, (y + 1) % max(C, 2), y)
    onehot = F.one_hot(said, max(C, 2)).permute(0, 3, 1, 2).float()
    if sigmoid and C == 1:
        onehot = onehot[:, 1:]
    return ((12.0 * onehot - 6.0) + torch.randn(onehot.shape, generator=gen)).contiguous()


def eager_hard(logits, y, keep=None, thresh=None, min_kept=0):
    """F.cross_entropy(reduction="none") + torch.topk; a threshold needs the count on the host"""
    l = F.cross_entropy(logits, y, reduction="none").flatten()
    K = max(1, int(l.numel() * keep)) if keep is not None else 1
    if thresh is not None:
        K = max(K, min_kept, int((l > -math.log(thresh)).sum().item()))
    return torch.topk(l, min(K, l.numel())).values.mean()


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

    def train(crit, z, *args):
        def run():
            zz = z.detach().requires_grad_(True)
            crit(zz, *args).backward()
        return run

    for head, C in (("softmax", 2), ("softmax", 9), ("sigmoid", 1), ("sigmoid", 9)):
        gen = torch.Generator().manual_seed(10 * C + (head == "sigmoid"))
        sig = head == "sigmoid"
        labels = organ_labels(B, C, H, W, gen)
        data = {"organ": (organ_logits(labels, C, gen, sig), labels),
                "noise": (torch.randn(B, C, H, W, generator=gen).mul_(2.5), torch.randint(0, max(C, 2), (B, H, W), generator=gen))}
        for kind, (z, y) in data.items():
            z = z.cuda()
            if sig:                                        # planes: the one-hot map (C = 1: the foreground)
                t = F.one_hot(y, max(C, 2)).permute(0, 3, 1, 2)[:, (1 if C == 1 else 0):].to(torch.uint8).contiguous().cuda()
            else:
                t = y.cuda()
            tag = "%s_%d_%s" % (head, C, kind)
            for mode, kw in MODES.items():
                steps["hard_%s_%s" % (mode, tag)] = train(HardPixelLoss(C, head=head, **kw).cuda(), z, t)
            steps["hard_fwd_topk_%s" % tag] = lambda z=z, t=t, C=C, head=head: hard_pixel_values(z, t, C, head=head, keep=0.1)
            if not sig:
                steps["seg_loss_%s" % tag] = train(SegLoss(ce_weight=None, dice_weight=None).cuda(), z, t)
                for mode, kw in MODES.items():
                    steps["eager_torch_%s_%s" % (mode, tag)] = train(lambda zz, yy, kw=kw: eager_hard(zz, yy, **kw), z, t)
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
    kernel_us = {}
    for name in names:
        if name.startswith("hard_topk_"):
            hip.prof_begin(None)
            for _ in range(a.iters * 2):
                steps[name]()
            rec = hip.prof_end()
            kernel_us[name[len("hard_topk_"):]] = {k: round(v["total_us"] / v["launches"], 2) for k, v in sorted(rec.items())
                                                    if k.startswith(("hp_", "loss_zero"))}
    out = {"what": "batch %d of %dx%d, us per call (median of %d rounds x %d calls, variants alternating): HardPixelLoss forward + backward "
                   "(topk: keep=0.1; ohem: thresh=0.7, min_kept=100000), its forward alone (hard_pixel_values), SegLoss and the eager torch "
                   "composition (cross_entropy(reduction='none') + topk) on organ-like and on noise logits" % (B, H, W, a.rounds, a.iters),
           "device": torch.cuda.get_device_name(0),
           "us": {name: round(med[name], 1) for name in names}, "us_min": {name: round(min(us[name]), 1) for name in names},
           "aa_spread": round(abs(med[order[-1]] - med[names[0]]) / med[names[0]], 4), "kernel_us": kernel_us}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

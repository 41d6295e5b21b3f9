"""Cost of the soft-target criteria and the batch mixer at batch 8, 352 x 352, C = 2 and 9: SoftSegLoss forward plus backward under both
readers (a probability tensor, a Mixup pair), DistillLoss forward plus backward with an fp32 and a bf16 teacher under both heads, and
lmn_mix_batch (DeviceMix.mix on a three-channel batch with Mixup and CutMix rows); and the yardsticks on the same batch: SegLoss
forward plus backward and the eager torch compositions these entries replace (F.cross_entropy with a probability target plus the Dice
sums; log_softmax, softmax, kl_div and a mask; the indexed mix).  Per variant the median over --rounds of device-event timings of
--iters calls each; the variants alternate inside a round, so drift of the clocks lands on all of them, and the first variant is timed
a second time in the same rounds (the A/A pair: relative difference of the two medians).  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/gpu_soft_bench.py`.  Prints one JSON line; --out writes it to a file as well
(profiles/soft_bench.json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from lm_net_amd import DeviceMix, DistillLoss, MixedTarget, SegLoss, SoftSegLoss  # noqa: E402


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters   # us per call


def eager_soft(logits, q, smooth=1e-5):
    """F.cross_entropy with a probability target + the Dice of the float target (no void)."""
    p = torch.softmax(logits, 1)
    I, Z, Y = (p * q).sum((0, 2, 3)), (p * p).sum((0, 2, 3)), (q * q).sum((0, 2, 3))
    return F.cross_entropy(logits, q) + (1 - (2 * I + smooth) / (Z + Y + smooth)).mean()


def eager_kd(logits, teacher, valid, T, sigmoid):
    """The usual composition: log_softmax, softmax, kl_div and a mask (sigmoid heads: two binary cross entropies)."""
    if sigmoid:
        q = torch.sigmoid(teacher.float() / T)
        kl = F.binary_cross_entropy_with_logits(logits / T, q, reduction="none") - F.binary_cross_entropy_with_logits(teacher.float() / T, q, reduction="none")
        m = valid <= 1
    else:
        kl = F.kl_div(F.log_softmax(logits / T, 1), F.softmax(teacher.float() / T, 1), reduction="none").sum(1)
        m = valid < logits.shape[1]
    return T * T * (kl * m).sum() / m.sum().clamp_min(1)


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
    T = 4.0
    steps = {}
    for C in (2, 9):
        gen = torch.Generator().manual_seed(C)
        z = torch.randn(B, C, H, W, generator=gen).mul_(2.5).cuda()
        zt = (z + torch.randn(B, C, H, W, generator=gen).cuda()).contiguous()
        zt16 = zt.to(torch.bfloat16)
        y = torch.randint(0, C, (B, H, W), generator=gen).cuda()
        yb = y.flip(0).contiguous()
        planes = torch.randint(0, 2, (B, C, H, W), generator=gen, dtype=torch.uint8).cuda()
        q = torch.softmax(zt, 1).contiguous()
        pair = MixedTarget(y, yb, torch.rand(B, generator=gen).cuda())

        def train(crit, *args, z=z):
            def run():
                zz = z.detach().requires_grad_(True)
                crit(zz, *args).backward()
            return run
        steps["seg_loss_%d" % C] = train(SegLoss(ce_weight=None, dice_weight=None).cuda(), y)
        steps["soft_probs_%d" % C] = train(SoftSegLoss(C).cuda(), q)
        steps["soft_pair_%d" % C] = train(SoftSegLoss(C).cuda(), pair)
        steps["eager_torch_soft_probs_%d" % C] = train(eager_soft, q)
        for head, valid in (("softmax", y), ("sigmoid", planes)):
            for tag, teacher in (("f32", zt), ("bf16", zt16)):
                steps["distill_%s_%s_%d" % (head, tag, C)] = train(DistillLoss(C, temperature=T, head=head), teacher, valid)
            steps["eager_torch_distill_%s_%d" % (head, C)] = train(lambda zz, t, v, head=head: eager_kd(zz, t, v, T, head == "sigmoid"), zt, valid)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, H, W, generator=gen).cuda()
    y = torch.randint(0, 9, (B, H, W), generator=gen).cuda()
    mixer = DeviceMix(mixup_alpha=0.4, cutmix_alpha=1.0, generator=0)
    rows = mixer.sample(B, H, W)
    steps["mix_batch"] = lambda: mixer.mix(x, y, rows=rows)
    partner = torch.arange(B - 1, -1, -1).cuda()
    lam = torch.rand(B, generator=gen).cuda().view(B, 1, 1, 1)
    steps["eager_torch_mixup"] = lambda: (lam * x + (1 - lam) * x[partner], y, y[partner])
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
    out = {"what": "batch %d of %dx%d, us per call (median of %d rounds x %d calls, variants alternating): SoftSegLoss and DistillLoss forward + "
                   "backward (T = %g), DeviceMix.mix, SegLoss and the eager torch compositions on the same batch" % (B, H, W, a.rounds, a.iters, T),
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

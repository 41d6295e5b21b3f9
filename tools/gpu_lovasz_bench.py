"""Cost of the Lovasz losses at batch 8, 352 x 352, C = 2 and 9: LovaszLoss forward plus backward under both heads, per batch and
per image; the sort alone (lmn_lovasz_order on the same number of segments and elements, random keys) with the bytes its twelve
launches move as a fraction of the HBM peak; and the yardsticks on the same batch: SegLoss forward plus backward, the eager
composition everybody else runs (per class a torch.sort over all pixels, a cumsum, a gather and a dot product, through autograd) and
the eval forward of LM_Net(3, C).  Per variant the median over --rounds of device-event timings of --iters calls each; the variants
alternate inside a round, so drift of the clocks lands on all of them, and the first variant is timed a second time in the same
rounds (the A/A pair: relative difference of the two medians).  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/gpu_lovasz_bench.py`.  Prints one JSON line; --out writes it to a file as well
(profiles/lovasz_bench.json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from lm_net_amd import LM_Net, LovaszLoss, SegLoss, hip  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s, MI355X data sheet


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters   # us per call


def eager_lovasz_softmax(logits, labels):
    """The usual composition (classes="present", per batch, no void): what these entries replace."""
    C = logits.shape[1]
    p = torch.softmax(logits, 1).permute(0, 2, 3, 1).reshape(-1, C)
    lab = labels.reshape(-1)
    losses = []
    for c in range(C):
        fg = (lab == c).float()
        errors = (fg - p[:, c]).abs()
        es, perm = torch.sort(errors, dim=0, descending=True)
        gt = fg[perm]
        gts = gt.sum()
        jac = 1.0 - (gts - gt.cumsum(0)) / (gts + (1.0 - gt).cumsum(0))
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        losses.append(torch.dot(es, jac))
    return torch.stack(losses).mean()


def sort_bytes(S, P):
    """Bytes the four digit passes of lmn_lovasz_order read and write: the keys for the histogram; keys and payloads in and out of the
    scatter (no payload read in the first pass, no key written in the last); the digit table three times."""
    nb = (P + hip.LOVASZ_TILE - 1) // hip.LOVASZ_TILE
    return S * P * 4 * (4 + 4 + 3 + 3 + 4) + 4 * 3 * S * 256 * nb * 4


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
    steps, moved = {}, {}
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
        for per_image in (False, True):
            tag = "image" if per_image else "batch"
            steps["lovasz_softmax_%s_%d" % (tag, C)] = train(LovaszLoss(C, per_image=per_image), y)
            steps["lovasz_sigmoid_%s_%d" % (tag, C)] = train(LovaszLoss(C, head="sigmoid", per_image=per_image), t)
            S, P = hip.lovasz_segments(B, C, H, W, per_image)
            keys = torch.randint(-(1 << 31), 1 << 31, (S, P), generator=gen, dtype=torch.int64).to(torch.int32).cuda()
            ws = torch.empty(hip.lovasz_workspace(S, P), dtype=torch.uint8, device="cuda")
            perm = torch.empty((S, P), dtype=torch.int32, device="cuda")
            steps["sort_%s_%d" % (tag, C)] = lambda keys=keys, ws=ws, perm=perm: hip.lovasz_order(keys, ws, perm)
            moved["sort_%s_%d" % (tag, C)] = sort_bytes(S, P)
        steps["seg_loss_%d" % C] = train(SegLoss(ce_weight=None, dice_weight=None).cuda(), y)

        def eager(z=z, y=y):
            zz = z.detach().requires_grad_(True)
            eager_lovasz_softmax(zz, y).backward()
        steps["eager_torch_sort_softmax_batch_%d" % C] = eager
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
    out = {"what": "batch %d of %dx%d, us per call (median of %d rounds x %d calls, variants alternating): LovaszLoss forward + backward, "
                   "lmn_lovasz_order alone, and their yardsticks on the same batch" % (B, H, W, a.rounds, a.iters),
           "device": torch.cuda.get_device_name(0),
           "us": {name: round(med[name], 1) for name in names}, "us_min": {name: round(min(us[name]), 1) for name in names},
           "aa_spread": round(abs(med[order[-1]] - med[names[0]]) / med[names[0]], 4),
           "sort_bytes": moved,
           "sort_fraction_of_hbm_peak": {name: round(moved[name] / (med[name] * 1e-6) / HBM_PEAK, 4) for name in moved},
           "hbm_peak_bytes_per_s": HBM_PEAK}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

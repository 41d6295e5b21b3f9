"""Cost of the volume slicer on a 128 x 512 x 512 int16 case resized to 352 x 352 with context = 1 in batches of 8: the statistics
(open_case: two passes over the volume and the select) and the gather (slices: one launch), beside two yardsticks on the same output
bytes: the eager torch composition of the same batch (.float(), clamp, F.interpolate, stack) and DevicePreprocess on uint8 frames of
the same size writing the same number of fp32 bytes.  Per variant the median over --rounds of device-event timings of --iters calls
each; the variants alternate inside a round, so drift of the clocks lands on all of them, and the first variant is timed a second time
in the same rounds (the A/A pair: relative difference of the two medians).  The share of the HBM peak is the algorithmic bytes -- the
volume read twice for the statistics; the fp32 output written and the distinct source slices read once for the gather -- over the
median time, against 8 TB/s.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/gpu_slices_bench.py`.
Prints one JSON line; --out writes it to a file as well (profiles/slices_bench.json)."""
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

from lm_net_amd import VolumeSlicer  # noqa: E402
from lm_net_amd.data import DevicePreprocess  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s, the specified peak of an MI355X


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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--volume", type=int, nargs=3, default=(128, 512, 512), metavar=("D", "H", "W"))
    ap.add_argument("--size", type=int, nargs=2, default=(352, 352), metavar=("H", "W"))
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    (D, Hs, Ws), (h, w), B = a.volume, a.size, a.batch
    gen = torch.Generator().manual_seed(1)
    vol = torch.randint(-200, 400, (D, Hs, Ws), generator=gen, dtype=torch.int16)
    vol[torch.rand(D, Hs, Ws, generator=gen) < 0.5] = -1024            # half of the case is air
    vol = vol.cuda()
    lab = torch.randint(0, 3, (D, Hs, Ws), generator=gen, dtype=torch.uint8).cuda()
    frames = torch.randint(0, 256, (B, Hs, Ws, 3), generator=gen, dtype=torch.uint8).cuda()
    s = VolumeSlicer(size=(h, w), context=1, foreground=-1000, clip=(0.5, 99.5))
    s.open_case(vol, lab)
    pre = DevicePreprocess((h, w))
    z0 = D // 2
    torch.cuda.synchronize()
    lo, hi, mean, inv = (float(v) for v in s.table[0].cpu())

    def eager():
        zs = [torch.arange(z0 + d, z0 + d + B, device=vol.device).clamp_(0, D - 1) for d in (-1, 0, 1)]
        x = torch.stack([vol[i].float() for i in zs], 1)
        x = F.interpolate(x, size=(h, w), mode="bilinear", align_corners=False)
        return (x.clamp_(lo, hi) - mean) * inv

    steps = {"stats": lambda: s.open_case(vol, lab), "gather": lambda: s.slices(z0, z0 + B), "gather_image_only": None,
             "eager_torch": eager, "device_preprocess": lambda: pre(frames)}
    s_img = VolumeSlicer(size=(h, w), context=1, foreground=-1000, clip=(0.5, 99.5))
    s_img.open_case(vol)
    steps["gather_image_only"] = lambda: s_img.slices(z0, z0 + B)
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
    bytes_ = {"stats": 2 * 2 * D * Hs * Ws, "gather": 4 * B * 3 * h * w + B * h * w + 2 * (B + 2) * Hs * Ws + B * Hs * Ws,
              "gather_image_only": 4 * B * 3 * h * w + 2 * (B + 2) * Hs * Ws, "device_preprocess": 4 * B * 3 * h * w + 3 * B * Hs * Ws}
    out = {"what": "%dx%dx%d int16 -> %dx%d, context 1, batches of %d; us per call (median of %d rounds x %d calls, variants alternating)"
                   % (D, Hs, Ws, h, w, B, a.rounds, a.iters),
           "device": torch.cuda.get_device_name(0),
           "us": {name: round(med[name], 1) for name in names}, "us_min": {name: round(min(us[name]), 1) for name in names},
           "algorithmic_bytes": bytes_,
           "share_of_hbm_peak": {k: round(v / (med[k] * 1e-6) / HBM_PEAK, 4) for k, v in bytes_.items()},
           "aa_spread": round(abs(med[order[-1]] - med[names[0]]) / med[names[0]], 4)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

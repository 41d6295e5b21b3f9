"""DeviceAugment cost at batch 8, 530x622x3 -> 352x352 with every augmentation on (crop, SSR, ColorJitter; flips as drawn):
wall time per __call__ on device events (parameter H2D copy, buffer allocation and both kernels included; fixed parameters,
and freshly sampled ones) and the bytes the two kernels must move.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/gpu_augment_bench.py`.  Prints one JSON line.

`--oneof MEMBER|reference`: the same batch through `DeviceAugment(one_of=...)` (lmn_augment_oneof_u8): every sample on MEMBER
(p_oneof = 1), or the reference's nine-member mix at p_oneof = 0.4, as the MEDIAN of per-call device-event times (fixed parameters;
for the mix, one parameter set per call from a pool of 32 sampled batches), next to the same run's `one_of=None` median."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lm_net_amd.data import DeviceAugment  # noqa: E402


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters   # us per call


def median_us(fns, iters, mean=False):
    """Median (or mean) over `iters` calls of the device-event time of one call (the calls cycle through fns)."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for i, (s, e) in enumerate(ev):
        s.record()
        fns[i % len(fns)]()
        e.record()
    torch.cuda.synchronize()
    t = [s.elapsed_time(e) for s, e in ev]
    return float(np.mean(t) if mean else np.median(t)) * 1e3


def oneof_bench(a, img, mask, B, hs, ws, H, W):
    from lm_net_amd.data import ONEOF_MEMBERS, pack_oneof, pack_params
    if a.oneof != "reference" and a.oneof not in ONEOF_MEMBERS:
        raise SystemExit("--oneof: 'reference' or one of %s" % ", ".join(ONEOF_MEMBERS))
    mix = a.oneof == "reference"
    plain = DeviceAugment((H, W), generator=1, p_ssr=1.0, p_cj=1.0)
    aug = DeviceAugment((H, W), generator=1, p_ssr=1.0, p_cj=1.0, one_of="reference" if mix else [a.oneof], p_oneof=0.4 if mix else 1.0)
    sets = []
    for _ in range(32 if mix else 1):
        d = aug.sample_dicts(B, (hs, ws))
        sets.append((pack_params(d), pack_oneof(d, (H, W)), [None if s["oneof"] is None else s["oneof"]["op"] for s in d]))
    calls = [lambda p=p, o=o: aug(img, mask, params=p, oneof=o) for p, o, _ in sets]
    base = [lambda p=p: plain(img, mask, params=p) for p, _, _ in sets]
    for f in calls + base:
        f()
    for _ in range(a.warmup):
        calls[0](), base[0]()
    torch.cuda.synchronize()
    us_base, us = median_us(base, a.iters), median_us(calls, a.iters)
    us_base2, us_mean = median_us(base, a.iters), median_us(calls, max(a.iters, 8 * len(calls)), mean=True)
    fired = sum(o is not None for _, _, ops in sets for o in ops)
    print(json.dumps({"what": "DeviceAugment B=8 530x622x3 -> 352x352, one_of=%s, p_oneof=%s" % (a.oneof, aug.p_oneof),
                      "us_per_call_median": round(us, 1), "us_per_call_mean": round(us_mean, 1), "us_per_call_median_one_of_none": [round(us_base, 1), round(us_base2, 1)],
                      "us_per_sample_median": round(us / B, 2), "members_fired": "%d of %d samples" % (fired, B * len(sets))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--oneof", default=None, help="a OneOf member, or 'reference' for the nine-member mix at p_oneof=0.4 (comma-separated: one line each)")
    a = ap.parse_args()
    B, hs, ws, H, W = 8, 530, 622, 352, 352
    rng = np.random.default_rng(0)
    img = torch.from_numpy(rng.integers(0, 256, (B, hs, ws, 3), dtype=np.uint8)).cuda()
    mask = torch.from_numpy(rng.integers(0, 256, (B, hs, ws), dtype=np.uint8)).cuda()
    if a.oneof:
        for name in a.oneof.split(","):                       # several, comma-separated: one JSON line each
            a.oneof = name
            oneof_bench(a, img, mask, B, hs, ws, H, W)
        return
    aug = DeviceAugment((H, W), generator=1, p_ssr=1.0, p_cj=1.0)
    params = aug.sample(B, (hs, ws))
    assert all(p.apply_ssr and p.apply_cj and p.cj[1] != 1.0 for p in params)
    for _ in range(a.warmup):
        aug(img, mask, params=params)
    torch.cuda.synchronize()
    us_fixed = timed(lambda: aug(img, mask, params=params), a.iters)
    us_sampled = timed(lambda: aug(img, mask), a.iters)
    crop = sum(p.h * p.w * 4 for p in params)                 # 3 image bytes + 1 mask byte per crop-window pixel
    need = crop + 2 * B * H * W * 3 + B * 3 * H * W * 4 + B * H * W * 8
    print(json.dumps({"what": "DeviceAugment B=8 530x622x3 -> 352x352, all augmentations on",
                      "us_per_call_fixed_params": round(us_fixed, 1), "us_per_call_sampled_params": round(us_sampled, 1),
                      "required_bytes": need, "crop_window_bytes": crop}))


if __name__ == "__main__":
    main()

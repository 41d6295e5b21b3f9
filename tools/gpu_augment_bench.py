"""DeviceAugment cost at batch 8, 530x622x3 -> 352x352 with every augmentation on (crop, SSR, ColorJitter; flips as drawn):
wall time per __call__ on device events (parameter H2D copy, buffer allocation and both kernels included; fixed parameters,
and freshly sampled ones) and the bytes the two kernels must move.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/gpu_augment_bench.py`.  Prints one JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    B, hs, ws, H, W = 8, 530, 622, 352, 352
    rng = np.random.default_rng(0)
    img = torch.from_numpy(rng.integers(0, 256, (B, hs, ws, 3), dtype=np.uint8)).cuda()
    mask = torch.from_numpy(rng.integers(0, 256, (B, hs, ws), dtype=np.uint8)).cuda()
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

"""Cost of one optimizer step at the flat size of LM_Net(3, 2) (3.97 M parameters in 514 tensors): the one-launch AdamW, the extended
route of include/optim/lmnet_optim.h, and the torch route it replaces.  The median over --rounds of device-event timings of --iters steps
each, after warm-up, the variants alternating inside every round of one process:
  old_a, old_b        lmn_adamw_step, timed twice: |old_a - old_b| / old_a is the A/A spread of this run;
  ex_clip             lmn_optim_prepare + lmn_adamw_step_ex, one group, max_norm set (the reduction reads g once more);
  ex_full             the same with three groups (one frozen block), the skip flag, the two GradScaler scalars and an EMA buffer;
  torch_clip_adamw    torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW.step() over the 514 tensors;
  torch_scaler        GradScaler.unscale_ + clip_grad_norm_ + GradScaler.step(torch.optim.AdamW) + update(): the --apm loop of the
                      reference with clipping (scaler.step reads found_inf back: one host synchronisation per step).
Nothing is barred: the numbers are reported.  Prints one JSON line and writes it to --out (default profiles/optim_bench.json)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from lm_net_amd import LM_Net, hip  # noqa: E402
from lm_net_amd.optim import FusedAdamW  # noqa: E402


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters   # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_optim_bench: needs the GPU (no timing is taken on the CPU)")
    net = LM_Net(3, 2).cuda()
    opt = FusedAdamW(net, lr=1e-3, weight_decay=1e-2)
    L = opt._layout
    n = L["total"]
    gen = torch.Generator().manual_seed(1)
    g = torch.zeros(n)
    for p in L["order"]:
        lo, hi = L["offs"][id(p)]
        g[lo:hi] = torch.randn(hi - lo, generator=gen) * 1e-2
    g = g.cuda()
    p, m, v, ema = opt.flat_p.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), opt.flat_p.clone()
    max_norm = 1.0

    def workspace(rows):
        ws = torch.zeros(hip.optim_workspace(n), device="cuda")
        c0 = 2 * hip.optim_blocks(n) + hip.OPTIM_CTRL_WORDS
        for k, row in enumerate(rows):
            ws[c0 + 4 * k:c0 + 4 * k + 3] = torch.tensor(row, device="cuda")
        return ws
    q1 = torch.zeros(n // 4, dtype=torch.uint8, device="cuda")
    q3 = opt._qgroup.clone()
    lo, hi = L["blocks"]["conv1"]
    q3[:] = 0
    q3[L["blocks"]["down4"][0] // 4:] = 1                    # the encoder blocks (they come last in the layout) ...
    q3[lo // 4:hi // 4] = 2                                  # ... and conv1 frozen
    ws1, ws3 = workspace([(1e-3, 1e-2, 0.0)]), workspace([(1e-3, 1e-2, 0.0), (1e-4, 1e-2, 0.0), (1e-3, 1e-2, 1.0)])
    par1 = hip.optim_param((0.9, 0.999), 1e-8, max_norm, None, 0, 1)
    par3 = hip.optim_param((0.9, 0.999), 1e-8, max_norm, 0.999, hip.OPTIM_SKIP_NONFINITE, 3)
    scale, found = torch.tensor(1.0, device="cuda"), torch.tensor(0.0, device="cuda")
    step = [0]

    def old():
        step[0] += 1
        hip.adamw_step(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0 - 0.9 ** step[0], 1.0 - 0.999 ** step[0])

    def ex_clip():
        hip.optim_prepare(g, q1, par1, ws1)
        hip.adamw_step_ex(p, g, m, v, None, q1, par1, ws1)

    def ex_full():
        hip.optim_prepare(g, q3, par3, ws3, scale, found)
        hip.adamw_step_ex(p, g, m, v, ema, q3, par3, ws3)

    # the torch route on its own copies: 514 parameters with gradients of the same values
    tp = [torch.nn.Parameter(q.detach().clone()) for q in net.parameters()]
    for t, q in zip(tp, net.parameters()):
        lo, hi = L["offs"][id(q)]
        t.grad = g[lo:hi].view(q.shape).clone()
    topt = torch.optim.AdamW(tp, lr=1e-3, weight_decay=1e-2)
    sopt = torch.optim.AdamW(tp, lr=1e-3, weight_decay=1e-2)
    scaler = torch.amp.GradScaler("cuda", init_scale=1.0, growth_interval=1 << 30)
    scaler.scale(torch.zeros(1, device="cuda"))

    def torch_clip_adamw():
        torch.nn.utils.clip_grad_norm_(tp, max_norm)
        topt.step()

    def torch_scaler():
        scaler.unscale_(sopt)
        torch.nn.utils.clip_grad_norm_(tp, max_norm)
        scaler.step(sopt)
        scaler.update()

    variants = {"old_a": old, "old_b": old, "ex_clip": ex_clip, "ex_full": ex_full, "torch_clip_adamw": torch_clip_adamw,
                "torch_scaler": torch_scaler}
    for f in variants.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, f in variants.items():
            us[k].append(timed(f, a.iters))
    r = {k: round(statistics.median(t), 2) for k, t in us.items()}
    r["aa_spread"] = round(abs(r["old_a"] - r["old_b"]) / r["old_a"], 4)
    base = min(r["old_a"], r["old_b"])
    out = {"what": "one optimizer step over the %d floats of LM_Net(3, 2), us per step (median of %d rounds x %d steps, variants "
                   "alternating in one process; host launch cost included)" % (n, a.rounds, a.iters),
           "n": n, "tensors": len(tp), "us": r, "ex_clip_over_old": round(r["ex_clip"] / base, 3),
           "ex_full_over_old": round(r["ex_full"] / base, 3), "torch_clip_adamw_over_ex_clip": round(r["torch_clip_adamw"] / r["ex_clip"], 2),
           "torch_scaler_over_ex_full": round(r["torch_scaler"] / r["ex_full"], 2),
           "bytes_old": 7 * 4 * n, "bytes_ex_clip": 8 * 4 * n + n // 2}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""The step of tests/test_wide_model_gpu.py::test_wide_bf16_vs_fp32_path, N times in default mode from one state: per parameter the
   L2 distance of the bf16 gradient to the fp32 path (what the test bounds by 0.1 median / 0.4 worst) next to the L2 spread between the
   runs and the norm of the tensor.  A spread of the order of the distance means that the distance is noise, not error (DESIGN, wide
   variants).   python tools/gpu_wide_bf16_spread.py [variant=W3] [runs=5] [rows=12]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from lm_net_amd import LM_Net
from tools.detweights import det_input, fill_module
WIDE = {"W2": [24, 48, 96, 192, 384], "W3": [36, 72, 144, 288, 576], "W4": [48, 96, 192, 384, 768], "Wodd": [12, 36, 60, 84, 120]}
name = sys.argv[1] if len(sys.argv) > 1 else "W3"
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
rows = int(sys.argv[3]) if len(sys.argv) > 3 else 12
x = det_input((2, 3, 64, 64), "wide_bf16/x").cuda()
G = det_input((2, 2, 64, 64), "wide_bf16/G").cuda()

m = LM_Net(3, 2, filters=WIDE[name])
fill_module(m, 9)
for mod in m.modules():
    if isinstance(getattr(mod, "p", None), float):
        mod.p = 0.0
m = m.cuda().train()
sd = {k: v.clone() for k, v in m.state_dict().items()}
keys = [k for k, _ in m.named_parameters()]


def step(mode):
    m.load_state_dict(sd)
    m.compute_dtype = mode
    m.zero_grad(set_to_none=True)
    (m(x) * G).sum().backward()
    torch.cuda.synchronize()
    return [p.grad.detach().double().cpu() for p in m.parameters()]


ref = step("fp32")
gmax = max(float(r.norm()) for r in ref)
print("%s, 64x64 batch 2, %d default-mode runs per precision; largest gradient norm of the model %.3e" % (name, runs, gmax))
for mode in ("fp32", "bf16", "bf16-mma"):
    gs = [step(mode) for _ in range(runs)]
    tab = []
    for i, k in enumerate(keys):
        n = float(ref[i].norm())
        if float(ref[i].abs().max()) == 0 or k.endswith("expand_conv.0.bias") or k.endswith("fuse_conv.0.bias"):
            continue              # (the tensors the test leaves out: exact gradient 0)
        dist = [float((g[i] - ref[i]).norm()) / (n + 1e-30) for g in gs]
        spread = max(float((gs[a][i] - gs[b][i]).norm()) for a in range(runs) for b in range(a)) / (n + 1e-30)
        tab.append((max(dist), min(dist), spread, n, k, tuple(ref[i].shape), i, dist.index(max(dist)), dist.index(min(dist))))
    tab.sort(reverse=True)
    med = sorted(t[0] for t in tab)[len(tab) // 2]
    print("\n%s: %d tensors, median of the worst-run distance %.3g" % (mode, len(tab), med))
    print("%-44s %-16s %10s %10s %10s %10s" % ("parameter", "shape", "|g| fp32", "dist max", "dist min", "spread"))
    for dmax, dmin, spread, n, k, shp, *_ in tab[:rows]:
        print("%-44s %-16s %10.3e %10.3g %10.3g %10.3g" % (k, "x".join(map(str, shp)), n, dmax, dmin, spread))
    # where inside the worst weight matrix do its farthest and its nearest run differ?  One output row (one hidden unit of an SE
    # block: a ReLU that one image switches on or off) or all of them?
    w = next((t for t in tab if len(t[5]) >= 2), None)
    if w is not None and mode != "fp32":
        i, a, b = w[6], w[7], w[8]
        d = (gs[a][i] - gs[b][i]).reshape(w[5][0], -1).norm(dim=1) / (w[3] + 1e-30)
        top = torch.sort(d, descending=True)
        print("%s, run %d - run %d by output row (of |g|): %s; the other %d rows together %.3g" % (
            w[4], a, b, ", ".join("row %d %.3g" % (int(top.indices[j]), float(top.values[j])) for j in range(min(3, d.numel()))),
            max(d.numel() - 3, 0), float(top.values[3:].norm()) if d.numel() > 3 else 0.0))

"""Tile-slot census of the weight-gradient calls of one training step: which kernel instance, how many 16-channel tiles per side,
the block's tile shape, the tile sets of the grid, and how many of the issued tile slots hold channels.

    python tools/wgrad_tile_census.py --record profiles/wgrad_calls_352.json [--size 352] [--batch 8]     (GPU: one step, calls logged)
    python tools/wgrad_tile_census.py profiles/wgrad_calls_352.json [more.json ...]                       (host only: the table)

The table needs no GPU: the geometry of every recorded call comes from the library's own host arithmetic (lmn_conv_wgrad_workspace,
lmn_conv_wgrad_job: wgrad_setup in conv_wgrad.hip, the one source of truth of the launch), the instance name from the record (the
in-library timer's name of the kernel the call launched).  A block of NMT x NNT tile slots whose set reaches past NMTT / NNTT has slots
that hold no channels: wgrad3_kernel gives their waves to the valid tiles (LMN_WGRAD_FILL), wgrad_lds_kernel and the 1x1 kernels
multiply the zeros staged for them.
"""
import argparse
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def record(path, size, batch):
    import torch
    from bench import make_batch
    from lm_net_amd import LM_Net, hip
    from lm_net_amd.loss import SegLoss
    from lm_net_amd.optim import FusedAdamW
    dev = torch.device("cuda", 0)
    net = LM_Net(3, 2).to(dev).train()
    net._engine.branch_overlap = net._engine.overlap_wgrad = False     # one stream: the timer's names belong to the call around them
    opt = FusedAdamW(net, lr=1e-3, weight_decay=1e-4)
    crit = SegLoss(label_smoothing=1e-3).to(dev)
    x, y = make_batch(batch, size, size, dev, 1234)

    def step():
        loss = crit(net(x), y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    calls, real = [], hip.conv_wgrad

    def logged(srcs, dy, dW, db, **kw):
        hip.prof_begin("wgrad")
        try:
            return real(srcs, dy, dW, db, **kw)
        finally:
            names = sorted(n for n in hip.prof_end() if "reduce" not in n)
            views = [hip._as_view(s["view"] if isinstance(s, dict) else s) for s in srcs]
            vy = hip._as_view(dy)
            calls.append(dict(kernel=names, B=kw["B"], Hin=kw["Hin"], Win=kw["Win"], Hout=kw["Hout"], Wout=kw["Wout"], Cout=kw["Cout"],
                              ksize=kw.get("ksize", 1), stride=kw.get("stride", 1),
                              src=[dict(C=v.C, cstride=v.cstride, rp_w=v.rp, flags=(s.get("flags", 0) if isinstance(s, dict) else 0), scale=bool(isinstance(s, dict) and s.get("scale") is not None))
                                   for v, s in zip(views, srcs)],
                              dy_cstride=vy.cstride, dy_rp_w=vy.rp, dy_flags=kw.get("dy_flags", 0), bf16=bool(vy.t.dtype == torch.bfloat16), defer=bool(kw.get("defer", False))))
    hip.conv_wgrad = logged
    try:
        step()
        torch.cuda.synchronize()
    finally:
        hip.conv_wgrad = real
    with open(path, "w") as f:
        json.dump(dict(size=size, batch=batch, calls=calls), f, indent=0)
    print("%d weight-gradient calls of one %dx%d batch-%d step -> %s" % (len(calls), size, size, batch, path))


def geometry(c):
    """(NMTT, NNTT, NMT, NNT, tile sets, K-split blocks per set or 0) of a recorded call: host arithmetic of the library."""
    from lm_net_amd import hip
    lib = hip.load()
    a = hip.WgradArgs()
    a.B, a.Hout, a.Wout, a.Hin, a.Win = c["B"], c["Hout"], c["Wout"], c["Hin"], c["Win"]
    a.ksize, a.stride, a.nsrc, a.Cout = c["ksize"], c["stride"], len(c["src"]), c["Cout"]
    fake = 0x1000      # (any non-null pointer: the queries touch no memory)
    for i, s in enumerate(c["src"]):
        a.src[i].ptr, a.src[i].C, a.src[i].cstride, a.src[i].rp_w, a.src[i].flags = fake, s["C"], s["cstride"], s["rp_w"], s["flags"]
    a.dy, a.dy_cstride, a.dy_rp_w, a.dW = fake, c["dy_cstride"], c["dy_rp_w"], fake
    a.mma_dtype = hip.BF16 if c["bf16"] else hip.F32
    a.act_dtype = hip.BF16 if c["bf16"] else hip.F32
    nmtt = (c["Cout"] + 15) // 16
    nntt = sum((s["C"] + 15) // 16 for s in c["src"])
    m = re.search(r"<(?:9, )?(\d+), (\d+),", c["kernel"][0]) if c["kernel"] else None
    nmt, nnt = (int(m.group(1)), int(m.group(2))) if m else (0, 0)
    need = int(lib.lmn_conv_wgrad_workspace(C.byref(a)))
    nblk = 0
    if need > 0:
        a.workspace, a.workspace_floats = fake, need
        job = hip.ReduceJob()
        if lib.lmn_conv_wgrad_job(C.byref(a), C.byref(job)) == 0 and job.nblk > 0:
            assert (job.NMT, job.NNT) == (nmt, nnt) or not m, "tile shape of the library %s and of the recorded instance %s differ" % ((job.NMT, job.NNT), c["kernel"])
            nmt, nnt, nblk = job.NMT, job.NNT, job.nblk
            assert (job.NMTT, job.NNTT) == (nmtt, nntt)
    sets = -(-nmtt // nmt) * -(-nntt // nnt) if nmt and nnt else 0
    return nmtt, nntt, nmt, nnt, sets, nblk


def table(paths):
    for p in paths:
        with open(p) as f:
            rec = json.load(f)
        rows = {}
        for c in rec["calls"]:
            nmtt, nntt, nmt, nnt, sets, nblk = geometry(c)
            key = (c["kernel"][0] if c["kernel"] else "?", "%dx%dx%d" % (c["B"], c["Hout"], c["Wout"]), c["stride"], "+".join(str(s["C"]) for s in c["src"]), c["Cout"],
                   nmtt, nntt, nmt, nnt, sets, nblk)
            rows[key] = rows.get(key, 0) + 1
        print("## %dx%d, batch %d: %d weight-gradient calls per step (%s)\n" % (rec["size"], rec["size"], rec["batch"], len(rec["calls"]), os.path.basename(p)))
        print("| n | instance | dy map | s | cin | cout | NMTT x NNTT | NMT x NNT | sets | blocks/set | useful / issued slots |")
        print("|---|---|---|---|---|---|---|---|---|---|---|")
        fam = {}
        for key in sorted(rows, key=lambda k: (k[0].split("<")[0] not in ("wgrad3_kernel", "wgrad_lds_kernel"), k[0], -int(k[1].split("x")[1]), k[4], k[3])):
            kern, mp, st, cin, cout, nmtt, nntt, nmt, nnt, sets, nblk = key
            n = rows[key]
            useful, issued = nmtt * nntt, sets * nmt * nnt
            print("| %d | `%s` | %s | %d | %s | %d | %d x %d | %d x %d | %d | %s | %d / %d |" % (n, kern, mp, st, cin, cout, nmtt, nntt, nmt, nnt, sets, nblk or "atomics", useful, issued))
            f_ = fam.setdefault(kern, [0, 0, 0, 0])
            f_[0] += n
            f_[1] += n * (useful < issued)
            f_[2] += n * useful
            f_[3] += n * issued
        print("\n| instance | launches | with empty slots | useful / issued slots over its launches |")
        print("|---|---|---|---|")
        for kern in sorted(fam):
            n, npad, u, i = fam[kern]
            print("| `%s` | %d | %d | %d / %d |" % (kern, n, npad, u, i))
        print()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("calls", nargs="*", help="recorded call lists (JSON)")
    ap.add_argument("--record", metavar="JSON")
    ap.add_argument("--size", type=int, default=352)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    if a.record:
        record(a.record, a.size, a.batch)
    else:
        table(a.calls)

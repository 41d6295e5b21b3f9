"""Tiled inference cost on one 1024x1024 frame: tile 352, stride 176 (5 x 5 tiles), the identity and three mirrors (100 entries),
C = 2 and 9 classes, the three averaging modes.  Per variant the median over --rounds of device-event timings of --iters calls each,
after warm-up; the variants of a case alternate inside every round, and the blend is timed twice per round (the A/A spread):
  gather_us            lmn_tile_gather of all 100 entries in one launch (3 channels), gather_batches_us the 13 launches of 8 entries
                       TiledPredictor issues,
  blend_us             lmn_tile_blend over the 100 tile outputs, labels included where they are defined; `hbm_share` is its
                       algorithmic bytes (every tile output read once, the map and the labels written once) per second over the 8 TB/s
                       peak,
  eager_gather_us / eager_blend_us   the eager torch composition of the same results on the same device: F.pad, slicing, flip and
                       stack; one weighted += per entry on a padded canvas and a divide -- with the number of launches it issues
                       (`*_launches`; the kernels take 1),
  forward_us           the eval forward of LM_Net(3, C) over the same 100 tiles in 13 batches of 8 (the last one filled up).
Nothing is barred: the tool reports.  Prints one JSON line and writes it to --out."""
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
import torch.nn.functional as F  # noqa: E402

from lm_net_amd import hip  # noqa: E402
from lm_net_amd.infer import window_table  # noqa: E402

HBM_PEAK = 8e12
FLIPS = ("h", "v", "hv")
DIMS = {"": (), "h": (-1,), "v": (-2,), "hv": (-2, -1)}


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters   # us per call


def starts(L, t, s):
    V, _, n = hip.tile_axis(L, t, s)
    return [min(i * s, V - t) for i in range(n)]


def eager_gather(x, t, s, count):
    """F.pad (reflect; a no-op pad at this size, issued as the general loop would), slicing, flip, stack -> ([100, ch, t, t], launches)"""
    B, ch, H, W = x.shape
    Vh, ph, _ = hip.tile_axis(H, t, s)
    Vw, pw, _ = hip.tile_axis(W, t, s)
    v = F.pad(x, (pw, Vw - W - pw, ph, Vh - H - ph), mode="reflect")
    out, n = [], 1
    for y0 in starts(H, t, s):
        for x0 in starts(W, t, s):
            tile = v[0, :, y0:y0 + t, x0:x0 + t]
            out.append(tile)
            for f in FLIPS:
                out.append(torch.flip(tile, DIMS[f]))
                n += 1
    count[0] = n + 1
    return torch.stack(out)


def eager_blend(z, H, W, t, s, w2, mode, count):
    """one weighted += per entry on the canvas, a divide (and the arg-max) -> (map [1, C, H, W], launches)"""
    C = z.shape[1]
    num, den = torch.zeros((C, H, W), device=z.device), torch.zeros((H, W), device=z.device)
    e, n = 0, 2
    for y0 in starts(H, t, s):
        for x0 in starts(W, t, s):
            den[y0:y0 + t, x0:x0 + t] += w2
            n += 1
            for f in ("",) + FLIPS:
                g = z[e]
                if mode == "softmax":
                    g, n = torch.softmax(g, 0), n + 1
                elif mode == "sigmoid":
                    g, n = torch.sigmoid(g), n + 1
                if f:
                    g, n = torch.flip(g, DIMS[f]), n + 1
                num[:, y0:y0 + t, x0:x0 + t] += w2 * g
                n += 2
                e += 1
    out = num / (4.0 * den)
    n += 2
    if C >= 2 and mode != "sigmoid":
        out.argmax(0)
        n += 1
    count[0] = n
    return out[None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-forward", action="store_true", help="skip the model forward over the 100 tiles")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiles_bench.json"))
    a = ap.parse_args()
    H = W = 1024
    t, s, tb = 352, 176, 8
    dev = torch.device("cuda")
    x = torch.randn(1, 3, H, W, device=dev)
    p_src = hip.tile_param(1, 3, H, W, (t, t), (s, s), "reflect", FLIPS)
    E = hip.tile_entries(p_src)
    assert E == 100
    tiles = torch.empty((E, 3, t, t), device=dev)
    wt = torch.from_numpy(window_table(t)).to(dev)
    w2 = wt[:, None] * wt[None, :]
    out = {"what": "tiled inference, one 1024x1024 frame, tile 352, stride 176, 4 copies: %d entries; us per call (median of %d rounds x %d "
                   "calls)" % (E, a.rounds, a.iters), "entries": E}

    def rounds(variants):
        """variants: name -> fn; every round times each variant once, in turn -> name -> (median, min)"""
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                us[k].append(timed(fn, a.iters))
        return {k: (round(statistics.median(v), 1), round(min(v), 1)) for k, v in us.items()}

    def gather_batches():
        for e0 in range(0, E, tb):
            k = min(tb, E - e0)
            hip.tile_gather(x, p_src, e0, k, tiles[e0:e0 + k])

    cnt = [0]
    r = rounds({"gather_us": lambda: hip.tile_gather(x, p_src, 0, E, tiles), "gather_batches_us": gather_batches,
                "eager_gather_us": lambda: eager_gather(x, t, s, cnt)})
    hip.tile_gather(x, p_src, 0, E, tiles)
    assert torch.equal(tiles, eager_gather(x, t, s, cnt))
    gbytes = 2 * tiles.numel() * 4
    out["gather"] = dict({k: v[0] for k, v in r.items()}, gather_us_min=r["gather_us"][1], launches=1, batches_launches=(E + tb - 1) // tb,
                         eager_gather_launches=cnt[0], hbm_share=round(gbytes / (r["gather_us"][0] * 1e-6) / HBM_PEAK, 4))
    for C in (2, 9):
        z = torch.randn(E, C, t, t, device=dev)
        res, lab = torch.empty((1, C, H, W), device=dev), torch.empty((1, H, W), dtype=torch.uint8, device=dev)
        for mode in ("logits", "softmax", "sigmoid"):
            p = hip.tile_param(1, C, H, W, (t, t), (s, s), "reflect", FLIPS, mode)
            labels = lab if mode != "sigmoid" else None

            def blend():
                hip.tile_blend(z, p, wt, wt, res, labels)

            r = rounds({"blend_us": blend, "eager_blend_us": lambda: eager_blend(z, H, W, t, s, w2, mode, cnt), "blend_again_us": blend})
            blend()
            err = float((res - eager_blend(z, H, W, t, s, w2, mode, cnt)).abs().max())
            nbytes = z.numel() * 4 + res.numel() * 4 + (lab.numel() if labels is not None else 0)
            med = r["blend_us"][0]
            out["C%d_%s" % (C, mode)] = dict(
                {k: v[0] for k, v in r.items()}, blend_us_min=r["blend_us"][1], aa_spread=round(abs(r["blend_again_us"][0] - med) / med, 4),
                launches=1, eager_blend_launches=cnt[0], speedup_over_eager=round(r["eager_blend_us"][0] / med, 1),
                algorithmic_bytes=nbytes, hbm_share=round(nbytes / (med * 1e-6) / HBM_PEAK, 4), max_abs_diff_to_eager=err)
        if not a.no_forward:
            from lm_net_amd import LM_Net
            net = LM_Net(3, C).to(dev).eval()
            batch = torch.empty((tb, 3, t, t), device=dev)

            def forward():
                for e0 in range(0, E, tb):
                    k = min(tb, E - e0)
                    batch[:k].copy_(tiles[e0:e0 + k])
                    net(batch)

            with torch.no_grad():
                for _ in range(2):
                    forward()
                torch.cuda.synchronize()
                us = [timed(forward, 1) for _ in range(max(3, a.rounds // 2))]
            out["C%d_forward_us" % C] = round(statistics.median(us), 1)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

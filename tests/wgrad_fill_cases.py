"""Cases of tests/test_wgrad_tile_fill_gpu.py: 3x3 weight gradients whose 2 x 2-tile blocks have tile slots past the channel count
(conv_wgrad.hip, wgrad3_kernel: the waves of such slots take taps of the valid tiles; LMN_WGRAD_FILL=0 keeps them on the zeros).

``run(case)`` launches one case through the C ABI and returns (dW, db or None, {instance names launched}); ``reference(case)`` is fp64
F.conv2d autograd, computed once per case.  Run as a program it writes the result of run_switch_cases() to a file: the switch is read
once per process, so the test that compares LMN_WGRAD_FILL=0 with the default starts this file in a child process.
"""
import functools
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kernel_checks import DEV, R, dev, nhwc  # noqa: E402
from kernel_forms import launched  # noqa: E402
from lm_net_amd import hip  # noqa: E402

# the five channel pairs: tile sets with 2x2, 2x1, 1x2 and 1x1 valid tiles, and a partly filled channel tile
PAIRS = [(48, 48), (48, 32), (32, 48), (36, 72), (20, 48)]
# maps: one pixel tile per image row band; partial tiles, an image change inside a block's tile range
MAPS = [(1, 32, 32), (2, 33, 40)]


def case(cout, cins, B, H, W, pm=0, up=False, bias=True, drop=False, stride=1):
    """cins: channels per source.  up: H x W is the half-resolution source map.  pm: 0 fp32, 1 bf16 MFMA operands, 2 bf16 storage."""
    return (cout, tuple(cins) if isinstance(cins, (list, tuple)) else (cins,), B, H, W, pm, up, bias, drop, stride)


def _q(t, pm):   # bf16 modes: bf16-representable operands, as check_conv3_storage draws them (every product exact in fp32)
    return t.to(torch.bfloat16).double() if pm else t


def _drop_mask(B, H, W, C, seed, p):
    """keep / (1 - p) per element of a [B, H, W, C] source, as LMN_SRC_DROP regenerates it (check_conv_dropout: an identity 1x1 conv
    over ones with the mask applied on load)."""
    eye = torch.eye(C, dtype=torch.float64).view(C, C, 1, 1)
    out = torch.empty(B, H, W, C, device=DEV)
    hip.conv_fwd([dict(view=torch.ones(B, H, W, C, device=DEV), flags=hip.SRC_DROP, drop_seed=seed, drop_p=p)], hip.conv_pack(dev(eye), 1, [C]), out,
                 B=B, Hin=H, Win=W, Hout=H, Wout=W, Cout=C)
    return out.double().cpu().permute(0, 3, 1, 2)


DROP_SEED, DROP_P = 4711, 0.25


@functools.lru_cache(maxsize=None)
def operands(c):
    cout, cins, B, H, W, pm, up, bias, drop, stride = c
    cin = sum(cins)
    x = _q(R(B, cin, H, W, seed=701), pm)
    Hi, Wi = (2 * H, 2 * W) if up else (H, W)
    Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
    dy = _q(R(B, cout, Ho, Wo, seed=702), pm)
    return x, dy


@functools.lru_cache(maxsize=None)
def reference(c):
    """(dW, db) of fp64 F.conv2d autograd (bilinear x2 / the dropout mask applied to the source first)."""
    cout, cins, B, H, W, pm, up, bias, drop, stride = c
    x, dy = operands(c)
    xin = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True) if up else x
    if drop:
        xin = xin * _drop_mask(B, H, W, cins[0], DROP_SEED, DROP_P)
    w = torch.zeros(cout, sum(cins), 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    F.conv2d(xin, w, b, stride=stride, padding=1).backward(dy)
    return w.grad, b.grad


def run(c):
    cout, cins, B, H, W, pm, up, bias, drop, stride = c
    x, dy = operands(c)
    dt = torch.bfloat16 if pm == 2 else torch.float32
    Hi, Wi = (2 * H, 2 * W) if up else (H, W)
    Ho, Wo = dy.shape[2:]
    srcs, off = [], 0
    for ch in cins:
        v = nhwc(x[:, off:off + ch]).to(dt)
        off += ch
        if up:
            srcs.append(dict(view=v, flags=hip.SRC_UP2))
        elif drop:
            srcs.append(dict(view=v, flags=hip.SRC_DROP, drop_seed=DROP_SEED, drop_p=DROP_P))
        else:
            srcs.append(v)
    dyd = nhwc(dy).to(dt)
    dW = torch.zeros(cout, sum(cins), 3, 3, device=DEV)
    db = torch.zeros(cout, device=DEV) if bias else None
    mma0 = hip._MMA[0]
    hip._MMA[0] = hip.BF16 if pm else hip.F32
    try:
        if up:
            assert hip.conv_wgrad_up2_ok(srcs[0]["view"], dyd, B=B, Hin=Hi, Win=Wi, Cout=cout)
        _, names = launched(lambda: hip.conv_wgrad(srcs, dyd, dW, db, B=B, Hin=Hi, Win=Wi, Hout=Ho, Wout=Wo, Cout=cout, ksize=3, stride=stride))
    finally:
        hip._MMA[0] = mma0
    return dW, db, names


# the switch test: 3 x 3 tiles (a full set, both half sets, the one-tile corner), fp32 and bf16 storage, the bilinear x2 source
SWITCH_CASES = [case(48, 48, 2, 33, 40), case(48, 48, 2, 33, 40, pm=2), case(48, 48, 1, 17, 20, up=True)]


SENTINEL = 12345.0


def run_switch_cases():
    """(dW of SWITCH_CASES with fixed-order reductions, floats of the first case's block partials that no wave wrote).  The workspace of
    the K-split partials is filled with SENTINEL first; the count runs up to the last float written.  With one wave per tile slot every
    float of every block partial is written (zeros for the slots past the channel count); a slot without a wave stays as it was."""
    det0 = hip.get_deterministic()
    hip.set_deterministic(True)
    try:
        ws = hip._workspace(torch.zeros(1, device=DEV).device, 1)
        ws.fill_(SENTINEL)
        out = [run(SWITCH_CASES[0])[0].cpu()]
        torch.cuda.synchronize()
        written = (ws != SENTINEL).nonzero()
        holes = int((ws[:int(written[-1]) + 1] == SENTINEL).sum()) if written.numel() else -1
        out += [run(c)[0].cpu() for c in SWITCH_CASES[1:]]
        torch.cuda.synchronize()
    finally:
        hip.set_deterministic(det0)
    return out, holes


if __name__ == "__main__":
    torch.save(run_switch_cases(), sys.argv[1])

"""float64 torch restatement of one FusedAdamW step on the extended route (include/optim/lmnet_optim.h), in the order the device takes:
unscale -> non-finite check -> clip_grad_norm_ -> per-group AdamW -> EMA, or nothing at all when the step is skipped.  Flat tensors,
one group id per ELEMENT (`elem_groups` expands the per-quad bytes).  tests/test_optim_cpu.py pins it to torch.optim.AdamW +
torch.nn.utils.clip_grad_norm_ in float64."""
import math

import torch


def elem_groups(qgroup):
    """per-quad group bytes -> per-element group ids (int64)"""
    return qgroup.to(torch.int64).cpu().repeat_interleave(4)


def seeded(n, seed, scale=1.0):
    """n float32 values in about [-3 scale, 3 scale], reproducible"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * scale).float()


class State:
    def __init__(self, p, m=None, v=None, ema=None, step=0):
        self.p = p.detach().double().cpu().clone()
        self.m = torch.zeros_like(self.p) if m is None else m.detach().double().cpu().clone()
        self.v = torch.zeros_like(self.p) if v is None else v.detach().double().cpu().clone()
        self.ema = None if ema is None else ema.detach().double().cpu().clone()
        self.step, self.skipped = int(step), 0


def step(st, g, gid, table, betas=(0.9, 0.999), eps=1e-8, max_norm=None, ema_decay=None, grad_scale=None, found_inf=False,
         skip_nonfinite=False):
    """One step on State `st` from the flat gradient g (float32 values, possibly scaled by grad_scale).  table: [(lr, weight_decay,
    frozen)] per group.  -> dict(skip, grad_norm, coef, nonfinite)"""
    g = g.detach().cpu()
    live = ~torch.tensor([bool(t[2]) for t in table])[gid]
    nonfinite = int((~torch.isfinite(g[live])).sum())
    inv_scale = 1.0 if grad_scale is None else float(torch.tensor(1.0 / float(grad_scale), dtype=torch.float32))
    gu = g.double() * inv_scale
    skip = bool(skip_nonfinite) and (nonfinite > 0 or bool(found_inf))
    norm = float(torch.sqrt((gu[live] ** 2).sum())) if bool(live.any()) else 0.0
    coef = 1.0 if max_norm is None else min(1.0, float(max_norm) / (norm + 1e-6))
    info = dict(skip=skip, grad_norm=norm, coef=coef, nonfinite=nonfinite)
    if skip:
        st.skipped += 1
        return info
    st.step += 1
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** st.step, 1.0 - b2 ** st.step
    lr = torch.tensor([float(t[0]) for t in table], dtype=torch.float64)[gid]
    wd = torch.tensor([float(t[1]) for t in table], dtype=torch.float64)[gid]
    ge = gu * coef
    p = st.p * (1.0 - lr * wd)
    m = b1 * st.m + (1.0 - b1) * ge
    v = b2 * st.v + (1.0 - b2) * ge * ge
    p = p - (lr / bc1) * (m / (torch.sqrt(v) / math.sqrt(bc2) + eps))
    st.p, st.m, st.v = torch.where(live, p, st.p), torch.where(live, m, st.m), torch.where(live, v, st.v)
    if ema_decay is not None:
        st.ema = torch.where(live, ema_decay * st.ema + (1.0 - ema_decay) * st.p, st.ema)
    return info

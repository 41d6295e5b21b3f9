"""GPU: lmn_optim_prepare and lmn_adamw_step_ex alone (include/optim/lmnet_optim.h) against the float64 restatement tests/optim_ref.py.

Sizes: one quad; one quad past a wave; one quad past three blocks; one quad past the grid cap (cap x 1024 + 4 floats: the reduction's
blocks take a second grid-stride iteration).  Group maps: "mixed" changes group every five quads (inside a wave) and holds a group of
one quad; "ends" adds a frozen group at the start and at the end of the buffer."""
import functools

import pytest
import torch

import optim_ref as R
from helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
CAP = 1024
SIZES = [4, 4 * 64 + 4, 4 * 256 * 3 + 4, CAP * 1024 + 4]
TABLE = [(1e-2, 0.1, False), (1e-3, 0.0, False), (5e-3, 0.01, False), (1e-2, 0.1, True)]      # group 3 is frozen
BETAS, EPS, EMA, SCALE = (0.9, 0.99), 1e-8, 0.9, 256.0


def qmap(n, kind):
    n4 = n // 4
    q = ((torch.arange(n4) // 5) % 2).to(torch.uint8)
    if n4 > 2:
        q[n4 // 2] = 2                                   # a group of one quad
    if kind == "ends":
        k = (n4 + 7) // 8
        q[:k] = 3
        q[n4 - k:] = 3
    return q


@functools.lru_cache(maxsize=None)
def case(n, kind):
    """host inputs of one size / group map and the float64 norm of the live gradient (computed once, never modified)"""
    q = qmap(n, kind)
    gid = R.elem_groups(q)
    t = dict(p=R.seeded(n, 11), g=R.seeded(n, 12) * SCALE, m=R.seeded(n, 13, 0.1), v=R.seeded(n, 14).abs(), ema=R.seeded(n, 15))
    live = gid != 3
    norm = float(torch.sqrt((t["g"][live].double() ** 2).sum())) / SCALE
    return q, gid, t, live, norm


def workspace(n, step0=0):
    from lm_net_amd import hip
    ws = torch.zeros(hip.optim_workspace(n))
    c0 = 2 * hip.optim_blocks(n)
    for k, (lr, wd, frozen) in enumerate(TABLE):
        ws[c0 + 16 + 4 * k:c0 + 16 + 4 * k + 3] = torch.tensor([lr, wd, 1.0 if frozen else 0.0])
    ws.view(torch.int32)[c0 + hip.OPTIM_STEP] = step0
    return ws.to(DEV), c0


def device_step(n, kind, g=None, max_norm=None, step0=2, found_inf=None, skip=True, ema=True, scaled=True):
    """prepare + step_ex on fresh copies of the case's buffers -> (tensors, control block as int32 / float32 host views)"""
    from lm_net_amd import hip
    q, _, t, _, _ = case(n, kind)
    d = {k: v.to(DEV) for k, v in t.items()}
    if g is not None:
        d["g"] = g.to(DEV)
    ws, c0 = workspace(n, step0)
    param = hip.optim_param(BETAS, EPS, max_norm, EMA if ema else None, hip.OPTIM_SKIP_NONFINITE if skip else 0, len(TABLE))
    qd = q.to(DEV)
    gs = torch.tensor(SCALE, device=DEV) if scaled else None
    fi = None if found_inf is None else torch.tensor(float(found_inf), device=DEV)
    hip.optim_prepare(d["g"], qd, param, ws, gs, fi)
    hip.adamw_step_ex(d["p"], d["g"], d["m"], d["v"], d["ema"] if ema else None, qd, param, ws)
    torch.cuda.synchronize()
    d["ws"] = ws
    ctrl = ws[c0:c0 + 16].cpu()
    return d, ctrl.view(torch.int32), ctrl


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("kind", ["mixed", "ends"])
@pytest.mark.parametrize("n", SIZES)
def test_grad_norm_and_clip_coefficient(n, kind):
    """grad_norm against float64.  Yardstick: torch.linalg.vector_norm in fp32 on the same (unscaled) values; our relative error may
    be 4 x its error plus 4 ulp (4.8e-7).  max_norm is half the float64 norm, so coef < 1 holds by construction."""
    from lm_net_amd import hip
    _, _, t, live, norm = case(n, kind)
    d, ci, cf = device_step(n, kind, max_norm=0.5 * norm if norm > 0 else 1.0)
    got = float(cf[hip.OPTIM_GRAD_NORM])
    assert ci[hip.OPTIM_SKIP] == 0 and ci[hip.OPTIM_NONFINITE] == 0 and ci[hip.OPTIM_STEP] == 3
    assert float(cf[hip.OPTIM_INV_SCALE]) == 1.0 / SCALE
    if norm == 0.0:                                       # every quad frozen: nothing to sum, nothing to clip
        assert got == 0.0 and float(cf[hip.OPTIM_COEF]) == 1.0
        return
    yard = float(torch.linalg.vector_norm((t["g"][live] / SCALE).to(DEV)))
    e_ours, e_yard = abs(got - norm) / norm, abs(yard - norm) / norm
    assert e_ours <= 4 * e_yard + 4.8e-7, "grad_norm rel err %.3e, torch fp32 vector_norm %.3e (n=%d %s)" % (e_ours, e_yard, n, kind)
    coef_dev = d["ws"][2 * hip.optim_blocks(n) + hip.OPTIM_COEF]
    assert bool((coef_dev < 1.0).item())
    assert abs(float(coef_dev) - 0.5 * norm / (norm + 1e-6)) < 1e-6


@pytest.mark.parametrize("n", SIZES)
def test_two_calls_bit_identical_in_both_determinism_modes(n):
    from lm_net_amd import hip
    _, _, _, _, norm = case(n, "ends")
    runs = []
    try:
        for mode in (False, True, False, True):
            hip.set_deterministic(mode)
            runs.append(device_step(n, "ends", max_norm=0.5 * norm if norm > 0 else 1.0)[0])
    finally:
        hip.set_deterministic(False)
    for r in runs[1:]:
        for k in ("p", "m", "v", "ema", "ws"):            # (ws: block partials, block counts, control block)
            assert same_bits(runs[0][k], r[k]), k


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
@pytest.mark.parametrize("n", SIZES)
def test_nonfinite_in_the_last_quad_skips_the_step(n, value):
    """The last float of the buffer: the tail quad, which sits in the last block at the middle sizes and in a block's second
    iteration at the largest."""
    from lm_net_amd import hip
    _, _, t, _, _ = case(n, "mixed")
    g = t["g"].clone()
    g[n - 1] = value
    d, ci, _ = device_step(n, "mixed", g=g, max_norm=1.0)
    assert ci[hip.OPTIM_SKIP] == 1 and ci[hip.OPTIM_NONFINITE] == 1 and ci[hip.OPTIM_STEP] == 2 and ci[hip.OPTIM_SKIPPED] == 1
    for k in ("p", "m", "v", "ema"):
        assert same_bits(d[k].cpu(), t[k]), k
    # an incoming found_inf alone skips too; without the skip flag (and without a scaler) the same gradient is stepped
    d, ci, _ = device_step(n, "mixed", found_inf=1.0)
    assert ci[hip.OPTIM_SKIP] == 1 and ci[hip.OPTIM_NONFINITE] == 0 and ci[hip.OPTIM_STEP] == 2 and same_bits(d["p"].cpu(), t["p"])
    d, ci, _ = device_step(n, "mixed", found_inf=0.0)
    assert ci[hip.OPTIM_SKIP] == 0 and ci[hip.OPTIM_STEP] == 3 and not same_bits(d["p"].cpu(), t["p"])


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
@pytest.mark.parametrize("n", SIZES)
def test_nonfinite_in_a_frozen_group_is_not_counted(n, value):
    from lm_net_amd import hip
    _, gid, t, live, norm = case(n, "ends")
    g = t["g"].clone()
    g[0] = value                                          # the frozen group at the start ...
    g[n - 1] = value                                      # ... and at the end
    assert not bool(live[0]) and not bool(live[n - 1])
    d, ci, cf = device_step(n, "ends", g=g)
    assert ci[hip.OPTIM_SKIP] == 0 and ci[hip.OPTIM_NONFINITE] == 0 and ci[hip.OPTIM_STEP] == 3 and ci[hip.OPTIM_SKIPPED] == 0
    assert abs(float(cf[hip.OPTIM_GRAD_NORM]) - norm) <= 1e-5 * norm
    for k in ("p", "m", "v", "ema"):                      # frozen quads are not stored, live ones are finite
        out = d[k].cpu()
        assert same_bits(out[~live], t[k][~live]) and bool(torch.isfinite(out[live]).all()), k


@pytest.mark.parametrize("kind", ["mixed", "ends"])
@pytest.mark.parametrize("n", SIZES)
def test_one_step_against_the_restatement(n, kind):
    """Unscale, clip, per-group AdamW at step 3 and EMA against tests/optim_ref.py at 2e-6 relative (max |a - b| / max |b|: the bound
    of test_fused_adamw_matches_torch_adamw_and_exchanges_state for this comparison)."""
    from lm_net_amd import hip
    _, gid, t, live, norm = case(n, kind)
    mn = 0.5 * norm if norm > 0 else 1.0
    st = R.State(t["p"], t["m"], t["v"], t["ema"], step=2)
    info = R.step(st, t["g"], gid, TABLE, BETAS, EPS, mn, EMA, grad_scale=SCALE, skip_nonfinite=True)
    d, ci, cf = device_step(n, kind, max_norm=mn)
    assert not info["skip"] and ci[hip.OPTIM_SKIP] == 0 and ci[hip.OPTIM_STEP] == 3
    assert abs(float(cf[hip.OPTIM_COEF]) - info["coef"]) < 1e-6
    for k, ref in (("p", st.p), ("m", st.m), ("v", st.v), ("ema", st.ema)):
        out = d[k].cpu()
        assert same_bits(out[~live], t[k][~live]), k
        if bool(live.any()):
            assert rel_err(out[live], ref[live]) < 2e-6, (k, rel_err(out[live], ref[live]))
    # no EMA buffer, no scaler, no clipping: the plain per-group step
    st = R.State(t["p"], t["m"], t["v"], step=2)
    R.step(st, t["g"], gid, TABLE, BETAS, EPS)
    d, ci, cf = device_step(n, kind, ema=False, skip=False, scaled=False)
    assert float(cf[hip.OPTIM_GRAD_NORM]) == 0.0 and float(cf[hip.OPTIM_COEF]) == 1.0 and float(cf[hip.OPTIM_INV_SCALE]) == 1.0
    assert same_bits(d["ema"].cpu(), t["ema"])
    if bool(live.any()):
        for k, ref in (("p", st.p), ("m", st.m), ("v", st.v)):
            assert rel_err(d[k].cpu()[live], ref[live]) < 2e-6, k


@pytest.mark.parametrize("n", [4, 4 * 256 * 3 + 4])
def test_plain_adamw_step_vs_f64_owns_the_step_kernel(n):
    """lmn_adamw_step -- the one launch FusedAdamW issues per step when no group table, clipping or EMA is asked for -- against
    torch.optim.AdamW's update written out in float64, and (tests/kernel_forms.py) proof that this test launches the instance it owns."""
    from kernel_forms import launched, owned_by
    from lm_net_amd import hip
    lr, b1, b2, eps, wd, step = 1e-2, 0.9, 0.99, 1e-8, 0.1, 3
    p, g, m, v = R.seeded(n, 11), R.seeded(n, 12), R.seeded(n, 13, 0.1), R.seeded(n, 14).abs()
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p64, g64 = p.double() * (1.0 - lr * wd), g.double()
    m64 = b1 * m.double() + (1.0 - b1) * g64
    v64 = b2 * v.double() + (1.0 - b2) * g64 * g64
    p64 = p64 - (lr / bc1) * m64 / (torch.sqrt(v64) / bc2 ** 0.5 + eps)
    d = [t.to(DEV) for t in (p, g, m, v)]
    _, names = launched(lambda: hip.adamw_step(*d, lr, b1, b2, eps, wd, bc1, bc2))
    assert owned_by("tests/test_optim_kernels_gpu.py::test_plain_adamw_step_vs_f64_owns_the_step_kernel") <= names, names
    for got, ref, what in ((d[0], p64, "p"), (d[2], m64, "m"), (d[3], v64, "v")):
        assert rel_err(got, ref) < 2e-6, (what, n, rel_err(got, ref))      # (the bound of test_one_step_against_the_restatement)
    assert torch.equal(d[1].cpu(), g)

"""GPU: the kernels the wide LM_Net variants need (filters up to 4x the default; README "Wider variants").

  neighbourhood attention   any head_dim 1..32 (csrc/na_gen.hip) against oracle/natten_ref.py in fp64, K = 3 / 5 / 7, fp32 and
                            bf16 storage; LMN_NA_GENERAL=1 runs the general kernels on the head dims of the channel-quad kernels
                            too, and the two forms agree (which form ran is read from the in-library kernel timer)
  GFT attention             head_dim 33..128 (csrc/gattn.hip, padded width 64 / 128) against fp64 softmax(QK^T)V and its autograd
  LayerNorm                 rows of 744..1536 channels (csrc/rows.hip ln_*_wide_kernel)
  deterministic mode        bit-identical results of two runs
"""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from kernel_forms import launched, owned_by

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
HEADS = 12


def _r(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _rel(got, ref):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def _na_case(B, H, W, hd, K, seed=0):
    """fp64 oracle: out, dqkv, drpb of natten_ref for qkv [B,H,W,3C], rpb [12][2K-1][2K-1], dout [B,H,W,C]."""
    from oracle import natten_ref
    C = HEADS * hd
    qkv = _r(B, H, W, 3 * C, seed=seed).requires_grad_(True)
    rpb = (_r(HEADS, 2 * K - 1, 2 * K - 1, seed=seed + 1) * 0.5).requires_grad_(True)
    q, k, v = qkv.reshape(B, H, W, 3, HEADS, hd).permute(3, 0, 4, 1, 2, 5).unbind(0)
    attn = torch.softmax(natten_ref.na2d_qkrpb(q * hd ** -0.5, k, rpb, K), -1)
    out = natten_ref.na2d_av(attn, v, K).permute(0, 2, 3, 1, 4).reshape(B, H, W, C)
    dout = _r(B, H, W, C, seed=seed + 2)
    out.backward(dout)
    return qkv.detach(), rpb.detach(), dout, out.detach(), qkv.grad, rpb.grad


def _na_run(qkv, rpb, dout, dt):
    from lm_net_amd import hip
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    qd, dd = qkv.to(DEV, dt), dout.to(DEV, dt)
    rp = rpb.to(DEV, torch.float32)
    out = torch.full((B, H, W, C), float("nan"), device=DEV, dtype=dt)
    hip.na_fwd(qd, rp, out, HEADS)
    dqkv = torch.full((B, H, W, C3), float("nan"), device=DEV, dtype=dt)
    drpb = torch.zeros_like(rp)
    hip.na_bwd(qd, rp, dd, dqkv, drpb, HEADS)
    torch.cuda.synchronize()
    return out, dqkv, drpb


NA_OWNER = "tests/test_wide_kernels_gpu.py::test_na_general_head_dims_vs_oracle_f64"
GATTN_OWNER = "tests/test_wide_kernels_gpu.py::test_gattn_wide_head_dim_vs_f64"
LN_OWNER = "tests/test_wide_kernels_gpu.py::test_layernorm_wide_rows_vs_f64"


def _na_any_instances(hd, dt):
    """The three na_any_* instances csrc/na_gen.hip (LMN_NG_SELECT) picks for a head dim: lanes per head, vector width of a lane's
    loads, size of its register array."""
    lanes = 2 if hd > 16 and hd % 2 == 0 else 1
    hl = hd // lanes
    vw = 4 if hl % 4 == 0 else 2 if hl % 2 == 0 else 1
    hm = 16 if lanes == 2 else 8 if hl <= 8 else 16 if hl <= 16 else 32
    t = "float" if dt == torch.float32 else "__bf16"
    return {"na_any_%s_kernel<%d, %d, %d, %s>" % (k, lanes, vw, hm, t) for k in ("fwd", "bwd_q", "bwd_kv")}


# maps with partial tiles / blocks and maps no larger than K + 1
NA_MAPS = {3: [(2, 13, 11), (1, 4, 4)], 5: [(1, 13, 10), (1, 6, 6)], 7: [(1, 15, 9), (1, 8, 8)]}


@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("hd", [3, 5, 6, 7, 12, 18, 20, 24, 31, 32])
def test_na_general_head_dims_vs_oracle_f64(hd, K):
    for (B, H, W) in NA_MAPS[K]:
        qkv, rpb, dout, o_ref, dq_ref, drpb_ref = _na_case(B, H, W, hd, K, seed=hd * 10 + K)
        for dt in (torch.float32, torch.bfloat16):
            if dt == torch.bfloat16:   # bf16 storage: compare with the oracle run on the bf16-rounded operands
                qkv_b, dout_b = qkv.to(torch.bfloat16).double(), dout.to(torch.bfloat16).double()
                _, _, _, o_ref_b, dq_ref_b, drpb_ref_b = _na_case_from(qkv_b, rpb, dout_b, K)
                tol_o, tol_g = 1e-2, 2e-2
            else:
                o_ref_b, dq_ref_b, drpb_ref_b = o_ref, dq_ref, drpb_ref
                tol_o, tol_g = 1e-5, 2e-4
            (out, dqkv, drpb), names = launched(lambda: _na_run(qkv, rpb, dout, dt))
            tag = "hd=%d K=%d %dx%dx%d %s" % (hd, K, B, H, W, dt)
            want = _na_any_instances(hd, dt)          # this test owns them (tests/kernel_forms.py): it must launch them, and only them
            assert want <= owned_by(NA_OWNER) and want == {n for n in names if n.startswith("na_")}, (tag, sorted(names), sorted(want))
            assert _rel(out, o_ref_b) < tol_o, (tag, "out", _rel(out, o_ref_b))
            assert _rel(dqkv, dq_ref_b) < tol_g, (tag, "dqkv", _rel(dqkv, dq_ref_b))
            assert _rel(drpb, drpb_ref_b) < tol_g, (tag, "drpb", _rel(drpb, drpb_ref_b))


def _na_case_from(qkv, rpb, dout, K):
    from oracle import natten_ref
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    hd = C // HEADS
    qkv = qkv.clone().requires_grad_(True)
    rpb = rpb.clone().requires_grad_(True)
    q, k, v = qkv.reshape(B, H, W, 3, HEADS, hd).permute(3, 0, 4, 1, 2, 5).unbind(0)
    attn = torch.softmax(natten_ref.na2d_qkrpb(q * hd ** -0.5, k, rpb, K), -1)
    out = natten_ref.na2d_av(attn, v, K).permute(0, 2, 3, 1, 4).reshape(B, H, W, C)
    out.backward(dout)
    return qkv.detach(), rpb.detach(), dout, out.detach(), qkv.grad, rpb.grad


_AB_SCRIPT = r"""
import json, sys, torch
sys.path.insert(0, %r)
from lm_net_amd import hip
res = {}
for hd in (1, 2, 4, 8, 16):
    for K in (3, 5):
        g = torch.Generator().manual_seed(hd * 10 + K)
        B, H, W, C = 2, 19, 23, 12 * hd
        qkv = torch.randn(B, H, W, 3 * C, generator=g).cuda()
        rpb = (torch.randn(12, 2 * K - 1, 2 * K - 1, generator=g) * 0.5).cuda()
        dout = torch.randn(B, H, W, C, generator=g).cuda()
        out = torch.empty(B, H, W, C, device="cuda")
        dqkv = torch.empty(B, H, W, 3 * C, device="cuda")
        drpb = torch.zeros_like(rpb)
        hip.prof_begin()
        hip.na_fwd(qkv, rpb, out, 12)
        hip.na_bwd(qkv, rpb, dout, dqkv, drpb, 12)
        names = sorted(hip.prof_end())
        torch.save((out.cpu(), dqkv.cpu(), drpb.cpu()), %r + "/ab_%%d_%%d.pt" %% (hd, K))
        res["%%d_%%d" %% (hd, K)] = names
print("AB-JSON " + json.dumps(res))
"""


def _ab_run(tmp, general):
    env = dict(os.environ)
    env.pop("LMN_NA_GENERAL", None)
    if general:
        env["LMN_NA_GENERAL"] = "1"
    d = os.path.join(tmp, "gen" if general else "quad")
    os.makedirs(d, exist_ok=True)
    p = subprocess.run([sys.executable, "-c", _AB_SCRIPT % (ROOT, d)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    import json
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("AB-JSON ")][-1]
    return d, json.loads(line[8:])


def test_na_general_switch_matches_quad_kernels(tmp_path):
    """LMN_NA_GENERAL=1 (a fresh process each: the switch is read once) runs the general kernels on hd 1, 2, 4, 8, 16, which otherwise
    take the channel-quad kernels: the kernel names prove which form ran, and the two forms agree."""
    dq, names_q = _ab_run(str(tmp_path), False)
    dg, names_g = _ab_run(str(tmp_path), True)
    for key in names_q:
        assert names_q[key] and not any("na_any_" in n for n in names_q[key]), (key, names_q[key])
        assert names_g[key] and all("na_any_" in n for n in names_g[key]), (key, names_g[key])
        hd, K = (int(v) for v in key.split("_"))
        a = torch.load(os.path.join(dq, "ab_%d_%d.pt" % (hd, K)))
        b = torch.load(os.path.join(dg, "ab_%d_%d.pt" % (hd, K)))
        for what, u, v in zip(("out", "dqkv", "drpb"), a, b):
            assert _rel(v, u) < 2e-5, (key, what, _rel(v, u))


@pytest.mark.parametrize("hd", [6, 24])
def test_na_general_deterministic_bit_identical(hd):
    from lm_net_amd import hip
    qkv, rpb, dout, *_ = _na_case(2, 17, 14, hd, 5, seed=7)
    hip.set_deterministic(True)
    try:
        a = _na_run(qkv, rpb, dout, torch.float32)
        b = _na_run(qkv, rpb, dout, torch.float32)
    finally:
        hip.set_deterministic(False)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("N", [70, 484, 1024])
@pytest.mark.parametrize("hd", [33, 62, 93, 124, 128])
def test_gattn_wide_head_dim_vs_f64(hd, N):
    from lm_net_amd import hip
    B, C = 1 if N > 500 else 2, HEADS * hd
    qkv = (_r(B, N, 3 * C, seed=hd + N) * 0.7).requires_grad_(True)
    q, k, v = qkv.view(B, N, 3, HEADS, hd).permute(2, 0, 3, 1, 4).unbind(0)
    p = torch.softmax((q @ k.transpose(-2, -1)) * hd ** -0.5, -1)
    o_ref = (p @ v).transpose(1, 2).reshape(B, N, C)
    do = _r(B, N, C, seed=hd + N + 1)
    o_ref.backward(do)
    qd = qkv.detach().float().to(DEV)
    out = torch.full((B, N, C), float("nan"), device=DEV)
    lse = torch.empty(B, HEADS, N, device=DEV)
    dqkv = torch.full((B, N, 3 * C), float("nan"), device=DEV)
    delta = torch.empty(B, HEADS, N, device=DEV)
    dod = do.float().to(DEV)
    _, names = launched(lambda: (hip.gattn_fwd(qd, out, lse, HEADS), hip.gattn_bwd(qd, out, dod, lse, dqkv, delta, HEADS)))
    want = {"gattn_%s_kernel<%d, float>" % (k, 64 if hd <= 64 else 128) for k in ("fwd", "bwd_q", "bwd_kv")}
    assert want <= owned_by(GATTN_OWNER) and names == want, (sorted(names), sorted(want))     # (this test owns them: tests/kernel_forms.py)
    assert _rel(out, o_ref) < 1e-5, _rel(out, o_ref)
    assert _rel(dqkv, qkv.grad) < 2e-4, _rel(dqkv, qkv.grad)


@pytest.mark.parametrize("C", [744, 1116, 1488, 1536])
def test_layernorm_wide_rows_vs_f64(C):
    from lm_net_amd import hip
    n = 301
    x = _r(n, C, seed=C).requires_grad_(True)
    g, b = (_r(C, seed=C + 1).abs() + 0.5).requires_grad_(True), _r(C, seed=C + 2).requires_grad_(True)
    y_ref = F.layer_norm(x, (C,), g, b, 1e-5)
    dy, dres = _r(n, C, seed=C + 3), _r(n, C, seed=C + 4)
    y_ref.backward(dy)
    f = lambda t: t.detach().float().to(DEV)
    y = torch.full((n, C), float("nan"), device=DEV)
    dx = torch.full((n, C), float("nan"), device=DEV)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    _, names = launched(lambda: (hip.ln_fwd(f(x), f(g), f(b), y), hip.ln_bwd(f(x), f(g), f(dy), f(dres), dx, dg, db)))
    want = {"ln_fwd_wide_kernel<float>", "ln_bwd_wide_kernel<float>"}
    assert want == owned_by(LN_OWNER) and want <= names, (sorted(names), sorted(want))        # (this test owns them: tests/kernel_forms.py)
    assert _rel(y, y_ref) < 1e-5
    assert _rel(dx, x.grad + dres) < 1e-5
    assert _rel(dg, g.grad) < 2e-4
    assert _rel(db, b.grad) < 2e-4
    hip.set_deterministic(True)
    try:
        outs = []
        for _ in range(2):
            dx2 = torch.empty(n, C, device=DEV)
            dg2, db2 = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
            hip.ln_bwd(f(x), f(g), f(dy), f(dres), dx2, dg2, db2)
            outs.append((dx2, dg2, db2))
        torch.cuda.synchronize()
    finally:
        hip.set_deterministic(False)
    assert all(torch.equal(u, v) for u, v in zip(*outs))

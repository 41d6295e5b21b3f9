"""Kernel checks for the instances that only the wider envelope selects (tests/test_kernel_census_envelope_gpu.py): wide variants,
na_kernel_size 5 / 7, bf16 storage at those widths, the "bf16-mma" precision.  Same shape as kernel_checks.py -- rows of
(name, rel_err, tol), every check wrapped by kernel_forms.owner_check -- and driven by tests/test_kernels_envelope_gpu.py.

fp32 instances are compared with float64.  A bf16-STORAGE instance is compared, on bf16-representable inputs, with the fp32-storage
launch of the same kernel, which a float64 check holds (named at each block): what may differ is the rounding of the stored outputs."""
import torch
import torch.nn.functional as F

import kernel_checks as kc
from kernel_checks import DEV, R, TOL, bf, dev, rel
from kernel_forms import form_row, launched, owner_check
from lm_net_amd import hip
from oracle import natten_ref

HEADS = 12


def r16(*shape, seed, scale=1.0):
    """bf16-representable fp32 device tensor."""
    return dev((R(*shape, seed=seed) * scale).to(torch.bfloat16).double())


def _same(a, b):
    return 0.0 if all(torch.equal(u, v) for u, v in zip(a, b)) else 1.0


def _deterministic_pair(fn):
    """fn() twice in deterministic mode -> 0.0 when every output of the two launches is bit-identical."""
    hip.set_deterministic(True)
    try:
        a, b = fn(), fn()
        torch.cuda.synchronize()
    finally:
        hip.set_deterministic(False)
    return _same(a, b)


# ------------------------------------------------------------------------------------------------ bf16 storage at the wide widths
@owner_check
def check_wide_bf16_rows():
    """The bf16-storage forms of the kernels the wide variants and the larger windows add: global attention at head dims above 32
    (gattn_*_kernel<64 | 128, __bf16>), LayerNorm rows above 512 channels (ln_*_wide_kernel<__bf16>) and the run-time-K neighbourhood
    attention (na_*_gen_kernel<hd, __bf16>, K = 5 / 7).  Their fp32-storage forms are held to float64 by
    tests/test_wide_kernels_gpu.py (test_gattn_wide_head_dim_vs_f64, test_layernorm_wide_rows_vs_f64) and kernel_checks.check_na.
    Each is launched again twice in deterministic mode: bit-identical."""
    rows = []
    # ---- global attention, VALU form at padded width 64 / 128: both widths, their boundaries (33, 64 | 65, 128), the W3 head dim 93; N = 70
    #      and 484 end in a ragged row block (32 rows a block at width 64 and 128) and, at 484, in a ragged key chunk (64 / 32 keys)
    for hd in (33, 64, 65, 93, 128):
        for N in (70, 484):
            B, Cn = 2 if N == 70 else 1, HEADS * hd
            qkv, do = bf(r16(B, N, 3 * Cn, seed=401, scale=0.7)).float(), r16(B, N, Cn, seed=402)

            def run(cv, dt_):
                out, lse = torch.full((B, N, Cn), float("nan"), device=DEV, dtype=dt_), torch.empty(B, HEADS, N, device=DEV)
                hip.gattn_fwd(cv(qkv), out, lse, HEADS)
                dqkv, delta = torch.full((B, N, 3 * Cn), float("nan"), device=DEV, dtype=dt_), torch.empty(B, HEADS, N, device=DEV)
                hip.gattn_bwd(cv(qkv), out, cv(do), lse, dqkv, delta, HEADS)
                return out.float(), dqkv.float(), lse, delta

            o32 = run(lambda t: t, torch.float32)
            o16, names = launched(lambda: run(bf, torch.bfloat16))
            tag = " hd=%d N=%d" % (hd, N)
            D = 64 if hd <= 64 else 128
            rows.append(form_row("bf16 storage wide gattn" + tag, names, ["gattn_%s_kernel<%d, __bf16>" % (k, D) for k in ("fwd", "bwd_q", "bwd_kv")], ["gattn_fwd_mfma", "gattn_bwd_q_mfma", "gattn_bwd_kv_mfma"]))
            # (the VALU kernels convert q, k, v, out and dout to fp32 as they load them -- ld1 / stage_rows in csrc/gattn.hip -- and
            #  contract in fp32: only the stored out and dqkv round, 8e-3; lse stays fp32.  The backward of the bf16 launch reads its own
            #  ROUNDED out for delta = dout . out: a sum of hd products whose factor moved by 2^-9 relative, inside the same 8e-3)
            rows.append(("bf16 storage wide gattn_fwd out" + tag, rel(o16[0], o32[0]), 8e-3))
            rows.append(("bf16 storage wide gattn_fwd lse" + tag, rel(o16[2], o32[2]), 2e-4))
            rows.append(("bf16 storage wide gattn_bwd dqkv" + tag, rel(o16[1], o32[1]), 8e-3))
            rows.append(("bf16 storage wide gattn deterministic, two launches bit-identical" + tag, _deterministic_pair(lambda: run(bf, torch.bfloat16)), 0.5))
    # ---- LayerNorm over rows wider than 512 channels (one wave per row): the narrowest and the widest GFT width of the wide variants;
    #      301 rows: a ragged last block of 4 rows
    for Cn in (744, 1536):
        n = 301
        xl, dyl, drl = r16(n, Cn, seed=411), r16(n, Cn, seed=412), r16(n, Cn, seed=413)
        gl, bl = dev(R(Cn, seed=414).abs() + 0.5), dev(R(Cn, seed=415))

        def run(cv, dt_):
            y = torch.full((n, Cn), float("nan"), device=DEV, dtype=dt_)
            hip.ln_fwd(cv(xl), gl, bl, y)
            dxl, dg, db = torch.full((n, Cn), float("nan"), device=DEV, dtype=dt_), torch.zeros(Cn, device=DEV), torch.zeros(Cn, device=DEV)
            hip.ln_bwd(cv(xl), gl, cv(dyl), cv(drl), dxl, dg, db)
            return y.float(), dxl.float(), dg, db

        o32 = run(lambda t: t, torch.float32)
        o16, names = launched(lambda: run(bf, torch.bfloat16))
        rows.append(form_row("bf16 storage wide ln C=%d" % Cn, names, ["ln_fwd_wide_kernel<__bf16>", "ln_bwd_wide_kernel<__bf16>"], ["ln_fwd_kernel<", "ln_bwd_kernel<"]))
        # (x, dy and dres become fp32 in ld4, statistics and sums are fp32: y and dx round when stored, dgamma / dbeta stay fp32)
        rows.append(("bf16 storage wide ln_fwd y C=%d" % Cn, rel(o16[0], o32[0]), 8e-3))
        rows.append(("bf16 storage wide ln_bwd dx(+res) C=%d" % Cn, rel(o16[1], o32[1]), 8e-3))
        rows.append(("bf16 storage wide ln_bwd dgamma / dbeta C=%d" % Cn, max(rel(o16[2], o32[2]), rel(o16[3], o32[3])), 2e-4))
        rows.append(("bf16 storage wide ln deterministic, two launches bit-identical C=%d" % Cn, _deterministic_pair(lambda: run(bf, torch.bfloat16)), 0.5))
    # ---- neighbourhood attention with a 5x5 / 7x7 window: the maps and head dims of check_na's K = 5 / 7 rows (maps no larger than
    #      K + 1: 5x5, 7x7; partial blocks: 23x18, 22x15)
    for K, (B, H, W, hd) in [(5, s) for s in [(2, 7, 9, 1), (1, 5, 5, 2), (1, 9, 6, 4), (2, 23, 18, 2), (1, 11, 12, 8), (1, 5, 21, 16)]] + \
                            [(7, s) for s in [(1, 7, 7, 1), (2, 9, 12, 2), (1, 22, 15, 4), (1, 8, 13, 8)]]:
        Cn = HEADS * hd
        qkv, do = r16(B, H, W, 3 * Cn, seed=421), r16(B, H, W, Cn, seed=423)
        rpb = dev(R(HEADS, 2 * K - 1, 2 * K - 1, seed=422) * 0.5)

        def run(cv, dt_):
            o = torch.full((B, H, W, Cn), float("nan"), device=DEV, dtype=dt_)
            hip.na_fwd(cv(qkv), rpb, o, HEADS)
            g, r = torch.full((B, H, W, 3 * Cn), float("nan"), device=DEV, dtype=dt_), torch.zeros_like(rpb)
            hip.na_bwd(cv(qkv), rpb, cv(do), g, r, HEADS)
            return o.float(), g.float(), r

        o32 = run(lambda t: t, torch.float32)
        o16, names = launched(lambda: run(bf, torch.bfloat16))
        tag = " K=%d hd=%d %dx%d" % (K, hd, H, W)
        rows.append(form_row("bf16 storage na" + tag + ": general-K kernels", names, ["na_%s_gen_kernel<%d, __bf16>" % (k, hd) for k in ("fwd", "bwd_q", "bwd_kv")],
                             ["na_fwd_kernel<", "na_bwd_fused", "na_bwd_q_kernel<", "na_bwd_kv_kernel<", "na_any"]))
        # (ldv converts on load, the window sums are fp32: out and dqkv round when stored, the bias-table gradient stays fp32)
        rows.append(("bf16 storage na_fwd" + tag, rel(o16[0], o32[0]), 8e-3))
        rows.append(("bf16 storage na_bwd dqkv" + tag, rel(o16[1], o32[1]), 8e-3))
        rows.append(("bf16 storage na_bwd drpb" + tag, rel(o16[2], o32[2]), 2e-4))
        rows.append(("bf16 storage na deterministic, two launches bit-identical" + tag, _deterministic_pair(lambda: run(bf, torch.bfloat16)), 0.5))
    return rows


# ------------------------------------------------------------------------------------------------ head dim 16 of the 3x3 window
@owner_check
def check_na_hd16():
    """na_*_kernel<16, float>: the LDS-tiled 3x3 kernels at head dim 16 (filters[3] = 192 of W2, 8x8 and 44x44 maps), against
    oracle/natten_ref.py in float64 as kernel_checks.check_na holds head dims 1..8.  A 3x3 map (no interior), the W2 maps, and a map
    whose tiles end two short of the border."""
    rows = []
    K, hd = 3, 16
    for (B, H, W) in [(1, 3, 3), (2, 8, 8), (1, 9, 6), (1, 17, 19), (1, 44, 44)]:
        Cn = HEADS * hd
        qkv = R(B, H, W, 3 * Cn, seed=91).requires_grad_(True)
        rpb = (R(HEADS, 2 * K - 1, 2 * K - 1, seed=92) * 0.5).requires_grad_(True)
        q, k, v = qkv.reshape(B, H, W, 3, HEADS, hd).permute(3, 0, 4, 1, 2, 5).unbind(0)
        attn = torch.softmax(natten_ref.na2d_qkrpb(q * hd ** -0.5, k, rpb, K), -1)
        o_ref = natten_ref.na2d_av(attn, v, K).permute(0, 2, 3, 1, 4).reshape(B, H, W, Cn)
        do = R(B, H, W, Cn, seed=93)
        o_ref.backward(do)
        tag = " K=3 hd=16 %dx%d" % (H, W)
        out = torch.full((B, H, W, Cn), float("nan"), device=DEV)
        dqkv = torch.full((B, H, W, 3 * Cn), float("nan"), device=DEV)
        drpb = torch.zeros(HEADS, 2 * K - 1, 2 * K - 1, device=DEV)
        _, names = launched(lambda: (hip.na_fwd(dev(qkv), dev(rpb), out, HEADS), hip.na_bwd(dev(qkv), dev(rpb), dev(do), dqkv, drpb, HEADS)))
        rows.append(form_row("na" + tag + ": LDS-tiled kernels, q pass + k/v pass", names, ["na_fwd_kernel<16, float>", "na_bwd_q_kernel<16, float>", "na_bwd_kv_kernel<16, float>"],
                             ["na_fwd_gen", "na_bwd_fused", "na_bwd_q_gen", "na_bwd_kv_gen", "na_any"]))
        rows.append(("na_fwd" + tag, rel(out, o_ref), TOL))
        rows.append(("na_bwd dqkv" + tag, rel(dqkv, qkv.grad), 2e-4))
        rows.append(("na_bwd drpb" + tag, rel(drpb, rpb.grad), 2e-4))
    return rows


# ------------------------------------------------------------------------------------------------ row kernels of the wide variants
@owner_check
def check_rows_envelope():
    """Row kernels that take another form at the wide widths or in a deploy-mode bf16 forward: avgpool_fwd_kernel (more than 256
    channels: a block per output pixel; W3 pools 288 channels, W4 384), bnact_fwd_kernel<__bf16> (BatchNorm + activation from
    running statistics), ln_bwd_kernel<16, __bf16> (16 lanes a row: 48 channels)."""
    rows = []
    for (B, Ho, Wo, f, Cn) in [(2, 3, 4, 2, 288), (1, 2, 3, 4, 384), (1, 1, 1, 8, 1020)]:     # (1020: the last float4 slot of a 1024-wide row stays empty)
        x = R(B, Cn, Ho * f, Wo * f, seed=501).to(torch.bfloat16).double()
        y_ref = F.adaptive_avg_pool2d(x, (Ho, Wo))
        xd = kc.nhwc(x)
        b32, b16 = torch.zeros(B, Ho, Wo, Cn + 8, device=DEV), torch.zeros(B, Ho, Wo, Cn + 8, device=DEV, dtype=torch.bfloat16)
        _, n32 = launched(lambda: hip.avgpool_fwd(xd, hip.V(b32, 4, Cn), f))
        _, n16 = launched(lambda: hip.avgpool_fwd(bf(xd), hip.V(b16, 4, Cn), f))
        tag = " f=%d C=%d" % (f, Cn)
        rows.append(form_row("avgpool_fwd" + tag + ": block per output pixel", n32 | n16, ["avgpool_fwd_kernel<float>", "avgpool_fwd_kernel<__bf16>"], ["avgpool_fwd_wave"]))
        rows.append(("avgpool_fwd (into slice) vs fp64" + tag, rel(kc.nchw(b32[..., 4:4 + Cn]), y_ref), TOL))
        rows.append(("avgpool_fwd: the slice's neighbours stay untouched" + tag, float(b32[..., :4].abs().max() + b32[..., 4 + Cn:].abs().max() + b16[..., :4].float().abs().max() + b16[..., 4 + Cn:].float().abs().max()), 0.0))
        rows.append(("bf16 storage avgpool_fwd" + tag, rel(b16[..., 4:4 + Cn].float(), b32[..., 4:4 + Cn]), 8e-3))     # (fp32 sums; the stored mean rounds)
    # BatchNorm + activation from given coefficients (eval forward): the fp32 form is held to fp64 by kernel_checks.check_bn_tail
    for Cn, n, act in ((24, 403, hip.ACT_GELU), (96, 77, hip.ACT_HSWISH)):
        z = r16(n, Cn, seed=511, scale=1.3)
        a, b = dev(R(Cn, seed=512).abs() + 0.5), dev(R(Cn, seed=513))
        y32, y16 = torch.full((n, Cn), float("nan"), device=DEV), torch.full((n, Cn), float("nan"), device=DEV, dtype=torch.bfloat16)
        hip.bnact_fwd(z, a, b, y32, act)
        _, names = launched(lambda: hip.bnact_fwd(bf(z), a, b, y16, act))
        rows.append(form_row("bf16 storage bnact_fwd C=%d" % Cn, names, ["bnact_fwd_kernel<__bf16>"]))
        zz = z.double().cpu() * a.double().cpu() + b.double().cpu()
        ref = kc.gelu(zz) if act == hip.ACT_GELU else zz * torch.clamp(zz + 3, 0, 6) / 6
        rows.append(("bnact_fwd vs fp64 C=%d" % Cn, rel(y32, ref), TOL))
        rows.append(("bf16 storage bnact_fwd C=%d" % Cn, rel(y16.float(), y32), 8e-3))
    # LayerNorm backward at 48 channels (16 lanes a row), bf16 storage: the fp32 form is held to fp64 by kernel_checks.check_ln
    Cn, n = 48, 203
    xl, dyl, drl = r16(n, Cn, seed=521), r16(n, Cn, seed=522), r16(n, Cn, seed=523)
    gl = dev(R(Cn, seed=524).abs() + 0.5)
    outs = []
    for cv, dt_ in ((lambda t: t, torch.float32), (bf, torch.bfloat16)):
        dxl, dg, db = torch.full((n, Cn), float("nan"), device=DEV, dtype=dt_), torch.zeros(Cn, device=DEV), torch.zeros(Cn, device=DEV)
        _, names = launched(lambda: hip.ln_bwd(cv(xl), gl, cv(dyl), cv(drl), dxl, dg, db))
        outs.append((dxl.float(), dg, db))
    rows.append(form_row("bf16 storage ln_bwd C=48: 16 lanes a row", names, ["ln_bwd_kernel<16, __bf16>"]))
    rows.append(("bf16 storage ln_bwd dx(+res) C=48", rel(outs[1][0], outs[0][0]), 8e-3))
    rows.append(("bf16 storage ln_bwd dgamma / dbeta C=48", max(rel(outs[1][1], outs[0][1]), rel(outs[1][2], outs[0][2])), 2e-4))
    return rows


# ------------------------------------------------------------------------------------------------ 1x1 weight gradients, other tile shapes
@owner_check
def check_wgrad_1x1_envelope():
    """The direct 1x1 weight-gradient kernels pick (cout tiles x cin tiles) a block from the channel counts (wgrad_tile_shape,
    csrc/conv_wgrad.hip); the wide variants, the 64-class head and bf16 storage select shapes the default model never does.  Channel
    counts of the layers that selected them, against fp64 einsum, on the smallest maps that keep the direct kernels (32 pixels).
    bf16 storage draws bf16-representable operands: products exact, fp32 sums (2e-4), except under the on-load GELU x gate, which
    rounds the operand (1e-2, as kernel_checks.check_conv_rp)."""
    rows = []
    f32, b16 = torch.float32, torch.bfloat16
    to_rp = hip.nhwc_to_rp4
    kern = lambda k, m, n, pm: "%s<%d, %d, %d>" % (k, m, n, pm)
    cases = [
        # (what, B, H, W, Cin, Cout, storage, row-planar dy, expected instance)
        ("head of 64 classes, 12 -> 64", 2, 6, 8, 12, 64, f32, False, kern("wgrad_1x1w_kernel", 4, 1, 0)),
        ("head of W3, 36 -> 4 (2 classes on 4 rows)", 2, 6, 8, 36, 4, f32, False, kern("wgrad_1x1w_kernel", 1, 3, 0)),
        ("head of W3, 36 -> 4 (2 classes on 4 rows)", 2, 6, 8, 36, 4, b16, False, kern("wgrad_1x1_kernel", 1, 3, 2)),
        ("stem expand conv of W2, 4 -> 48, dy row-planar", 2, 6, 8, 4, 48, f32, True, kern("wgrad_1x1w_kernel", 3, 1, 4)),
        ("stem expand conv of W3, 4 -> 72, dy row-planar", 1, 5, 8, 4, 72, f32, True, kern("wgrad_1x1w_kernel", 3, 1, 4)),
        ("stem expand conv of W2, 4 -> 48, dy row-planar", 2, 6, 8, 4, 48, b16, True, kern("wgrad_1x1_kernel", 3, 1, 6)),
    ]
    for what, B, H, W, Cin, Cout, dt, rp, want in cases:
        q = (lambda t: t) if dt == f32 else (lambda t: t.to(b16).double())
        prev = hip._MMA[0]
        hip._MMA[0] = hip.F32 if dt == f32 else hip.BF16
        try:
            xr, dyr = q(R(B, Cin, H, W, seed=531)), q(R(B, Cout, H, W, seed=532))
            x, dy = kc.nhwc(xr).to(dt).contiguous(), kc.nhwc(dyr).to(dt).contiguous()
            dW, db = torch.zeros(Cout, Cin, device=DEV), torch.zeros(Cout, device=DEV)
            _, names = launched(lambda: hip.conv_wgrad([x], to_rp(dy) if rp else dy, dW, db, B=B, Hin=H, Win=W, Hout=H, Wout=W, Cout=Cout))
        finally:
            hip._MMA[0] = prev
        tag = " %s %dx%dx%d %s" % (what, B, H, W, "bf16" if dt == b16 else "fp32")
        rows.append(form_row("wgrad 1x1" + tag, names, [want]))
        rows.append(("wgrad 1x1 dW / db vs fp64" + tag, max(rel(dW, torch.einsum("bchw,bihw->ci", dyr, xr)), rel(db, dyr.sum((0, 2, 3)))), 2e-4))
    # pointwise + shortcut conv of Wodd's first block: sources (row-planar pre with GELU x gate: 36 channels, x: 12), dy 12
    for dt, want in ((f32, kern("wgrad_1x1w_kernel", 1, 4, 4)), (b16, kern("wgrad_1x1w_kernel", 1, 4, 6))):
        B, H, W, Cin, E, Cout = 2, 6, 8, 12, 36, 12
        q = (lambda t: t) if dt == f32 else (lambda t: t.to(b16).double())
        prev = hip._MMA[0]
        hip._MMA[0] = hip.F32 if dt == f32 else hip.BF16
        try:
            xr, prer, dyr = q(R(B, Cin, H, W, seed=541)), q(R(B, E, H, W, seed=542)), q(R(B, Cout, H, W, seed=543))
            gater = R(B, E, seed=544).abs()
            x, pre, dy = (kc.nhwc(t).to(dt).contiguous() for t in (xr, prer, dyr))
            dW, db = torch.zeros(Cout, E + Cin, device=DEV), torch.zeros(Cout, device=DEV)
            _, names = launched(lambda: hip.conv_wgrad([dict(view=to_rp(pre), scale=dev(gater), flags=hip.SRC_GELU), x], dy, dW, db,
                                                       B=B, Hin=H, Win=W, Hout=H, Wout=W, Cout=Cout))
        finally:
            hip._MMA[0] = prev
        tag = " Wodd pointwise + shortcut 36 + 12 -> 12 %s" % ("bf16" if dt == b16 else "fp32")
        gx = kc.gelu(prer) * gater.view(B, E, 1, 1)
        rows.append(form_row("wgrad 1x1" + tag, names, [want]))
        rows.append(("wgrad 1x1 dW / db vs fp64" + tag, max(rel(dW, torch.einsum("bchw,bihw->ci", dyr, torch.cat([gx, xr], 1))), rel(db, dyr.sum((0, 2, 3)))), 2e-4 if dt == f32 else 1e-2))
    return rows


# ------------------------------------------------------------------------------------------------ BatchNorm backward of the wide expand convs
@owner_check
def check_bn_bwd_rp_wide():
    """expand_conv backward (1x1 conv recomputed, batch-statistics BatchNorm + Hardswish backward in the epilogue: BN_BWD1 statistics
    pass, BN_BWD2 applying pass, as kernel_checks.check_conv_bn_epilogues) with ROW-PLANAR dx1 and dz at more than 80 output channels
    -- the M-split kernel, which W3 and W4 reach (expand convs of 144 and more channels) and the default model never does.  fp32
    against the fp64 autograd of the reference graph; bf16 storage on bf16-representable x, w and dx1 (the recomputed z is then
    exact): stored dz rounds (8e-3), gamma / beta gradients stay fp32 (2e-4)."""
    rows = []
    f32, b16 = torch.float32, torch.bfloat16
    for (B, H, W, Cin, E) in [(2, 8, 8, 48, 96), (1, 5, 8, 72, 144)]:
        for dt in (f32, b16):
            q = (lambda t: t) if dt == f32 else (lambda t: t.to(b16).double())
            x = q(R(B, Cin, H, W, seed=551))
            w, b = q(R(E, Cin, 1, 1, seed=552, scale=0.4)), R(E, seed=553)
            g, be = (R(E, seed=554).abs() + 0.5).requires_grad_(True), R(E, seed=555).requires_grad_(True)
            dx1 = q(R(B, E, H, W, seed=556))
            zr = F.conv2d(x, w, b).requires_grad_(True)
            h2 = F.batch_norm(zr, None, None, g, be, True, 0.1, 1e-5)
            (h2 * torch.clamp(h2 + 3, 0, 6) / 6).backward(dx1)
            N = B * H * W
            z = zr.detach()
            mean, rstd = z.mean((0, 2, 3)), 1 / torch.sqrt(z.var((0, 2, 3), unbiased=False) + 1e-5)
            prev = hip._MMA[0]
            hip._MMA[0] = hip.F32 if dt == f32 else hip.BF16
            try:
                wp = hip.conv_pack(dev(w), 1, [Cin])
                xd, aux = kc.nhwc(x).to(dt).contiguous(), hip.nhwc_to_rp4(kc.nhwc(dx1).to(dt).contiguous())
                kw = dict(B=B, Hin=H, Win=W, Hout=H, Wout=W, Cout=E, bias=dev(b))
                st = torch.zeros(2, E, device=DEV)
                _, n1 = launched(lambda: hip.conv_fwd([xd], wp, None, epilogue=hip.EP_BN_BWD1, act=hip.ACT_HSWISH, p=(dev(mean), dev(rstd), dev(g), dev(be)),
                                                      aux=aux, stats=st, stats_mode=hip.STATS_EP, **kw))
                A = dev(g.detach() * rstd)
                dg, db_, c1, c2, c3 = (torch.zeros(E, device=DEV) for _ in range(5))
                hip.bn_bwd_coef(st, N, A, dg, db_, c1, c2, c3, True)
                dz = hip.rp4(torch.full((B, H, W, E), float("nan"), device=DEV, dtype=dt))
                _, n2 = launched(lambda: hip.conv_fwd([xd], wp, dz, epilogue=hip.EP_BN_BWD2, act=hip.ACT_HSWISH,
                                                      p=(dev(mean), dev(rstd), c1, c2, c3, dev(g), dev(be)), aux=aux, **kw))
            finally:
                hip._MMA[0] = prev
            pm = 4 if dt == f32 else 6
            tag = " %d->%d %dx%dx%d %s" % (Cin, E, B, H, W, "bf16" if dt == b16 else "fp32")
            rows.append(form_row("conv BN_BWD1 statistics pass, row-planar dx1" + tag, n1, ["conv_tileM_kernel<1, 1, 3, %d, false, false>" % pm]))
            rows.append(form_row("conv BN_BWD2 applying pass, row-planar dx1 and dz" + tag, n2, ["conv_tileM_kernel<1, 1, 4, %d, false, false>" % pm]))
            rows.append(("conv BN_BWD1 row-planar: dgamma / dbeta" + tag, max(rel(dg, g.grad), rel(db_, be.grad)), 2e-4))
            rows.append(("conv BN_BWD2 row-planar: dz" + tag, rel(kc.nchwE(dz), zr.grad), 2e-4 if dt == f32 else 8e-3))
    return rows


# ------------------------------------------------------------------------------------------------ bf16 matrix-core operands on fp32 storage
# (not in the list: check_conv_dma1 packs two weights into one buffer at fp32 offsets, and the bf16 pack is half as long; the
#  BatchNorm-backward rows of check_conv_large score the largest element of 1.4 M, and Hardswish's derivative jumps by 0.5 at +-3: a
#  recomputed z that rounds across the jump costs 0.25 of the largest element; the same rows on 144 pixels are in the
#  list.  check_conv_rp, check_conv3_storage and the DGELU widths of
#  check_conv_bn_epilogues carry "bf16-mma" cases of their own, on bf16-representable operands at their fp32 tolerances)
MMA_FAMILIES = ["check_conv_fwd", "check_conv_bwd_data", "check_conv_wgrad", "check_conv_dropout", "check_conv_bn_epilogues", "check_ln_linear",
                "check_conv_up2", "check_fused_sources_modes", "check_conv_dma3", "check_conv_dmaM", "check_zpath"]


@owner_check
def check_conv_mma_forms():
    """compute_dtype = "bf16-mma": fp32 activations in memory, operands rounded to bf16 as they are staged, fp32 accumulation.  Every
    conv / weight-gradient instance carries the operand type as a template argument, so the step launches a second set of instances
    (`conv_tile_kernel<1, 2, 0, false, 1, ...>` beside `<..., 0, ...>`).  The float64 checks of the conv family are run again with
    bf16 operands, as kernel_checks.check_conv_bf16 runs five of them, at its rounding tolerance: 1e-2 (two operands rounded to 8
    significant bits, 2^-8 a product, averaged over the reduction) wherever the fp32 tolerance is tighter.  Their rows of dispatch
    claims (form_row) name the fp32-operand instances and are left out: which instances ran here is this check's own last row."""
    rows = []
    prev = hip._MMA[0]
    hip._MMA[0] = hip.BF16
    try:
        for fam in MMA_FAMILIES:
            for n, e, t in getattr(kc, fam)():
                if n.startswith("form:"):
                    continue
                rows.append(("bf16-mma " + n, e, max(t, 1e-2) if 1e-20 < t < 1e-2 else t))
    finally:
        hip._MMA[0] = prev
    return rows

"""GPU: the C entries that do not allocate through the engine, each called on tensors carved out of a GuardPool (tests/guard.py):
inputs, outputs, parameter tables and workspaces end flush against canary bytes, workspaces and packed weights get exactly the bytes
their size query returns.  After each call: the canaries are intact, the inputs are unchanged, and the outputs equal, bit for bit,
those of the same call on ordinary tensors (both start from the same 0xFF poison, so elements a kernel leaves alone compare too).
Entries that sum with float atomics run in deterministic mode; the kernel_checks.py families keep their own fp64 references and
tolerances.  Two ways of putting a call into the pool:

  * direct calls of the `hip.` wrappers on pool tensors (_call);
  * for code that allocates for itself -- the wrappers' own `torch.empty` (packed weights, K-split scratch), DeviceAugment,
    DevicePostprocess, SurfaceDistanceMeter and every check_* of kernel_checks.py -- the module's `torch` global is replaced by a
    proxy whose device factories carve from the pool (_PoolTorch): the code under test runs unchanged, with exact-size buffers."""

import numpy as np
import pytest
import torch

from guard import GuardPool, LaunchLog

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _bytes(t):
    return t.contiguous().view(torch.uint8).flatten()


def _poison(shape, dtype):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV).view(dtype).view(tuple(shape))


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(1234 + seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _randint(lo, hi, shape, dtype, seed=0):
    g = torch.Generator().manual_seed(4321 + seed)
    return torch.randint(lo, hi, shape, generator=g).to(dtype).to(DEV)


def _call(what, fn, ins, outs):
    """fn(t) with t = {name: tensor}: once on ordinary tensors, once inside a pool.  ins: name -> tensor (must come back unchanged);
    outs: name -> (shape, dtype) (starts as poison) or a tensor (an in/out operand: starts from these values)."""
    def fresh(spec):
        return spec.clone() if isinstance(spec, torch.Tensor) else _poison(*spec)
    t = {k: v.clone() for k, v in ins.items()}
    t.update({k: fresh(s) for k, s in outs.items()})
    fn(t)
    torch.cuda.synchronize()
    ref = {k: t[k].clone() for k in outs}
    sizes = [v.numel() * v.element_size() for v in t.values()]
    pool = GuardPool(DEV, GuardPool.size_for(sizes))
    t = {k: pool.take(k, None, None, init=v) for k, v in ins.items()}
    for k, s in outs.items():
        if isinstance(s, torch.Tensor):
            t[k] = pool.take(k, None, None, init=s)
            del pool.inputs[k]
        else:
            t[k] = pool.take(k, s[0], s[1])
    fn(t)
    pool.assert_clean(what)
    pool.assert_inputs_unchanged()
    bad = [k for k in outs if not torch.equal(_bytes(t[k]), _bytes(ref[k]))]
    assert not bad, (what, "pool run differs from the ordinary run", bad)
    return ref


class _PoolTorch:
    """Stands in for the `torch` global of a module: everything passes through, except that tensors the factories below create on
    the device are carved from the pool with their exact size (`empty*` keeps the poison, the others are copied in)."""
    FACTORIES = ("empty", "zeros", "ones", "full", "tensor", "arange", "randn", "rand", "randint", "empty_like", "zeros_like",
                 "ones_like", "full_like")

    def __init__(self, pool):
        self._pool = pool

    def __getattr__(self, name):
        real = getattr(torch, name)
        if name not in self.FACTORIES:
            return real
        pool = self._pool

        def factory(*a, **k):
            t = real(*a, **k)
            if not t.is_cuda:
                return t
            nm = "%s#%d %s" % (name, len(pool.entries) if pool is not None else 0, tuple(t.shape))
            if pool is None:
                return _poison(t.shape, t.dtype) if name.startswith("empty") else t
            if name.startswith("empty"):
                return pool.take(nm, t.shape, t.dtype)
            p = pool.take(nm, None, None, init=t)
            del pool.inputs[nm]
            return p
        return factory


def _into(pool, name, t):
    return pool.take(name, None, None, init=t)


@pytest.fixture
def deterministic():
    from lm_net_amd import hip
    was = hip.get_deterministic()
    hip.set_deterministic(True)
    try:
        yield
    finally:
        hip.set_deterministic(was)


# ------------------------------------------------------------------------------------------------------------- loss and confusion
@pytest.mark.parametrize("Cn", [2, 3, 4, 8, 5, 9, 33, 64])
def test_segloss_and_confusion(Cn, deterministic):
    """Templated (2, 3, 4, 8) and general class counts; B = 3 at 33x47: HW = 1551 is no multiple of 64 or 256."""
    from lm_net_amd import hip
    B, H, W = 3, 33, 47
    logits = _rand(B, Cn, H, W, seed=Cn)
    target = _randint(0, Cn, (B, H, W), torch.int64, seed=Cn)
    w_ce, w_dice = _rand(Cn, seed=1).abs() + 0.5, _rand(Cn, seed=2).abs() + 0.5
    ins = dict(logits=logits, target=target, w_ce=w_ce, w_dice=w_dice)
    ref = _call("segloss_fwd C=%d" % Cn, lambda t: hip.segloss_fwd(t["logits"], t["target"], t["w_ce"], t["w_dice"], 1e-3, 1e-5,
                                                                     t["sums"], t["coef"], t["loss"]),
                ins, dict(sums=((3 + 3 * Cn,), torch.float32), coef=((3 + 2 * Cn,), torch.float32), loss=((1,), torch.float32)))
    assert bool(torch.isfinite(ref["loss"]).all()) and bool(torch.isfinite(ref["coef"]).all())
    gscale = torch.full((1,), 0.75, device=DEV)
    ref = _call("segloss_bwd C=%d" % Cn, lambda t: hip.segloss_bwd(t["logits"], t["target"], t["w_ce"], t["coef"], t["gscale"], t["d"]),
                dict(logits=logits, target=target, w_ce=w_ce, coef=ref["coef"], gscale=gscale), dict(d=((B, Cn, H, W), torch.float32)))
    assert bool(torch.isfinite(ref["d"]).all())
    ref = _call("confusion C=%d" % Cn, lambda t: hip.confusion(t["logits"], t["target"], t["counts"]),
                dict(logits=logits, target=target), dict(counts=torch.zeros(Cn, Cn, device=DEV)))
    assert float(ref["counts"].sum()) == B * H * W
    pred = _randint(0, Cn + 1, (B, H, W), torch.uint8, seed=7)          # (Cn itself: a prediction outside [0, C) is not counted)
    ref = _call("confusion_labels C=%d" % Cn, lambda t: hip.confusion_labels(t["pred"], t["target"], t["counts"]),
                dict(pred=pred, target=target), dict(counts=torch.zeros(Cn, Cn, device=DEV)))
    assert float(ref["counts"].sum()) == int((pred < Cn).sum())


# ------------------------------------------------------------------------------------------ optimiser and flat-buffer utilities
@pytest.mark.parametrize("n", [4, 1028, 4100])
def test_adamw_step(n):
    """n = 4, and just over one block for blocks of 256 threads x 4 floats and of 1024 x 4 (lmn_adamw_step takes n % 4 == 0)."""
    from lm_net_amd import hip
    p, g, m, v = _rand(n, seed=1), _rand(n, seed=2), _rand(n, seed=3, scale=0.1), _rand(n, seed=4).abs()
    _call("adamw_step n=%d" % n, lambda t: hip.adamw_step(t["p"], t["g"], t["m"], t["v"], 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.1, 0.001),
          dict(g=g), dict(p=p, m=m, v=v))


@pytest.mark.parametrize("n", [4, 257, 1025, 4099])
def test_flat_utilities(n):
    """fill at any n; add at the next multiple of 4 (lmn_add takes n % 4 == 0)."""
    from lm_net_amd import hip
    ref = _call("fill n=%d" % n, lambda t: hip.fill(t["x"], 2.5), {}, dict(x=((n,), torch.float32)))
    assert bool((ref["x"] == 2.5).all())
    n = (n + 3) // 4 * 4
    a, b, c, d = (_rand(n, seed=10 + i) for i in range(4))
    _call("add2 n=%d" % n, lambda t: hip.add(t["a"], t["b"], None, None, t["o"]), dict(a=a, b=b), dict(o=((n,), torch.float32)))
    _call("add4 n=%d" % n, lambda t: hip.add(t["a"], t["b"], t["c"], t["d"], t["o"]), dict(a=a, b=b, c=c, d=d), dict(o=((n,), torch.float32)))
    _call("add in place n=%d" % n, lambda t: hip.add(t["a"], t["b"]), dict(b=b), dict(a=a))
    ab = a.to(torch.bfloat16)
    _call("add bf16 n=%d" % n, lambda t: hip.add(t["a"], t["b"], None, None, t["o"]), dict(a=ab, b=b.to(torch.bfloat16)), dict(o=((n,), torch.bfloat16)))


@pytest.mark.parametrize("rows", [4, 1031])
def test_strided_utilities(rows, deterministic):
    """colsum / copy_slice / copy2d / affine2 on channel slices that END exactly at the end of their buffers."""
    from lm_net_amd import hip
    V = hip.V
    x = _rand(rows, 20, seed=1)
    for off, Cn in ((8, 12), (0, 20), (16, 4)):
        _call("colsum", lambda t: hip.colsum(V(t["x"], off, Cn), t["o"]), dict(x=x), dict(o=torch.zeros(Cn, device=DEV)))
        _call("copy_slice", lambda t: hip.copy_slice(V(t["x"], off, Cn), V(t["y"], 32 - Cn, Cn)), dict(x=x), dict(y=((rows, 32), torch.float32)))
        _call("copy_slice bf16", lambda t: hip.copy_slice(V(t["x"], off, Cn), V(t["y"], 32 - Cn, Cn)), dict(x=x.to(torch.bfloat16)),
              dict(y=((rows, 32), torch.bfloat16)))
    for cols in (1, 7, 20):
        _call("copy2d", lambda t: hip.copy2d(t["x"].view(-1)[20 - cols:], t["y"], rows, cols, 20, cols),
              dict(x=x), dict(y=((rows, cols), torch.float32)))
    for Cn, dt in ((12, torch.float32), (12, torch.bfloat16), (4, torch.float32)):
        u, v, coef = _rand(rows, Cn, seed=2).to(dt), _rand(rows, Cn, seed=3).to(dt), _rand(3, Cn, seed=4)
        _call("affine2", lambda t: hip.affine2(t["u"], t["v"], t["coef"], t["y"]), dict(u=u, v=v, coef=coef), dict(y=((rows, Cn), dt)))


@pytest.mark.parametrize("Cn", [4, 12, 372])
def test_bn_fold(Cn):
    """Eval-mode BatchNorm folded into (A, shift): the one entry of the norm family kernel_checks.py reaches only through the model."""
    from lm_net_amd import hip
    rm, rv, ga, be = _rand(Cn, seed=1), _rand(Cn, seed=2).abs() + 0.1, _rand(Cn, seed=3), _rand(Cn, seed=4)
    ref = _call("bn_fold C=%d" % Cn, lambda t: hip.bn_fold(t["rm"], t["rv"], t["ga"], t["be"], 1e-5, t["mean"], t["rstd"], t["A"], t["shift"]),
                dict(rm=rm, rv=rv, ga=ga, be=be), {k: ((Cn,), torch.float32) for k in ("mean", "rstd", "A", "shift")})
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())


# ------------------------------------------------------------------------------------------------------------------ input pipeline
@pytest.mark.parametrize("Cn", [1, 2, 3, 9])
def test_layout_conversions(Cn):
    from lm_net_amd import hip
    B, H, W = 2, 7, 13
    cs = (Cn + 3) // 4 * 4
    x = _rand(B, Cn, H, W, seed=Cn)
    for dt in (torch.float32, torch.bfloat16):
        ref = _call("nchw_to_nhwc C=%d" % Cn, lambda t: hip.nchw_to_nhwc(t["x"], t["y"]), dict(x=x), dict(y=((B, H, W, cs), dt)))
        assert torch.equal(ref["y"][..., :Cn].float(), x.permute(0, 2, 3, 1).to(dt).float())
    z = _rand(B, H, W, cs, seed=20 + Cn)
    for dt in (torch.float32, torch.bfloat16):
        ref = _call("nhwc_to_nchw C=%d" % Cn, lambda t: hip.nhwc_to_nchw(t["z"], t["o"]), dict(z=z.to(dt)), dict(o=((B, Cn, H, W), torch.float32)))
        assert torch.equal(ref["o"], z.to(dt)[..., :Cn].permute(0, 3, 1, 2).float())


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("mask_mode", [0, 1])
def test_preprocess_u8(channels, mask_mode):
    from lm_net_amd import hip
    B, Hs, Ws, H, W = 3, 37, 53, 32, 48
    img = _randint(0, 256, (B, Hs, Ws, channels), torch.uint8, seed=1)
    msk = _randint(0, 256 if mask_mode == 0 else 9, (B, Hs, Ws), torch.uint8, seed=2)
    flips = torch.tensor([0, 1, 3], dtype=torch.uint8, device=DEV)
    mean, std = (0.4, 0.5, 0.6)[:channels], (0.2, 0.25, 0.3)[:channels]
    outs = dict(out=((B, channels, H, W), torch.float32), labels=((B, H, W), torch.int64))
    ref = _call("preprocess_u8_ex", lambda t: hip.preprocess_u8_ex(t["img"], t["msk"], t["flips"], t["out"], t["labels"], mean, std,
                                                                    channels, mask_mode), dict(img=img, msk=msk, flips=flips), outs)
    assert bool(torch.isfinite(ref["out"]).all()) and int(ref["labels"].min()) >= 0
    _call("preprocess_u8_ex images only", lambda t: hip.preprocess_u8_ex(t["img"], None, None, t["out"], None, mean, std, channels, mask_mode),
          dict(img=img), dict(out=outs["out"]))
    if channels == 3 and mask_mode == 0:
        got = _call("preprocess_u8", lambda t: hip.preprocess_u8(t["img"], t["msk"], t["flips"], t["out"], t["labels"], mean, std),
                    dict(img=img, msk=msk, flips=flips), outs)
        assert torch.equal(got["out"], ref["out"]) and torch.equal(got["labels"], ref["labels"])


@pytest.mark.parametrize("channels", [1, 3])
def test_augment_u8_ragged_batch(channels, monkeypatch):
    """DeviceAugment with its own allocations (out, labels, scratch, gray sums, the device parameter table) carved from the pool;
    a ragged batch: every sample has its own valid size inside the padded frame buffer."""
    from lm_net_amd import data, hip
    B, Hs, Ws = 4, 61, 83
    img = _randint(0, 256, (B, Hs, Ws, channels), torch.uint8, seed=3)
    msk = _randint(0, 5, (B, Hs, Ws), torch.uint8, seed=4)
    hw = np.array([[61, 83], [33, 47], [17, 83], [60, 19]], dtype=np.int64)
    mean, std = (0.4, 0.5, 0.6)[:channels], (0.2, 0.25, 0.3)[:channels]

    def run():
        aug = data.DeviceAugment((48, 64), mean=mean, std=std, channels=channels, mask_mode="labels", generator=11, p_ssr=0.7, p_cj=0.7)
        params = aug.sample(B, hw)
        return aug, aug(img_t, msk_t, params=params, src_hw=hw)

    img_t, msk_t = img.clone(), msk.clone()
    _, (x0, y0) = run()
    torch.cuda.synchronize()
    pool = GuardPool(DEV, 4 << 20)
    img_t, msk_t = _into(pool, "images", img), _into(pool, "masks", msk)
    monkeypatch.setattr(data, "torch", _PoolTorch(pool))
    with LaunchLog() as log:
        aug, (x1, y1) = run()
    pool.assert_clean("augment_u8")
    pool.assert_inputs_unchanged()
    assert "augment_u8" in log.names                           # hip.augment_u8
    assert len(pool.entries) >= 7                              # images, masks + out, labels, scratch, gray sums, parameter table
    assert torch.equal(_bytes(x0), _bytes(x1)) and torch.equal(y0, y1) and bool(torch.isfinite(x1).all())


# -------------------------------------------------------------------------------------------------------------- surface distances
def _blobs(B, H, W, K, seed):
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    out = torch.zeros(B, H, W, dtype=torch.int64)
    g = np.random.default_rng(seed)
    for b in range(B):
        for k in range(1, K):
            cy, cx, r = g.uniform(0, H), g.uniform(0, W), g.uniform(1, max(2, min(H, W) / 3))
            out[b][((yy - cy) ** 2 + (xx - cx) ** 2) <= r * r] = k
    return out.to(DEV)


@pytest.mark.parametrize("shape", [(2, 2, 2), (2, 63, 63), (2, 65, 65), (2, 352, 352), (1, 1024, 1000)])
def test_surface_dist(shape, monkeypatch):
    """SurfaceDistanceMeter.update with its workspace (exactly lmn_surface_workspace bytes) and statistics carved from the pool, in
    one chunk and with a workspace budget that forces one call per sample and class."""
    from lm_net_amd import hip, metrics
    B, H, W = shape
    K = 4
    pred, target = _blobs(B, H, W, K, 1), _blobs(B, H, W, K, 2)
    logits = _rand(B, K, H, W, seed=5)
    one = hip.surface_workspace(1, 1, H, W)
    for budget in (256.0, (one + 1) / float(1 << 20)):
        for p in (pred, logits):
            def run(p_, t_):
                m = metrics.SurfaceDistanceMeter(K, workspace_mb=budget)
                m.update(p_, t_)
                return m
            m0 = run(p, target)
            torch.cuda.synchronize()
            bs, ks = m0.chunking(B, H, W)
            calls = -(-B // bs) * -(-(K - 1) // ks)
            pool = GuardPool(DEV, hip.surface_workspace(bs, ks, H, W) + p.numel() * p.element_size() + target.numel() * 8
                             + (1 << 20) + 8192 * (5 + 2 * calls))
            pp, tt = _into(pool, "pred", p), _into(pool, "target", target)
            with monkeypatch.context() as mp:
                mp.setattr(metrics, "torch", _PoolTorch(pool))
                with LaunchLog() as log:
                    m1 = run(pp, tt)
            pool.assert_clean("surface_dist %s budget %.3f MB" % (shape, budget))
            pool.assert_inputs_unchanged()
            assert "surface_dist" in log.names                 # hip.surface_dist
            assert log.names.count("surface_dist") == calls
            assert calls == 1 if budget == 256.0 else (calls > 1 or H < 63), (calls, bs, ks)     # the small budget really chunks
            want = hip.surface_workspace(bs, ks, H, W)         # the one workspace serves every chunk of the update
            assert any(e[2] == want and e[0].startswith("empty#") for e in pool.entries), (want, [e[2] for e in pool.entries])
            for a, b in zip(m0._si + m0._sf, m1._si + m1._sf):
                assert torch.equal(_bytes(a), _bytes(b))


# ------------------------------------------------------------------------------------------------------------------ post-processing
@pytest.mark.parametrize("shape", [(2, 2, 2), (2, 33, 65), (1, 1024, 1000)])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_post_clean_render_and_cc_label(shape, connectivity, monkeypatch):
    """DevicePostprocess (lmn_post_clean with exactly lmn_post_workspace bytes, lmn_post_render into a ragged frame batch) and
    .components (lmn_cc_label) with every buffer carved from the pool."""
    from lm_net_amd import hip, post
    B, H, W = shape
    K = 4
    logits = _rand(B, K, H, W, seed=9) + 2.0 * torch.nn.functional.one_hot(_blobs(B, H, W, K, 3), K).permute(0, 3, 1, 2).float()
    Hs, Ws = H + 5, W + 3
    frames = _randint(0, 256, (B, Hs, Ws, 3), torch.uint8, seed=6)
    hw = np.array([[Hs, Ws], [max(1, Hs // 2), max(1, Ws - 1)]][:B], dtype=np.int64)

    def run(lg, fr):
        pp = post.DevicePostprocess(K, connectivity=connectivity, keep_largest=[1], min_area=3, fill_holes=True, alpha=0.5)
        o = pp(lg, src_hw=hw, frames=fr)
        r, a = pp.components(lg)
        return [o.labels_net, o.labels, o.overlay, o.stats, r, a]

    ref = run(logits, frames)
    torch.cuda.synchronize()
    pool = GuardPool(DEV, hip.post_workspace(B, H, W) + logits.numel() * 4 + 5 * frames.numel() + 12 * B * H * W + (1 << 20))
    lg, fr = _into(pool, "logits", logits), _into(pool, "frames", frames)
    monkeypatch.setattr(post, "torch", _PoolTorch(pool))
    with LaunchLog() as log:
        got = run(lg, fr)
    pool.assert_clean("post %s c%d" % (shape, connectivity))
    pool.assert_inputs_unchanged()
    for w in ("post_clean", "post_render", "cc_label"):        # hip.post_clean hip.post_render hip.cc_label
        assert w in log.names, w
    assert any(e[2] == hip.post_workspace(B, H, W) and e[0].startswith("empty#") for e in pool.entries)
    for a, b in zip(ref, got):
        assert torch.equal(_bytes(a), _bytes(b))


# ---------------------------------------------------------------------------------------------------------- packing and convolutions
def test_conv_pack_exact_size_feeds_conv_fwd(monkeypatch):
    """conv_pack / conv_pack_t write `out` of exactly lmn_conv_pack_size floats (fp32 and bf16 forms) and one conv_fwd reads it;
    a recorded PackPlan re-packs the same buffer with lmn_conv_pack_batch."""
    from lm_net_amd import hip
    for mma in (hip.F32, hip.BF16):
        for (k, cins, cout, B, H, W) in [(1, [12], 24, 2, 9, 7), (1, [24, 12], 12, 2, 6, 7), (3, [12], 12, 2, 10, 11), (3, [4], 12, 1, 8, 9),
                                         (1, [372], 744, 1, 6, 6)]:
            cin = sum(cins)
            w = torch.nn.Parameter(_rand(cout, cin, k, k, seed=k + cout, scale=0.1))
            xs = [_rand(B, H, W, c, seed=c) for c in cins]
            dy = _rand(B, H, W, cout, seed=77)

            def run(pool):
                hip._MMA[0] = mma
                plan = hip.PackPlan()
                hip._PLAN[0] = plan
                try:
                    src = [_into(pool, "x%d" % i, x) for i, x in enumerate(xs)] if pool else xs
                    d = _into(pool, "dy", dy) if pool else dy
                    wp = hip.conv_pack(w, k, cins)
                    assert wp.numel() == hip.conv_pack_size(k, cout, cins)
                    out = pool.take("out", (B, H, W, cout)) if pool else _poison((B, H, W, cout), torch.float32)
                    hip.conv_fwd(src, wp, out, B=B, Hin=H, Win=W, Hout=H, Wout=W, Cout=cout, ksize=k)
                    res = [wp.clone(), out]
                    if len(cins) == 1:
                        rows = (cin + 3) // 4 * 4
                        wt = hip.conv_pack_t(w, k, 0, rows)
                        assert wt.numel() == hip.conv_pack_size(k, rows, [cout])
                        dx = pool.take("dx", (B, H, W, rows)) if pool else _poison((B, H, W, rows), torch.float32)
                        hip.conv_fwd([d], wt, dx, B=B, Hin=H, Win=W, Hout=H, Wout=W, Cout=rows, ksize=k, transposed=1)
                        res += [wt.clone(), dx]
                    torch.cuda.synchronize()
                    first = wp.clone()
                    wp.view(torch.uint8).fill_(0xFF)
                    plan.refresh()                              # hip.PackPlan: one lmn_conv_pack_batch launch re-packs every job
                    torch.cuda.synchronize()
                    assert plan.fresh and torch.equal(_bytes(hip.conv_pack(w, k, cins)), _bytes(first))
                    return res
                finally:
                    hip._MMA[0], hip._PLAN[0] = hip.F32, None

            with monkeypatch.context() as mp:
                mp.setattr(hip, "torch", _PoolTorch(None))       # (ordinary tensors, but starting from the same poison)
                ref = run(None)
            pool = GuardPool(DEV, 64 << 20)
            with monkeypatch.context() as mp:
                mp.setattr(hip, "torch", _PoolTorch(pool))
                got = run(pool)
            pool.assert_clean("conv_pack k%d %s->%d mma %d" % (k, cins, cout, mma))
            pool.assert_inputs_unchanged()
            for a, b in zip(ref, got):
                assert torch.equal(_bytes(a), _bytes(b))


# ------------------------------------------------------------------------------------------------------------ model kernel families
def _family_checks():
    import kernel_checks as kc
    return sorted(n for n in dir(kc) if n.startswith("check_") and callable(getattr(kc, n)))


class _SizingPool:
    """The interface of GuardPool that _PoolTorch and the patches below use, handing out ordinary tensors: a first run of a check
    through it tells how many bytes the real pool needs."""

    def __init__(self, guard=4096):
        self.guard, self.need, self.entries, self.inputs = guard, guard + 512, [], {}

    def take(self, name, shape, dtype=torch.float32, init=None):
        t = init.clone() if init is not None else _poison(tuple(int(d) for d in shape), dtype)
        self.entries.append((name, 0, t.numel() * t.element_size()))
        self.need += t.numel() * t.element_size() + self.guard + 512
        if init is not None:
            self.inputs[name] = None
        return t

    def alloc(self, device, shape, dtype=torch.float32):
        return self.take("alloc", shape, dtype)


def _run_family(monkeypatch, name, pool):
    import kernel_checks as kc
    from lm_net_amd import hip
    proxy = _PoolTorch(pool)
    real_rp, real_bf = hip.nhwc_to_rp4, kc.bf

    def keep(t, what):
        nm = "%s#%d %s" % (what, len(pool.entries), tuple(t.shape))
        p = pool.take(nm, None, None, init=t)
        del pool.inputs[nm]
        return p

    def bf(t):
        return keep(real_bf(t), "bf16")

    with monkeypatch.context() as mp:
        mp.setattr(kc, "torch", proxy)
        mp.setattr(hip, "torch", proxy)
        mp.setattr(kc, "dev", lambda t: keep(t.to(torch.float32).to(kc.DEV).contiguous(), "dev"))
        mp.setattr(kc, "bf", bf)
        mp.setattr(hip, "nhwc_to_rp4", lambda t: hip.rp4(keep(real_rp(t), "rp4")))
        mp.setattr(hip, "_workspace", lambda device, nfloats: pool.take("workspace#%d" % len(pool.entries), (int(nfloats),)))
        hip._ALLOC[0] = pool.alloc
        try:
            with LaunchLog() as log:
                rows = getattr(kc, name)()
        finally:
            hip._ALLOC[0] = None
    torch.cuda.synchronize()
    return rows, log


@pytest.mark.parametrize("name", _family_checks())
def test_model_kernel_families(name, monkeypatch):
    """Every check_* of kernel_checks.py (enumerated from the module; all its shapes, the smallest and the most ragged of each family
    included) with the device tensors it creates carved from one pool: the uploaded inputs (`dev`, `nhwcE`, the bf16 forms made by
    `bf`), the NaN-filled outputs, statistics and gradient buffers (the module's `torch` factories), the wrappers' packed weights
    (exactly lmn_conv_pack_size floats), the K-split scratch (`hip._workspace`: exactly the floats lmn_conv_wgrad_workspace asks for,
    instead of the 16 M float buffer that never tests it as a bound) and the deferred K-split workspaces (`hip._ALLOC[0]`: exactly
    gy * nblk * per floats).  NOT in the pool: tensors a check derives with tensor methods (`.clone()` of an uploaded tensor, slices
    re-made contiguous): those stay ordinary allocations.  The rows keep their fp64 references and tolerances; the canaries must be
    intact.  (No inputs-unchanged assertion here: the checks hand some uploaded tensors to the kernels as in/out operands, running
    statistics for one.)  The check runs twice: once to size the pool, once inside it."""
    sizing = _SizingPool()
    _run_family(monkeypatch, name, sizing)
    pool = GuardPool(DEV, sizing.need)
    rows, log = _run_family(monkeypatch, name, pool)
    pool.assert_clean(name)
    assert log.names and len(pool.entries) == len(sizing.entries), (name, len(log.names), len(pool.entries), len(sizing.entries))
    bad = [(n, e, t) for n, e, t in rows if not e <= t]
    assert not bad, name + "\n" + "\n".join("%s: err %.3e > tol %.1e" % r for r in bad)
    print("    %s: %d pool tensors, %d launches, %d canary bytes of %d" % (name, len(pool.entries), len(log.names), pool.guard_bytes(),
                                                                           pool.nbytes))

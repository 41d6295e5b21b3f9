"""GPU: the whole LM-Net pass inside a guarded arena (tests/guard.py).

Every intermediate of a pass comes from `Engine.alloc`; with `Engine.arena` set to a `GuardedArena` each of them ends flush against
canary bytes and starts out holding poison (NaN) or junk instead of the zeros of fresh device memory.  Each configuration runs three
times from fresh models -- (a) ordinary allocations, (b) poisoned bodies, (c) junk bodies -- in deterministic mode, and

  * the canaries are intact after every forward and after every backward (writes past a tensor's end),
  * logits, loss, every gradient, every parameter after the optimiser step and every BatchNorm buffer are `torch.equal` across
    (a), (b), (c) (a read of memory the pass never wrote, or a read past a tensor's end, would make them differ) and finite.

No tolerance anywhere: every comparison is exact.  Each run prints how many allocations and canary bytes it checked (pytest -s).
Configurations weakened to guard + finiteness only: none."""
import pytest
import torch

from guard import GuardedArena, LaunchLog, pollute_allocator
from helpers import no_dropout
from tools.detweights import det_input, disc_labels, fill_module

pytestmark = pytest.mark.gpu

WIDE = {"W2": [24, 48, 96, 192, 384], "Wodd": [12, 36, 60, 84, 120]}
SERIAL = dict(branch_overlap=False, overlap_wgrad=False)


def _labels(B, H, W, K):
    if K == 2:
        return disc_labels(B, H, W)
    yy, xx = torch.arange(H)[:, None], torch.arange(W)[None, :]
    return torch.stack([((yy // 7 + xx // 5 + b) % K) for b in range(B)]).long().contiguous()


def _model(channel=3, n_classes=2, seed=31, drop=True, dtype=None, cfg=None, det=True, **kw):
    from lm_net_amd import LM_Net
    m = LM_Net(channel, n_classes, **kw)
    fill_module(m, seed)
    if not drop:
        no_dropout(m)
    m = m.cuda()
    m.compute_dtype = dtype
    m.deterministic = det
    for k, v in (cfg or {}).items():
        assert hasattr(m._engine, k), k
        setattr(m._engine, k, v)
    return m


def _count_allocs(m):
    """Count what the passes of `m` ask `Engine.alloc` for: [allocations, floats rounded to granules as Engine.alloc_floats does]."""
    eng, stat = m._engine, [0, 0]
    inner = eng.alloc

    def alloc(device, shape, dtype=torch.float32):
        n = 1
        for d in shape:
            n *= int(d)
        stat[0] += 1
        stat[1] += ((n if dtype == torch.float32 else (n + 1) // 2) + 63) & ~63
        return inner(device, shape, dtype)
    eng.alloc = alloc
    return stat


def _train(make, x, y, steps, body, size=None, n_classes=2, input_grad=False):
    """`steps` training steps of a fresh model; body None: ordinary allocations (returns the arena size the guarded runs need)."""
    from lm_net_amd.loss import SegLoss
    from lm_net_amd.optim import FusedAdamW
    m = make().train()
    stat = _count_allocs(m)
    arena = None
    if body is not None:
        arena = m._engine.arena = GuardedArena(size, x.device, body=body)
    crit = (SegLoss(label_smoothing=1e-3) if n_classes == 2 else SegLoss(None, None, label_smoothing=1e-3)).cuda()
    opt = FusedAdamW(m, lr=1e-3, weight_decay=1e-4)
    out = []
    for s in range(steps):
        if input_grad:
            x = x.detach().clone().requires_grad_(True)
        logits = m(x)
        torch.cuda.synchronize()
        if arena is not None:
            arena.assert_clean("after forward %d" % s)
        loss = crit(logits, y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.cuda.synchronize()
        if arena is not None:
            arena.assert_clean("after backward %d" % s)
        out += [("logits%d" % s, logits.detach().clone()), ("loss%d" % s, loss.detach().clone())]
        out += [("grad%d/%s" % (s, k), p.grad.detach().clone()) for k, p in m.named_parameters()]
        if input_grad:
            out.append(("grad%d/input" % s, x.grad.detach().clone()))
        opt.step()
        torch.cuda.synchronize()
    out += [("param/" + k, p.detach().clone()) for k, p in m.named_parameters()]
    out += [("buffer/" + k, b.detach().clone()) for k, b in m.named_buffers()]
    if arena is not None:
        arena.assert_clean("after the last optimiser step")
        assert arena.count == stat[0] and arena.used == stat[1]
        print("    guarded[%s]: %d allocations, %d canary bytes of %d" % (body, arena.count, arena.guard_bytes(), arena.raw.numel()))
        m._engine.arena = None
        return out
    return out, GuardedArena.floats_for(stat[1], stat[0])


def _infer(make, x, body, size=None):
    m = make()
    stat = _count_allocs(m)
    arena = None
    if body is not None:
        arena = m._engine.arena = GuardedArena(size, x.device, body=body)
    with torch.no_grad():
        y = m(x)
    torch.cuda.synchronize()
    out = [("logits", y.detach().clone())]
    if arena is not None:
        arena.assert_clean("after the eval forward")
        assert arena.count == stat[0] and arena.used == stat[1]
        print("    guarded[%s]: %d allocations, %d canary bytes of %d" % (body, arena.count, arena.guard_bytes(), arena.raw.numel()))
        m._engine.arena = None
        return out
    return out, GuardedArena.floats_for(stat[1], stat[0])


def _same(ref, got, what):
    assert [k for k, _ in ref] == [k for k, _ in got], what
    bad = [k for (k, u), (_, v) in zip(ref, got) if not torch.equal(u, v)]
    assert not bad, (what, len(bad), bad[:8])


def _finite(res, what):
    bad = [k for k, t in res if t.is_floating_point() and not bool(torch.isfinite(t).all())]
    assert not bad, (what, len(bad), bad[:8])


def _three_way(runner, what):
    """runner(body, size) -> results: ordinary, poisoned and junk runs agree bit for bit and are finite."""
    from lm_net_amd import hip
    was = hip.get_deterministic()
    try:
        print("\n  %s" % (what,))
        ref, size = runner(None, None)
        _finite(ref, (what, "ordinary"))
        for body in ("nan", "junk"):
            got = runner(body, size)
            _finite(got, (what, body))
            _same(ref, got, (what, body))
        # ... and what the pass allocates OUTSIDE Engine.alloc (the wrappers' packed weights and scratch, loss and optimiser buffers, the
        # tensors at the autograd boundary): ordinary allocations again, from a caching allocator whose free blocks hold poison / junk
        for body in ("nan", "junk"):
            pollute_allocator(torch.device("cuda"), body)
            got, _ = runner(None, None)
            _finite(got, (what, "allocator " + body))
            _same(ref, got, (what, "allocator " + body))
        return ref
    finally:
        hip.set_deterministic(was)


def _train3(what, shape, steps=2, cfgs=({}, SERIAL), channel=3, n_classes=2, input_grad=False, **kw):
    B, H, W = shape
    x = det_input((B, channel, H, W), "guard/x").cuda()
    y = _labels(B, H, W, n_classes).cuda()
    refs = []
    for cfg in cfgs:
        def make():
            return _model(channel, n_classes, cfg=cfg, **kw)
        refs.append(_three_way(lambda body, size: _train(make, x, y, steps, body, size, n_classes, input_grad), (what, shape, cfg)))
    return refs


# ------------------------------------------------------------------------------------------------------------- 1, 2: default shape
def test_default_training_step_fp32():
    """Configuration 1: LM_Net(3, 2) at (2, 3, 96, 128), fp32, two steps, multi-stream and serial schedules (which must also agree
    with each other).  Prints the wrappers the pass issues (pytest -s)."""
    with LaunchLog() as log:
        multi, serial = _train3("fp32", (2, 96, 128))
    _same(multi, serial, "multi-stream vs serial")
    print("    wrappers reached: %s" % " ".join(sorted(set(log.names))))


@pytest.mark.parametrize("mode", ["bf16", "bf16-mma"])
def test_default_training_step_bf16(mode):
    """Configuration 2: bf16 storage (two elements per arena float, odd element counts end mid-float) and bf16 MFMA operands."""
    _train3(mode, (2, 96, 128), dtype=mode)


def test_unfused_launch_forms():
    """The launch-by-launch forms the engine keeps for A/B runs (own launches for BatchNorm bookkeeping, LayerNorm, bilinear x2,
    squeeze-excite, un-chained convs, the two-pass expand-conv gradient, K-split reductions flushed per layer): same three-way check,
    and with it the entries the fused default never calls run inside the guard."""
    cfg = dict(SERIAL, fuse_bn=False, fuse_se=0, _fuse_se0=0, zpath=False, chain_on=False, zpath_m=False, fuse_ln=False, fuse_up=False,
               fuse_up_wgrad=False, fuse_se_wfin=False, fuse_bn_tail=False, fuse_ln_bwd=False, defer_reduce=False)
    with LaunchLog() as log:
        _train3("unfused", (2, 64, 96), cfgs=(cfg, dict(SERIAL, zpath_m=False)))
    print("    wrappers reached: %s" % " ".join(sorted(set(log.names))))
    for w in ("ln_fwd", "up2_fwd", "bn_finalize", "bn_bwd_coef", "bnact_fwd", "bnact_bwd", "dw_fwd", "dw_bwd", "dw_bwd_coef",
              "dw_finalize_merge", "se_bwd_dm", "se_bwd_params", "affine2"):       # launches the fused default does not make
        assert w in log.names, w


# ------------------------------------------------------------------------------------------------------------- 3: recorded plans
def test_plans_inside_guarded_arena(monkeypatch):
    """Configuration 3: enable_plans() with `LM_Net.Arena` replaced by a GuardedArena factory: two warm-ups, the recorded step, two
    replays; canaries intact after every step (the replays re-issue the recorded launches on the recorded addresses), results equal
    to an unguarded plan run bit for bit (dropout off, as the plan-versus-eager comparison of test_model_gpu.py)."""
    import sys
    from lm_net_amd import hip
    L = sys.modules["lm_net_amd.LM_Net"]          # (the module: the package attribute of that name is the class)
    from lm_net_amd.loss import SegLoss
    from lm_net_amd.optim import FusedAdamW
    x = det_input((2, 3, 96, 128), "guard/x").cuda()
    y = disc_labels(2, 96, 128).cuda()
    arenas = []
    was = hip.get_deterministic()

    def run(body):
        arenas.clear()
        if body is not None:
            # one canary granule per allocation on top of the production size: a training step of this model makes < 16384 of them
            def factory(nfloats, device):
                arenas.append(GuardedArena(int(nfloats) + 64 * 16384, device, body=body))
                return arenas[-1]
            monkeypatch.setattr(L, "Arena", factory)
        else:
            monkeypatch.undo()
        m = _model(drop=False).train()
        m.enable_plans()
        crit = SegLoss(label_smoothing=1e-3).cuda()
        opt = FusedAdamW(m, lr=1e-3, weight_decay=1e-4)
        out = []
        for s in range(5):
            loss = crit(m(x), y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            torch.cuda.synchronize()
            for a in arenas:
                a.assert_clean("after step %d" % s)
            out += [("loss%d" % s, loss.detach().clone())] + [("grad%d/%s" % (s, k), p.grad.detach().clone()) for k, p in m.named_parameters()]
            opt.step()
        torch.cuda.synchronize()
        out += [("param/" + k, p.detach().clone()) for k, p in m.named_parameters()]
        out += [("buffer/" + k, b.detach().clone()) for k, b in m.named_buffers()]
        ps = [p for p in m._plans.values() if p.fwd is not None]
        assert len(ps) == 1 and ps[0].bwd is not None
        if body is not None:
            assert len(arenas) == 1 and ps[0].arena is arenas[0]
            for a in arenas:
                a.assert_clean("at the end")
                print("    plans[%s]: %d allocations, %d canary bytes of %d" % (body, a.count, a.guard_bytes(), a.raw.numel()))
        return out

    try:
        ref = run(None)
        _finite(ref, "plans")
        for body in ("nan", "junk"):
            got = run(body)
            _finite(got, ("plans", body))
            _same(ref, got, ("plans", body))
    finally:
        hip.set_deterministic(was)


# ------------------------------------------------------------------------------------------------------------- 4: inference
@pytest.mark.parametrize("shape", [(1, 32, 32), (2, 64, 96)])
@pytest.mark.parametrize("deploy", [False, True])
def test_eval_and_deploy_forward(shape, deploy):
    """Configuration 4: eval forward under no_grad, as trained and in the structural_reparam (deploy) form."""
    from lm_net_amd import LM_Net
    B, H, W = shape
    x = det_input((B, 3, H, W), "guard/x").cuda()

    def make():
        m = LM_Net(3, 2)
        fill_module(m, 31)
        m.eval()
        if deploy:
            m.structural_reparam()
        m = m.cuda()
        m.deterministic = True
        return m

    for cfg in ({}, SERIAL):
        def make_cfg():
            m = make()
            for k, v in cfg.items():
                setattr(m._engine, k, v)
            return m
        _three_way(lambda body, size: _infer(make_cfg, x, body, size), ("eval", shape, deploy, cfg))


# ------------------------------------------------------------------------------------------------------------- 5, 6: edges, variants
@pytest.mark.parametrize("shape", [(1, 32, 32), (2, 32, 48), (5, 48, 48)])
def test_minimum_and_ragged_training_shapes(shape):
    """Configuration 5: the smallest input of the pyramid, batch 1, an odd batch, tiles that are mostly padding."""
    _train3("edge", shape)


@pytest.mark.parametrize("name", ["W2", "Wodd"])
def test_wide_variants(name):
    """Configuration 6a: wide filters at 64x64 (channel counts that are not multiples of the cout tiles)."""
    _train3(name, (2, 64, 64), filters=WIDE[name])


@pytest.mark.parametrize("cfg", [(1, 9), (3, 14)])
def test_multiclass_variants(cfg):
    """Configuration 6b: one input channel (padded 1 -> 4) with nine classes, and fourteen classes (a head that is not a multiple of 4)."""
    _train3("LM_Net%s" % (cfg,), (2, 64, 64), channel=cfg[0], n_classes=cfg[1])


@pytest.mark.parametrize("mode", [None, "bf16", "bf16-mma"])
@pytest.mark.parametrize("cfg", [(1, 9), (3, 14), (3, 2)])
def test_input_gradient_and_padded_channels(cfg, mode):
    """The input gradient (x.requires_grad: the stem's data gradient, un-padded from NHWC4 to NCHW) in fp32, bf16 and bf16-mma, with
    the 1 -> 4 padded input and heads that are not multiples of 4."""
    _train3("input gradient %s %s" % (cfg, mode), (2, 64, 64), channel=cfg[0], n_classes=cfg[1], input_grad=True, dtype=mode)


@pytest.mark.parametrize("mode", [None, "bf16", "bf16-mma"])
@pytest.mark.parametrize("cfg", [(3, 2), (1, 9)])
def test_default_mode_kernels_stay_finite_and_inside(cfg, mode):
    """The DEFAULT (non-deterministic) mode runs kernels the bit-exact configurations never launch: the squeeze-excite gate formed by
    the last block of the depthwise forward (ticket), float-atomic statistics instead of slots.  Its results differ from run to run in
    the last bits, so there is no three-way equality here -- and no tolerance either: the canaries must be intact and every result
    finite with poisoned bodies (a read of unwritten memory yields NaN) and from a caching allocator whose free blocks hold poison,
    and the canaries intact with junk bodies."""
    from lm_net_amd import hip
    was = hip.get_deterministic()
    x = det_input((2, cfg[0], 64, 64), "guard/x").cuda()
    y = _labels(2, 64, 64, cfg[1]).cuda()
    try:
        for sched in ({}, SERIAL):
            def make():
                return _model(cfg[0], cfg[1], cfg=sched, dtype=mode, det=False)
            ref, size = _train(make, x, y, 2, None, None, cfg[1], True)
            _finite(ref, ("default mode", cfg, mode, sched))
            for body in ("nan", "junk"):
                got = _train(make, x, y, 2, body, size, cfg[1], True)
                if body == "nan":
                    _finite(got, ("default mode", cfg, mode, sched, body))
            pollute_allocator(torch.device("cuda"), "nan")
            got, _ = _train(make, x, y, 2, None, None, cfg[1], True)
            _finite(got, ("default mode", cfg, mode, sched, "allocator nan"))
    finally:
        hip.set_deterministic(was)


@pytest.mark.parametrize("K", [5, 7])
def test_attention_windows(K):
    """Configuration 6c: neighborhood-attention windows 5 and 7 (112x128: the coarsest attention map is 14x16 >= K)."""
    _train3("window %d" % K, (2, 112, 128), na_kernel_size=K)


# ------------------------------------------------------------------------------------------------------------- 7: production shape
def test_production_dispatch_352():
    """Configuration 7: one step at (2, 3, 352, 352) reaches the production dispatch (LDS-DMA convolutions, multi-chunk tiles, the
    byte-exact deferred K-split workspaces with the next tensor one granule on)."""
    _train3("352", (2, 352, 352), steps=1)


def test_launch_trace_finds_no_launch_that_depends_on_the_prefill():
    """The locating mode itself on a real pass: one serial training step at (1, 3, 32, 32) in a poisoned and in a junk arena with
    LaunchLog(trace=True) -- canaries checked after EVERY launch, and no launch's completely written outputs differ between the two."""
    from lm_net_amd import hip
    was = hip.get_deterministic()
    x = det_input((1, 3, 32, 32), "guard/x").cuda()
    y = _labels(1, 32, 32, 2).cuda()
    try:
        def make():
            return _model(cfg=SERIAL)
        _, size = _train(make, x, y, 1, None, None)
        logs = []
        for body in ("nan", "junk"):
            arena = GuardedArena(size, x.device, body=body)
            m = make().train()
            m._engine.arena = arena
            with LaunchLog(arena, trace=True) as log:
                out = m(x)
                (out * out).mean().backward()
                torch.cuda.synchronize()
            m._engine.arena = None
            assert len(log.trace) == len(log.names) > 300
            logs.append(log)
        assert logs[0].names == logs[1].names
        assert LaunchLog.first_divergence(*logs) is None, LaunchLog.first_divergence(*logs)
    finally:
        hip.set_deterministic(was)


# ------------------------------------------------------------------------------------------------------------- the detector itself
def test_detector_reports_a_corrupted_guard_float():
    """Sensitivity: one canary float of a GuardedArena overwritten through `arena.buf` by an ordinary torch op is reported, with the
    allocation it follows and its offset; a clean arena reports nothing."""
    for body in ("nan", "junk"):
        a = GuardedArena(4096, torch.device("cuda"), body=body)
        t0 = a.alloc((3, 5))
        t1 = a.alloc((7,), torch.bfloat16)
        t0.fill_(1.0)
        t1.fill_(2.0)
        assert a.check() == []
        end1 = t1.data_ptr() + 14 - a.buf.data_ptr()          # first byte after t1: the other half of its last float
        k = end1 // 4 + 2                                     # a whole float two floats on
        a.buf[k:k + 1].add_(1.0) if body == "junk" else a.buf[k:k + 1].fill_(0.0)
        got = a.check()
        assert len(got) == 1 and got[0][0].startswith("#1 ") and got[0][1] == "after", got
        assert got[0][2] >= 4 * k - end1 and got[0][3] <= 4 * k + 3 - end1, got
        with pytest.raises(AssertionError):
            a.assert_clean()

"""CPU: the guard-band helper itself (tests/guard.py) -- layout, detector sensitivity, and the coverage manifest that ties every C
entry with a device output pointer to a GPU guard test."""
import os
import re

import pytest
import torch

import guard
from guard import GuardedArena, GuardPool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def _off(pool_buf, t):
    return t.data_ptr() - pool_buf.data_ptr()


# ---------------------------------------------------------------------------------------------------------------------- layout
def test_pool_layout_alignment_flush_end_and_guard_sizes():
    p = GuardPool(CPU, 1 << 16, guard=4096)
    assert p.buf.dtype == torch.uint8 and bool((p.buf == 0xFF).all())
    specs = [("a", (3, 5), torch.float32), ("b", (7,), torch.bfloat16), ("c", (13,), torch.uint8), ("d", (2, 3), torch.int64),
             ("e", (1,), torch.float64), ("f", (0,), torch.float32), ("g", (5,), torch.int32)]
    ts = [(n, p.take(n, s, d)) for n, s, d in specs]
    prev_end = 0
    for (n, s, d), (_, t) in zip(specs, ts):
        nb = t.numel() * t.element_size()
        a = [e[1] for e in p.entries if e[0] == n][0]
        assert nb == 0 or a == _off(p.buf, t)                        # (an empty tensor has no address)
        assert t.dtype == d and tuple(t.shape) == s and t.is_contiguous()
        assert a % 256 == 0, n                                       # aligned start
        assert a - prev_end >= 4096, n                               # a full guard before ...
        assert (n, a, nb) in p.entries                               # ... the size is NOT rounded: the next byte is canary
        assert nb == {"a": 60, "b": 14, "c": 13, "d": 48, "e": 8, "f": 0, "g": 20}[n]
        prev_end = a + nb
    assert p.nbytes - prev_end >= 4096                               # ... and after the last tensor
    assert p.check() == []
    # the poison reads as NaN / -1 / 255
    assert bool(torch.isnan(p.t["a"]).all()) and bool(torch.isnan(p.t["b"].float()).all())
    assert bool((p.t["d"] == -1).all()) and bool((p.t["c"] == 255).all())
    # the byte directly after each tensor belongs to the guard
    p.check()
    for n, a, nb in p.entries:
        assert int(p.mask[a + nb]) == 1 and (nb == 0 or (int(p.mask[a]) == 0 and int(p.mask[a + nb - 1]) == 0)) and int(p.mask[a - 1]) == 1


def test_pool_init_inputs_and_exhaustion():
    p = GuardPool(CPU, 3 * 4096 + 1024, guard=4096)
    src = torch.arange(11, dtype=torch.float32)
    t = p.take("x", None, None, init=src)
    assert torch.equal(t, src) and p.unchanged("x") and p.check() == []
    t[3] = 7.0
    assert not p.unchanged("x")
    with pytest.raises(AssertionError):
        p.assert_inputs_unchanged()
    p.assert_inputs_unchanged(skip=("x",))
    with pytest.raises(RuntimeError, match="exhausted"):
        p.take("big", (4096,), torch.float32)
    with pytest.raises(KeyError):
        p.take("x", (1,), torch.float32)


@pytest.mark.parametrize("body", ["nan", "junk"])
def test_arena_layout_matches_production_arena(body):
    from lm_net_amd.engine import Arena
    shapes = [((3, 5), torch.float32), ((7,), torch.bfloat16), ((64,), torch.float32), ((2, 3, 5, 9), torch.bfloat16),
              ((129,), torch.bfloat16), ((1,), torch.float32), ((128,), torch.bfloat16)]
    g, a = GuardedArena(8192, CPU, body=body), Arena(8192, CPU)
    prev_end = 0
    for shape, dt in shapes:
        off_a = a.off
        tg, ta = g.alloc(shape, dt), a.alloc(shape, dt)
        assert tg.shape == ta.shape and tg.dtype == ta.dtype and tg.is_contiguous()
        n = tg.numel()
        nf = n if dt == torch.float32 else (n + 1) // 2
        assert a.off - off_a == (nf + 63) & ~63                      # the production rounding: (n + 1) // 2 floats for bf16 ...
        start = _off(g.buf, tg)
        assert start % 256 == 0 and start - prev_end >= 256          # ... the same here, plus one whole canary granule
        prev_end = start + 4 * ((nf + 63) & ~63)
        name, a0, nb = g.entries[-1]
        assert a0 == start and nb == n * tg.element_size() and str(tuple(shape)) in name
    assert g.count == len(shapes) and g.used == a.off and g.off == a.off + 64 * (len(shapes) + 1)
    assert g.check() == []
    # tail padding inside the last granule, the granule between allocations and the unallocated rest are all canary
    for _, a0, nb in g.entries:
        assert int(g.mask[a0 + nb]) == 1 and int(g.mask[a0 - 1]) == 1 and int(g.mask[a0]) == 0
    assert int(g.mask[-1]) == 1 and int(g.mask[4 * g.off]) == 1
    assert g.guard_bytes() == g.raw.numel() - sum(e[2] for e in g.entries)
    if body == "nan":
        assert all(bool(torch.isnan(g.alloc(s, d).float()).all()) for s, d in shapes[:2])
    else:
        for s, d in ((( 1000,), torch.float32), ((1001,), torch.bfloat16)):
            v = g.alloc(s, d).double()
            assert bool(torch.isfinite(v).all()) and float(v.abs().min()) >= 1024 and float(v.abs().max()) < 2049
            assert bool((v > 0).any()) and bool((v < 0).any())
            if d == torch.float32:
                assert bool((v[:-1] * v[1:] < 0).all())                # signs alternate
    assert GuardedArena.floats_for(a.off, len(shapes)) >= a.off + 64 * (len(shapes) + 1)


def test_arena_exhaustion():
    g = GuardedArena(256, CPU)
    g.alloc((64,))
    with pytest.raises(RuntimeError, match="arena exhausted"):
        g.alloc((65,))


@pytest.mark.parametrize("fill", ["junk", "poison"])
def test_pools_carve_every_tensor_at_its_exact_size(fill):
    """guard.pools / guard.sizes, which the guard tests of the feature headers share: a pool of size_for the tensors, inputs copied in
    and registered, outputs at their exact sizes, and the fill each file names."""
    inputs = dict(x=torch.arange(7, dtype=torch.float32), y=torch.arange(5, dtype=torch.int64))
    outputs = dict(u=((3, 5), torch.uint8), f=((9,), torch.float32), e=((0,), torch.uint8))
    plain, pool, guarded = guard.pools(inputs, outputs, CPU, fill=fill)
    assert isinstance(pool, GuardPool) and pool.nbytes == -(-GuardPool.size_for([28, 40, 15, 36, 0]) // 256) * 256
    assert list(plain) == list(guarded) == ["x", "y", "u", "f", "e"] and all(guarded[k] is pool.t[k] for k in guarded)
    assert guard.sizes(pool, plain) == dict(x=28, y=40, u=15, f=36, e=0)
    assert set(pool.inputs) == {"x", "y"} and all(torch.equal(plain[k], inputs[k]) and torch.equal(guarded[k], inputs[k]) for k in inputs)
    pool.assert_clean()
    pool.assert_inputs_unchanged()
    for d in (plain, guarded):
        assert bool((d["u"] == (guard.JUNK if fill == "junk" else guard.POISON)).all())
    if fill == "junk":
        assert all(bool((d["f"].view(torch.uint8) == guard.JUNK).all()) for d in (plain, guarded))
    else:
        assert bool((guarded["f"].view(torch.uint8) == guard.POISON).all())      # untouched: the pool's own poison
    with pytest.raises(AssertionError):
        guard.sizes(pool, dict(plain, f=plain["f"][:8]))
    with pytest.raises(ValueError, match="fill"):
        guard.pools(inputs, outputs, CPU, fill=0xA5)
    with pytest.raises(TypeError):
        guard.pools(inputs, outputs, CPU)                                         # no default: a file names its fill


# ------------------------------------------------------------------------------------------------------------------ sensitivity
def test_pool_detector_names_tensor_side_and_offset():
    p = GuardPool(CPU, 1 << 16)
    a = p.take("a", (5,), torch.float32)
    b = p.take("b", (9,), torch.uint8)
    c = p.take("c", (4,), torch.float32)
    assert p.check() == []
    ob = _off(p.buf, b)
    p.buf[ob + 9] = 0                                                # the byte directly after b
    assert p.check() == [("b", "after", 0, 0)]
    p.buf[ob + 9] = 0xFF
    p.buf[ob + 9 + 17] = 1
    p.buf[ob + 9 + 40] = 2
    assert p.check() == [("b", "after", 17, 40)]
    p.buf[ob + 9 + 17] = p.buf[ob + 9 + 40] = 0xFF
    p.buf[_off(p.buf, c) - 1] = 3                                    # the byte directly before c
    assert p.check() == [("c", "before", -17, -17)]
    p.buf[_off(p.buf, c) - 1] = 0xFF
    p.buf[_off(p.buf, a) - 2] = 3
    p.buf[-1] = 0
    got = p.check()
    last = p.nbytes - 1 - (_off(p.buf, c) + 16)
    assert sorted(got) == [("a", "before", -22, -22), ("c", "after", last, last)]
    with pytest.raises(AssertionError, match="guard bytes damaged"):
        p.assert_clean()
    # writes INSIDE the tensors are not reports
    p.buf[_off(p.buf, a) - 2] = 0xFF
    p.buf[-1] = 0xFF
    a.fill_(1.0); b.fill_(0); c.fill_(2.0)
    p.assert_clean()


@pytest.mark.parametrize("body", ["nan", "junk"])
def test_arena_detector_names_allocation(body):
    g = GuardedArena(4096, CPU, body=body)
    t0, t1 = g.alloc((3, 5)), g.alloc((7,), torch.bfloat16)
    t0.fill_(1.0); t1.fill_(2.0)
    assert g.check() == []
    end1 = _off(g.buf, t1) + 14
    g.raw[end1] ^= 0x55                                              # the second half of t1's last float: tail padding is canary
    assert g.check() == [(g.entries[1][0], "after", 0, 0)]
    g.raw[end1] ^= 0x55
    g.buf[3000] = 0.5                                                # the unallocated rest
    got = g.check()
    assert len(got) == 1 and got[0][:2] == (g.entries[1][0], "after") and 4 * 3000 - end1 <= got[0][2] <= got[0][3] <= 4 * 3000 + 3 - end1
    with pytest.raises(AssertionError, match="#1 "):
        g.assert_clean()


def test_launch_trace_names_the_launch_that_read_unwritten_memory():
    """LaunchLog(trace=True) + first_divergence: the same three 'launches' in a poisoned and in a junk arena; the second one reads a
    tensor nobody wrote.  (The launches are torch ops here; `hip._check(0, name)` is what every wrapper calls after its launch.)"""
    from guard import LaunchLog
    from lm_net_amd import hip
    logs = []
    for body in ("nan", "junk"):
        g = GuardedArena(4096, CPU, body=body)
        with LaunchLog(g, trace=True) as log:
            t0, t1, t2, t3 = g.alloc((40,)), g.alloc((40,)), g.alloc((9,)), g.alloc((40,))
            t0.copy_(torch.arange(40.0)); hip._check(0, "produce")
            t1.copy_(t0 * 2); hip._check(0, "double")
            t3.copy_(t1 + torch.nan_to_num(t2[3], nan=5.0)); hip._check(0, "reads_unwritten")      # (the clamp that swallows a NaN)
            t2.fill_(1.0); hip._check(0, "late_writer")
        assert log.names == ["produce", "double", "reads_unwritten", "late_writer"]
        logs.append(log)
    n, what, differ, stale = LaunchLog.first_divergence(*logs)
    assert (n, what) == (3, "reads_unwritten") and differ == [logs[0].guarded.entries[3][0]]
    assert logs[0].guarded.entries[2][0] in stale and logs[0].guarded.entries[0][0] not in stale
    assert LaunchLog.first_divergence(logs[0], logs[0]) is None
    assert hip._check.__module__ == "lm_net_amd.hip"                  # the hook is removed on exit


# ------------------------------------------------------------------------------------------------------------ coverage manifest
EXEMPT_OK = re.compile(r"^lmn_(abi_version|last_error|sizeof_\w+|\w+_workspace|\w+_pack_size|\w+_ok|\w+_job|conv_dma_config|"
                       r"stream_\w+|event_\w+|set_priority_stream|set_deterministic|get_deterministic|plan_\w+|prof_\w+)$")


def test_manifest_partitions_the_c_abi():
    from lm_net_amd import hip
    cov, ex = set(guard.COVERED), set(guard.EXEMPT)
    assert not (cov & ex), sorted(cov & ex)
    assert len(set(hip.EXPORTS)) == len(hip.EXPORTS) == sum(len(v) for v in hip.HEADERS.values()) == 139
    assert cov | ex == set(hip.EXPORTS), (sorted(set(hip.EXPORTS) - cov - ex), sorted((cov | ex) - set(hip.EXPORTS)))
    bad = sorted(k for k in ex if not EXEMPT_OK.match(k))
    assert not bad, "entries with a device output pointer need a guard test: %s" % bad
    assert all(isinstance(v, str) and v for v in guard.EXEMPT.values())
    # the pattern must not swallow an entry that writes device memory
    for k in ("lmn_conv_fwd", "lmn_conv_pack", "lmn_conv_pack_batch", "lmn_conv_wgrad", "lmn_wgrad_reduce_batch", "lmn_fill", "lmn_surface_dist",
              "lmn_post_clean", "lmn_cc_label", "lmn_adamw_step", "lmn_dw_fwd_bn", "lmn_reparam_fold", "lmn_augment_oneof_u8",
              "lmn_segloss_ex_fwd", "lmn_segloss_ex_bwd", "lmn_image_stats", "lmn_sigloss_fwd", "lmn_sigloss_bwd", "lmn_sigmoid_stats",
              "lmn_optim_prepare", "lmn_adamw_step_ex", "lmn_tile_gather", "lmn_tile_blend", "lmn_curve_hist", "lmn_volume_labels", "lmn_volume_dist",
              "lmn_cc3d_label", "lmn_volpost_clean", "lmn_lesion_match", "lmn_dist_map", "lmn_dist_loss_fwd", "lmn_dist_loss_bwd", "lmn_lovasz_order",
              "lmn_lovasz_fwd", "lmn_lovasz_bwd", "lmn_region_fwd", "lmn_region_bwd", "lmn_slices_stats", "lmn_slices_gather", "lmn_soft_fwd",
              "lmn_soft_bwd", "lmn_mix_batch", "lmn_hard_fwd", "lmn_hard_bwd"):
        assert not EXEMPT_OK.match(k) and k in cov, k


def _code(src):
    """Python source without its docstrings: a mention there is no call and no assertion.  (Comments stay: the tests that reach an
    entry through a class of the package and assert it with `in log.names` name their `hip.` wrapper in a comment beside that.)"""
    return re.sub(r"""(?s)\"{3}.*?\"{3}|'{3}.*?'{3}""", '""', src)


def test_manifest_matches_the_gpu_test_sources():
    """Every COVERED entry names a test function that exists in its file and whose body calls (or, for the model file, lists as
    reached and asserts at run time) the entry's `hip.` wrapper -- or, where it reaches the entry through a class of the package,
    compares a LaunchLog's `names` with a list that holds the wrapper's name; the wrapper's source really issues that C entry.
    In a file of guard.STRICT the function must do both, and hold the file's words: it runs the entry on a guard pool and checks it.
    A docstring counts for nothing."""
    from lm_net_amd import hip
    src = {f: _code(open(os.path.join(ROOT, f)).read()) for f in sorted({v[0] for v in guard.COVERED.values()} | {guard.MODEL})}
    hip_src = open(os.path.join(ROOT, "lm_net_amd", "hip.py")).read()
    kc_src = _code(open(os.path.join(ROOT, "tests", "kernel_checks.py")).read())
    assert "dir(kc)" in src[guard.KERN] and 'startswith("check_")' in src[guard.KERN]      # the families are enumerated, not listed
    for entry, (f, test, wrapper) in sorted(guard.COVERED.items()):
        assert f in src, (entry, f)
        fn = re.search(r"^def %s\(.*?(?=^def |^class |^@|\Z)" % re.escape(test), src[f], re.M | re.S)
        assert fn, (entry, test)
        if test == "test_model_kernel_families":                     # runs every check_* of kernel_checks.py: the call is there
            assert re.search(r"\bhip\.%s\(" % re.escape(wrapper), kc_src), (entry, wrapper)
        else:
            called = re.search(r"\bhip\.%s\b" % re.escape(wrapper), fn.group(0))       # (inside the named test function)
            logged = any('"%s"' % wrapper in m for m in re.findall(r"\.names == \[([^\]]*)\]", fn.group(0)))
            assert called or logged, (entry, wrapper)
            if f in guard.STRICT:
                assert re.search(r"\bhip\.%s\(" % re.escape(wrapper), fn.group(0)) and logged, (entry, wrapper, bool(called), logged)
                missing = [w for w in guard.STRICT[f] if w not in fn.group(0)]
                assert not missing, (entry, test, missing)
        assert callable(getattr(hip, wrapper)), (entry, wrapper)
        body = re.search(r"^def %s\(.*?(?=^def |^class |\Z)" % re.escape(wrapper), hip_src, re.M | re.S)
        if body is None:                                             # a class (PackPlan.refresh issues lmn_conv_pack_batch)
            body = re.search(r"^class %s\b.*?(?=^class |^def |\Z)" % re.escape(wrapper), hip_src, re.M | re.S)
        assert body is not None and re.search(r"\b%s\b" % entry, body.group(0)), (entry, wrapper)
    assert set(guard.STRICT) <= set(src) and all("assert_clean" in words for words in guard.STRICT.values())
    # the stripping itself: a docstring that names a wrapper satisfies neither rule
    fake = _code('"""calls hip.fake_wrapper( and asserts log.names == ["fake_wrapper"]"""\nx = 1\n' + "'''hip.fake_wrapper('''\n")
    assert "fake_wrapper" not in fake and "x = 1" in fake

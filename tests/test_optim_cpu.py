"""CPU: the host side of the extended FusedAdamW route (include/optim/lmnet_optim.h): registry and header agree, the struct mirror and the
workspace arithmetic, the per-quad group map, decay_groups, the partition checks, the state-dict exchange with torch.optim.AdamW over
three groups, the argument checks of the two entries (rejected before any HIP call), and the float64 restatement tests/optim_ref.py
against torch.optim.AdamW + clip_grad_norm_ (no GPU needed)."""
import ctypes
import os
import re

import pytest
import torch

import optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- ABI
def test_registry_header_and_struct_agree():
    """The feature's own part of the registry: the literal list, its place in hip.HEADERS, the one struct with its size and field
    offsets, the #defines (one of them derived) and the workspace arithmetic.  (Header / export / layout / return-type checks:
    tests/test_host_cpu.py.)"""
    from lm_net_amd import hip
    lib = hip.load()
    assert hip.SYMBOLS_OPTIM == ["lmn_sizeof_optim_param", "lmn_optim_workspace", "lmn_optim_prepare", "lmn_adamw_step_ex"]
    assert hip.HEADERS["optim/lmnet_optim.h"] is hip.SYMBOLS_OPTIM and (hip.OptimParam, "lmn_sizeof_optim_param") in hip.STRUCTS
    header = open(os.path.join(ROOT, "include", "optim", "lmnet_optim.h")).read()
    assert re.findall(r"^\}\s*(lmn_\w+_t)\s*;", header, re.M) == ["lmn_optim_param_t"]
    defs = {k: int(v) for k, v in re.findall(r"^#define (LMN_OPTIM_\w+) (\d+)\b", header, re.M)}
    assert lib.lmn_sizeof_optim_param() == ctypes.sizeof(hip.OptimParam) == defs["LMN_OPTIM_PARAM_BYTES"] == hip.OPTIM_PARAM_BYTES == 64
    for name in ("MAX_GROUPS", "GRID_CAP", "SKIP_NONFINITE", "NORM", "CTRL_WORDS", "SKIP", "STEP", "SKIPPED", "GRAD_NORM", "INV_SCALE",
                 "COEF", "INV_BC1", "INV_SQRT_BC2", "NONFINITE"):
        assert defs["LMN_OPTIM_" + name] == getattr(hip, "OPTIM_" + name), name
    # field offsets of the mirror: two doubles, three floats, two ints, padding
    offs = {f[0]: getattr(hip.OptimParam, f[0]).offset for f in hip.OptimParam._fields_}
    assert offs == dict(beta1=0, beta2=8, eps=16, max_norm=20, ema_decay=24, flags=28, n_groups=32, _pad=36)
    # workspace: 2 blocks' words + control block + group table, blocks capped at 1024
    cap = hip.OPTIM_GRID_CAP
    for n, blocks in ((4, 1), (1024, 1), (1028, 2), (4 * 256 * 3 + 4, 4), (cap * 1024, cap), (cap * 1024 + 4, cap), (3966716, cap)):
        assert hip.optim_blocks(n) == blocks, n
        assert int(lib.lmn_optim_workspace(ctypes.c_int64(n))) == hip.optim_workspace_words(n) == 2 * blocks + 16 + 64, n
    assert int(lib.lmn_optim_workspace(ctypes.c_int64(0))) == hip.optim_workspace_words(0) == 0


def test_optim_param_flags():
    from lm_net_amd import hip
    p = hip.optim_param()
    assert (p.flags, p.max_norm, p.n_groups) == (0, 0.0, 1) and p.ema_decay < 0
    assert hip.optim_param(max_norm=2.0).flags == hip.OPTIM_NORM
    assert hip.optim_param(flags=hip.OPTIM_SKIP_NONFINITE).flags == hip.OPTIM_NORM | hip.OPTIM_SKIP_NONFINITE
    assert hip.optim_param(ema_decay=0.5, n_groups=3).ema_decay == 0.5


def _entry(which, null=None, n=64, scalars=True, **kw):
    """lmn_optim_prepare / lmn_adamw_step_ex with fake device pointers: every case here must be rejected before any HIP call."""
    from lm_net_amd import hip
    lib = hip.load()
    fake = ctypes.c_void_p(0x1000)
    p = hip.optim_param(**{k: v for k, v in kw.items() if k in ("betas", "eps", "max_norm", "ema_decay", "flags", "n_groups")})
    for k in ("raw_flags", "raw_groups"):
        if k in kw:
            setattr(p, dict(raw_flags="flags", raw_groups="n_groups")[k], kw[k])
    if which == "prepare":
        a = dict(g=fake, qgroup=fake, param=ctypes.byref(p), ws=fake)
        if null:
            a[null] = None
        rc = lib.lmn_optim_prepare(a["g"], ctypes.c_int64(n), a["qgroup"], a["param"], a["ws"], fake if scalars else None,
                                   fake if scalars else None, None)
    else:
        a = dict(p=fake, g=fake, m=fake, v=fake, ema=kw.get("ema", fake), qgroup=fake, param=ctypes.byref(p), ws=fake)
        if null:
            a[null] = None
        rc = lib.lmn_adamw_step_ex(a["p"], a["g"], a["m"], a["v"], a["ema"], ctypes.c_int64(n), a["qgroup"], a["param"], a["ws"], None)
    return rc, lib.lmn_last_error().decode()


@pytest.mark.parametrize("which", ["prepare", "step"])
def test_entries_reject_bad_arguments(which):
    from lm_net_amd import hip
    what = "optim_prepare" if which == "prepare" else "adamw_step_ex"
    for name in (("g", "qgroup", "param", "ws") if which == "prepare" else ("p", "g", "m", "v", "qgroup", "param", "ws")):
        rc, err = _entry(which, null=name)
        assert rc == -1 and err == what + ": null pointer", (name, err)
    for n in (0, -4, 6, 1023):
        rc, err = _entry(which, n=n)
        assert rc == -1 and "multiple of 4" in err and err.startswith(what), (n, err)
    for ng in (0, 17, -1):
        rc, err = _entry(which, raw_groups=ng)
        assert rc == -1 and "n_groups=%d not in [1, 16]" % ng in err, (ng, err)
    for betas in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.5), (0.9, 1.5)):
        rc, err = _entry(which, betas=betas)
        assert rc == -1 and "outside [0, 1)" in err, (betas, err)
    for eps in (0.0, -1e-8):
        rc, err = _entry(which, eps=eps)
        assert rc == -1 and "eps" in err and "not positive" in err, (eps, err)
    rc, err = _entry(which, ema_decay=1.5)
    assert rc == -1 and "ema_decay" in err and "above 1" in err
    for kw in (dict(max_norm=1.0), dict(flags=hip.OPTIM_SKIP_NONFINITE)):        # (optim_param switches NORM on: take it off again)
        rc, err = _entry(which, raw_flags=kw.get("flags", 0), **kw)
        assert rc == -1 and "need LMN_OPTIM_NORM" in err, (kw, err)
    if which == "step":
        rc, err = _entry(which, ema_decay=0.9, ema=None)
        assert rc == -1 and "without an EMA buffer" in err


def test_python_wrappers_check_sizes_before_the_library():
    from lm_net_amd import hip
    g, q, ws = torch.zeros(64), torch.zeros(16, dtype=torch.uint8), torch.zeros(hip.optim_workspace_words(64))
    with pytest.raises(ValueError, match="group bytes"):
        hip.optim_prepare(g, q[:15], hip.optim_param(), ws)
    with pytest.raises(ValueError, match="workspace of"):
        hip.optim_prepare(g, q, hip.optim_param(), ws[:-1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.optim_prepare(g, q, hip.optim_param(), ws)
    with pytest.raises(ValueError, match="differ in size"):
        hip.adamw_step_ex(g[:60], g, g, g, None, q, hip.optim_param(), ws)


# ---------------------------------------------------------------- the group map
def test_quad_groups_on_a_toy_layout():
    """Parameters of 5, 4, 1, 9 and 8 floats at 16-byte aligned offsets (the layout rule of LM_Net._ensure_grad_layout): the one-quad
    parameters sit between two groups, and the padding quads (floats 5..7 and 25..27) belong to their parameter's group."""
    from lm_net_amd.optim import quad_groups
    spans = [(0, 5), (8, 12), (12, 13), (16, 25), (28, 36)]
    q = quad_groups(spans, [0, 1, 2, 1, 0], 36)
    assert q.dtype == torch.uint8 and q.tolist() == [0, 0, 1, 2, 1, 1, 1, 0, 0]
    e = R.elem_groups(q)
    assert e.numel() == 36 and e[5:8].tolist() == [0, 0, 0] and e[12:16].tolist() == [2] * 4 and e[25:28].tolist() == [1] * 3
    for bad, msg in (((([(0, 5), (6, 12)]), [0, 1], 12), "16-byte aligned"), (([(0, 5), (4, 12)], [0, 1], 12), "shares a quad"),
                     (([(0, 4)], [0], 8), "belong to no parameter"), (([(0, 4)], [16], 4), "outside"), (([(0, 4)], [0], 6), "multiple of 4"),
                     (([(0, 9)], [0], 8), "16-byte aligned")):
        with pytest.raises(ValueError, match=msg):
            quad_groups(*bad)


def test_quad_groups_of_the_model_layout():
    from lm_net_amd import LM_Net
    from lm_net_amd.optim import decay_groups, quad_groups
    net = LM_Net(3, 2, filters=[12] * 5)
    L = net._ensure_grad_layout()
    groups = decay_groups(net, 1e-2)
    gid = {id(p): k for k, g in enumerate(groups) for p in g["params"]}
    q = quad_groups([L["offs"][id(p)] for p in L["order"]], [gid[id(p)] for p in L["order"]], L["total"])
    assert q.numel() * 4 == L["total"] and set(q.tolist()) == {0, 1}
    for p in L["order"]:
        a, b = L["offs"][id(p)]
        assert a % 4 == 0 and set(q[a // 4:(b + 3) // 4].tolist()) == {gid[id(p)]}


def test_decay_groups():
    from lm_net_amd import LM_Net
    from lm_net_amd.optim import decay_groups
    net = LM_Net(3, 2, filters=[12] * 5)
    groups = decay_groups(net, 0.05)
    assert groups.model is net and len(groups) == 2
    assert groups[0]["weight_decay"] == 0.05 and groups[1]["weight_decay"] == 0.0 and "lr" not in groups[0]
    names = {id(p): n for n, p in net.named_parameters()}
    assert all(p.dim() >= 2 and not names[id(p)].endswith("bias") for p in groups[0]["params"])
    assert all(p.dim() <= 1 or names[id(p)].endswith("bias") for p in groups[1]["params"])
    assert any(names[id(p)].endswith("bias") for p in groups[1]["params"]) and any(names[id(p)].endswith("weight") and p.dim() == 1
                                                                                   for p in groups[1]["params"])
    assert sorted(id(p) for g in groups for p in g["params"]) == sorted(id(p) for p in net.parameters())
    # frozen parameters get a group of their own; lr is handed on
    frozen = list(net.conv1.parameters())
    for p in frozen:
        p.requires_grad_(False)
    groups = decay_groups(net, 0.05, lr=3e-4)
    assert len(groups) == 3 and groups[2]["frozen"] is True and {id(p) for p in groups[2]["params"]} == {id(p) for p in frozen}
    assert all(g["lr"] == 3e-4 for g in groups)
    # a longer no_decay list moves parameters over
    more = decay_groups(net, 0.05, no_decay=("bias", "output_layer.weight"))
    assert len(more[0]["params"]) == len(groups[0]["params"]) - 1


def test_partition_errors():
    from lm_net_amd import LM_Net
    from lm_net_amd.optim import FusedAdamW, decay_groups
    net = LM_Net(3, 2, filters=[12] * 5)
    ps = list(net.parameters())
    with pytest.raises(TypeError, match="model=net"):
        FusedAdamW([dict(params=ps)])                                         # a plain list does not know its model
    with pytest.raises(ValueError, match="in no group"):
        FusedAdamW([dict(params=ps[1:])], model=net)
    with pytest.raises(ValueError, match="appears in groups 0 and 1"):
        FusedAdamW([dict(params=ps), dict(params=ps[:1])], model=net)
    with pytest.raises(ValueError, match="do not belong to the model"):
        FusedAdamW([dict(params=ps + [torch.nn.Parameter(torch.zeros(3))])], model=net)
    with pytest.raises(ValueError, match="1..16"):
        FusedAdamW([dict(params=[p]) for p in ps[:16]] + [dict(params=ps[16:])], model=net)
    with pytest.raises(TypeError, match="dict"):
        FusedAdamW([ps], model=net)
    with pytest.raises(ValueError, match="shared by all groups"):
        FusedAdamW([dict(params=ps, betas=(0.8, 0.9))], model=net)
    with pytest.raises(ValueError, match="max_norm"):
        FusedAdamW(net, max_norm=0.0)
    with pytest.raises(ValueError, match="ema_decay"):
        FusedAdamW(net, ema_decay=1.5)
    with pytest.raises(RuntimeError, match="GPU first"):                      # a valid partition gets as far as the device check
        FusedAdamW(decay_groups(net, 1e-2), lr=1e-3)
    ps[3].requires_grad_(False)
    with pytest.raises(ValueError, match="only in a frozen group"):
        FusedAdamW(net)
    with pytest.raises(ValueError, match="only in a frozen group"):
        FusedAdamW([dict(params=ps)], model=net)
    with pytest.raises(ValueError, match="only in a frozen group"):
        FusedAdamW([dict(params=ps[:3] + ps[4:]), dict(params=[ps[3]], frozen=False)], model=net)
    with pytest.raises(RuntimeError, match="GPU first"):
        FusedAdamW([dict(params=ps[:3] + ps[4:]), dict(params=[ps[3]], frozen=True)], model=net)


# ---------------------------------------------------------------- state exchange
def _toy():
    """five parameters in three groups (the third frozen) and their flat layout"""
    g = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g, dtype=torch.float64)) for s in ((3, 2), (5,), (1,), (2, 2, 2), (7,))]
    ps[4].requires_grad_(False)
    groups = [dict(params=[ps[0], ps[3]], lr=1e-2, weight_decay=0.1), dict(params=[ps[1], ps[2]], lr=1e-3, weight_decay=0.0),
              dict(params=[ps[4]], lr=1e-2, weight_decay=0.1)]
    offs, pos = {}, 0
    for p in (ps[3], ps[0], ps[4], ps[1], ps[2]):                              # (a layout order that is not the groups' order)
        offs[id(p)] = (pos, pos + p.numel())
        pos += (p.numel() + 3) // 4 * 4
    return ps, groups, offs, pos


def test_state_dict_round_trip_three_groups_against_torch_adamw():
    from lm_net_amd.optim import pack_state, unpack_state
    ps, groups, offs, total = _toy()
    oa = torch.optim.AdamW(groups, betas=(0.9, 0.99))
    g = torch.Generator().manual_seed(6)
    for _ in range(2):
        for p in ps[:4]:
            p.grad = torch.randn(p.shape, generator=g, dtype=torch.float64)
        oa.step()
    sd = oa.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2, 3]                                 # torch keeps no state for the frozen parameter
    # torch -> flat
    mine = [dict(params=list(gr["params"]), frozen=(k == 2)) for k, gr in enumerate(groups)]
    m, v = torch.zeros(total, dtype=torch.float64), torch.zeros(total, dtype=torch.float64)
    assert unpack_state(sd, mine, offs, m, v) == 2
    assert [gr["lr"] for gr in mine] == [1e-2, 1e-3, 1e-2] and [gr["weight_decay"] for gr in mine] == [0.1, 0.0, 0.1]
    assert mine[0]["betas"] == (0.9, 0.99) and [gr["frozen"] for gr in mine] == [False, False, True]
    for i, p in enumerate([ps[0], ps[3], ps[1], ps[2]]):
        a, b = offs[id(p)]
        assert torch.equal(m[a:b].view(p.shape), sd["state"][i]["exp_avg"]) and torch.equal(v[a:b].view(p.shape), sd["state"][i]["exp_avg_sq"])
    a, b = offs[id(ps[4])]
    assert float(m[a:(b + 3) // 4 * 4].abs().max()) == 0.0 and float(m[total - 3:].abs().max()) == 0.0      # frozen parameter, padding
    # flat -> torch layout: indices count through the groups, every parameter has the three entries, hyper-parameters travel
    out = pack_state(mine, offs, m, v, 2)
    assert [gr["params"] for gr in out["param_groups"]] == [[0, 1], [2, 3], [4]] == [gr["params"] for gr in sd["param_groups"]]
    assert sorted(out["state"]) == [0, 1, 2, 3, 4] and all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in out["state"].values())
    assert all(float(s["step"]) == 2.0 for s in out["state"].values())
    for i in range(4):
        assert torch.equal(out["state"][i]["exp_avg"], sd["state"][i]["exp_avg"]), i
        assert torch.equal(out["state"][i]["exp_avg_sq"], sd["state"][i]["exp_avg_sq"]), i
    # a fresh torch optimizer accepts it and continues exactly like the one that never stopped
    ps2, groups2, _, _ = _toy()
    with torch.no_grad():
        for p2, p in zip(ps2, ps):
            p2.copy_(p)
    ob = torch.optim.AdamW(groups2, betas=(0.5, 0.5))
    ob.load_state_dict(out)
    for p, p2 in zip(ps[:4], ps2[:4]):
        p.grad = torch.randn(p.shape, generator=g, dtype=torch.float64)
        p2.grad = p.grad.clone()
    oa.step(); ob.step()
    for p, p2 in zip(ps, ps2):
        assert torch.equal(p, p2)
    # mismatches are refused
    with pytest.raises(ValueError, match="parameter groups"):
        unpack_state(sd, mine[:2], offs, m, v)
    sd["state"][1]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError, match="step counts differ"):
        unpack_state(sd, mine, offs, m, v)


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("max_norm", [None, "half", "double"])
def test_restatement_equals_torch_adamw_and_clip_grad_norm(max_norm):
    """tests/optim_ref.py in float64 against torch.optim.AdamW groups + torch.nn.utils.clip_grad_norm_ on random data: three steps,
    three groups with their own lr / weight decay, a frozen parameter, a scaled gradient, and an EMA restated by hand."""
    ps, groups, offs, total = _toy()
    oa = torch.optim.AdamW(groups, betas=(0.9, 0.99), eps=1e-8)
    live = [p for p in ps if p.requires_grad]
    gid = torch.zeros(total, dtype=torch.int64)
    flat = torch.zeros(total, dtype=torch.float64)
    for k, gr in enumerate(groups):
        for p in gr["params"]:
            a, b = offs[id(p)]
            gid[a:(b + 3) // 4 * 4] = k
            flat[a:b] = p.detach().reshape(-1)
    table = [(1e-2, 0.1, False), (1e-3, 0.0, False), (1e-2, 0.1, True)]
    st = R.State(flat, ema=flat)
    ema = [p.detach().clone() for p in ps]
    gen = torch.Generator().manual_seed(7)
    scale = 1024.0
    for it in range(3):
        g = torch.zeros(total, dtype=torch.float64)
        for p in ps:                                                           # (the frozen parameter has a gradient in the flat buffer too)
            a, b = offs[id(p)]
            g[a:b] = torch.randn(p.numel(), generator=gen, dtype=torch.float64)
        for p in live:
            a, b = offs[id(p)]
            p.grad = g[a:b].view(p.shape).clone()
        norm = float(torch.sqrt(sum((p.grad ** 2).sum() for p in live)))
        mn = None if max_norm is None else norm * (0.5 if max_norm == "half" else 2.0)
        if mn is not None:
            total_norm = torch.nn.utils.clip_grad_norm_(live, mn)
            assert abs(float(total_norm) - norm) < 1e-12 * norm
        oa.step()
        for e, p in zip(ema[:4], ps[:4]):
            e.mul_(0.9).add_(0.1 * p.detach())
        info = R.step(st, g * scale, gid, table, betas=(0.9, 0.99), eps=1e-8, max_norm=mn, ema_decay=0.9, grad_scale=scale,
                      skip_nonfinite=True)
        assert info["skip"] is False and abs(info["grad_norm"] - norm) < 1e-12 * norm
        assert (info["coef"] < 1.0) == (max_norm == "half")
        for p, e in zip(ps, ema):
            a, b = offs[id(p)]
            assert float((st.p[a:b].view(p.shape) - p.detach()).abs().max()) < 1e-13, it
            assert float((st.ema[a:b].view(p.shape) - e).abs().max()) < 1e-13, it
    assert st.step == 3 and st.skipped == 0
    a, b = offs[id(ps[4])]
    assert torch.equal(st.p[a:b], flat[a:b]) and float(st.m[a:b].abs().max()) == 0.0     # frozen: untouched
    # a non-finite value skips the whole step and leaves everything as it was; in the frozen group it is not counted
    before = (st.p.clone(), st.m.clone(), st.v.clone(), st.ema.clone())
    bad = g.clone()
    bad[offs[id(ps[1])][0]] = float("inf")
    info = R.step(st, bad, gid, table, ema_decay=0.9, skip_nonfinite=True)
    assert info["skip"] and info["nonfinite"] == 1 and (st.step, st.skipped) == (3, 1)
    assert all(torch.equal(x, y) for x, y in zip(before, (st.p, st.m, st.v, st.ema)))
    info = R.step(st, g, gid, table, ema_decay=0.9, skip_nonfinite=True, found_inf=True)
    assert info["skip"] and info["nonfinite"] == 0 and (st.step, st.skipped) == (3, 2)
    bad = g.clone()
    bad[offs[id(ps[4])][0]] = float("nan")
    info = R.step(st, bad, gid, table, ema_decay=0.9, skip_nonfinite=True)
    assert not info["skip"] and info["nonfinite"] == 0 and st.step == 4

"""GPU: lm_net_amd.optim.FusedAdamW on LM_Net(3, 2) at 2 x 3 x 64 x 64: parameter groups with clipping against torch.optim.AdamW groups
+ clip_grad_norm_, the torch.amp.GradScaler protocol, graph capture of step(), the EMA and the unchanged one-launch route.  As in
test_fused_adamw_matches_torch_adamw_and_exchanges_state the optimizer under comparison is fed the SAME gradient values (Adam's
m / sqrt(v) turns the last-bit noise of two separate backward passes into O(lr) differences)."""
import pytest
import torch

import optim_ref as R
from guard import LaunchLog
from helpers import no_dropout, rel_err
from tools.detweights import det_input, fill_module

pytestmark = pytest.mark.gpu
ENCODER = ("conv1", "conv2", "conv3", "conv4", "down1", "down2", "down3", "down4")


def _net(seed=3):
    from lm_net_amd import LM_Net
    m = LM_Net(3, 2)
    fill_module(m, seed)
    no_dropout(m)
    return m.cuda().train()


def _data():
    return det_input((2, 3, 64, 64), "optim/x").cuda(), det_input((2, 2, 64, 64), "optim/G").cuda()


def _groups(net, lr, wd):
    """decoder at lr, encoder at lr / 10, a no-decay group (1-D tensors and biases), conv1 frozen (requires_grad=False)"""
    frozen = list(net.conv1.parameters())
    for p in frozen:
        p.requires_grad_(False)
    fz = {id(p) for p in frozen}
    dec, enc, plain = [], [], []
    for name, p in net.named_parameters():
        if id(p) in fz:
            continue
        if p.dim() <= 1 or name.endswith("bias"):
            plain.append(p)
        elif name.split(".")[0] in ENCODER:
            enc.append(p)
        else:
            dec.append(p)
    return [dict(params=dec, lr=lr, weight_decay=wd), dict(params=enc, lr=lr / 10, weight_decay=wd),
            dict(params=plain, lr=lr, weight_decay=0.0), dict(params=frozen, frozen=True)]


def _static_grads(opt, flat):
    """make `flat` the model's gradient buffer: every p.grad a view of it (what LM_Net's backward leaves behind)"""
    L = opt._layout
    for p in L["order"]:
        a, b = L["offs"][id(p)]
        p.grad = flat[a:b].view(p.shape) if p.requires_grad else None
    opt.net._grad_flat = flat


def _seeded_flat(opt, seed, scale=1e-2):
    """a seeded flat gradient with zero padding, as the model's backward writes it"""
    L = opt._layout
    g = torch.zeros(L["total"])
    vals = R.seeded(L["total"], seed, scale)
    for p in L["order"]:
        a, b = L["offs"][id(p)]
        g[a:b] = vals[a:b]
    return g.cuda()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def test_groups_and_clipping_match_torch_adamw_groups_and_clip_grad_norm():
    from lm_net_amd.optim import FusedAdamW
    a, b = _net(), _net()
    x, G = _data()
    lr, wd = 1e-3, 1e-2
    (b(x) * G).sum().backward()                                    # a first gradient, to place max_norm well below the norms to come
    norm0 = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in b.parameters())))
    max_norm = 0.1 * norm0
    ga, gb = _groups(a, lr, wd), _groups(b, lr, wd)
    frozen0 = [p.detach().clone() for p in gb[3]["params"]]
    oa = torch.optim.AdamW([g for g in ga if not g.get("frozen")], lr=lr, weight_decay=wd)
    ob = FusedAdamW(gb, lr=lr, weight_decay=wd, max_norm=max_norm, model=b)
    assert ob.extended and [g["lr"] for g in ob.param_groups] == [lr, lr / 10, lr, lr] and ob.param_groups[3]["frozen"] is True
    live_a = [p for p in a.parameters() if p.requires_grad]
    for it in range(3):
        ob.zero_grad(set_to_none=True)
        (b(x) * G).sum().backward()
        for pa, pb in zip(a.parameters(), b.parameters()):
            pa.grad = pb.grad.detach().clone() if pb.requires_grad else None
        with LaunchLog() as log:
            ob.step()
        assert log.names == ["optim_prepare", "adamw_step_ex"]
        total = float(torch.nn.utils.clip_grad_norm_(live_a, max_norm))
        assert total > max_norm and bool((ob.clip_coef < 1.0).item())          # clipping is active, on the device too
        assert abs(float(ob.grad_norm) - total) < 1e-5 * total
        oa.step()
    assert int(ob.device_step) == 3 and int(ob.skipped) == 0 and ob.step_count == 3
    for (n1, p1), (_, p2) in zip(a.named_parameters(), b.named_parameters()):
        assert rel_err(p2, p1) < 2e-6, n1
    for p, p0 in zip(gb[3]["params"], frozen0):                    # the frozen block: bit-identical
        assert torch.equal(_bits(p), _bits(p0))
    # the state goes to a torch optimizer with the same four groups and back
    sd = ob.state_dict()
    assert [len(g["params"]) for g in sd["param_groups"]] == [len(g["params"]) for g in gb] and float(sd["state"][0]["step"]) == 3.0
    oc = torch.optim.AdamW(ga, lr=lr, weight_decay=wd)
    oc.load_state_dict(sd)
    ob.load_state_dict(oc.state_dict())
    assert ob.step_count == 3 and [g["lr"] for g in ob.param_groups] == [lr, lr / 10, lr, lr]


def test_grad_scaler_protocol():
    """The reference's three --apm lines on a plain FusedAdamW(model): a normal step equals the step on the unscaled gradient (the
    scale is a power of two: bit for bit), a step with an inf is skipped on the device and halves the scale, the next one is good."""
    from lm_net_amd.optim import FusedAdamW
    b, c = _net(), _net()
    x, G = _data()
    ob, oc = FusedAdamW(b, lr=1e-3, weight_decay=1e-2), FusedAdamW(c, lr=1e-3, weight_decay=1e-2)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    assert ob._step_supports_amp_scaling and not ob.extended

    def scaled_step(poison=False):
        ob.zero_grad(set_to_none=True)
        scaler.scale((b(x) * G).sum()).backward()
        s = scaler.get_scale()
        for pc, pb in zip(c.parameters(), b.parameters()):
            pc.grad = pb.grad.detach() / s                         # (exact: a power of two)
        if poison:
            next(iter(b.parameters())).grad.view(-1)[0] = float("inf")
        scaler.step(ob)
        scaler.update()
        return s

    assert scaled_step() == 1024.0
    oc.step()
    assert ob.extended and int(ob.device_step) == 1 and ob.step_count == 1 and not hasattr(ob, "grad_scale")
    assert abs(float(ob.grad_norm) - float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in c.parameters())))) < 1e-5 * float(ob.grad_norm)
    for k in ("flat_p", "exp_avg", "exp_avg_sq"):
        assert torch.equal(_bits(getattr(ob, k)), _bits(getattr(oc, k))), k
    before = [getattr(ob, k).clone() for k in ("flat_p", "exp_avg", "exp_avg_sq")]
    scaled_step(poison=True)
    assert scaler.get_scale() == 512.0 and int(ob.device_step) == 1 and int(ob.skipped) == 1
    for k, t in zip(("flat_p", "exp_avg", "exp_avg_sq"), before):
        assert torch.equal(_bits(getattr(ob, k)), _bits(t)), k
    assert scaled_step() == 512.0
    oc.step()
    assert int(ob.device_step) == 2 and int(ob.skipped) == 1 and scaler.get_scale() == 512.0
    for k in ("flat_p", "exp_avg", "exp_avg_sq"):
        assert torch.equal(_bits(getattr(ob, k)), _bits(getattr(oc, k))), k


def test_step_inside_a_captured_graph():
    """opt.step() captured once (a linear chain: the reduction, its one-block finish, the step kernel), replayed three times on a
    static gradient buffer, against three eager steps of a twin; a changed lr inside a capture is refused."""
    from lm_net_amd.optim import FusedAdamW
    b, c = _net(), _net()
    ob = FusedAdamW(_groups(b, 1e-3, 1e-2), max_norm=0.05, ema_decay=0.9, model=b)
    oc = FusedAdamW(_groups(c, 1e-3, 1e-2), max_norm=0.05, ema_decay=0.9, model=c)
    gb, gc = _seeded_flat(ob, 20), _seeded_flat(oc, 20)
    _static_grads(ob, gb)
    _static_grads(oc, gc)
    ob.step(); oc.step()                                           # one eager step each (also loads the kernels before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with LaunchLog() as log:
            ob.step()
    assert log.names == ["optim_prepare", "adamw_step_ex"] and int(ob.device_step) == 1     # (captured, not run)
    for k in (21, 22, 23):
        gb.copy_(_seeded_flat(ob, k))
        graph.replay()
        gc.copy_(_seeded_flat(oc, k))
        oc.step()
    torch.cuda.synchronize()
    assert int(ob.device_step) == int(oc.device_step) == 4 and bool((ob.clip_coef < 1.0).item())
    for k in ("flat_p", "exp_avg", "exp_avg_sq", "ema", "_ws"):
        assert torch.equal(_bits(getattr(ob, k)), _bits(getattr(oc, k))), k
    # a scheduler moved lr: inside a capture the table cannot be refreshed
    ob.param_groups[0]["lr"] = 5e-4
    g2 = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match=r"sync_groups\(\)"):
        with torch.cuda.graph(g2):
            ob.step()
    assert ob.sync_groups() is True and ob.sync_groups() is False
    g3 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g3):
        ob.step()
    g3.replay()
    oc.param_groups[0]["lr"] = 5e-4
    oc.step()                                                      # eager: step() refreshes the table by itself
    torch.cuda.synchronize()
    assert int(ob.device_step) == 5 and torch.equal(_bits(ob.flat_p), _bits(oc.flat_p))


def test_ema_and_swap():
    from lm_net_amd import LM_Net
    from lm_net_amd.optim import FusedAdamW
    b = _net()
    x, _ = _data()
    opt = FusedAdamW(b, lr=1e-2, weight_decay=1e-2, ema_decay=0.9)
    assert opt.extended and torch.equal(_bits(opt.ema), _bits(opt.flat_p)) and opt.ema.data_ptr() != opt.flat_p.data_ptr()
    gid = R.elem_groups(opt._qgroup)
    st = R.State(opt.flat_p, ema=opt.ema)
    for k in (31, 32, 33):
        g = _seeded_flat(opt, k)
        _static_grads(opt, g)
        opt.step()
        R.step(st, g, gid, [(1e-2, 1e-2, False)], ema_decay=0.9)
    assert rel_err(opt.ema, st.ema) < 2e-6 and rel_err(opt.flat_p, st.p) < 2e-6
    assert float((opt.ema - opt.flat_p).abs().max()) > 1e-3        # the average lags behind
    # evaluation under the swap: the logits of a model that holds the EMA values; the swap restores the parameters bit for bit
    b.eval()
    twin = LM_Net(3, 2)
    no_dropout(twin)
    twin = twin.cuda().eval()
    twin.load_state_dict(b.state_dict())
    L = opt._layout
    with torch.no_grad():
        for pt, p in zip(twin.parameters(), b.parameters()):
            a, e = L["offs"][id(p)]
            pt.copy_(opt.ema[a:e].view(p.shape))
        p_before, ema_before = opt.flat_p.clone(), opt.ema.clone()
        plain = b(x)
        with opt.swap_ema():
            assert torch.equal(_bits(opt.flat_p), _bits(ema_before)) and torch.equal(_bits(opt.ema), _bits(p_before))
            averaged = b(x)
        want = twin(x)
    assert torch.equal(_bits(opt.flat_p), _bits(p_before)) and torch.equal(_bits(opt.ema), _bits(ema_before))
    # Two eval passes over the same weights differ in the order of the model's float atomics (non-deterministic mode), so the logits
    # are compared at 1e-5 relative: a tenth of the suite's bar for logits of equal weights (1e-4), far above fp32 reordering noise.
    # The EMA weights are not the parameters: their logits differ by much more than that.
    e_same, e_other = rel_err(averaged, want), rel_err(plain, want)
    assert e_same < 1e-5 < 1e-4 < e_other, "logits under swap_ema vs EMA-loaded twin %.3e, plain parameters vs twin %.3e" % (e_same, e_other)
    with pytest.raises(RuntimeError, match="ema_decay"):
        with FusedAdamW(_net(), lr=1e-3).swap_ema():
            pass


def test_unchanged_route_and_its_bit_equality_with_the_extended_one():
    """FusedAdamW(model) launches lmn_adamw_step alone, count on the host; one group without options on the extended route (forced
    here) gives the same bits after one step: the step kernel keeps adamw_kernel's arithmetic and order, g * 1 * 1 is exact."""
    from lm_net_amd.optim import FusedAdamW
    b, c = _net(), _net()
    ob, oc = FusedAdamW(b, lr=1e-3, weight_decay=1e-2), FusedAdamW(c, lr=1e-3, weight_decay=1e-2)
    assert not ob.extended and not oc.extended
    oc.extended = True                                             # one group, no option: the extended kernels on the same problem
    oc.sync_groups()
    gb, gc = _seeded_flat(ob, 40), _seeded_flat(oc, 40)
    _static_grads(ob, gb)
    _static_grads(oc, gc)
    start = ob.flat_p.clone()
    with LaunchLog() as log:
        ob.step()
    assert log.names == ["adamw_step"] and ob.step_count == 1 and int(ob.device_step) == 0
    with LaunchLog() as log:
        oc.step()
    assert log.names == ["optim_prepare", "adamw_step_ex"] and oc.step_count == 1
    assert not torch.equal(_bits(ob.flat_p), _bits(start))
    for k in ("flat_p", "exp_avg", "exp_avg_sq"):
        assert torch.equal(_bits(getattr(ob, k)), _bits(getattr(oc, k))), k
    # two more steps: the bias corrections formed on the device from its own count are those formed on the host
    for seed in (41, 42):
        gb.copy_(_seeded_flat(ob, seed))
        gc.copy_(_seeded_flat(oc, seed))
        ob.step(); oc.step()
    assert ob.step_count == oc.step_count == 3
    for k in ("flat_p", "exp_avg", "exp_avg_sq"):
        assert torch.equal(_bits(getattr(ob, k)), _bits(getattr(oc, k))), k

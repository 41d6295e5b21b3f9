"""Helpers of tests/test_model_life_gpu.py: a model that has lived through a history of passes against a TWIN --
a freshly constructed model loaded with the same state, which always runs launch by launch.  In deterministic mode the same pass
on both must give the same bits, whatever the first one (or the process) has done before."""
from collections import OrderedDict

import torch

from helpers import no_dropout, rel_err
from tools.detweights import det_input, disc_labels, fill_module

# the smallest shapes that differ in everything that keys or sizes state: batch, height and width change upwards and downwards
A = (2, 3, 32, 48)
B = (1, 3, 48, 32)
C = (3, 3, 64, 32)
D = (2, 3, 32, 32)      # the minimum map
NAME = {A: "A", B: "B", C: "C", D: "D"}


def xin(shape, tag="x"):
    return det_input(shape, "life/%s/%s" % (NAME[shape], tag)).cuda()


def gout(shape, n_classes=2):
    return det_input((shape[0], n_classes) + shape[2:], "life/%s/G" % NAME[shape]).cuda()


def labels(shape):
    return disc_labels(shape[0], shape[2], shape[3]).cuda()


def model(seed, train=True, deterministic=True, dropout=False):
    from lm_net_amd import LM_Net
    m = LM_Net(3, 2)
    fill_module(m, seed)
    if not dropout:
        no_dropout(m)
    m = m.cuda().train(train)
    m.deterministic = deterministic
    return m


def twin(m, opt=None, deterministic=True):
    """A new LM_Net with m's constructor arguments, values (new storage), train / eval flag and precision; dropout off, no plans, no
    graphs.  With `opt`: (twin, a new FusedAdamW on it loaded from opt.state_dict())."""
    from lm_net_amd import LM_Net
    from lm_net_amd.optim import FusedAdamW
    t = LM_Net(m.channel, m.n_classes, filters=list(m.filters), deep_supervision=m.deep_supervision,
               na_kernel_size=m.natt4.att1.kernel_size)
    t.load_state_dict(m.state_dict())
    no_dropout(t)
    t = t.cuda().train(m.training)
    t.compute_dtype = m.compute_dtype
    t.deterministic = deterministic
    if opt is None:
        return t
    g = opt.param_groups[0]
    topt = FusedAdamW(t, lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"])
    topt.load_state_dict(opt.state_dict())
    return t, topt


def collect(m, out, grads=True, opt=None, loss=None, x=None):
    torch.cuda.synchronize()
    r = OrderedDict(logits=out.detach().clone())
    if loss is not None:
        r["loss"] = loss.detach().clone()
    if grads:
        if x is not None and x.grad is not None:
            r["grad/input"] = x.grad.detach().clone()
        for k, p in m.named_parameters():
            r["grad/" + k] = p.grad.detach().clone()
    for k, b in m.named_buffers():
        r["buffer/" + k] = b.detach().clone()
    if opt is not None:
        for k, p in m.named_parameters():
            r["param/" + k] = p.detach().clone()
    return r


def one_pass(m, x, G=None, crit=None, y=None, opt=None):
    """One pass of m in the mode it is in.  No G and no crit: a forward under no_grad (gradients: none).  Otherwise forward +
    backward of sum(logits * G) or crit(logits, y), then opt.step() if given.  Returns an ordered dict name -> tensor: logits,
    (loss), grad/<parameter>, buffer/<buffer> after the pass, and param/<parameter> after the step."""
    if G is None and crit is None:
        with torch.no_grad():
            out = m(x)
        return collect(m, out, grads=False)
    if opt is not None:
        opt.zero_grad(set_to_none=True)
    for p in m.parameters():
        p.grad = None
    if x.requires_grad:
        x.grad = None
    out = m(x)
    loss = crit(out, y) if crit is not None else (out * G).sum()
    loss.backward()
    if opt is not None:
        opt.step()
    return collect(m, out, opt=opt, loss=loss if crit is not None else None, x=x if x.requires_grad else None)


def same(a, b, where):
    """torch.equal on every tensor of two results; names the first one that differs and the step of the history."""
    assert list(a) == list(b), (where, sorted(set(a) ^ set(b))[:6])
    for k in a:
        u, v = a[k], b[k]
        if not torch.equal(u, v):
            bad = [n for n in a if not torch.equal(a[n], b[n])]
            d = float((u.double() - v.double()).abs().max())
            raise AssertionError("%s: %s differs from the twin (max |d| %.3e, rel %.3e); %d of %d tensors differ: %s"
                                 % (where, k, d, rel_err(u, v), len(bad), len(a), bad[:8]))


def agree(pairs, gmax):
    """The rule of test_plan_mode_matches_host_launches for two default-mode runs of one schedule (float-atomic arrival order, the
    Hardswish kink): every parameter within 2e-2 (or 1e-5 of the largest gradient: the exactly-zero pre-BatchNorm biases), the
    concatenated gradient within 3e-3."""
    pairs = list(pairs)
    for k, u, v in pairs:
        assert rel_err(u, v) < 2e-2 or float((u - v).abs().max()) < 1e-5 * gmax, (k, rel_err(u, v))
    fu, fv = (torch.cat([t[i].reshape(-1) for t in pairs]) for i in (1, 2))
    assert rel_err(fu, fv) < 3e-3, rel_err(fu, fv)


def agree_grads(ra, rb):
    ks = [k for k in ra if k.startswith("grad/")]
    gmax = max(float(rb[k].abs().max()) for k in ks)
    agree(((k, ra[k], rb[k]) for k in ks), gmax)


def checkpoint(m, where, x, G=None, opt=None, crit=None, y=None):
    """Twin m, run the same pass on both, require the same bits.  Returns (result of m, result of the twin)."""
    if opt is not None:
        t, topt = twin(m, opt)
    else:
        t, topt = twin(m), None
    rm = one_pass(m, x, G, crit=crit, y=y, opt=opt)
    rt = one_pass(t, x, G, crit=crit, y=y, opt=topt)
    same(rm, rt, where)
    return rm, rt


def plan_of(m, shape, training=True, taped=True):
    """The recorded plan of (shape, mode, tape) -- told by what it recorded, not by the fields of its key."""
    for ps in m._plans.values():
        if ps.x is None or tuple(ps.x.shape) != tuple(shape) or (ps.cx is not None) != taped:
            continue
        if not taped or getattr(ps.cx, "training", None) == training:
            return ps
    return None


def move_storage(m):
    """Every parameter into new storage (what model.to(), a checkpoint load through .data, or building a flattening optimizer
    does), then one weight changed in place: a pass that still reads the old storage computes with the old value."""
    for p in m.parameters():
        p.data = p.data.clone()
    with torch.no_grad():
        m.down1[0].weight.mul_(1.25)
        m.output_layer.weight.mul_(0.5)


def move_into_vacated_storage(m):
    """natt4.att1.qkv.weight [3C, C] moves away and natt4.att1.proj.weight [C, C] moves to the address it left (what flattening the
    parameters in another order does): two 1x1 operators over the same C input channels, so the packed-weight job recorded for that
    address describes another matrix."""
    q, p = m.natt4.att1.qkv.weight, m.natt4.att1.proj.weight
    old = q.data
    assert old.numel() > p.numel() and q.shape[1] == p.shape[1]
    q.data = old.clone()
    with torch.no_grad():
        old.view(-1)[:p.numel()].copy_(p.data.reshape(-1))
    p.data = old.view(-1)[:p.numel()].view(p.shape)
    assert p.data_ptr() == old.data_ptr() and q.data_ptr() != old.data_ptr()

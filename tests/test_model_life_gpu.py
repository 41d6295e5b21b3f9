"""GPU: history independence.  Whatever a model -- or the process -- has done before, a pass on it equals, bit for bit,
the same pass on a fresh model loaded with the same state.  Every other test gives a model one shape, one mode and one precision for
its whole life; here a model walks through shapes, modes, precisions, recorded plans, pending tapes, a second model, passes that
raised and moved parameter storage, and is compared at checkpoints with a twin (tests/life.py) that runs launch by launch.  All in
deterministic mode (same state, same input -> same bits) except test 8 (graph capture is refused there), which uses the default-mode
rule of test_plan_mode_matches_host_launches."""
import pytest
import torch

import life
from helpers import rel_err
from life import A, B, C, D, NAME, checkpoint, gout, model, one_pass, plan_of, same, twin, xin

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(autouse=True)
def _deterministic_off_afterwards():
    from lm_net_amd import hip
    try:
        yield
    finally:
        hip.set_deterministic(False)


# ------------------------------------------------------------------ 0. the premise
def test_control_two_twins_agree():
    """Two twins of one model give equal passes at A and at C (implied by test_deterministic_mode_is_bit_reproducible; restated so
    that a failure of the tests below can be read)."""
    m = model(41)
    for shp in (A, C):
        t1, t2 = twin(m), twin(m)
        same(one_pass(t1, xin(shp), gout(shp)), one_pass(t2, xin(shp), gout(shp)), "control, train %s" % NAME[shp])
        t1.eval(); t2.eval()
        same(one_pass(t1, xin(shp)), one_pass(t2, xin(shp)), "control, eval %s" % NAME[shp])


# ------------------------------------------------------------------ 1. shape walk, launch by launch  (+ 9. the oracle anchor)
WALK = (A, C, A, D, B, C, A)


@pytest.fixture(scope="module")
def walked():
    """The training walk of test 1, run once: [(where, result of the worn model, result of its twin)] at the checkpoints before
    the 3rd, 5th and 7th pass, and the state the 7th pass started from (test 9).  The 7th pass asks for the input gradient too."""
    from lm_net_amd import hip
    try:
        m = model(43)
        cps, state, x7 = [], None, None
        for i, shp in enumerate(WALK):
            x, G = xin(shp), gout(shp)
            if i == len(WALK) - 1:
                state = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
                x = x.requires_grad_(True)
                x7 = x
            if i in (2, 4, 6):
                t = twin(m)
                rm = one_pass(m, x, G)
                cps.append(("walk (train) pass %d at %s" % (i + 1, NAME[shp]), rm, one_pass(t, x, G)))
            else:
                one_pass(m, x, G)
        return cps, state, x7.detach().cpu()
    finally:
        hip.set_deterministic(False)


def test_shape_walk_train(walked):
    """ZeroPool.need larger and smaller than the pass needs, the weight-gradient workspaces, the deterministic scratch and the
    flat gradient buffer after passes of other sizes."""
    assert len(walked[0]) == 3
    for where, rm, rt in walked[0]:
        assert "grad/output_layer.weight" in rm
        same(rm, rt, where)
    assert "grad/input" in walked[0][-1][1]


def test_shape_walk_eval():
    m = model(43, train=False)
    for i, shp in enumerate(WALK):
        if i in (2, 4, 6):
            checkpoint(m, "walk (eval) pass %d at %s" % (i + 1, NAME[shp]), xin(shp))
        else:
            one_pass(m, xin(shp))


def test_worn_model_vs_oracle(walked):
    """Anchor (rules out "equal and both wrong"): the last checkpoint of the walk -- a training pass at A on a model that has been
    through six passes of four shapes -- against oracle.lmnet_ref on the CPU in fp64: logits, input gradient, every parameter
    gradient, at the tolerances of test_minimum_and_ragged_sizes_vs_oracle."""
    from helpers import no_dropout
    from oracle.lmnet_ref import LM_Net as Oracle
    cps, state, x = walked
    rm = cps[-1][1]
    ora = Oracle(3, 2).double()
    ora.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in state.items()})
    no_dropout(ora)
    ora.train()
    xo = x.double().requires_grad_(True)
    yo = ora(xo)
    (yo * gout(A).cpu().double()).sum().backward()
    assert rel_err(rm["logits"], yo) < TOL
    assert rel_err(rm["grad/input"], xo.grad) < 2e-3
    gmax = max(float(p.grad.abs().max()) for p in ora.parameters())
    for k, po in ora.named_parameters():
        err = float((rm["grad/" + k].cpu().double() - po.grad).abs().max())
        assert err < 4e-3 * float(po.grad.abs().max()) or err < 5e-5 * gmax, (k, err)


# ------------------------------------------------------------------ 2. mode and precision walk at one shape
def test_mode_and_precision_walk():
    """PackPlan holds fp32 and bf16 jobs side by side, eval-mode BatchNorm folds sit next to train packs, and the squeeze-excite
    fusion switch of set_deterministic is toggled; checkpoint after each return to fp32 deterministic training."""
    m = model(47)
    x, G = xin(A), gout(A)
    one_pass(m, x, G)                                   # train
    m.eval()
    one_pass(m, x)                                      # eval, no_grad
    one_pass(m, x, G)                                   # eval with a tape
    m.train()
    checkpoint(m, "mode walk: train after eval / eval tape", x, G)
    for cd in ("bf16", "bf16-mma"):
        m.compute_dtype = cd
        r = one_pass(m, x, G)
        assert torch.isfinite(r["logits"]).all()
    m.compute_dtype = "fp32"
    checkpoint(m, "mode walk: fp32 after bf16 / bf16-mma", x, G)
    m.deterministic = False
    for _ in range(2):
        one_pass(m, x, G)                               # (default mode: not compared)
    m.deterministic = True
    checkpoint(m, "mode walk: deterministic after two default-mode passes", x, G)


# ------------------------------------------------------------------ 3. recorded plans over interleaved shapes and modes
@pytest.mark.parametrize("variant", ["plans", "direct_grads", "adamw"])
def test_plans_interleaved(variant):
    """Each (shape, mode) is recorded between passes of another shape (A's recording follows a pass of B: the engine-wide ZeroPool
    has seen the other shape when A's arena is filled); the last replay of each key equals an eager twin; with FusedAdamW between
    the passes the replays follow the weights and the optimizer reads the static buffer of the shape that just ran."""
    from lm_net_amd.optim import FusedAdamW
    m = model(53)
    opt = FusedAdamW(m, lr=1e-3, weight_decay=1e-4) if variant == "adamw" else None
    m.enable_plans(direct_grads=variant == "direct_grads")
    X, G = {s: xin(s) for s in (A, B)}, {s: gout(s) for s in (A, B)}
    for shp in (A, A, B, A, B, B, A):
        one_pass(m, X[shp], G[shp], opt=opt)
    m.eval()
    for _ in range(3):
        one_pass(m, X[A])
    m.train()
    ta, tb, ev = plan_of(m, A), plan_of(m, B), plan_of(m, A, False, False)
    assert len([p for p in m._plans.values() if p.fwd is not None]) == 3
    assert ta.fwd is not None and ta.bwd is not None and tb.fwd is not None and tb.bwd is not None and ev is not None and ev.fwd is not None
    for shp, ps in ((A, ta), (B, tb)):
        checkpoint(m, "%s: last replay of train %s" % (variant, NAME[shp]), X[shp], G[shp], opt=opt)
        assert plan_of(m, shp) is ps and not ps.pending
        if opt is not None:
            assert opt._flat_grad().data_ptr() == ps.flat.data_ptr(), NAME[shp]
    m.eval()
    checkpoint(m, "%s: replay of eval A" % variant, X[A])
    # (a tape in eval mode: same shape, precision and tape flag as the recorded training plan of A -- only the mode tells them apart)
    checkpoint(m, "%s: eval A with a tape beside the recorded training plan of A" % variant, X[A], G[A])
    m.train()
    m.enable_plans(False)
    assert m._plans == {}
    m.enable_plans(direct_grads=variant == "direct_grads")
    checkpoint(m, "%s: after enable_plans(False) / enable_plans()" % variant, X[A], G[A], opt=opt)


# ------------------------------------------------------------------ 4. pending tapes
def _grads(m):
    torch.cuda.synchronize()
    g = {"grad/" + k: p.grad.detach().clone() for k, p in m.named_parameters()}
    for p in m.parameters():
        p.grad = None
    return g


def _part(r, prefix):
    return {k: v for k, v in r.items() if k.startswith(prefix)}


def _buffers(m):
    torch.cuda.synchronize()
    return {"buffer/" + k: b.detach().clone() for k, b in m.named_buffers()}


@pytest.mark.parametrize("plans", [False, True])
def test_pending_tapes(plans):
    """Forwards whose backwards come later, in another order, or after an eval forward of another shape: each gradient equals the
    one a twin produces for that single pass, the BatchNorm buffers those of a twin that ran the same forwards in the same order."""
    m = model(59)
    if plans:
        m.enable_plans()
    for shp in (A, A, A, B, B, B):
        one_pass(m, xin(shp), gout(shp))
    if plans:
        assert plan_of(m, A).bwd is not None and plan_of(m, B).bwd is not None
    for p in m.parameters():
        p.grad = None
    tag = "plans" if plans else "eager"
    # forward A, forward B, backward B, backward A
    t = twin(m)
    ra, rb = one_pass(t, xin(A), gout(A)), one_pass(t, xin(B), gout(B))
    ya, yb = m(xin(A)), m(xin(B))
    (yb * gout(B)).sum().backward()
    gb = _grads(m)
    (ya * gout(A)).sum().backward()
    ga = _grads(m)
    assert torch.equal(ya, ra["logits"]) and torch.equal(yb, rb["logits"]), tag
    same(gb, _part(rb, "grad/"), "%s: fwd A, fwd B, BACKWARD B, backward A" % tag)
    same(ga, _part(ra, "grad/"), "%s: fwd A, fwd B, backward B, BACKWARD A" % tag)
    same(_buffers(m), _part(rb, "buffer/"), "%s: buffers after fwd A, fwd B" % tag)
    # two forwards of A (two inputs), then both backwards -- in either order
    for order in ((0, 1), (1, 0)):
        t = twin(m)
        xs = [xin(A), xin(A, "x2")]
        rs = [one_pass(t, x, gout(A)) for x in xs]
        ys = [m(x) for x in xs]
        for i in order:
            (ys[i] * gout(A)).sum().backward()
            same(dict(_grads(m), logits=ys[i].detach()), dict(_part(rs[i], "grad/"), logits=rs[i]["logits"]),
                 "%s: two forwards of A, backward %d of order %s" % (tag, i, order))
        same(_buffers(m), _part(rs[1], "buffer/"), "%s: buffers after two forwards of A" % tag)
    # an eval forward of another shape between a training forward and its backward
    t = twin(m)
    ra = one_pass(t, xin(A), gout(A))
    t.eval()
    rc = one_pass(t, xin(C))
    ya = m(xin(A))
    m.eval()
    with torch.no_grad():
        yc = m(xin(C))
    m.train()
    (ya * gout(A)).sum().backward()
    assert torch.equal(yc, rc["logits"]), "%s: eval C inside a pending pass of A" % tag
    same(dict(_grads(m), logits=ya.detach()), dict(_part(ra, "grad/"), logits=ra["logits"]), "%s: backward A after an eval forward of C" % tag)
    same(_buffers(m), _part(rc, "buffer/"), "%s: buffers after train A, eval C" % tag)


# ------------------------------------------------------------------ 5. two models in one process
def test_two_models_alternate_and_share_event_slots():
    """A training student and an eval-mode teacher alternate at A and C over every module-level and library-level cache; then a
    model whose engine has the student's numbered events (slot_base repeats every 16 engines) trains beside it."""
    from lm_net_amd import LM_Net
    from helpers import no_dropout
    from tools.detweights import fill_module
    S, T = model(61), model(67, train=False)
    for shp in (A, C, A, C):
        one_pass(T, xin(shp))
        one_pass(S, xin(shp), gout(shp))
    checkpoint(T, "teacher (eval) at C beside a training student", xin(C))
    checkpoint(S, "student (train) at C beside an eval teacher", xin(C), gout(C))
    checkpoint(T, "teacher (eval) at A", xin(A))
    checkpoint(S, "student (train) at A", xin(A), gout(A))
    from lm_net_amd.engine import Engine
    for _ in range(16):                      # (host construction only, no storage: each engine takes the next four event slots)
        if 4 * (Engine._instances % 16) == S._engine.slot_base:
            break
        with torch.device("meta"):
            LM_Net(3, 2)
    n = LM_Net(3, 2)
    assert n._engine.slot_base == S._engine.slot_base and n._engine is not S._engine
    fill_module(n, 71)
    no_dropout(n)
    n = n.cuda().train()
    n.deterministic = True
    for shp in (A, C):
        one_pass(S, xin(shp), gout(shp))
        one_pass(n, xin(shp), gout(shp))
    checkpoint(S, "student beside a model with the same event slots", xin(A), gout(A))
    checkpoint(n, "the model with the student's event slots", xin(A), gout(A))


# ------------------------------------------------------------------ 6. a pass that raised
class _Boom(Exception):
    pass


@pytest.mark.parametrize("recording", [False, True])
@pytest.mark.parametrize("where", ["forward", "backward"])
def test_a_pass_that_raised(monkeypatch, where, recording):
    """A Python exception on the host in the middle of a forward (hip.avgpool_fwd) or of a backward (engine.probe), launch by launch
    and while a plan is being recorded: the next full pass of that model and of a second model equals its twin, and the failed
    recording leaves the shape running launch by launch (_drop_plan).  No kernel gets bad arguments."""
    from lm_net_amd import hip
    m, other = model(73), model(79)
    x, G = xin(A), gout(A)
    if recording:
        m.enable_plans()
    for _ in range(2):
        one_pass(m, x, G)
    one_pass(other, xin(C), gout(C))
    for p in m.parameters():
        p.grad = None
    fired = []
    if where == "forward":
        real = hip.avgpool_fwd

        def avgpool(*a, **kw):
            if not fired and a[2] == 8:         # the second of the four pyramid poolings
                fired.append(1)
                raise _Boom("life: raised in the middle of the forward")
            return real(*a, **kw)
        monkeypatch.setattr(hip, "avgpool_fwd", avgpool)
        with pytest.raises(_Boom):
            m(x)
    else:
        def probe(tag, mod, tensors):
            if not fired and tag == "nat_bwd:na":
                fired.append(1)
                raise _Boom("life: raised in the middle of the backward")
        monkeypatch.setattr(m._engine, "probe", probe)
        y = m(x)
        if recording:
            assert plan_of(m, A).fwd is not None and plan_of(m, A).bwd is None      # the forward was recorded, the backward is next
        with pytest.raises(_Boom):
            (y * G).sum().backward()
        monkeypatch.setattr(m._engine, "probe", None)
    assert fired
    torch.cuda.synchronize()
    if recording:
        assert all(ps.fwd is None and ps.bwd is None for ps in m._plans.values())      # nothing truncated is kept
    for p in m.parameters():
        p.grad = None
    tag = "after a %s that raised %s" % (where, "while recording" if recording else "launch by launch")
    checkpoint(m, "the model " + tag, x, G)
    if recording:
        assert all(ps.fwd is None for ps in m._plans.values())                          # that pass ran launch by launch
    checkpoint(other, "a second model " + tag, xin(C), gout(C))
    checkpoint(m, "the model, other shape, " + tag, xin(C), gout(C))


# ------------------------------------------------------------------ 7. parameter storage moved
def test_storage_moved_launch_by_launch():
    """PackPlan's documented re-record: every parameter in new storage, one weight changed in place."""
    m = model(83)
    for shp in (A, C, A):
        one_pass(m, xin(shp), gout(shp))
    assert m._engine.packs_fwd.jobs and m._engine.packs_bwd.jobs
    life.move_storage(m)
    checkpoint(m, "launch by launch after the parameters moved", xin(A), gout(A))
    with torch.no_grad():
        m.down1[0].weight.mul_(0.8)
    checkpoint(m, "second pass after the move (the new jobs are part of the batched re-pack now)", xin(A), gout(A))
    checkpoint(m, "third pass after the move, other shape", xin(C), gout(C))
    m.eval()
    checkpoint(m, "eval after the parameters moved", xin(C))


def test_storage_moved_into_the_place_of_another_parameter():
    """The packed-weight jobs are keyed by the weight's address: a parameter that moves to the address another one left (same kernel
    size and input channels, another row count) must not be served that one's job.  PackPlan.refresh compares every job's address
    with its parameter's and records anew.  (With that comparison taken out this case still passes -- the first rows of the two
    packed forms coincide -- and the plain move fails or passes with the blocks the allocator hands back: DESIGN 5m.)"""
    m = model(83)
    for shp in (A, C, A):
        one_pass(m, xin(shp), gout(shp))
    life.move_into_vacated_storage(m)
    checkpoint(m, "a parameter at the address another one left", xin(A), gout(A))
    checkpoint(m, "second pass with a parameter at the address another one left", xin(C), gout(C))


def test_storage_moved_under_plans():
    """Recorded launches carry the parameters' addresses: after a move the model must follow the new storage (or raise) -- never
    compute with the old one.  LM_Net.forward drops its plans and graphs when a parameter's address changed."""
    m = model(89)
    m.enable_plans()
    x, G = xin(A), gout(A)
    for _ in range(4):
        one_pass(m, x, G)
    m.eval()
    for _ in range(4):
        one_pass(m, x)
    m.train()
    assert plan_of(m, A).bwd is not None and plan_of(m, A, False, False).fwd is not None
    life.move_storage(m)
    checkpoint(m, "plans after the parameters moved (train)", x, G)
    assert all(ps.fwd is None for ps in m._plans.values())                  # pinned: the plans were dropped, the pass ran launch by launch
    m.eval()
    checkpoint(m, "plans after the parameters moved (eval)", x)
    m.train()
    for _ in range(3):
        one_pass(m, x, G)                                                   # warms up and records again, on the new storage
    assert plan_of(m, A).bwd is not None
    checkpoint(m, "plans recorded again on the new storage", x, G)


def test_storage_moved_under_inference_graph():
    """The same for the captured inference forward (default mode: capture is refused in deterministic mode), against an eager twin
    at the 1e-5 of test_inference_graph_replay_matches_eager_and_follows_the_weights."""
    m = model(97, train=False, deterministic=False)
    m.enable_graphs()
    x = xin(A)
    for _ in range(4):
        one_pass(m, x)
    assert sum(g.fwd is not None for g in m._graphs.values()) == 1
    before = one_pass(m, x)["logits"]
    life.move_storage(m)
    t = twin(m, deterministic=False)
    got, want = one_pass(m, x)["logits"], one_pass(t, x)["logits"]
    assert rel_err(want, before) > 1e-2                                     # (the changed weights do change the logits)
    assert rel_err(got, want) < 1e-5
    assert all(g.fwd is None for g in m._graphs.values())                   # pinned: the graph was dropped
    for _ in range(3):
        got = one_pass(m, x)["logits"]                                      # captured again on the new storage
    assert sum(g.fwd is not None for g in m._graphs.values()) == 1 and rel_err(got, want) < 1e-5


def test_structural_reparam_after_a_history():
    m = model(101)
    m.enable_plans()
    for shp in (A, A, A, A, C, D):
        one_pass(m, xin(shp), gout(shp))
    m.eval()
    for shp in (A, A, A, C):
        one_pass(m, xin(shp))
    t = twin(m)
    m.structural_reparam()
    t.structural_reparam()
    assert m._plans == {} and len(m.state_dict()) == len(t.state_dict()) == 510
    for shp in (A, C):
        same(one_pass(m, xin(shp)), one_pass(t, xin(shp)), "deploy form after a history, %s" % NAME[shp])


# ------------------------------------------------------------------ 8. default mode and graphs
def _nbt(m):
    return {int(b) for k, b in m.named_buffers() if k.endswith("num_batches_tracked")}


def test_graphs_interleaved_default_mode():
    """enable_graphs(): training passes A A A B B B A B with inference replays of A and C between them.  Default mode, so the
    comparison with the eager twin is the `agree` rule of test_plan_mode_matches_host_launches (life.agree) and 1e-5 for the
    inference replays; num_batches_tracked counts every training pass whatever route it took."""
    m = model(103, deterministic=False)
    m.enable_graphs()
    X, G = {s: xin(s) for s in (A, B, C)}, {s: gout(s) for s in (A, B)}
    seq = (A, A, A, B, B, B, A, B)
    n_train, last = 0, {}
    for i, shp in enumerate(seq):
        final = i >= len(seq) - 2
        t = twin(m, deterministic=False) if final else None
        rm = one_pass(m, X[shp], G[shp])
        n_train += 1
        if final:
            rt = one_pass(t, X[shp], G[shp])
            assert rel_err(rm["logits"], rt["logits"]) < TOL, NAME[shp]
            life.agree_grads(rm, rt)
        m.eval()
        es = (A, C)[i % 2]
        ye = one_pass(m, X[es])["logits"]
        if final:                                                           # the fourth forward of this shape: a replay
            last[es] = rel_err(ye, one_pass(twin(m, deterministic=False), X[es])["logits"])
        m.train()
    assert sum(g.fwd is not None for g in m._graphs.values()) == 4          # train A, train B, infer A, infer C
    assert _nbt(m) == {n_train}
    assert set(last) == {A, C} and max(last.values()) < 1e-5, last


def test_graphs_redraw_dropout_across_shapes():
    """Dropout on: two consecutive training steps differ by more than the 1e-3 of test_graph_mode_matches_host_launches..., within
    one shape and across a shape switch (the device-side counter moves with every training pass of the model)."""
    c = model(11, deterministic=False, dropout=True)
    c.enable_graphs()
    outs = {A: [], B: []}
    seq = (A, A, A, A, B, B, B, B, A, B)
    for shp in seq:
        o = c(xin(shp))
        o.sum().backward()
        outs[shp].append(o.detach().clone())
        for p in c.parameters():
            p.grad = None
    assert sum(g.fwd is not None for g in c._graphs.values()) == 2
    for shp in (A, B):
        o = outs[shp]
        assert float((o[2] - o[3]).abs().max()) > 1e-3, NAME[shp]           # within one shape: the captured pass and its first replay
        assert float((o[3] - o[4]).abs().max()) > 1e-3, NAME[shp]           # across a shape switch: two replays with the other shape between
    assert _nbt(c) == {len(seq)}


# ------------------------------------------------------------------ 10. satellites: one object across small, large, small
def _sat_logits(shape, n=2, scale=3.0):
    from tools.detweights import det_input, disc_labels
    B_, _, H, W = shape
    lg = det_input((B_, n, H, W), "life/sat/%s" % NAME[shape]) * scale
    lg[:, 1] += (disc_labels(B_, H, W).float() * 2 - 1) * 1.5
    return lg.cuda()


@pytest.mark.parametrize("route", ["default", "extended"])
def test_satellite_segloss_across_shapes(route):
    """One SegLoss through A, C, A (deterministic mode: the loss kernels sum in a fixed order): loss value and dlogits equal those
    of a freshly constructed SegLoss, bit for bit."""
    from lm_net_amd import hip
    from lm_net_amd.loss import SegLoss
    kw = dict(label_smoothing=1e-3) if route == "default" else dict(label_smoothing=1e-3, focal_scale=0.5, ignore_index=255)
    hip.set_deterministic(True)
    used = SegLoss(**kw).cuda()
    assert used.extended == (route == "extended")
    for i, shp in enumerate((A, C, A)):
        lg, y = _sat_logits(shp), life.labels(shp)

        def run(crit):
            l = lg.clone().requires_grad_(True)
            out = crit(l, y)
            (out * 1.5).backward()
            torch.cuda.synchronize()
            return out.detach().clone(), l.grad.clone()

        (lu, gu), (lf, gf) = run(used), run(SegLoss(**kw).cuda())
        assert torch.isfinite(lu) and float(gu.abs().max()) > 0
        assert torch.equal(lu, lf) and torch.equal(gu, gf), (i, NAME[shp], float(lu), float(lf))


def test_satellite_curvemeter_across_shapes():
    """CurveMeter(softmax) keeps one scratch per (B, HW): two keys in the order small, large, small; integer histograms, exact."""
    from lm_net_amd import CurveMeter
    used, fresh = CurveMeter(2, "softmax", 101), []
    for shp in (A, C, A):
        v, y = _sat_logits(shp), life.labels(shp)
        used.update(v, y)
        f = CurveMeter(2, "softmax", 101)
        f.update(v, y)
        fresh.append(f.raw())
    assert len(used._ws) == 2
    raw = used.raw()
    assert raw.shape[0] == 2 + 3 + 2 and int(raw.sum()) == 2 * sum(s[0] * s[2] * s[3] for s in (A, C, A))
    assert torch.equal(raw, torch.cat(fresh))


def test_satellite_postprocess_across_shapes():
    """DevicePostprocess takes its workspace from the allocator at every call (a recycled block after the first): labels, resized
    labels and statistics of small, large, small equal those of a fresh object."""
    from lm_net_amd.post import DevicePostprocess
    kw = dict(keep_largest=True, min_area=4, fill_holes=True)
    used = DevicePostprocess(2, **kw)
    for i, shp in enumerate((A, C, A)):
        lg = _sat_logits(shp)
        hw = (shp[2] + 5, shp[3] - 3)
        a, b = used(lg, src_hw=hw), DevicePostprocess(2, **kw)(lg, src_hw=hw)
        torch.cuda.synchronize()
        assert int(a.labels_net.sum()) > 0
        for name in ("labels_net", "labels", "stats"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (i, NAME[shp], name)


def test_satellite_tiled_predictor_across_frame_sizes():
    """One TiledPredictor and one model over two frame sizes (small, large, small; deterministic mode): map and labels equal those
    of a fresh predictor on the same model."""
    from lm_net_amd import LM_Net, hip
    from lm_net_amd.infer import TiledPredictor
    from tools.detweights import det_input, fill_module
    net = LM_Net(3, 2, filters=[12] * 5)
    fill_module(net, 5)
    net = net.cuda().eval()
    hip.set_deterministic(True)
    kw = dict(tile=64, overlap=0.5, flips=("h",))
    used = TiledPredictor(net, **kw)
    for i, (B_, H, W) in enumerate(((1, 40, 50), (2, 100, 150), (1, 40, 50))):
        x = det_input((B_, 3, H, W), "life/tiles/%dx%d" % (H, W)).cuda()
        r = used(x)
        mu, lu = r.map.clone(), r.labels.clone()
        f = TiledPredictor(net, **kw)(x)
        assert tuple(mu.shape) == (B_, 2, H, W)
        assert torch.equal(mu, f.map) and torch.equal(lu, f.labels), (i, H, W, float((mu - f.map).abs().max()))
    assert len(used._cache) == 2

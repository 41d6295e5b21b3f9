"""GPU: wide LM_Net variants (filters up to 4x the default; README "Wider variants") through whole passes.

  W2 [24,48,96,192,384]  W3 [36,72,144,288,576]  W4 [48,96,192,384,768]  Wodd [12,36,60,84,120]

Each fp32 training step (batch-statistics BatchNorm, dropout off) is checked against float64 goldens of the REAL reference
(tests/golden/wide_*.npz, tools/make_golden_wide.py) with the tolerances of tests/test_configs_gpu.py: logits, every parameter
gradient, the input gradient and the BatchNorm running statistics.  Then bf16 against the fp32 HIP path, eval and structural_reparam
against the CPU oracle (oracle/lmnet_ref.py, pinned to the reference at these widths by tests/test_wide_cpu.py), plan replay against
host launch (deterministic mode), an enable_graphs step, and the envelope check.
"""
import pytest
import torch

from helpers import no_dropout, rel_err
from tools.detweights import det_input, fill_module

pytestmark = pytest.mark.gpu
TOL = 1e-4
WIDE = {
    "W2": [24, 48, 96, 192, 384],
    "W3": [36, 72, 144, 288, 576],
    "W4": [48, 96, 192, 384, 768],
    "Wodd": [12, 36, 60, 84, 120],
}


def _pair(filters, seed):
    from lm_net_amd import LM_Net
    from oracle.lmnet_ref import LM_Net as Oracle
    ora = Oracle(3, 2, filters=filters)
    fill_module(ora, seed)
    no_dropout(ora)
    m = LM_Net(3, 2, filters=filters)
    fill_module(m, seed)
    no_dropout(m)
    return ora, m.cuda()


def _golden_train_step(name, size, B, tol_g=4e-3, tol_affine=2.5e-2):
    """One training step against tests/golden/wide_<name>_<size>_b<B>.npz: the REAL reference run in float64 on the same name-keyed
    weights / inputs (tools/make_golden_wide.py), checked as tests/test_configs_gpu.py checks its goldens: logits 1e-4 of their
    largest element; gradients on the sampled entries 4e-3 (weights) / 2.5e-2 (1-D parameters) of the tensor's largest element and
    2e-3 on every tensor's L2 norm; BatchNorm running statistics 1e-4."""
    import numpy as np
    from lm_net_amd import LM_Net
    from helpers import load_golden
    from tools.make_golden_f64 import sample_index
    key = "wide_%s_%d_b%d" % (name, size, B)
    g = load_golden(key + ".npz")
    size, B, seed = (int(v) for v in g["meta"])
    filters = [int(v) for v in g["filters"]]
    assert filters == WIDE[name]
    m = LM_Net(3, 2, filters=filters)
    fill_module(m, seed)
    no_dropout(m)
    m = m.cuda().train()
    x = det_input((B, 3, size, size), key + "/x").cuda().requires_grad_(True)
    y = m(x)
    yf = y.detach().flatten().cpu().double()
    ys = yf[torch.from_numpy(sample_index(yf.numel(), 32768))].numpy()
    assert float(np.abs(ys - g["logits/sample"]).max()) < TOL * float(g["logits/stat"][0]), name
    assert abs(float(yf.norm()) - float(g["logits/stat"][1])) < TOL * float(g["logits/stat"][1]), name
    (y * det_input(tuple(y.shape), key + "/G").cuda()).sum().backward()
    torch.cuda.synchronize()
    gmax = max(float(g["gstat/" + k][0]) for k, _ in m.named_parameters())

    def check(tag, grad, stat, samp):
        gf = grad.detach().flatten().cpu().double()
        gs = gf[torch.from_numpy(sample_index(gf.numel()))].numpy()
        err = float(np.abs(gs - samp).max())
        if err < 2e-5 * gmax:          # pre-BatchNorm biases (exact gradient 0) and other tiny tensors: absolute scale
            return
        assert err < (tol_affine if grad.dim() == 1 else tol_g) * float(stat[0]), (name, tag, err, float(stat[0]))
        assert abs(float(gf.norm()) - float(stat[1])) < 2e-3 * float(stat[1]), (name, tag, float(gf.norm()), float(stat[1]))

    check("input", x.grad, g["gx/stat"], g["gx/sample"])
    for k, p in m.named_parameters():
        check(k, p.grad, g["gstat/" + k], g["gsamp/" + k])
    for k, v in m.state_dict().items():
        if "running_" in k:
            assert rel_err(v, g["state/" + k]) < 1e-4, (name, k)


@pytest.mark.parametrize("name", list(WIDE))
def test_wide_train_step_64_batch2_vs_reference_f64(name):
    _golden_train_step(name, 64, 2)


def test_w2_train_step_352_batch2_vs_reference_f64():
    _golden_train_step("W2", 352, 2)


@pytest.mark.parametrize("name", ["W3", "Wodd"])
def test_wide_bf16_vs_fp32_path(name):
    """bf16 storage (and bf16-mma) against the fp32 HIP path of the same model, with the distances test_model_gpu's configs[2] test
    states against fp32 goldens: logits 4e-2 of their range / 1.6e-2 in L2 (train 5e-2 / 3e-2), input gradient 0.1 in L2, parameter
    gradients 0.1 median / 0.4 worst in L2."""
    def l2(a, b):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return float((a - b).norm() / (b.norm() + 1e-30))

    x = det_input((2, 3, 64, 64), "wide_bf16/x").cuda()
    G = det_input((2, 2, 64, 64), "wide_bf16/G").cuda()

    def run(mode):
        _, m = _pair(WIDE[name], 9)
        m.compute_dtype = mode
        m.eval()
        with torch.no_grad():
            ye = m(x)
        m.train()
        xg = x.clone().requires_grad_(True)
        yt = m(xg)
        (yt * G).sum().backward()
        torch.cuda.synchronize()
        return ye, yt.detach(), xg.grad, [(k, p.grad) for k, p in m.named_parameters()]

    ref = run("fp32")
    for mode in ("bf16", "bf16-mma"):
        ye, yt, gx, grads = run(mode)
        assert 2e-4 < rel_err(ye, ref[0]) < 4e-2 and l2(ye, ref[0]) < 1.6e-2, (mode, rel_err(ye, ref[0]))
        assert rel_err(yt, ref[1]) < 5e-2 and l2(yt, ref[1]) < 3e-2, (mode, rel_err(yt, ref[1]))
        assert l2(gx, ref[2]) < 0.1, mode
        errs = sorted((l2(g, gr), k) for (k, g), (_, gr) in zip(grads, ref[3]) if float(gr.abs().max()) > 0 and
                      not (k.endswith("expand_conv.0.bias") or k.endswith("fuse_conv.0.bias")))
        assert errs[len(errs) // 2][0] < 0.1 and errs[-1][0] < 0.4, (mode, errs[len(errs) // 2], errs[-1])
    # autocast selects the bf16 path
    _, m = _pair(WIDE[name], 9)
    m.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ya = m(x)
    assert rel_err(ya, ref[0]) > 2e-4 and rel_err(ya, ref[0]) < 4e-2


@pytest.mark.parametrize("name", ["W2", "Wodd"])
def test_wide_eval_and_structural_reparam_vs_oracle(name):
    ora, m = _pair(WIDE[name], 11)
    ora.eval()
    m.eval()
    x = det_input((2, 3, 64, 96), "wide_eval/x")
    with torch.no_grad():
        yo = ora(x)
        yg = m(x.cuda())
    assert rel_err(yg, yo) < TOL, rel_err(yg, yo)
    ora.structural_reparam()
    m.structural_reparam()
    with torch.no_grad():
        yo2 = ora(x)
        yg2 = m(x.cuda())
    assert rel_err(yg2, yo2) < TOL, rel_err(yg2, yo2)
    assert rel_err(yo2, yo) < 1e-4


def test_wide_plan_replay_equals_host_launch_deterministic_and_graph_step():
    """W3 (general neighbourhood-attention kernels at every level, GFT head_dim 93): in deterministic mode the recorded plan's replay
    is bit-identical to the launch-by-launch step; an enable_graphs step runs and agrees with the host step."""
    from lm_net_amd import hip
    x = det_input((2, 3, 64, 64), "wide_plan/x").cuda()
    G = det_input((2, 2, 64, 64), "wide_plan/G").cuda()

    def step(m):
        m.zero_grad(set_to_none=True)
        y = m(x)
        (y * G).sum().backward()
        torch.cuda.synchronize()
        return y.detach().clone(), [p.grad.detach().clone() for p in m.parameters()]

    hip.set_deterministic(True)
    try:
        _, m = _pair(WIDE["W3"], 13)
        m.train()
        m.deterministic = True
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        host = step(m)
        m.load_state_dict(sd)
        m.enable_plans(True)
        runs = []
        for _ in range(4):                   # two sizing passes, one recording, one replay
            m.load_state_dict(sd)
            runs.append(step(m))
        for y, gr in runs[2:]:
            assert torch.equal(y, host[0])
            assert all(torch.equal(u, v) for u, v in zip(gr, host[1]))
        m.enable_plans(False)
    finally:
        hip.set_deterministic(False)
    _, m = _pair(WIDE["W3"], 13)
    m.train()
    ref = step(m)
    m.enable_graphs(True)
    for _ in range(3):
        yg, gg = step(m)
    assert rel_err(yg, ref[0]) < 1e-3
    assert torch.isfinite(yg).all()


@pytest.mark.parametrize("name", ["W3", "Wodd"])
def test_wide_bf16_step_deterministic_twice_bit_identical(name):
    """bf16 storage on the wide instances (general neighbourhood attention, VALU global attention at head dim 93 / 26, wide
    LayerNorm rows), deterministic mode: two steps from one state agree bit for bit -- logits, input gradient, every parameter
    gradient.  Float-atomic noise is switched off here, so a difference is a race or an uninitialised read (DESIGN, wide variants:
    the default-mode spread of the bf16 gradients)."""
    from lm_net_amd import hip
    x = det_input((2, 3, 64, 64), "wide_det16/x").cuda()
    G = det_input((2, 2, 64, 64), "wide_det16/G").cuda()
    hip.set_deterministic(True)
    try:
        _, m = _pair(WIDE[name], 21)
        m.train()
        m.deterministic = True
        m.compute_dtype = "bf16"
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        runs = []
        for _ in range(2):
            m.load_state_dict(sd)
            m.zero_grad(set_to_none=True)
            xg = x.clone().requires_grad_(True)
            y = m(xg)
            (y * G).sum().backward()
            torch.cuda.synchronize()
            runs.append((y.detach().clone(), xg.grad.detach().clone(), [(k, p.grad.detach().clone()) for k, p in m.named_parameters()]))
    finally:
        hip.set_deterministic(False)
    (ya, gxa, ga), (yb, gxb, gb) = runs
    assert torch.isfinite(ya).all() and float(ya.abs().max()) > 0
    assert torch.equal(ya, yb), "logits differ"
    assert torch.equal(gxa, gxb), "input gradient differs"
    differ = [k for (k, u), (_, v) in zip(ga, gb) if not torch.equal(u, v)]
    assert not differ, "%d of %d parameter gradients differ between two deterministic bf16 steps: %s" % (len(differ), len(ga), differ[:8])


@pytest.mark.parametrize("filters", [[12, 24, 48, 396, 192], [48, 96, 192, 384, 828]])
def test_outside_envelope_raises_before_launch(filters):
    from lm_net_amd import LM_Net, hip
    m = LM_Net(3, 2, filters=filters).cuda()      # construction stays possible
    x = torch.zeros(1, 3, 64, 64, device="cuda")
    hip.prof_begin()
    with pytest.raises(ValueError) as e:
        m(x)
    assert hip.prof_end() == {}                   # nothing was launched
    assert ("396" in str(e.value) and "head_dim 33" in str(e.value)) or ("1548" in str(e.value) and "1536" in str(e.value))


def test_wide_fused_loss_and_adamw_step():
    """W2: the fused CE + Dice loss (lm_net_amd.loss.SegLoss) and the one-launch AdamW (lm_net_amd.optim.FusedAdamW) on a wide
    model's step: the loss against its PyTorch form on the same logits, the updated parameters against torch.optim.AdamW fed the
    same gradients."""
    import torch.nn.functional as F
    from lm_net_amd.loss import SegLoss
    from lm_net_amd.optim import FusedAdamW
    from tools.detweights import disc_labels
    _, m = _pair(WIDE["W2"], 17)
    m.train()
    ref = [p.detach().clone().requires_grad_(True) for p in m.parameters()]
    opt = FusedAdamW(m, lr=1e-3, weight_decay=1e-4)
    topt = torch.optim.AdamW(ref, lr=1e-3, weight_decay=1e-4)
    crit = SegLoss(ce_weight=(1.0, 4.0), dice_weight=(1.0, 4.0), label_smoothing=0.001).cuda()
    x = det_input((2, 3, 64, 64), "wide_opt/x").cuda()
    y = disc_labels(2, 64, 64, 3).cuda()
    out = m(x)
    loss = crit(out, y)
    lo = out.detach().double()
    ce = F.cross_entropy(lo, y.long(), weight=torch.tensor([1.0, 4.0], device="cuda", dtype=torch.float64), label_smoothing=0.001)
    p = torch.softmax(lo, 1)
    dice = 0.0
    for i, w in enumerate((1.0, 4.0)):
        t = (y == i).double()
        dice = dice + (1 - (2 * (p[:, i] * t).sum() + 1e-5) / ((p[:, i] ** 2).sum() + (t * t).sum() + 1e-5)) * w
    assert abs(float(loss) - float(ce + dice / 2)) < 1e-4 * abs(float(ce + dice / 2))
    opt.zero_grad(set_to_none=True)
    loss.backward()
    for r, q in zip(ref, m.parameters()):
        r.grad = q.grad.detach().clone()
    opt.step()
    topt.step()
    torch.cuda.synchronize()
    worst = max(float((q.detach() - r.detach()).abs().max()) for q, r in zip(m.parameters(), ref))
    assert worst < 1e-6, worst


def _ddp_worker(rank, world, port, q):
    import os
    import torch.distributed as dist
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.cuda.set_device(0)
        from lm_net_amd import LM_Net
        from lm_net_amd.ddp import DistributedLMNet
        net = LM_Net(3, 2, filters=WIDE["Wodd"])
        fill_module(net, seed=rank)
        no_dropout(net)
        net = net.cuda().train()
        x = det_input((2, 3, 64, 64), "wide_ddp/x%d" % rank).cuda()
        model = DistributedLMNet(net, bucket_bytes=1 << 20, first_bucket_bytes=256 << 10)
        hooks = (net.grad_begin_hook, net.grad_ready_hook, net.grad_finish_hook)
        net.grad_begin_hook = net.grad_ready_hook = net.grad_finish_hook = None
        net(x).square().mean().backward()
        local = torch.cat([p.grad.flatten() for p in net.parameters()]).clone()
        net.zero_grad(set_to_none=True)
        for bn in [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]:
            bn.reset_running_stats()
        net.grad_begin_hook, net.grad_ready_hook, net.grad_finish_hook = hooks
        model(x).square().mean().backward()
        torch.cuda.synchronize()
        reduced = torch.cat([p.grad.flatten() for p in net.parameters()]).cpu()
        gathered = [torch.zeros_like(local.cpu()) for _ in range(world)]
        dist.all_gather(gathered, local.cpu())
        expect = sum(gathered) / world
        q.put((rank, float((reduced - expect).abs().max() / (expect.abs().max() + 1e-30))))
        dist.destroy_process_group()
    except Exception as e:  # noqa: BLE001  (surface the failure in the parent)
        q.put((rank, repr(e)))


def test_wide_two_rank_ddp_step_on_one_gpu():
    """Wodd through lm_net_amd.ddp.DistributedLMNet, two gloo ranks sharing the test GPU: after backward every rank holds the mean of
    the per-rank gradients."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in ps]
    res = [q.get(timeout=240) for _ in range(2)]
    [p.join(60) for p in ps]
    for rank, err in res:
        assert isinstance(err, float), "rank %d failed: %s" % (rank, err)
        assert err < 1e-5, (rank, err)

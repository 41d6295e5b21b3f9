"""GPU: the entries of include/optim/lmnet_optim.h inside guard bands (tests/guard.py): the guard manifest's test of these entries.
Every buffer of lmn_optim_prepare and lmn_adamw_step_ex -- parameters, gradient, both moments, the EMA, the group bytes, the two
GradScaler scalars and the workspace at exactly lmn_optim_workspace(n) words -- is carved from a GuardPool at its exact size, canaries
flush against each; the skip path must leave everything but the workspace's reduction words and control block as it was."""
import pytest
import torch

import optim_ref as R
from guard import GuardPool, LaunchLog

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.mark.parametrize("n", [4, 4 * 256 + 4])
def test_prepare_and_step_entries(n):
    """n = 4 (one quad) and one quad past a block of 256 lanes."""
    from lm_net_amd import hip
    words = hip.optim_workspace(n)
    c0 = 2 * hip.optim_blocks(n)
    assert words == hip.optim_workspace_words(n) == c0 + 16 + 64
    q = (torch.arange(n // 4) % 3).to(torch.uint8)
    q[-1] = 1                                                                   # the last quad is live (group 2 is frozen)
    ws0 = torch.zeros(words)
    for k, row in enumerate(((1e-2, 0.1, 0.0), (1e-3, 0.0, 0.0), (1e-2, 0.1, 1.0))):
        ws0[c0 + 16 + 4 * k:c0 + 16 + 4 * k + 3] = torch.tensor(row)
    inputs = dict(p=R.seeded(n, 1), g=R.seeded(n, 2) * 256.0, m=R.seeded(n, 3, 0.1), v=R.seeded(n, 4).abs(), ema=R.seeded(n, 5), qgroup=q,
                  ws=ws0, grad_scale=torch.tensor([256.0]), found_inf=torch.tensor([0.0]))
    param = hip.optim_param((0.9, 0.99), 1e-8, max_norm=0.5, ema_decay=0.9, flags=hip.OPTIM_SKIP_NONFINITE, n_groups=3)

    def run(t):
        hip.optim_prepare(t["g"], t["qgroup"], param, t["ws"], t["grad_scale"], t["found_inf"])
        hip.adamw_step_ex(t["p"], t["g"], t["m"], t["v"], t["ema"], t["qgroup"], param, t["ws"])
        torch.cuda.synchronize()

    plain = {k: v.to(DEV) for k, v in inputs.items()}
    run(plain)
    pool = GuardPool(DEV, GuardPool.size_for([v.numel() * v.element_size() for v in inputs.values()]))
    guarded = {k: pool.take(k, None, None, init=v.to(DEV)) for k, v in inputs.items()}
    with LaunchLog(pool) as log:
        run(guarded)
    pool.assert_clean("optimizer entries")
    pool.assert_inputs_unchanged(skip=("p", "m", "v", "ema", "ws"))             # the gradient, the group bytes and the scalars are read-only
    assert log.names == ["optim_prepare", "adamw_step_ex"]
    sizes = {e[0]: e[2] for e in pool.entries}
    assert sizes["ws"] == 4 * words and sizes["qgroup"] == n // 4 and sizes["p"] == sizes["ema"] == 4 * n and sizes["found_inf"] == 4
    for k in ("p", "m", "v", "ema", "ws"):                                      # bit-identical to ordinary allocations
        assert torch.equal(plain[k].view(torch.int32), guarded[k].view(torch.int32)), k
    ctrl = guarded["ws"][c0:c0 + 16].view(torch.int32).cpu()
    assert ctrl[hip.OPTIM_SKIP] == 0 and ctrl[hip.OPTIM_STEP] == 1 and ctrl[hip.OPTIM_SKIPPED] == 0 and ctrl[hip.OPTIM_NONFINITE] == 0
    assert not torch.equal(guarded["p"], pool.inputs["p"]) and torch.equal(guarded["ws"][c0 + 16:], pool.inputs["ws"][c0 + 16:])
    frozen = (R.elem_groups(q) == 2).to(DEV)
    for k in ("p", "m", "v", "ema"):                                            # a frozen quad is not stored
        assert torch.equal(guarded[k][frozen], pool.inputs[k][frozen]), k

    # the skip path: a NaN in the last quad.  Nothing is stored outside the workspace's reduction words and control block.
    after = {k: guarded[k].clone() for k in ("p", "m", "v", "ema", "ws")}
    guarded["g"][-1] = float("nan")
    pool.inputs["g"] = guarded["g"].clone()
    with LaunchLog(pool) as log:
        run(guarded)
    pool.assert_clean("optimizer entries, skip path")
    pool.assert_inputs_unchanged(skip=("p", "m", "v", "ema", "ws"))
    for k in ("p", "m", "v", "ema"):
        assert torch.equal(after[k].view(torch.int32), guarded[k].view(torch.int32)), k
    assert torch.equal(after["ws"][c0 + 16:], guarded["ws"][c0 + 16:])          # the group table
    ctrl = guarded["ws"][c0:c0 + 16].view(torch.int32).cpu()
    assert ctrl[hip.OPTIM_SKIP] == 1 and ctrl[hip.OPTIM_STEP] == 1 and ctrl[hip.OPTIM_SKIPPED] == 1 and ctrl[hip.OPTIM_NONFINITE] == 1
    assert torch.equal(ctrl[9:], torch.zeros(7, dtype=torch.int32))             # the spare words stay zero

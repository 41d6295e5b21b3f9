"""GPU: the entries of include/lmnet_loss.h inside guard bands (tests/guard.py): the guard manifest's test of these
entries.  Every buffer of lmn_segloss_ex_fwd, lmn_segloss_ex_bwd
and lmn_image_stats -- logits, labels, both weight vectors, `sums` and `coef` at exactly the header's float counts, loss4, gscale,
dlogits, the uint8 prediction and stats -- is carved from a GuardPool at its exact size, canaries flush against each."""
import pytest
import torch

import void_ref as V
from guard import GuardPool, LaunchLog

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.mark.parametrize("C", [2, 64])
def test_loss_and_image_stats_entries(C):
    from lm_net_amd import hip
    B, H, W = 2, 37, 45
    key = "guard_loss/%d" % C
    lg = (V.det_input((B, C, H, W), key + "/lg") * 2.5).to(DEV)
    y = V.with_void(V.labels(B, H, W, C, key + "/y"), key + "/v").to(DEV)
    wce, wdice = V.weights(key + "/wce", C).to(DEV), V.weights(key + "/wdice", C).to(DEV)
    gscale = torch.tensor([0.37], device=DEV)
    pred = lg.argmax(1).to(torch.uint8)
    param = hip.loss_param(255, 1e-3, 1e-5, 0.7, 1.3, 0.5, 1.5, 0.25)            # every term on

    def run(t):
        hip.segloss_ex_fwd(t["logits"], t["labels"], t["w_ce"], t["w_dice"], param, t["sums"], t["coef"], t["loss4"])
        hip.segloss_ex_bwd(t["logits"], t["labels"], t["w_ce"], t["coef"], t["gscale"], param, t["dlogits"])
        hip.image_stats(t["logits"], t["labels"], C, 255, t["stats"])
        hip.image_stats(t["pred"], t["labels"], C, 255, t["stats8"])
        torch.cuda.synchronize()

    shapes = {"sums": ((hip.loss_sums_floats(C),), torch.float32), "coef": ((hip.loss_coef_floats(C),), torch.float32),
              "loss4": ((4,), torch.float32), "dlogits": (tuple(lg.shape), torch.float32), "stats": ((B, C, 4), torch.int64),
              "stats8": ((B, C, 4), torch.int64)}
    inputs = {"logits": lg, "labels": y, "w_ce": wce, "w_dice": wdice, "gscale": gscale, "pred": pred}
    hip.set_deterministic(True)
    try:
        plain = dict(inputs, **{k: torch.empty(s, device=DEV, dtype=dt) for k, (s, dt) in shapes.items()})
        run(plain)
        nbytes = [t.numel() * t.element_size() for t in plain.values()]
        pool = GuardPool(DEV, GuardPool.size_for(nbytes))
        guarded = {k: pool.take(k, None, None, init=v) for k, v in inputs.items()}
        guarded.update({k: pool.take(k, s, dt) for k, (s, dt) in shapes.items()})
        with LaunchLog(pool) as log:
            run(guarded)
    finally:
        hip.set_deterministic(False)
    pool.assert_clean("loss entries")
    pool.assert_inputs_unchanged()
    assert log.names == ["segloss_ex_fwd", "segloss_ex_bwd", "image_stats", "image_stats"]
    sizes = {e[0]: e[2] for e in pool.entries}
    assert sizes["sums"] == 4 * (4 + 3 * C) and sizes["coef"] == 4 * (4 + 2 * C) and sizes["loss4"] == 16
    assert sizes["stats"] == B * C * 4 * 8 and sizes["pred"] == B * H * W and sizes["dlogits"] == 4 * B * C * H * W
    for k in ("loss4", "coef", "dlogits"):                                        # bit-identical to ordinary allocations
        assert torch.equal(plain[k].view(torch.int32), guarded[k].view(torch.int32)), k
    assert torch.equal(plain["stats"], guarded["stats"]) and torch.equal(plain["stats8"], guarded["stats"])
    assert bool(torch.isfinite(guarded["loss4"]).all()) and float(guarded["loss4"][3]) > 0

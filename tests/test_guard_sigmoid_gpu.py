"""GPU: the entries of include/lmnet_sigmoid.h inside guard bands (tests/guard.py): the guard manifest's test of these
entries.  Every buffer of lmn_sigloss_fwd, lmn_sigloss_bwd and
lmn_sigmoid_stats -- logits, the target, the three weight vectors, `sums` and `coef` at exactly the header's sizes, loss4, gscale,
dlogits, stats and the uint8 label maps -- is carved from a GuardPool at its exact size, canaries flush against each.  HW = 37 * 45
is odd (one element per lane, and the int64 / uint8 planes end on no 16-byte boundary); 36 * 44 runs the four-element form, whose
16-byte loads and stores end flush with the buffers."""
import pytest
import torch

import sigmoid_ref as S
from guard import GuardPool, LaunchLog

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.mark.parametrize("H, W", [(37, 45), (36, 44)])
@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8])
@pytest.mark.parametrize("C", [1, 64])
def test_loss_and_stats_entries(C, dtype, H, W):
    from lm_net_amd import hip
    B = 2
    key = "guard_sig/%d" % C
    lg = S.logits((B, C, H, W), key + "/lg").to(DEV)
    t = S.targets((B, C, H, W), key + "/t", key + "/v").to(dtype).to(DEV)
    wb, pw, wd = (S.weights("%s/%s" % (key, n), C).to(DEV) for n in ("wbce", "pw", "wdice"))
    gscale = torch.tensor([0.37], device=DEV)
    param = hip.sig_param(1e-5, 0.7, 1.3, 0.5, 1.5, 0.25, hip.sig_target_kind(t))            # every term on
    lt = hip.sig_logit_threshold(0.3)

    def run(x):
        hip.sigloss_fwd(x["logits"], x["target"], x["w_bce"], x["pos_weight"], x["w_dice"], param, x["sums"], x["coef"], x["loss4"])
        hip.sigloss_bwd(x["logits"], x["target"], x["pos_weight"], x["coef"], x["gscale"], param, x["dlogits"])
        hip.sigmoid_stats(x["logits"], x["target"], lt, x["stats"], x["labels"])
        hip.sigmoid_stats(x["logits"], x["target"], lt, x["stats_only"], None)
        hip.sigmoid_stats(x["logits"], None, lt, None, x["labels_only"])
        torch.cuda.synchronize()

    shapes = {"sums": ((hip.sig_sums_words(C),), torch.int32), "coef": ((hip.sig_coef_floats(C),), torch.float32),
              "loss4": ((4,), torch.float32), "dlogits": (tuple(lg.shape), torch.float32), "stats": ((B, C, 4), torch.int64),
              "stats_only": ((B, C, 4), torch.int64), "labels": (tuple(lg.shape), torch.uint8), "labels_only": (tuple(lg.shape), torch.uint8)}
    inputs = {"logits": lg, "target": t, "w_bce": wb, "pos_weight": pw, "w_dice": wd, "gscale": gscale}
    hip.set_deterministic(True)
    try:
        plain = dict(inputs, **{k: torch.empty(s, device=DEV, dtype=dt) for k, (s, dt) in shapes.items()})
        run(plain)
        nbytes = [x.numel() * x.element_size() for x in plain.values()]
        pool = GuardPool(DEV, GuardPool.size_for(nbytes))
        guarded = {k: pool.take(k, None, None, init=v) for k, v in inputs.items()}
        guarded.update({k: pool.take(k, s, dt) for k, (s, dt) in shapes.items()})
        with LaunchLog(pool) as log:
            run(guarded)
    finally:
        hip.set_deterministic(False)
    pool.assert_clean("sigmoid entries")
    pool.assert_inputs_unchanged()
    assert log.names == ["sigloss_fwd", "sigloss_bwd", "sigmoid_stats", "sigmoid_stats", "sigmoid_stats"]
    sizes = {e[0]: e[2] for e in pool.entries}
    assert sizes["sums"] == 4 * 6 * C and sizes["coef"] == 4 * 4 * C and sizes["loss4"] == 16
    assert sizes["stats"] == B * C * 4 * 8 and sizes["labels"] == B * C * H * W and sizes["dlogits"] == 4 * B * C * H * W
    assert sizes["target"] == B * C * H * W * (8 if dtype == torch.int64 else 1)
    for k in ("loss4", "coef", "dlogits"):                                        # bit-identical to ordinary allocations
        assert torch.equal(plain[k].view(torch.int32), guarded[k].view(torch.int32)), k
    for k in ("stats", "stats_only", "labels", "labels_only"):
        assert torch.equal(plain[k], guarded[k]), k
    assert torch.equal(guarded["stats"], guarded["stats_only"]) and torch.equal(guarded["labels"], guarded["labels_only"])
    assert bool(torch.isfinite(guarded["loss4"]).all()) and float(guarded["loss4"][3]) > 0

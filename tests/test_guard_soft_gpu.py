"""GPU: the three entries of include/soft/lmnet_soft.h that write device memory -- lmn_soft_fwd, lmn_soft_bwd, lmn_mix_batch -- inside
guard bands (tests/guard.py): the guard manifest's tests of these entries.  Every buffer -- the logits and every target tensor, the
workspace at exactly lmn_soft_workspace bytes, sums, counts, coef, the terms and dlogits; the batch, the labels, the device copy of the
rows and the four outputs of the mixer -- is carved from a GuardPool at its exact size, canaries flush against each, and every body
the entries write starts filled with junk (0xA5 bytes).  The shapes are the smallest templated one, the smallest general-C one, the
four-pixel bf16 route and the scalar sigmoid one, in ordinary and in deterministic mode."""
import numpy as np
import pytest
import torch

import soft_ref as R
from guard import JUNK, LaunchLog, pools, sizes

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("head,shape,reader", [
    ("softmax", (1, 2, 1, 1), "probs"),                    # the smallest templated shape
    ("softmax", (2, 3, 5, 7), "pair"),
    ("softmax", (2, 5, 3, 3), "probs"),                    # the smallest general-C shape: C = 5
    ("softmax", (2, 5, 3, 3), "pair"),
    ("softmax", (2, 5, 3, 3), "teacher_f32"),
    ("softmax", (2, 5, 3, 4), "teacher_bf16"),             # H * W % 4 == 0: four pixels per lane, general C
    ("softmax", (2, 4, 2, 2), "teacher_bf16"),             # the same, templated
    ("softmax", (2, 2, 5, 7), "teacher_bf16"),             # odd H * W: one pixel per lane
    ("sigmoid", (2, 1, 5, 7), "teacher_f32"),              # odd H * W: the scalar sigmoid route
    ("sigmoid", (2, 3, 5, 7), "teacher_bf16"),
    ("sigmoid", (2, 3, 2, 6), "teacher_bf16")])            # the vector sigmoid route
def test_soft_loss_entries(head, shape, reader, det):
    """Forward and backward with every buffer at its exact size and junk in it: the same bits as with ordinary allocations (in
    deterministic mode; the count in either), and the values of the restatement."""
    from lm_net_amd import hip
    B, C, H, W = shape
    rd, hd = R.READERS.index(reader), ("softmax", "sigmoid").index(head)
    seg = reader in ("probs", "pair")
    r = R.inputs(B, C, H, W, reader, head, seed=5, void=0.0 if H * W == 1 else 0.2, dtype=np.uint8)
    ws_bytes = hip.soft_workspace(rd, hd, B, C, H, W)
    inputs = dict(logits=torch.from_numpy(r.lg), gscale=torch.tensor([0.5]))
    if reader == "probs":
        inputs.update(target=torch.from_numpy(r.q))
    elif reader == "pair":
        inputs.update(ya=torch.from_numpy(r.ya), yb=torch.from_numpy(r.yb), lam=torch.from_numpy(r.lam))
    else:
        zt = torch.from_numpy(r.zt)
        inputs.update(target=zt.to(torch.bfloat16) if reader == "teacher_bf16" else zt, ya=torch.from_numpy(r.valid))
    if seg:
        inputs.update(w_ce=torch.tensor([1.0 + 0.5 * k for k in range(C)]), w_dice=torch.tensor([2.0 - 0.25 * k for k in range(C)]))
    outputs = dict(workspace=((ws_bytes,), torch.uint8), sums=((1 + 3 * C,), torch.float32), counts=((1,), torch.int32),
                   coef=((1 + 2 * C,), torch.float32), terms=((3,), torch.float32), dlogits=(r.lg.shape, torch.float32))
    T, eps = (1.0, 0.1) if seg else (4.0, 0.0)

    def run(x):
        g = x.get
        hip.soft_fwd(x["logits"], rd, hd, g("target"), g("ya"), g("yb"), g("lam"), T, eps, 1e-5, 0.7, 1.3 if seg else 0.0, g("w_ce"), g("w_dice"),
                     x["workspace"], x["sums"], x["counts"], x["coef"], x["terms"])
        hip.soft_bwd(x["logits"], rd, hd, g("target"), g("ya"), g("yb"), g("lam"), T, eps, g("w_ce"), x["coef"], x["gscale"], x["dlogits"])
        torch.cuda.synchronize()

    was = hip.get_deterministic()
    hip.set_deterministic(det)
    try:
        plain, pool, guarded = pools(inputs, outputs, DEV, fill="junk")
        run(plain)
        with LaunchLog(pool) as log:
            run(guarded)
    finally:
        hip.set_deterministic(was)
    pool.assert_clean("soft loss entries")
    pool.assert_inputs_unchanged()
    assert log.names == ["soft_fwd", "soft_bwd"]
    got = sizes(pool, plain)
    assert got["workspace"] == ws_bytes and got["terms"] == 12 and got["dlogits"] == 4 * r.lg.size and got["counts"] == 4
    assert torch.equal(plain["counts"], guarded["counts"])
    if det:
        for name in outputs:
            if name != "workspace":
                assert torch.equal(plain[name].view(torch.uint8), guarded[name].view(torch.uint8)), name
    else:                                                  # the workspace is neither read nor written outside deterministic mode
        assert bool((guarded["workspace"] == JUNK).all())
    terms = guarded["terms"].cpu().numpy().astype(np.float64)
    d = guarded["dlogits"].cpu().numpy().astype(np.float64)
    if seg:
        ref = R.loss_and_grad(r, reader, gscale=0.5, w_ce=inputs["w_ce"].numpy(), w_dice=inputs["w_dice"].numpy(), eps=eps, ce_scale=0.7, dice_scale=1.3)
        assert all(abs(g - w) <= 1e-5 * abs(w) for g, w in zip(terms, (ref.loss, ref.ce, ref.dice))), (terms, ref.loss, ref.ce, ref.dice)
    else:
        ref = R.loss_and_grad(r, reader, head, T=T, scale=0.7, gscale=0.5)
        assert abs(terms[0] - ref.loss) <= 0.7e-5 * ref.magnitude and abs(terms[1] - ref.kd) <= 1e-5 * ref.magnitude, (terms, ref.loss, ref.magnitude)
    assert int(guarded["counts"][0]) == ref.N
    assert np.abs(d - ref.grad).max() <= 1e-4 * np.abs(ref.grad).max()


@pytest.mark.parametrize("dtype", [np.uint8, np.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("shape,soft", [((1, 1, 2, 2), True), ((3, 3, 9, 11), True), ((2, 2, 4, 8), True), ((3, 2, 5, 8), False)], ids=str)
def test_mix_batch_entry(shape, soft, dtype):
    """The mixer with every buffer at its exact size: the rows' device copy at 32 B bytes, the outputs bit-equal to the restatement,
    yb_out NULL when no row is a mixup row."""
    from lm_net_amd import hip
    B, Cin, H, W = shape
    rng = np.random.default_rng(7)
    x = rng.standard_normal(shape).astype(np.float32)
    y = rng.integers(0, 5, (B, H, W)).astype(dtype)
    y[rng.random(y.shape) < 0.2] = R.VOID
    modes = [(R.MIXUP if soft else R.NONE, R.CUTMIX, R.NONE)[b % 3] for b in range(B)]
    boxes = [(0, 0, H, W) if b % 2 else (H // 2, 1, H, W - 1) for b in range(B)]
    rows = hip.mix_rows([B - 1 - b for b in range(B)], modes, rng.random(B).astype(np.float32), boxes)
    inputs = dict(x=torch.from_numpy(x), y=torch.from_numpy(y))
    outputs = dict(rows_dev=((B, hip.MIX_ROW_WORDS), torch.int32), x_out=(shape, torch.float32), ya=((B, H, W), inputs["y"].dtype),
                   lam=((B,), torch.float32))
    if soft:
        outputs.update(yb=((B, H, W), inputs["y"].dtype))

    def run(t):
        hip.mix_batch(t["x"], t["y"], rows, t["rows_dev"], t["x_out"], t["ya"], t.get("yb"), t["lam"])
        torch.cuda.synchronize()

    plain, pool, guarded = pools(inputs, outputs, DEV, fill="junk")
    run(plain)
    with LaunchLog(pool) as log:
        run(guarded)
    pool.assert_clean("mix_batch")
    pool.assert_inputs_unchanged()
    assert log.names == ["mix_batch"]
    got = sizes(pool, plain)
    assert got["rows_dev"] == 32 * B and got["lam"] == 4 * B and got["x_out"] == 4 * x.size
    want = dict(zip(("x_out", "ya", "yb", "lam"), R.mix(x, y, rows)))
    for name in outputs:
        if name != "rows_dev":
            g = guarded[name].cpu().numpy()
            assert g.dtype == want[name].dtype and g.tobytes() == want[name].tobytes(), name
            assert torch.equal(plain[name], guarded[name]), name
    assert np.array_equal(guarded["rows_dev"].cpu().numpy(), rows)

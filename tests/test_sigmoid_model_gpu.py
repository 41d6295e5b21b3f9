"""GPU: one-logit (binary) and multi-label LM_Net models trained with lm_net_amd.SigmoidSegLoss.

One fp32 train step of the HIP path (batch-statistics BatchNorm, dropout off) against the CPU oracle on the same weights with the
float64 restatement of the loss (tests/sigmoid_ref.py) as its criterion: logits, input gradient and every parameter gradient, with
the method and the tolerances of tests/test_multiclass_model_gpu.py::_oracle_step; eval and structural_reparam against the oracle at
that file's TOL; a short training loop on binary int64 masks with void pixels."""
import numpy as np
import pytest
import torch

import sigmoid_ref as S
from helpers import no_dropout, rel_err
from tools.detweights import det_input, fill_module

pytestmark = pytest.mark.gpu
TOL = 1e-4
FILTERS = (12, 24, 48, 96, 192)


def _pair(channel, n_classes, seed):
    from lm_net_amd import LM_Net
    from oracle.lmnet_ref import LM_Net as Oracle
    ora = Oracle(channel, n_classes, filters=list(FILTERS))
    fill_module(ora, seed)
    no_dropout(ora)
    m = LM_Net(channel, n_classes, filters=list(FILTERS))
    fill_module(m, seed)
    no_dropout(m)
    return ora, m.cuda()


def _oracle_step(channel, n_classes, seed, crit_kw, ref_kw, target_dtype=torch.int64, size=64):
    """fp32 train step of the HIP path with SigmoidSegLoss against the CPU oracle with the restated loss on the same weights."""
    from lm_net_amd import SigmoidSegLoss
    ora, m = _pair(channel, n_classes, seed)
    ora.train()
    m.train()
    key = "sig_model/%d/%d" % (channel, n_classes)
    x = det_input((2, channel, size, size), key + "/x")
    t = S.targets((2, n_classes, size, size), key + "/t", key + "/v")       # overlapping planes, 20 % void
    xo = x.clone().requires_grad_(True)
    yo = ora(xo)
    lo = S.loss_terms(yo, t, **ref_kw)
    lo[0].backward()
    xg = x.cuda().requires_grad_(True)
    yg = m(xg)
    crit = SigmoidSegLoss(**crit_kw).cuda()
    lg = crit(yg, t.to(target_dtype).cuda())
    lg.backward()
    torch.cuda.synchronize()
    assert yg.shape == (2, n_classes, size, size)
    assert rel_err(yg, yo) < TOL, rel_err(yg, yo)
    for k in range(4):
        got, ref = float(crit.terms[k]), float(lo[k])
        print("term %d: got %.9g oracle %.9g" % (k, got, ref))
        # (the logits agree to TOL of their maximum, ~1e-4 * 5; every term is a mean or a ratio of means with |d term / d z| <= the
        #  largest weight per element, so a term moves by at most weight * 5e-4 absolute: 1e-3 of terms of the order 1)
        assert (got == 0.0) if ref == 0.0 else abs(got - ref) < 1e-3 * abs(ref)
    assert rel_err(xg.grad, xo.grad) < 2e-3, rel_err(xg.grad, xo.grad)
    go = dict(ora.named_parameters())
    gmax = max(float(p.grad.abs().max()) for p in go.values())
    for k, p in m.named_parameters():
        ref = go[k].grad
        err = float((p.grad.cpu() - ref).abs().max())
        if err < 2e-5 * gmax:
            continue
        assert err < (2.5e-2 if p.dim() == 1 else 4e-3) * float(ref.abs().max()), (k, err, float(ref.abs().max()))


@pytest.mark.parametrize("channel", [3, 1])
def test_one_logit_train_step_vs_oracle(channel):
    _oracle_step(channel, 1, 31, dict(pos_weight=[4.0]), dict(pos_weight=[4.0]))


def test_multilabel_train_step_vs_oracle():
    w = [S.weights("sig_model/ml/%s" % n, 3) for n in ("wbce", "pw", "wdice")]
    _oracle_step(3, 3, 33, dict(bce_weight=w[0].tolist(), pos_weight=w[1].tolist(), dice_weight=w[2].tolist(), focal_scale=0.5),
                 dict(w_bce=w[0], pos_weight=w[1], w_dice=w[2], focal_scale=0.5), target_dtype=torch.uint8)


def test_eval_and_structural_reparam_vs_oracle():
    ora, m = _pair(3, 1, 11)
    ora.eval()
    m.eval()
    x = det_input((2, 3, 64, 96), "sig_model/eval/x")
    with torch.no_grad():
        yo = ora(x)
        yg = m(x.cuda())
    assert yg.shape == (2, 1, 64, 96)
    assert rel_err(yg, yo) < TOL, rel_err(yg, yo)
    ora.structural_reparam()
    m.structural_reparam()
    with torch.no_grad():
        yo2 = ora(x)
        yg2 = m(x.cuda())
    assert rel_err(yg2, yo2) < TOL, rel_err(yg2, yo2)
    assert rel_err(yo2, yo) < 1e-4


def test_short_training_loop_on_binary_masks_with_void_pixels():
    """LM_Net(3, 1) + FusedAdamW + SigmoidSegLoss(pos_weight=[4]) on DevicePreprocess's int64 {0, 1} [B, H, W] masks with a band of
    void pixels; SigmoidStatsMeter on the last logits."""
    from lm_net_amd import LM_Net, SigmoidSegLoss, SigmoidStatsMeter
    from lm_net_amd.data import DevicePreprocess
    from lm_net_amd.optim import FusedAdamW
    rng = np.random.default_rng(5)
    B = 2
    img = torch.from_numpy(rng.integers(0, 256, (B, 90, 120, 3), dtype=np.uint8)).cuda()
    mask = torch.from_numpy((rng.integers(0, 256, (B, 90, 120)) > 180).astype(np.uint8) * 255).cuda()
    x, y = DevicePreprocess((64, 96))(img, mask)
    assert y.dtype == torch.int64 and y.shape == (B, 64, 96) and set(y.unique().tolist()) <= {0, 1}
    y[:, 10:14] = 255                                             # not annotated
    m = LM_Net(3, 1)
    fill_module(m, 7)
    m = m.cuda().train()
    before = [p.detach().clone() for p in m.parameters()]
    opt = FusedAdamW(m, lr=1e-3)
    crit = SigmoidSegLoss(pos_weight=[4.0]).cuda()
    for _ in range(3):
        m.zero_grad(set_to_none=True)
        out = m(x)
        loss = crit(out, y)
        loss.backward()
        torch.cuda.synchronize()
        terms = crit.terms.cpu()
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(terms).all())
        assert float(terms[0]) == float(terms[1:].sum()) and float(terms[3]) == 0.0
        assert all(p.grad is not None and not bool(torch.isnan(p.grad).any()) for p in m.parameters())
        opt.step()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    assert sum(int(not torch.equal(a, p.detach())) for a, p in zip(before, m.parameters())) > len(before) // 2
    meter = SigmoidStatsMeter(1)
    meter.update(out.detach(), y)
    assert np.array_equal(meter.raw().cpu().numpy(), S.stats(out.detach().cpu().numpy(), y.cpu().numpy()))
    assert int(meter.raw().sum()) == int((y <= 1).sum())

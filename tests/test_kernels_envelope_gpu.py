"""GPU: the kernel instances that only the wider envelope selects, each against float64 or, for bf16 storage, against the
float64-checked fp32-storage launch of the same kernel (kernel_checks_envelope.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _run(fn):
    rows = fn()
    torch.cuda.synchronize()
    bad = [(n, e, t) for n, e, t in rows if not e <= t]
    assert not bad, "\n".join("%s: err %.3e > tol %.1e" % r for r in bad)


def _mk(name):
    def test():
        import kernel_checks_envelope as kce
        _run(getattr(kce, name))
    test.__name__ = "test_" + name[6:]
    return test


for _n in ["check_wide_bf16_rows", "check_na_hd16", "check_rows_envelope", "check_wgrad_1x1_envelope", "check_bn_bwd_rp_wide", "check_conv_mma_forms"]:
    globals()["test_" + _n[6:]] = _mk(_n)

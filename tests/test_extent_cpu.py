"""CPU: the limits by extent (README, "Limits by extent"), pinned by message, and the periodic-batch helper of tests/extent.py.

A refusal is host arithmetic that runs before any launch, so the C entries are called here with small fake pointers (as the other
_cpu tests do) at the FIRST refused extent, and lmn_last_error is read.  The accepted side is pinned only through entries that stay host
arithmetic (lmn_conv_chain_ok, lmn_conv_wgrad_up2_ok, lmn_conv_wgrad_workspace, ConfusionMeter's splitter): an accepted extent of a
launching entry is never called without a device."""
import ctypes as C

import pytest
import torch

import extent as X
from kernel_checks import R
from lm_net_amd import hip
from lm_net_amd.metrics import CONFUSION_MAX_PIXELS, _confusion_calls

FAKE = C.c_void_p(0x1000)


def _err(rc):
    return rc, hip.load().lmn_last_error().decode()


def _refused(rc, *words):
    rc, msg = _err(rc)
    assert rc != 0 and all(w in msg for w in words), (rc, msg)


# ------------------------------------------------------------------------------------------------------------------ counting entries
@pytest.mark.parametrize("entry", ["lmn_confusion", "lmn_confusion_labels"])
def test_confusion_refuses_2_24_pixels(entry):
    fn = getattr(hip.load(), entry)
    for B, HW in ((1, 1 << 24), (1, 4097 * 4097), (64, 512 * 512), (4, 1 << 22)):
        _refused(fn(FAKE, FAKE, B, 2, C.c_int64(HW), FAKE, None), "2^24", "pixels", str(B * HW))
    _refused(fn(FAKE, FAKE, 1, 65, C.c_int64(16), FAKE, None), "not in [2, 64]")         # (the limit is tested after the class count)


def test_confusion_meter_splits_below_the_limit():
    """The pieces ConfusionMeter hands to the entries: each below 2^24 pixels, contiguous, of the prediction's rank, covering every
    pixel exactly once and in order -- whole images while one fits, else pixel ranges of one image."""
    assert CONFUSION_MAX_PIXELS == (1 << 24) - 1
    for B, H, W, lim in ((1, 4097, 4097, CONFUSION_MAX_PIXELS), (5, 2049, 2049, CONFUSION_MAX_PIXELS), (64, 512, 512, CONFUSION_MAX_PIXELS),
                         (2, 8, 8, CONFUSION_MAX_PIXELS), (3, 5, 7, 34), (3, 5, 7, 35), (3, 5, 7, 36), (3, 5, 7, 70), (2, 5, 7, 4)):
        y = (torch.arange(B * H * W, dtype=torch.int32) % 251).to(torch.uint8).view(B, H, W)
        for pred in (y.view(B, 1, H, W).expand(B, 2, H, W).contiguous(), y.clone()):
            pieces = list(_confusion_calls(pred, y, lim))
            assert all(t.numel() <= lim and p.is_contiguous() and t.is_contiguous() and p.dim() == pred.dim() and t.dim() == 3 and
                       p.shape[0] == t.shape[0] and p.numel() == t.numel() * (2 if pred.dim() == 4 else 1) for p, t in pieces)
            assert torch.equal(torch.cat([t.reshape(-1) for _, t in pieces]), y.reshape(-1))
            if pred.dim() == 4:
                assert all(torch.equal(p[:, c].reshape(-1), t.reshape(-1)) for p, t in pieces for c in range(2))
            else:
                assert all(torch.equal(p.reshape(-1), t.reshape(-1)) for p, t in pieces)
            if B * H * W <= lim:
                assert len(pieces) == 1 and pieces[0][0] is pred
    assert [t.shape[0] for _, t in _confusion_calls(torch.zeros(5, 2049, 2049, dtype=torch.uint8), torch.zeros(5, 2049, 2049, dtype=torch.uint8))] == [3, 2]


# ------------------------------------------------------------------------------------------------------------------------ conv_fwd
def _conv_args(B, H, W, cin, cout, k=1, residual=False, stats=False):
    a = hip.ConvArgs()
    a.B, a.Hout, a.Wout, a.Hin, a.Win = B, H, W, H, W
    a.ksize, a.stride, a.transposed, a.nsrc, a.Cout = k, 1, 0, 1, cout
    a.src[0].ptr, a.src[0].C, a.src[0].cstride = 0x1000, cin, cin
    a.wpack, a.out, a.out_cstride = 0x1000, 0x1000, cout
    if residual:
        a.residual, a.res_cstride = 0x1000, cout
    if stats:
        a.stats, a.stats_mode, a.stats_rep = 0x1000, hip.STATS_SUM_SQ, 1
    a.epilogue, a.mma_dtype, a.act_dtype = hip.EP_LINEAR, hip.F32, hip.F32
    return a


def test_conv_fwd_refuses_2_31_elements():
    lib = hip.load()
    _refused(lib.lmn_conv_fwd(C.byref(_conv_args(2048, 256, 256, 16, 4)), None), "source 0 larger than 2^31 elements")      # exactly 2^31
    _refused(lib.lmn_conv_fwd(C.byref(_conv_args(2048, 256, 256, 4, 16)), None), "output larger than 2^31 elements")
    _refused(lib.lmn_conv_fwd(C.byref(_conv_args(1366, 256, 256, 12, 24)), None), "output larger than 2^31 elements")       # 8 GiB of fp32


def test_conv_chain_predicate_switches_at_0x7fffffff_bytes():
    """lmn_conv_chain_ok is dma1_select, the predicate of the LDS-DMA 1x1 form: every span below 0x7fffffff bytes.  The chained pair of
    kernel_checks.check_conv_dma1 (24 + 12 -> 12 with on-load GELU, then 12 -> 24 with SUM_SQ statistics) at 256 x 256: the widest operand has 24
    channels, 6 MiB per image, so B = 341 (2046 MiB) is taken and B = 342 (2052 MiB) is not."""
    lib = hip.load()

    def ok(B):
        a = _conv_args(B, 256, 256, 24, 12)
        a.nsrc = 2
        a.src[0].flags = hip.SRC_GELU
        a.src[1].ptr, a.src[1].C, a.src[1].cstride = 0x1000, 12, 12
        a.chain.wpack, a.chain.out, a.chain.Cout, a.chain.out_cstride = 0x1000, 0x1000, 24, 24
        a.chain.stats, a.chain.stats_mode, a.chain.stats_rep, a.chain.epilogue = 0x1000, hip.STATS_SUM_SQ, 1, hip.EP_LINEAR
        return lib.lmn_conv_chain_ok(C.byref(a))
    assert ok(8) == 1 and ok(341) == 1
    assert ok(342) == 0 and ok(683) == 0


# ---------------------------------------------------------------------------------------------------------------------- conv_wgrad
def _wgrad_args(B, H, W, cin, cout, k=3, up2=False):
    a = hip.WgradArgs()
    a.B, a.Hout, a.Wout, a.Hin, a.Win = B, H, W, H, W
    a.ksize, a.stride, a.nsrc, a.Cout = k, 1, 1, cout
    a.src[0].ptr, a.src[0].C, a.src[0].cstride = 0x1000, cin, cin
    a.src[0].flags = hip.SRC_UP2 if up2 else 0
    a.dy, a.dy_cstride, a.dW, a.db = 0x1000, cout, 0x1000, 0x1000
    a.mma_dtype, a.act_dtype = hip.F32, hip.F32
    return a


def test_conv_wgrad_refusals():
    lib = hip.load()
    _refused(lib.lmn_conv_wgrad(C.byref(_wgrad_args(2048, 256, 256, 16, 4)), None), "source 0 larger than 2^31 elements")   # exactly 2^31
    _refused(lib.lmn_conv_wgrad(C.byref(_wgrad_args(2048, 256, 256, 4, 16)), None), "dy larger than 2^31 elements")
    # pixel steps: B * ceil(Hout * Wout / 4) reaches 2^31 with 4-channel operands of 2^33 elements each
    _refused(lib.lmn_conv_wgrad(C.byref(_wgrad_args(32768, 512, 512, 4, 4)), None), "too many pixels")


def test_conv_wgrad_up2_names_the_byte_limit():
    """LMN_SRC_UP2 exists in the wgrad3 form only, which is taken while every operand is below 0xfffffff0 bytes (counted at the
    upsampled size): 12 -> 12 over 256 x 256 is 3 MiB per image, so B = 1365 is taken and B = 1366 is not -- the predicate says no
    beforehand, and the entry's refusal names bytes, not the map's width."""
    lib = hip.load()
    assert lib.lmn_conv_wgrad_up2_ok(C.byref(_wgrad_args(8, 256, 256, 12, 12, up2=True))) == 1
    assert lib.lmn_conv_wgrad_up2_ok(C.byref(_wgrad_args(1365, 256, 256, 12, 12, up2=True))) == 1
    assert lib.lmn_conv_wgrad_up2_ok(C.byref(_wgrad_args(1366, 256, 256, 12, 12, up2=True))) == 0
    _refused(lib.lmn_conv_wgrad(C.byref(_wgrad_args(1366, 256, 256, 12, 12, up2=True)), None), "LMN_SRC_UP2", str(1366 * 256 * 256 * 12 * 4) + " bytes",
             "4294967280-byte limit", "lmn_up2_fwd")
    _refused(lib.lmn_conv_wgrad(C.byref(_wgrad_args(8, 16, 16, 12, 12, up2=True)), None), "LMN_SRC_UP2 needs the wgrad3 form")   # width, not size
    # the workspace bound does not depend on B beyond the block cap: the same on both sides of the byte threshold
    ws = [int(lib.lmn_conv_wgrad_workspace(C.byref(_wgrad_args(B, 256, 256, 12, 12)))) for B in (683, 1365, 1366)]
    assert ws[0] == ws[1] == ws[2] > 0


# ------------------------------------------------------------------------------------------------ depthwise, attention, row kernels
def test_depthwise_refuses_2_gib():
    """E = 24 at 128 x 128 is 1.5 MiB per image in fp32: B = 1365 (2047.5 MiB) is the last count accepted, B = 1366 the first refused; bf16
    storage doubles the counts.  (The row offset in soffset counts against the descriptor's 2^31 - 1 records: past 2 GiB every access
    would be out of range -- tests/test_extent_kernels_gpu.py runs the last accepted count.)"""
    lib = hip.load()
    for B, dt in ((1366, hip.F32), (2731, hip.BF16), (2731, hip.F32)):
        words = ("dw_fwd", "%d x 128 x 128 x 24" % B, "below 2 GiB")
        _refused(lib.lmn_dw_fwd(FAKE, FAKE, FAKE, B, 128, 128, 24, FAKE, FAKE, None, None, dt, None), *words)
        _refused(lib.lmn_dw_stats(FAKE, B, 128, 128, 24, FAKE, FAKE, FAKE, FAKE, FAKE, None, dt, None), "dw statistics", words[1], "below 2 GiB")
        _refused(lib.lmn_dw_bwd(FAKE, FAKE, FAKE, B, 128, 128, 24, *([FAKE] * 11), dt, None), "dw_bwd", words[1], "below 2 GiB")


def test_neighborhood_attention_refuses_2_31_items():
    """The item index (pixel x channel quad) is the only limit: 32768 x 256 x 256 pixels of one quad is 2^31 items."""
    lib = hip.load()
    words = ("32768 x 256 x 256 x 4 channels", "32-bit item index")
    _refused(lib.lmn_na_fwd(FAKE, FAKE, FAKE, 32768, 256, 256, 4, 1, 3, C.c_float(1.0), hip.F32, None), *words)
    _refused(lib.lmn_na_bwd(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 32768, 256, 256, 4, 1, 3, C.c_float(1.0), hip.F32, None), *words)


def test_neighborhood_attention_general_path_refuses_2_31_items():
    """A head dim without a channel-quad kernel (here 3) takes the per-head kernels of na_gen.hip, whose item is (pixel, head, half):
    B * H * W * heads * 2 < 2^31, a tighter bound than the quad kernels' B * H * W * C / 4.  4096 x 256 x 256 pixels of 4 heads is the
    first refused extent (2^31 items); the quad kernels would take these 12 channels up to three times as many pixels."""
    lib = hip.load()
    words = ("4096 x 256 x 256 x 4 heads", "32-bit item index")
    _refused(lib.lmn_na_fwd(FAKE, FAKE, FAKE, 4096, 256, 256, 4, 3, 3, C.c_float(1.0), hip.F32, None), "na_fwd", *words)
    _refused(lib.lmn_na_bwd(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 4096, 256, 256, 4, 3, 3, C.c_float(1.0), hip.F32, None), "na_bwd", *words)


def test_global_attention_refuses_65536_images():
    """gattn's only limit by extent: the image (and head) index is a grid dimension."""
    lib = hip.load()
    _refused(lib.lmn_gattn_fwd(FAKE, FAKE, FAKE, 65536, 64, 3, 8, C.c_float(1.0), hip.F32, None), "gattn_fwd", "B=65536 images", "65535")
    _refused(lib.lmn_gattn_bwd(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 65536, 64, 3, 8, C.c_float(1.0), hip.F32, None), "gattn_bwd", "B=65536 images", "65535")


def test_gap_pool_reports_like_guard_pool():
    """extent.gap_pool: the layout of guard.GuardPool, the detector restricted to the gaps between tensors."""
    from guard import GuardPool
    pool = X.gap_pool("cpu", GuardPool.size_for([100, 64, 12]))
    a, b = pool.take("a", (25,)), pool.take("b", (64,), torch.uint8)
    pool.take("c", None, init=torch.ones(3))
    a.fill_(1.0), b.fill_(7)
    assert pool.check() == [] and pool.unchanged("c")
    ea, eb = pool.entries[0], pool.entries[1]
    assert ea[1] % 256 == 0 and eb[1] - (ea[1] + ea[2]) >= 4096
    pool.raw[ea[1] + ea[2]] = 0                     # the first byte past a
    pool.raw[eb[1] - 1] = 3                         # the last byte before b
    pool.raw[-1] = 1                                # the end of the pool
    bad = pool.check()
    assert bad[0][:3] == ("a", "after", 0) and bad[0][3] == eb[1] - 1 - (ea[1] + ea[2]) and bad[1][:2] == ("c", "after")
    with pytest.raises(AssertionError, match="guard bytes damaged"):
        pool.assert_clean()


def test_avgpool_fwd_refuses_2_31_pixels():
    """Both forms of lmn_avgpool_fwd index OUTPUT pixels in 32 bits (the wave form's total, the block form's grid and its blockIdx.x
    decode): 2^31 pixels is the first refused extent, whatever the channel count."""
    lib = hip.load()
    for Cn in (4, 512):
        _refused(lib.lmn_avgpool_fwd(FAKE, FAKE, 32768, 256, 256, 2, Cn, Cn, Cn, hip.F32, None), "avgpool_fwd", "2147483648 output pixels", "2^31 pixels")


def test_row_kernels_refuse_their_row_offsets():
    lib = hip.load()
    # up2_fwd: four source rows' worth of an image, 4 * Win * Hin * cstride elements, must stay below 2^31; and B * 2 * Hin rows
    _refused(lib.lmn_up2_fwd(FAKE, FAKE, 1, 4096, 4096, 32, 32, 32, hip.F32, None), "up2_fwd", "32-bit row offsets")
    _refused(lib.lmn_up2_fwd(FAKE, FAKE, 1 << 20, 1024, 8, 4, 4, 4, hip.F32, None), "up2_fwd", "32-bit row offsets")
    _refused(lib.lmn_up2_bwd(FAKE, FAKE, 1, 8, 1 << 20, 4, 1024, 4, hip.F32, None), "up2_bwd", "32-bit row offsets")
    _refused(lib.lmn_up2_bwd(FAKE, FAKE, 1 << 21, 1024, 8, 4, 4, 4, hip.F32, None), "up2_bwd", "32-bit row offsets")
    _refused(lib.lmn_avgpool_bwd(FAKE, FAKE, 1 << 20, 1024, 8, 2, 4, 4, 4, 0, hip.F32, None), "avgpool_bwd", "32-bit row / column indices")


# -------------------------------------------------------------------------------------------------------------- the helper itself
def test_period_rule():
    # the negative example: power-of-two images with a period of two -- 2^31 bytes away lies the same image
    assert X.period_violations(256 * 256 * 16, 4, period=2) == ["2^31 bytes", "2^31 elements", "2^32 bytes", "2^32 elements"]
    with pytest.raises(AssertionError, match="whole number of periods"):
        X.assert_period("x", 256 * 256 * 16, 4, period=2)
    with pytest.raises(AssertionError, match="whole number of periods"):
        X.fill_periodic(torch.empty(5, 8, 8, 16), torch.zeros(2, 8, 8, 16))
    # P = 3 never divides a power of two: every image of the extent cases passes
    for elements in (256 * 256 * 12, 256 * 256 * 16, 256 * 256 * 24, 128 * 128 * 24, 44 * 44 * 96, 64 * 64 * 36, 1):
        for itemsize in (2, 4, 8):
            assert X.period_violations(elements, itemsize) == []
    assert X.P == 3 and X.counts(10) == [4, 3, 3] and X.counts(3) == [1, 1, 1] and X.counts(2) == [1, 1, 0] and sum(X.counts(1366)) == 1366


@pytest.mark.parametrize("B", [1, 2, 3, 7, 11])
def test_periodic_expectations_equal_a_direct_reference(B):
    """A 3x3 conv with bias over a small periodic batch: per-image outputs and the batch sums from the tile alone equal those of the
    batch spelled out in fp64; rel_periodic scores like kernel_checks.rel, in any chunking, and sees one wrong element."""
    import torch.nn.functional as F
    from kernel_checks import rel
    tile = R(X.P, 4, 6, 5, seed=401) + 2.0
    w, b = R(8, 4, 3, 3, seed=402), R(8, seed=403) + 3.0
    xb = X.fill_periodic(torch.empty(B, 4, 6, 5, dtype=torch.float64), tile)
    assert torch.equal(xb, X.expected_images(tile, B)) and torch.equal(xb[B - 1], tile[(B - 1) % 3])
    direct = F.conv2d(xb, w, b, padding=1)
    ref = F.conv2d(tile, w, b, padding=1)
    assert torch.equal(X.expected_images(ref, B), direct)
    for chunk in (1, 1 << 26):
        assert X.rel_periodic(direct, ref, chunk) == 0.0
    got = direct.float()
    scale = float(direct.abs().max() / ref.abs().max())              # (the score's denominator is the largest element of all P images)
    assert abs(X.rel_periodic(got, ref) - rel(got, direct) * scale) <= 1e-15 and 0 < X.rel_periodic(got, ref) < 1e-6
    assert B < X.P or scale == 1.0
    bad = direct.clone()
    bad[B - 1, 3, 2, 1] += 0.5
    assert abs(X.rel_periodic(bad, ref, 1) - 0.5 / float(ref.abs().max())) < 1e-12 or B < 3      # (B < 3: the reference's max is over all P images)
    assert X.rel_periodic(bad, ref, 1) > 0.01
    bad[0, 0, 0, 0] = float("nan")
    assert X.rel_periodic(bad, ref) == float("inf")
    assert X.rel_periodic(direct[:, :, :5], ref) == float("inf")                                 # another shape
    parts, absol = ref.sum((2, 3)), ref.abs().sum((2, 3))
    want = direct.sum((0, 2, 3))
    assert torch.allclose(X.expected_sum(parts, B), want, rtol=1e-13, atol=0)
    assert X.rel_reduced(want.float(), X.expected_sum(parts, B), X.expected_sum(absol, B)) < 1e-6
    assert X.rel_reduced(torch.full_like(want, float("nan")), X.expected_sum(parts, B), X.expected_sum(absol, B)) == float("inf")


def test_reduction_refuses_a_cancelling_reference():
    parts = torch.tensor([[1.0, -1.0], [-1.0, 1.0], [1e-3, 0.0]], dtype=torch.float64)
    with pytest.raises(AssertionError, match="nearly cancels"):
        X.rel_reduced(torch.zeros(2), X.expected_sum(parts, 6), X.expected_sum(parts.abs(), 6))

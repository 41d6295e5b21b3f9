"""GPU: every kernel family on both sides of each decision that depends on how much data ONE call sees, or -- where a family states
no limit in bytes -- with its main operand past 4 GiB.

Every case is a periodic batch (tests/extent.py): the smallest image of the family's existing check that its forms accept, the batch
count just below / just past the boundary, all operands carved from one guarded pool, the large inputs compared with what was written
into them after the call.  A case ends in exactly one of two ways: the result is right within the family's existing tolerance (1e-4
pointwise, 2e-4 for the reduced sums and for the gradients the existing checks hold to 2e-4; kernel_checks.py), or -- the refusals,
tests/test_extent_cpu.py -- the entry says no before any launch.  Which instance ran is asserted on both sides of a switch.

Images and counts (fp32 unless stated; the LDS-DMA forms take 12 / 24-channel sources, so no operand of theirs can be exactly 2^31
bytes -- 3 * 2^k never is -- and "one byte past the `< 0x7fffffff` predicate" is pinned on the tile kernel with 16-channel calls):

  conv_fwd 1x1 12 -> 24 + SUM_SQ statistics, 256 x 256 (out: 6 MiB per image): B = 341 (2046 MiB, conv_dma1), 342 (first past
      0x7fffffff: conv_tile), 683 (out past 4 GiB)
  conv_fwd 1x1 and 3x3 16 -> 16, 256 x 256 (4 MiB per image and operand): B = 512 (exactly 2^31 bytes); 1x1 also 1025 (past 4 GiB)
  conv_fwd 3x3 12 -> 12, 256 x 256 (3 MiB): B = 682 (2046 MiB, conv_dma3), 683 (conv_tile), 1366 (past 4 GiB); with a residual at
      682 / 683 and with a residual slice of a 48 / 52-channel tensor at 682; stride 2 (12 -> 24) and the transposed form at 1366
  conv_fwd 3x3 96 -> 96, 44 x 44 (726 KiB): B = 2888 (conv_dmaM), 2889 (conv_tileM), 5778 (past 4 GiB)
  conv_wgrad 3x3 12 -> 12, 256 x 256: B = 683 (past 2 GiB: wgrad3_kernel on 32-bit byte offsets), 1365 (4095 MiB, the last count
      wgrad3_kernel takes), 1366 (past 0xfffffff0: wgrad_lds_kernel); the last two also in deterministic mode; at 1366 also the
      materialised route of a refused LMN_SRC_UP2 call (up2_fwd, then the plain gradient)
  conv_wgrad 1x1 12 -> 24, 256 x 256: B = 342 (dy past 2 GiB), 683 (dy past 4 GiB)
  bnact_fwd, bnact_bwd_stats, bnact_bwd, ln_fwd, ln_bwd, copy_slice, colsum, nchw_to_nhwc, nhwc_to_nchw: 1366 images of
      256 x 256 x 12 (4098 MiB)
  up2_fwd / up2_bwd, avgpool_fwd / avgpool_bwd (f = 2): 5462 images with the 128 x 128 x 12 side at 4096.5 MiB
  dw_stats, dw_fwd, dw_bwd_stats, dw_bwd: row-planar 128 x 128 x 24: B = 1365 in fp32 and 2730 in bf16 storage (2047.5 MiB, the last
      counts accepted); dw_fwd_bn and dw_bwd_bn at 1365
  na_fwd / na_bwd, 64 x 64 x 12 heads of dim 1 (qkv 576 KiB): K = 3 LDS-tiled, K = 3 direct, K = 5 at B = 3641 and 7283
  gattn_fwd / gattn_bwd, 484 tokens x 12 heads x 31: B = 1989 (qkv past 4 GiB)

Reading of the address arithmetic, before anything was launched: conv_tile / conv_tileM / wgrad_lds / wgrad_1x1w form 32-bit ELEMENT
offsets from pixel indices that are clamped to 0 before the product (halo and tail lanes load element 0 and discard it), and the
entries refuse 2^31 elements; conv_dma1 / conv_dma3 / conv_dmaM and wgrad3_kernel form 32-bit BYTE offsets inside buffer descriptors
sized to the operand (an offset outside reads 0 / is dropped) and are dispatched only below 0x7fffffff / 0xfffffff0 bytes; the other
families are described at their cases below.  Not from the pool: the scratch the library allocates for itself (the K-split workspace
of conv_wgrad, the deterministic slots), which the C side or a cached torch allocation owns."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import extent as X
from kernel_checks import R, TOL
from kernel_forms import launched

pytestmark = pytest.mark.gpu

RTOL = 2e-4          # atomically reduced sums (kernel_checks.py header)
SHIFT = 3.0          # the bias of the forward cases and the mean of the weight-gradient operands: sums whose addends do not cancel


def _hit(names, prefix):
    return any(n.startswith(prefix) for n in names)


def _forms(names, want, never):
    assert all(_hit(names, p) for p in want) and not any(_hit(names, p) for p in never), (want, never, sorted(names))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _unchanged(name, t, tile):
    """A periodic operand still holds exactly what fill_periodic wrote (GuardPool.assert_inputs_unchanged knows only the tensors taken
    with init=, the small tables): a stray store INTO a large input, 2^31 or 2^32 away from its target, shows here."""
    assert X.rel_periodic(t, tile.to(t.dtype)) == 0.0, "operand %s was changed by the call" % name


@functools.lru_cache(maxsize=2)
def _fwd_ref(k, s, cin, cout, H, W, transposed, residual):
    """fp64 reference of the P tile images (NHWC) and the per-image partials of the SUM_SQ statistics and of their absolute addends."""
    w = R(cout, cin, k, k, seed=302, scale=1.0 / math.sqrt(cin * k * k))
    if transposed:
        x = R(X.P, cout, H, W, seed=301)                                  # (dy of the forward conv: cout channels in, cin out)
        y, b = torch.nn.grad.conv2d_input((X.P, cin, H, W), w, x, stride=s, padding=k // 2), None
    else:
        x = R(X.P, cin, H, W, seed=301)
        b = R(cout, seed=303) + SHIFT
        y = F.conv2d(x, w, b, stride=s, padding=k // 2)
    parts = torch.stack([y.sum((2, 3)), (y * y).sum((2, 3))], 1)          # [P, 2, C]
    absol = torch.stack([y.abs().sum((2, 3)), (y * y).sum((2, 3))], 1)
    res = R(*y.shape, seed=304) if residual else None
    return _nhwc(x), w, b, _nhwc(y if res is None else y + res), parts, absol, None if res is None else _nhwc(res)


FWD = [
    # id, k, s, cin, cout, H, W, B, transposed, residual, statistics, kernel that must run, kernels that must not
    ("1x1 12->24 B=341 dma1", 1, 1, 12, 24, 256, 256, 341, 0, 0, 1, "conv_dma1_kernel<", ("conv_tile",)),
    ("1x1 12->24 B=342 tile", 1, 1, 12, 24, 256, 256, 342, 0, 0, 1, "conv_tile_kernel<1,", ("conv_dma",)),
    ("1x1 12->24 B=683 tile, out past 4 GiB", 1, 1, 12, 24, 256, 256, 683, 0, 0, 1, "conv_tile_kernel<1,", ("conv_dma",)),
    ("1x1 16->16 B=512 tile, exactly 2^31 bytes", 1, 1, 16, 16, 256, 256, 512, 0, 0, 0, "conv_tile_kernel<1,", ("conv_dma",)),
    ("1x1 16->16 B=1025 tile, past 4 GiB", 1, 1, 16, 16, 256, 256, 1025, 0, 0, 0, "conv_tile_kernel<1,", ("conv_dma",)),
    ("3x3 12->12 B=682 dma3", 3, 1, 12, 12, 256, 256, 682, 0, 0, 1, "conv_dma3_kernel<", ("conv_tile",)),
    ("3x3 12->12 B=683 tile", 3, 1, 12, 12, 256, 256, 683, 0, 0, 1, "conv_tile_kernel<9,", ("conv_dma",)),
    ("3x3 12->12 B=1366 tile, past 4 GiB", 3, 1, 12, 12, 256, 256, 1366, 0, 0, 1, "conv_tile_kernel<9,", ("conv_dma",)),
    ("3x3 16->16 B=512 tile, exactly 2^31 bytes", 3, 1, 16, 16, 256, 256, 512, 0, 0, 0, "conv_tile_kernel<9,", ("conv_dma",)),
    ("3x3 12->12 residual B=682 dma3", 3, 1, 12, 12, 256, 256, 682, 0, 1, 0, "conv_dma3_kernel<", ("conv_tile",)),
    ("3x3 12->12 residual B=683 tile", 3, 1, 12, 12, 256, 256, 683, 0, 1, 0, "conv_tile_kernel<9,", ("conv_dma",)),
    ("3x3 s2 12->24 B=1366 tile, source past 4 GiB", 3, 2, 12, 24, 256, 256, 1366, 0, 0, 1, "conv_tile_kernel<9,", ("conv_dma",)),
    ("3x3 12->12 transposed B=1366 tile, past 4 GiB", 3, 1, 12, 12, 256, 256, 1366, 1, 0, 0, "conv_tile_kernel<9,", ("conv_dma",)),
    ("3x3 96->96 B=2888 dmaM", 3, 1, 96, 96, 44, 44, 2888, 0, 0, 0, "conv_dmaM_kernel<", ("conv_tile",)),
    ("3x3 96->96 B=2889 tileM", 3, 1, 96, 96, 44, 44, 2889, 0, 0, 0, "conv_tileM_kernel<9,", ("conv_dma",)),
    ("3x3 96->96 B=5778 tileM, past 4 GiB", 3, 1, 96, 96, 44, 44, 5778, 0, 0, 0, "conv_tileM_kernel<9,", ("conv_dma",)),
]


@pytest.mark.parametrize("case", FWD, ids=[c[0] for c in FWD])
def test_conv_fwd_extent(case):
    from lm_net_amd import hip
    name, k, s, cin, cout, H, W, B, transposed, residual, stats, want, never = case
    x, w, b, y, parts, absol, res = _fwd_ref(k, s, cin, cout, H, W, bool(transposed), bool(residual))
    Ci, Co = x.shape[-1], y.shape[-1]                                     # channels in and out of THIS call
    Hi, Wi, Ho, Wo = x.shape[1], x.shape[2], y.shape[1], y.shape[2]
    wp = (hip.conv_pack_t(w.float().cuda(), k) if transposed else hip.conv_pack(w.float().cuda(), k, [cin]))
    nb = [4 * B * Hi * Wi * Ci, 4 * B * Ho * Wo * Co] + ([4 * B * Ho * Wo * Co] if residual else []) + [wp.numel() * wp.element_size(), 4 * Co, 8 * Co]
    with X.guarded_case(nb) as pool:
        xd = X.fill_periodic(pool.take("x", (B, Hi, Wi, Ci)), x)
        out = pool.take("out", (B, Ho, Wo, Co))                           # (poison: NaN wherever the kernel does not store)
        rd = X.fill_periodic(pool.take("residual", (B, Ho, Wo, Co)), res) if residual else None
        wpd = pool.take("wpack", None, init=wp)
        bd = pool.take("bias", None, init=b.float().cuda()) if b is not None else None
        sd = pool.take("stats", None, init=torch.zeros(2, Co, device="cuda")) if stats else None
        _, names = launched(lambda: hip.conv_fwd([xd], wpd, out, B=B, Hin=Hi, Win=Wi, Hout=Ho, Wout=Wo, Cout=Co, ksize=k, stride=s,
                                                 transposed=transposed, bias=bd, residual=rd, stats=sd,
                                                 stats_mode=hip.STATS_SUM_SQ if stats else hip.STATS_NONE))
        err = X.rel_periodic(out, y)
        print("%s: rel %.3g, launched %s" % (name, err, sorted(names)))
        _forms(names, [want], never)
        assert err <= TOL, (name, err)
        if stats:
            ers = X.rel_reduced(sd, X.expected_sum(parts, B), X.expected_sum(absol, B))
            print("%s: statistics rel %.3g" % (name, ers))
            assert ers <= RTOL, (name, ers)
        pool.assert_inputs_unchanged(skip=("stats",))
        _unchanged("x", xd, x)
        if residual:
            _unchanged("residual", rd, res)


@functools.lru_cache(maxsize=2)
def _wgrad_ref(k, cin, cout, H, W):
    """The P tile images of x and dy (NHWC, both drawn about SHIFT so that no gradient sum cancels) and the fp64 per-image partials of
    dW and db, plain and of the absolute addends."""
    x, dy = R(X.P, cin, H, W, seed=311) + SHIFT, R(X.P, cout, H, W, seed=312) + 0.5 * SHIFT
    gw = lambda a, g: torch.stack([torch.nn.grad.conv2d_weight(a[j:j + 1], (cout, cin, k, k), g[j:j + 1], padding=k // 2) for j in range(X.P)])
    return _nhwc(x), _nhwc(dy), gw(x, dy), gw(x.abs(), dy.abs()), dy.sum((2, 3)), dy.abs().sum((2, 3))


W3, WL, W1 = "wgrad3_kernel<", "wgrad_lds_kernel<9,", "wgrad_1x1w_kernel<"
WGRAD = [
    # id, k, cin, cout, B, deterministic, kernel that must run, kernels that must not
    ("3x3 12->12 B=683 wgrad3, past 2 GiB", 3, 12, 12, 683, 0, W3, (WL,)),
    ("3x3 12->12 B=1365 wgrad3, 4095 MiB", 3, 12, 12, 1365, 0, W3, (WL,)),
    ("3x3 12->12 B=1365 wgrad3, deterministic", 3, 12, 12, 1365, 1, W3, (WL,)),
    ("3x3 12->12 B=1366 lds, past 0xfffffff0", 3, 12, 12, 1366, 0, WL, (W3,)),
    ("3x3 12->12 B=1366 lds, deterministic", 3, 12, 12, 1366, 1, WL, (W3,)),
    ("1x1 12->24 B=342, dy past 2 GiB", 1, 12, 24, 342, 0, W1, (W3, WL)),
    ("1x1 12->24 B=683, dy past 4 GiB", 1, 12, 24, 683, 0, W1, (W3, WL)),
]


@pytest.mark.parametrize("case", WGRAD, ids=[c[0] for c in WGRAD])
def test_conv_wgrad_extent(case):
    from lm_net_amd import hip
    name, k, cin, cout, B, det, want, never = case
    H = W = 256
    x, dy, pw, aw, pb, ab = _wgrad_ref(k, cin, cout, H, W)
    with X.guarded_case([4 * B * H * W * cin, 4 * B * H * W * cout, 4 * cout * cin * k * k, 4 * cout]) as pool:
        xd = X.fill_periodic(pool.take("x", (B, H, W, cin)), x)
        dyd = X.fill_periodic(pool.take("dy", (B, H, W, cout)), dy)
        dW = pool.take("dW", None, init=torch.zeros(cout, cin, k, k, device="cuda"))
        db = pool.take("db", None, init=torch.zeros(cout, device="cuda"))
        was = hip.get_deterministic()
        hip.set_deterministic(bool(det))
        try:
            _, names = launched(lambda: hip.conv_wgrad([xd], dyd, dW, db, B=B, Hin=H, Win=W, Hout=H, Wout=W, Cout=cout, ksize=k))
        finally:
            hip.set_deterministic(was)
        ew = X.rel_reduced(dW, X.expected_sum(pw, B), X.expected_sum(aw, B))
        eb = X.rel_reduced(db, X.expected_sum(pb, B), X.expected_sum(ab, B))
        print("%s: dW rel %.3g, db rel %.3g, launched %s" % (name, ew, eb, sorted(names)))
        _forms(names, [want], never)
        assert ew <= RTOL and eb <= RTOL, (name, ew, eb)
        pool.assert_inputs_unchanged(skip=("dW", "db"))
        _unchanged("x", xd, x), _unchanged("dy", dyd, dy)


# ------------------------------------------------------------------------------------------------------------------------ row kernels
# bnact_fwd, ln_fwd, copy_slice, colsum and the two layout conversions state no limit: by reading, every row, pixel and element index
# of theirs is 64-bit (int64_t loop variables; `x + row * C`), so they are correct at any extent.  One case each with the main operand
# past 4 GiB: 1366 images of 256 x 256 x 12 fp32 (3 MiB each).
ROWS_B, ROWS_H, ROWS_W, ROWS_C = 1366, 256, 256, 12


@functools.lru_cache(maxsize=1)
def _rows_tile():
    return R(X.P, ROWS_H, ROWS_W, ROWS_C, seed=321) + 0.5


def _rows_case(name, out_shape, call, ref, extra=()):
    x = _rows_tile()
    nb = [4 * ROWS_B * x[0].numel(), 4 * ROWS_B * ref[0].numel()] + [4 * t.numel() for t in extra]
    with X.guarded_case(nb) as pool:
        xd = X.fill_periodic(pool.take("x", (ROWS_B,) + tuple(x.shape[1:])), x)
        out = pool.take("out", (ROWS_B,) + tuple(out_shape))
        small = [pool.take("p%d" % i, None, init=t.float().cuda()) for i, t in enumerate(extra)]
        _, names = launched(lambda: call(xd, out, *small))
        err = X.rel_periodic(out, ref)
        print("%s: rel %.3g, launched %s" % (name, err, sorted(names)))
        assert err <= TOL, (name, err)
        pool.assert_inputs_unchanged()
        _unchanged("x", xd, x)


def test_bnact_fwd_extent():
    from lm_net_amd import hip
    a, b = R(ROWS_C, seed=322) + 1.5, R(ROWS_C, seed=323)
    _rows_case("bnact_fwd", (ROWS_H, ROWS_W, ROWS_C), lambda x, y, ad, bd: hip.bnact_fwd(x, ad, bd, y, hip.ACT_NONE), _rows_tile() * a + b, (a, b))


def test_ln_fwd_extent():
    from lm_net_amd import hip
    g, b = R(ROWS_C, seed=324) + 1.5, R(ROWS_C, seed=325)
    ref = F.layer_norm(_rows_tile(), (ROWS_C,), g, b, eps=1e-5)
    _rows_case("ln_fwd", (ROWS_H, ROWS_W, ROWS_C), lambda x, y, gd, bd: hip.ln_fwd(x, gd, bd, y), ref, (g, b))


def test_copy_slice_extent():
    """Channels [4, 12) of the source into a dense 8-channel tensor: the source row stride differs from the destination's."""
    from lm_net_amd import hip
    _rows_case("copy_slice", (ROWS_H, ROWS_W, 8), lambda x, y: hip.copy_slice(hip.V(x, 4, 8), y), _rows_tile()[..., 4:].contiguous())


def test_layout_conversions_extent():
    from lm_net_amd import hip
    nchw = _rows_tile().permute(0, 3, 1, 2).contiguous()
    _rows_case("nhwc_to_nchw", (ROWS_C, ROWS_H, ROWS_W), lambda x, y: hip.nhwc_to_nchw(x, y), nchw)
    x = nchw
    with X.guarded_case([4 * ROWS_B * x[0].numel()] * 2) as pool:
        xd = X.fill_periodic(pool.take("x", (ROWS_B, ROWS_C, ROWS_H, ROWS_W)), x)
        out = pool.take("out", (ROWS_B, ROWS_H, ROWS_W, ROWS_C))
        hip.nchw_to_nhwc(xd, out)
        err = X.rel_periodic(out, _rows_tile())
        print("nchw_to_nhwc: rel %.3g" % err)
        assert err <= TOL, err


@pytest.mark.parametrize("det", [0, 1], ids=["default", "deterministic"])
def test_colsum_extent(det):
    """Column sums over 89.5 M rows (a batch reduction: data drawn about 0.5, so the addends do not cancel)."""
    from lm_net_amd import hip
    x = _rows_tile()
    with X.guarded_case([4 * ROWS_B * x[0].numel(), 4 * ROWS_C]) as pool:
        xd = X.fill_periodic(pool.take("x", (ROWS_B, ROWS_H, ROWS_W, ROWS_C)), x)
        out = pool.take("out", None, init=torch.zeros(ROWS_C, device="cuda"))
        was = hip.get_deterministic()
        hip.set_deterministic(bool(det))
        try:
            hip.colsum(xd, out)
        finally:
            hip.set_deterministic(was)
        err = X.rel_reduced(out, X.expected_sum(x.sum((1, 2)), ROWS_B), X.expected_sum(x.abs().sum((1, 2)), ROWS_B))
        print("colsum det=%d: rel %.3g" % (det, err))
        assert err <= RTOL, err


# -------------------------------------------------------------------------------------------------------------------- depthwise family
# Row-planar tensors of E = 24 channels at 128 x 128: 1.5 MiB per image in fp32.  The row offset travels in soffset, and the range check
# of a raw buffer counts it against the descriptor's num_records (0x7fffffff here): an access is in range while soffset + voffset <
# 2^31 - 1.  The entries used to accept 4 GiB; the first run of these cases at B = 1366 (2049 MiB) found the sums of dw_stats short of
# exactly the last 1 MiB of the tensor (relative error 4.94e-4 in the sums AND the sums of squares: 2/3 of one image in 1366), so the
# entries now refuse 2 GiB and more (tests/test_extent_cpu.py) and B = 1365 (2047.5 MiB), the last count accepted, runs here.  Below
# that, by reading (decode_pair / row_off / soA / soB in dwconv.hip), every product is unsigned and every row index is replaced by a
# row of the same image before the product, and a lane outside the image carries voffset 0x80000000 >= num_records.
DW_B = 1365
DW_E, DW_H, DW_W = 24, 128, 128
DW_PADS = [(2, 2), (1, 1), (1, 0), (0, 1)]


def _to_rp(t):
    """NCHW fp64 -> the ROW-PLANAR memory order of hip.rp4 (per image: [H, E / 4, W, 4]) under the shape [P, H, W, E]."""
    Pn, E, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(Pn, H, W, E // 4, 4).permute(0, 1, 3, 2, 4).contiguous().reshape(Pn, H, W, E)


def _gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


@functools.lru_cache(maxsize=2)
def _dw_ref(bf16=False):
    """The P tile images and every per-image expectation of the four passes, fp64.  Data about positive means (weights, x1, u, the
    coefficients) so that the batch sums do not cancel.  bf16: every ACTIVATION a pass reads (x1; pre and u of dw_bwd_stats; dpre of
    dw_bwd) is rounded to bf16 first, as check_bf16_storage_rows draws them, so only the outputs' rounding separates the bf16-storage
    kernels from this reference."""
    E, H, W = DW_E, DW_H, DW_W
    rd = (lambda t: t.to(torch.bfloat16).double()) if bf16 else (lambda t: t)
    x1 = rd(R(X.P, E, H, W, seed=331) + 1.0).requires_grad_(True)
    ws = [(R(E, 1, 5, 5, seed=332).abs() * 0.2).requires_grad_(True), (R(E, 1, 3, 3, seed=333).abs() * 0.3).requires_grad_(True),
          (R(E, 1, 3, 1, seed=334).abs() * 0.5).requires_grad_(True), (R(E, 1, 1, 3, seed=335).abs() * 0.5).requires_grad_(True)]
    A, shift = R(4, E, seed=336).abs() * 0.3 + 0.1, R(4, E, seed=337) * 0.1 + 0.2
    ys = [F.conv2d(x1, w, None, padding=p, groups=E) for w, p in zip(ws, DW_PADS)]
    pre = sum(A[i].view(1, E, 1, 1) * ys[i] + shift[i].view(1, E, 1, 1) for i in range(4)).detach()
    yd = [y.detach() for y in ys]
    d = dict(x1=x1.detach(), ws=[w.detach() for w in ws], A=A, shift=shift, pre=pre, gsum=_gelu(pre).sum((2, 3)))
    d["stats"] = torch.stack([torch.stack([y.sum((2, 3)), (y * y).sum((2, 3))], 1) for y in yd], 1)            # [P, 4, 2, E]
    d["stats_abs"] = torch.stack([torch.stack([y.abs().sum((2, 3)), (y * y).sum((2, 3))], 1) for y in yd], 1)
    # backward statistics: dpre = (u * s + dm) * gelu'(pre), sums of dpre and dpre * y_b
    u, s, dm = rd(R(X.P, E, H, W, seed=338) + 2.0), R(X.P, E, seed=339).abs() + 0.5, R(X.P, E, seed=340) * 0.01
    d["pre_in"] = rd(pre)                                                  # what dw_bwd_stats reads
    pl = d["pre_in"].clone().requires_grad_(True)
    (_gelu(pl) * (u * s.view(X.P, E, 1, 1) + dm.view(X.P, E, 1, 1))).sum().backward()
    dpre = pl.grad
    d.update(u=u, s=s, dm=dm, dpre=dpre)
    d["bstats"] = torch.stack([dpre.sum((2, 3))] + [(dpre * y).sum((2, 3)) for y in yd], 1)                       # [P, 5, E]
    d["bstats_abs"] = torch.stack([dpre.abs().sum((2, 3))] + [(dpre * y).abs().sum((2, 3)) for y in yd], 1)
    cA, cC, cD = R(4, E, seed=341).abs() * 0.5 + 0.5, R(4, E, seed=342) * 0.05, R(4, E, seed=343) * 0.05 + 0.1
    d["dpre_in"] = rd(dpre)                                                # what dw_bwd reads
    d["ys"] = yd
    dx1, dws, dws_abs = _dw_bwd_ref(d, cA, cC, cD)
    d.update(cA=cA, cC=cC, cD=cD, dx1=dx1, dws=dws, dws_abs=dws_abs)
    return d


def _dw_bwd_ref(d, cA, cC, cD):
    """dx1 and the per-image partials of the four weight gradients (plain and of the absolute addends) of the depthwise backward with
    f_b = cA dpre + cC y_b + cD, which is dL/dy_b of L = sum_b (cA dpre + cD) y_b + cC y_b^2 / 2."""
    E = DW_E
    x1 = d["x1"].clone().requires_grad_(True)
    ws = [w.clone().requires_grad_(True) for w in d["ws"]]
    ys = [F.conv2d(x1, w, None, padding=p, groups=E) for w, p in zip(ws, DW_PADS)]
    v = lambda c, i: c[i].view(1, E, 1, 1)
    fb = [v(cA, i) * d["dpre_in"] + v(cC, i) * ys[i].detach() + v(cD, i) for i in range(4)]
    dx1 = torch.autograd.grad(sum((fb[i] * ys[i]).sum() for i in range(4)), x1, retain_graph=True)[0]
    dws, dws_abs = [], []
    for i in range(4):
        dws.append(torch.stack([torch.autograd.grad((fb[i][j] * ys[i][j]).sum(), ws[i], retain_graph=True)[0] for j in range(X.P)]))
        ya = F.conv2d(x1.detach().abs(), ws[i], None, padding=DW_PADS[i], groups=E)
        dws_abs.append(torch.stack([torch.autograd.grad((fb[i][j].abs() * ya[j]).sum(), ws[i], retain_graph=True)[0] for j in range(X.P)]))
    return dx1, dws, dws_abs


def _dw_small(pool, d):
    return [pool.take("w%d" % i, None, init=w.float().cuda()) for i, w in enumerate(d["ws"])]


def _with_det(det, fn):
    from lm_net_amd import hip
    was = hip.get_deterministic()
    hip.set_deterministic(bool(det))
    try:
        return launched(fn)[1]
    finally:
        hip.set_deterministic(was)


DW_STORE = [(torch.float32, DW_B), (torch.bfloat16, 2 * DW_B)]          # the same bytes in either storage type: 2047.5 MiB
DW_IDS = ["fp32 B=%d" % DW_B, "bf16 B=%d" % (2 * DW_B)]
# bf16 storage: the bounds of check_bf16_storage_rows -- 8e-3 for a tensor rounded to bf16 on output (2^-8 per element), 5e-3 for the
# sums taken of a rounded dpre, 2e-4 for the statistics and weight gradients, which stay fp32
BTOL, BSUM = 8e-3, 5e-3


@pytest.mark.parametrize("dt,B", DW_STORE, ids=DW_IDS)
@pytest.mark.parametrize("det", [0, 1], ids=["default", "deterministic"])
def test_dw_stats_extent(det, dt, B):
    from lm_net_amd import hip
    ES, d = (2 if dt == torch.bfloat16 else 4), _dw_ref(dt == torch.bfloat16)
    nb = ES * B * DW_H * DW_W * DW_E
    with X.guarded_case([nb, 4 * 8 * DW_E] + [4 * w.numel() for w in d["ws"]]) as pool:
        x1 = hip.rp4(X.fill_periodic(pool.take("x1", (B, DW_H, DW_W, DW_E), dt), _to_rp(d["x1"])))
        wd = _dw_small(pool, d)
        stats = pool.take("stats", None, init=torch.zeros(4, 2, DW_E, device="cuda"))
        names = _with_det(det, lambda: hip.dw_stats(x1, *wd, stats))
        want, absol = X.expected_sum(d["stats"], B), X.expected_sum(d["stats_abs"], B)
        e0, e1 = X.rel_reduced(stats[:, 0], want[:, 0], absol[:, 0]), X.rel_reduced(stats[:, 1], want[:, 1], absol[:, 1])
        print("dw_stats B=%d det=%d: sum rel %.3g, sum of squares rel %.3g, launched %s" % (B, det, e0, e1, sorted(names)))
        assert e0 <= RTOL and e1 <= RTOL, (e0, e1)
        pool.assert_inputs_unchanged(skip=("stats",))
        _unchanged("x1", x1, _to_rp(d["x1"]))


@pytest.mark.parametrize("dt,B", DW_STORE, ids=DW_IDS)
def test_dw_fwd_extent(dt, B):
    from lm_net_amd import hip
    ES, d = (2 if dt == torch.bfloat16 else 4), _dw_ref(dt == torch.bfloat16)
    nb = ES * B * DW_H * DW_W * DW_E
    with X.guarded_case([nb, nb, 4 * B * DW_E, 4 * 25 * DW_E, 4 * DW_E]) as pool:
        x1 = hip.rp4(X.fill_periodic(pool.take("x1", (B, DW_H, DW_W, DW_E), dt), _to_rp(d["x1"])))
        pre = hip.rp4(pool.take("pre", (B, DW_H, DW_W, DW_E), dt))
        gsum = pool.take("gsum", None, init=torch.zeros(B, DW_E, device="cuda"))
        keff, beff = torch.empty(DW_E, 25, device="cuda"), torch.empty(DW_E, device="cuda")
        hip.dw_merge(*[w.float().cuda() for w in d["ws"]], d["A"].float().cuda(), d["shift"].float().cuda(), keff, beff)
        keff, beff = pool.take("keff", None, init=keff), pool.take("beff", None, init=beff)
        _, names = launched(lambda: hip.dw_fwd(x1, pre, gsum, keff, beff))
        ep, eg = X.rel_periodic(pre, _to_rp(d["pre"])), X.rel_periodic(gsum, d["gsum"])
        print("dw_fwd B=%d: pre rel %.3g, gsum rel %.3g, launched %s" % (B, ep, eg, sorted(names)))
        assert ep <= (TOL if ES == 4 else BTOL) and eg <= RTOL, (ep, eg)
        pool.assert_inputs_unchanged(skip=("gsum",))
        _unchanged("x1", x1, _to_rp(d["x1"]))


@pytest.mark.parametrize("dt,B", DW_STORE, ids=DW_IDS)
@pytest.mark.parametrize("det", [0, 1], ids=["default", "deterministic"])
def test_dw_bwd_stats_extent(det, dt, B):
    from lm_net_amd import hip
    ES, d = (2 if dt == torch.bfloat16 else 4), _dw_ref(dt == torch.bfloat16)
    nb = ES * B * DW_H * DW_W * DW_E
    with X.guarded_case([nb] * 4 + [4 * B * DW_E] * 2 + [4 * 5 * DW_E] + [4 * w.numel() for w in d["ws"]]) as pool:
        per = lambda name, t: hip.rp4(X.fill_periodic(pool.take(name, (B, DW_H, DW_W, DW_E), dt), _to_rp(t)))
        x1, pre, u = per("x1", d["x1"]), per("pre", d["pre_in"]), per("u", d["u"])
        s, dm = X.fill_periodic(pool.take("s", (B, DW_E)), d["s"]), X.fill_periodic(pool.take("dm", (B, DW_E)), d["dm"])
        dpre = hip.rp4(pool.take("dpre", (B, DW_H, DW_W, DW_E), dt))
        wd = _dw_small(pool, d)
        bstats = pool.take("bstats", None, init=torch.zeros(5, DW_E, device="cuda"))
        names = _with_det(det, lambda: hip.dw_bwd_stats(x1, pre, u, s, dm, dpre, *wd, bstats))
        ed = X.rel_periodic(dpre, _to_rp(d["dpre"]))
        want, absol = X.expected_sum(d["bstats"], B), X.expected_sum(d["bstats_abs"], B)
        es = max(X.rel_reduced(bstats[k], want[k], absol[k]) for k in range(5))
        print("dw_bwd_stats B=%d det=%d: dpre rel %.3g, sums rel %.3g, launched %s" % (B, det, ed, es, sorted(names)))
        assert ed <= (TOL if ES == 4 else BTOL) and es <= (RTOL if ES == 4 else BSUM), (ed, es)
        pool.assert_inputs_unchanged(skip=("bstats",))
        for n_, t_, k_ in (("x1", x1, "x1"), ("pre", pre, "pre_in"), ("u", u, "u")):
            _unchanged(n_, t_, _to_rp(d[k_]))
        _unchanged("s", s, d["s"]), _unchanged("dm", dm, d["dm"])


@pytest.mark.parametrize("dt,B", DW_STORE, ids=DW_IDS)
@pytest.mark.parametrize("det", [0, 1], ids=["default", "deterministic"])
def test_dw_bwd_extent(det, dt, B):
    from lm_net_amd import hip
    ES, d = (2 if dt == torch.bfloat16 else 4), _dw_ref(dt == torch.bfloat16)
    nb = ES * B * DW_H * DW_W * DW_E
    with X.guarded_case([nb] * 3 + [4 * 4 * DW_E] * 3 + [4 * w.numel() for w in d["ws"]] * 2) as pool:
        per = lambda name, t: hip.rp4(X.fill_periodic(pool.take(name, (B, DW_H, DW_W, DW_E), dt), _to_rp(t)))
        x1, dpre = per("x1", d["x1"]), per("dpre", d["dpre_in"])
        dx1 = hip.rp4(pool.take("dx1", (B, DW_H, DW_W, DW_E), dt))
        wd = _dw_small(pool, d)
        cs = [pool.take(n, None, init=d[n].float().cuda()) for n in ("cA", "cC", "cD")]
        dws = [pool.take("dw%d" % i, None, init=torch.zeros_like(w, dtype=torch.float32, device="cuda")) for i, w in enumerate(d["ws"])]
        names = _with_det(det, lambda: hip.dw_bwd(x1, dpre, dx1, *wd, *cs, *dws))
        ex = X.rel_periodic(dx1, _to_rp(d["dx1"]))
        ew = max(X.rel_reduced(dws[i], X.expected_sum(d["dws"][i], B), X.expected_sum(d["dws_abs"][i], B)) for i in range(4))
        print("dw_bwd B=%d det=%d: dx1 rel %.3g, dW rel %.3g, launched %s" % (B, det, ex, ew, sorted(names)))
        assert ex <= (TOL if ES == 4 else BTOL) and ew <= RTOL, (ex, ew)
        pool.assert_inputs_unchanged(skip=tuple("dw%d" % i for i in range(4)))
        _unchanged("x1", x1, _to_rp(d["x1"])), _unchanged("dpre", dpre, _to_rp(d["dpre_in"]))


# ------------------------------------------------------------------------------------------- the residual's bound, counted in elements
@pytest.mark.parametrize("rcs,want,never", [(48, "conv_dma3_kernel<", ("conv_tile",)), (52, None, ())],
                         ids=["res_cstride 48: dma3", "res_cstride 52: refused"])
def test_conv_fwd_wide_residual_extent(rcs, want, never):
    """conv_dma3's predicate bounds source and output in BYTES and the residual in ELEMENTS (< 0x7fffffff).  With the residual a
    12-channel slice of a wider tensor its extent is the largest of the call: 682 images of 256 x 256 keep source and output at
    2046 MiB, and the residual spans 682 * 65536 * res_cstride elements -- 2 145 386 496 at 48: conv_dma3 takes the call, with an
    8 GiB residual.  At 52 (2 324 168 704) it is not the predicate that answers but the entry, which counts res_cstride in its own
    2^31-element limit and refuses: the predicate's residual term can never be the one that decides (it is implied by the entry's)."""
    from lm_net_amd import hip
    B, H, W, Cn = 682, 256, 256, 12
    x, w, b, y0, _, _, _ = _fwd_ref(3, 1, Cn, Cn, H, W, False, False)
    rw = R(X.P, H, W, rcs, seed=305)
    y = y0 + rw[..., 4:4 + Cn]
    wp = hip.conv_pack(w.float().cuda(), 3, [Cn])
    with X.guarded_case([4 * B * H * W * Cn] * 2 + [4 * B * H * W * rcs, wp.numel() * wp.element_size(), 4 * Cn]) as pool:
        xd = X.fill_periodic(pool.take("x", (B, H, W, Cn)), x)
        out = pool.take("out", (B, H, W, Cn))
        rd = X.fill_periodic(pool.take("residual", (B, H, W, rcs)), rw)
        wpd, bd = pool.take("wpack", None, init=wp), pool.take("bias", None, init=b.float().cuda())
        call = lambda: hip.conv_fwd([xd], wpd, out, B=B, Hin=H, Win=W, Hout=H, Wout=W, Cout=Cn, ksize=3, bias=bd, residual=hip.V(rd, 4, Cn))
        if want is None:
            with pytest.raises(RuntimeError, match="larger than 2\\^31 elements"):
                call()
            return
        _, names = launched(call)
        err = X.rel_periodic(out, y)
        print("3x3 12->12 residual slice of %d channels B=%d: rel %.3g, launched %s" % (rcs, B, err, sorted(names)))
        _forms(names, [want], never)
        assert err <= TOL, err
        pool.assert_inputs_unchanged()
        _unchanged("x", xd, x), _unchanged("residual", rd, rw)


# --------------------------------------------------------------------------------------------------------------- neighborhood attention
# 64 x 64 maps, 12 heads of dim 1: qkv is 576 KiB per image; B = 3641 puts it past 2 GiB, B = 7283 past 4 GiB (the only limit is the
# 32-bit item index, B H W C / 4 < 2^31).  By reading na.hip: every image base, pixel offset and statistics offset is formed in 64
# bits from indices that are clamped into the image first -- except, before this change, `dout + pix * C` and `stat + pix * 2 * heads`
# of the K = 3 query pass (int products: wrong from 2^31 elements of dout on, which the item guard admits up to 2^33) and its padded
# trip count; they are 64-bit now.  At the extents here every product stays below 2^31 either way.
NA_H, NA_W, NA_HEADS = 64, 64, 12


@functools.lru_cache(maxsize=1)
def _na_ref(K):
    from oracle import natten_ref
    heads, Cn = NA_HEADS, NA_HEADS
    qkv = R(X.P, NA_H, NA_W, 3 * Cn, seed=351)
    # v rises along x and y: with a positive dout, dp - dsum has one sign per neighbour offset, so the sums of d rpb do not cancel
    qkv[..., 2 * Cn:] += 0.25 * torch.arange(NA_W, dtype=torch.float64).view(1, 1, NA_W, 1) + 0.15 * torch.arange(NA_H, dtype=torch.float64).view(1, NA_H, 1, 1)
    qkv.requires_grad_(True)
    rpb = (R(heads, 2 * K - 1, 2 * K - 1, seed=352) * 0.5).requires_grad_(True)
    q, k, v = qkv.reshape(X.P, NA_H, NA_W, 3, heads, 1).permute(3, 0, 4, 1, 2, 5).unbind(0)
    attn = torch.softmax(natten_ref.na2d_qkrpb(q * 1.0, k, rpb, K), -1)
    o = natten_ref.na2d_av(attn, v, K).permute(0, 2, 3, 1, 4).reshape(X.P, NA_H, NA_W, Cn)
    do = R(X.P, NA_H, NA_W, Cn, seed=353) + 1.0
    dq = torch.autograd.grad(o, qkv, do, retain_graph=True)[0]
    drpb = torch.stack([torch.autograd.grad(o[j], rpb, do[j], retain_graph=True)[0] for j in range(X.P)])
    # the absolute addends of d rpb: one backward per pixel is too many; bound them by the per-image sum of |dattn-logit| instead
    logits = natten_ref.na2d_qkrpb(q * 1.0, k, rpb, K)
    g = torch.autograd.grad(torch.softmax(logits, -1), logits, torch.autograd.grad(o, attn, do, retain_graph=True)[0])[0]   # dL/dlogit [P, heads, H, W, K*K]
    return qkv.detach(), rpb.detach(), o.detach(), do, dq, drpb, g.detach()


def _drpb_abs(g, K):
    """sum over the pixels of |dL/dlogit|, filed under the bias cell each neighbour reads (clamped windows: neighbour n of pixel (y, x)
    sits at offset (sy + ki - y, sx + kj - x)) -> [P, heads, 2K-1, 2K-1]."""
    Pn, heads, H, W, _ = g.shape
    out = torch.zeros(Pn, heads, 2 * K - 1, 2 * K - 1, dtype=torch.float64)
    r = K // 2
    ys, xs = torch.arange(H), torch.arange(W)
    sy, sx = (ys - r).clamp(0, H - K), (xs - r).clamp(0, W - K)
    for ki in range(K):
        for kj in range(K):
            oy, ox = (sy + ki - ys + K - 1), (sx + kj - xs + K - 1)                 # [H], [W] bias rows / columns
            a = g[..., ki * K + kj].abs()                                          # [P, heads, H, W]
            for by in oy.unique():
                for bx in ox.unique():
                    out[:, :, by, bx] += a[:, :, oy == by][:, :, :, ox == bx].sum((2, 3))
    return out


NA_CASES = [(3, False, 3641), (3, False, 7283), (3, True, 3641), (3, True, 7283), (5, False, 3641), (5, False, 7283)]


@pytest.mark.parametrize("K,direct,B", NA_CASES, ids=["K=%d%s B=%d" % (K, " direct" if d else "", B) for K, d, B in NA_CASES])
def test_na_fwd_extent(K, direct, B):
    from lm_net_amd import hip
    qkv, rpb, o, _, _, _, _ = _na_ref(K)
    Cn = NA_HEADS
    with X.guarded_case([4 * B * NA_H * NA_W * 3 * Cn, 4 * B * NA_H * NA_W * Cn, 4 * rpb.numel()]) as pool:
        qd = X.fill_periodic(pool.take("qkv", (B, NA_H, NA_W, 3 * Cn)), qkv)
        out = pool.take("out", (B, NA_H, NA_W, Cn))
        rd = pool.take("rpb", None, init=rpb.float().cuda())
        _, names = launched(lambda: hip.na_fwd(qd, rd, out, NA_HEADS, direct=direct))
        err = X.rel_periodic(out, o)
        print("na_fwd K=%d direct=%d B=%d: rel %.3g, launched %s" % (K, direct, B, err, sorted(names)))
        _forms(names, ["na_fwd_kernel<1, float>"] if K == 3 and not direct else ["na_fwd_gen_kernel<1, float>"],
               ["na_fwd_gen"] if K == 3 and not direct else ["na_fwd_kernel<"])
        assert err <= TOL, err
        pool.assert_inputs_unchanged()
        _unchanged("qkv", qd, qkv)


@pytest.mark.parametrize("K,direct,B", NA_CASES, ids=["K=%d%s B=%d" % (K, " direct" if d else "", B) for K, d, B in NA_CASES])
def test_na_bwd_extent(K, direct, B):
    from lm_net_amd import hip
    qkv, rpb, _, do, dq, drpb, g = _na_ref(K)
    Cn, npx = NA_HEADS, B * NA_H * NA_W
    with X.guarded_case([4 * npx * 3 * Cn] * 2 + [4 * npx * Cn, 4 * npx * 2 * NA_HEADS] + [4 * rpb.numel()] * 2) as pool:
        qd = X.fill_periodic(pool.take("qkv", (B, NA_H, NA_W, 3 * Cn)), qkv)
        dod = X.fill_periodic(pool.take("dout", (B, NA_H, NA_W, Cn)), do)
        dqd = pool.take("dqkv", (B, NA_H, NA_W, 3 * Cn))
        stat = pool.take("stat", (npx * 2 * NA_HEADS,))
        rd = pool.take("rpb", None, init=rpb.float().cuda())
        drd = pool.take("drpb", None, init=torch.zeros(NA_HEADS, 2 * K - 1, 2 * K - 1, device="cuda"))
        _, names = launched(lambda: hip.na_bwd(qd, rd, dod, dqd, drd, NA_HEADS, stat=stat, direct=direct))
        eq = X.rel_periodic(dqd, dq)
        er = X.rel_reduced(drd, X.expected_sum(drpb, B), X.expected_sum(_drpb_abs(g, K), B))
        print("na_bwd K=%d direct=%d B=%d: dqkv rel %.3g, drpb rel %.3g, launched %s" % (K, direct, B, eq, er, sorted(names)))
        _forms(names, ["na_bwd_fused_kernel<1, 3, float>"] if K == 3 and not direct else ["na_bwd_q_gen_kernel<1, float>", "na_bwd_kv_gen_kernel<1, float>"],
               ["na_bwd_q_gen", "na_bwd_kv_gen"] if K == 3 and not direct else ["na_bwd_fused", "na_bwd_q_kernel<", "na_bwd_kv_kernel<"])
        assert eq <= RTOL and er <= RTOL, (eq, er)                           # (dqkv: 2e-4 in check_na as well)
        pool.assert_inputs_unchanged(skip=("drpb",))
        _unchanged("qkv", qd, qkv), _unchanged("dout", dod, do)


# ------------------------------------------------------------------------------------- row kernels with reductions, resampling, pooling
# By reading rows.hip: ln_bwd and chan_kernel (bnact_bwd_stats, bnact_bwd) walk int64 rows (`x + row * C`); up2_fwd / up2_bwd /
# avgpool_bwd keep a 32-bit ROW index (B * 2 Hin, B * Hin, B * Hout * f: refused from 2^31 on) and form every address as
# (int64_t)row * width * cstride; avgpool_fwd keeps a 32-bit output PIXEL index (refused from 2^31 on, by this change) and forms
# addresses in 64 bits.  One case each with the largest operand past 4 GiB.
def _gelu_grad(t):
    tl = t.clone().requires_grad_(True)
    return torch.autograd.grad(_gelu(tl).sum(), tl)[0]


def test_ln_bwd_extent():
    """dx (+ residual gradient) per row; dgamma / dbeta over 89.5 M rows.  x carries a channel ramp, so that xhat -- and with a dy of
    positive mean the addends of dgamma -- keep one sign in the outer channels."""
    from lm_net_amd import hip
    Cn, B = ROWS_C, ROWS_B
    x = (R(X.P, ROWS_H, ROWS_W, Cn, seed=361) + 0.6 * torch.arange(Cn, dtype=torch.float64)).requires_grad_(True)
    g = (R(Cn, seed=362).abs() + 0.5).requires_grad_(True)
    b = R(Cn, seed=363).requires_grad_(True)
    dy, dres = R(X.P, ROWS_H, ROWS_W, Cn, seed=364) + 1.0, R(X.P, ROWS_H, ROWS_W, Cn, seed=365)
    y = F.layer_norm(x, (Cn,), g, b, 1e-5)
    dx = torch.autograd.grad(y, x, dy, retain_graph=True)[0] + dres
    xhat = ((x - x.mean(-1, keepdim=True)) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + 1e-5)).detach()
    pg, pb, ag, ab = (dy * xhat).sum((1, 2)), dy.sum((1, 2)), (dy * xhat).abs().sum((1, 2)), dy.abs().sum((1, 2))
    nb = 4 * B * ROWS_H * ROWS_W * Cn
    with X.guarded_case([nb] * 4 + [4 * Cn] * 3) as pool:
        shape = (B, ROWS_H, ROWS_W, Cn)
        xd, dyd, drd = (X.fill_periodic(pool.take(n, shape), t.detach()) for n, t in (("x", x), ("dy", dy), ("dres", dres)))
        dxd = pool.take("dx", shape)
        gd = pool.take("gamma", None, init=g.detach().float().cuda())
        dg, db = (pool.take(n, None, init=torch.zeros(Cn, device="cuda")) for n in ("dgamma", "dbeta"))
        _, names = launched(lambda: hip.ln_bwd(xd, gd, dyd, drd, dxd, dg, db))
        ex = X.rel_periodic(dxd, dx.detach())
        eg, eb = X.rel_reduced(dg, X.expected_sum(pg, B), X.expected_sum(ag, B)), X.rel_reduced(db, X.expected_sum(pb, B), X.expected_sum(ab, B))
        print("ln_bwd: dx rel %.3g, dgamma rel %.3g, dbeta rel %.3g, launched %s" % (ex, eg, eb, sorted(names)))
        assert ex <= TOL and eg <= RTOL and eb <= RTOL, (ex, eg, eb)
        pool.assert_inputs_unchanged(skip=("dgamma", "dbeta"))
        _unchanged("x", xd, x.detach()), _unchanged("dy", dyd, dy), _unchanged("dres", drd, dres)


def test_bnact_bwd_extent():
    """bnact_bwd_stats (sum dh, sum dh zhat over the rows) and bnact_bwd (dz = c1 dh - c2 - zhat c3) with GELU, from given statistics
    and coefficients (the per-row arithmetic does not know where they come from).  dy has a positive mean and the given mean lies
    below the data's, so neither sum cancels."""
    from lm_net_amd import hip
    Cn, B = ROWS_C, ROWS_B
    z, dy = R(X.P, ROWS_H, ROWS_W, Cn, seed=371) * 1.3 + 0.2, R(X.P, ROWS_H, ROWS_W, Cn, seed=372) + 2.0
    mean, rstd = R(Cn, seed=373) * 0.1 - 1.5, R(Cn, seed=374).abs() * 0.2 + 0.6
    ga, be = R(Cn, seed=375).abs() + 0.5, R(Cn, seed=376) * 0.3 + 0.5
    c1, c2, c3 = R(Cn, seed=377).abs() + 0.5, R(Cn, seed=378) * 0.1, R(Cn, seed=379) * 0.1
    zh = (z - mean) * rstd
    dh = dy * _gelu_grad(ga * zh + be)
    dz = c1 * dh - c2 - zh * c3
    parts, absol = torch.stack([dh.sum((1, 2)), (dh * zh).sum((1, 2))], 1), torch.stack([dh.abs().sum((1, 2)), (dh * zh).abs().sum((1, 2))], 1)
    nb = 4 * B * ROWS_H * ROWS_W * Cn
    with X.guarded_case([nb] * 3 + [4 * Cn] * 9) as pool:
        shape = (B, ROWS_H, ROWS_W, Cn)
        zd, dyd = X.fill_periodic(pool.take("z", shape), z), X.fill_periodic(pool.take("dy", shape), dy)
        dzd = pool.take("dz", shape)
        sm = {n: pool.take(n, None, init=t.float().cuda()) for n, t in (("mean", mean), ("rstd", rstd), ("gamma", ga), ("beta", be), ("c1", c1), ("c2", c2), ("c3", c3))}
        st = pool.take("stats", None, init=torch.zeros(2, Cn, device="cuda"))
        _, names = launched(lambda: (hip.bnact_bwd_stats(zd, dyd, sm["mean"], sm["rstd"], sm["gamma"], sm["beta"], st, hip.ACT_GELU),
                                     hip.bnact_bwd(zd, dyd, sm["mean"], sm["rstd"], sm["gamma"], sm["beta"], sm["c1"], sm["c2"], sm["c3"], dzd, hip.ACT_GELU)))
        want, ab = X.expected_sum(parts, B), X.expected_sum(absol, B)
        es = max(X.rel_reduced(st[k], want[k], ab[k]) for k in range(2))
        ez = X.rel_periodic(dzd, dz)
        print("bnact_bwd_stats: sums rel %.3g; bnact_bwd: dz rel %.3g; launched %s" % (es, ez, sorted(names)))
        assert es <= RTOL and ez <= RTOL, (es, ez)                           # (dz: 2e-4 in check_bn_tail as well)
        pool.assert_inputs_unchanged(skip=("stats",))
        _unchanged("z", zd, z), _unchanged("dy", dyd, dy)


UP_B, UP_H, UP_W, UP_C = 5462, 64, 64, 12        # the upsampled side: 128 x 128 x 12 = 768 KiB per image, 4096.5 MiB in all


def test_up2_extent():
    """Bilinear x2 (align_corners) and its adjoint with the upsampled tensor past 4 GiB."""
    from lm_net_amd import hip
    x = R(X.P, UP_C, UP_H, UP_W, seed=381).requires_grad_(True)
    y = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    dy = R(*y.shape, seed=382)
    dx = torch.autograd.grad(y, x, dy)[0]
    xs, ys_ = (UP_B, UP_H, UP_W, UP_C), (UP_B, 2 * UP_H, 2 * UP_W, UP_C)
    with X.guarded_case([4 * UP_B * UP_H * UP_W * UP_C, 16 * UP_B * UP_H * UP_W * UP_C]) as pool:
        xd = X.fill_periodic(pool.take("x", xs), _nhwc(x.detach()))
        yd = pool.take("y", ys_)
        hip.up2_fwd(xd, yd)
        e = X.rel_periodic(yd, _nhwc(y.detach()))
        print("up2_fwd: rel %.3g" % e)
        assert e <= TOL, e
        _unchanged("x", xd, _nhwc(x.detach()))
    with X.guarded_case([16 * UP_B * UP_H * UP_W * UP_C, 4 * UP_B * UP_H * UP_W * UP_C]) as pool:
        dyd = X.fill_periodic(pool.take("dy", ys_), _nhwc(dy))
        dxd = pool.take("dx", xs)
        hip.up2_bwd(dyd, dxd)
        e = X.rel_periodic(dxd, _nhwc(dx))
        print("up2_bwd: rel %.3g" % e)
        assert e <= TOL, e
        _unchanged("dy", dyd, _nhwc(dy))


def test_avgpool_extent():
    """Average pooling by 2 and its adjoint (overwriting and accumulating) with the full-resolution tensor past 4 GiB."""
    from lm_net_amd import hip
    B, Ho, Wo, Cn, f = UP_B, UP_H, UP_W, UP_C, 2
    x = R(X.P, Cn, Ho * f, Wo * f, seed=391).requires_grad_(True)
    y = F.avg_pool2d(x, f)
    dy, base = R(*y.shape, seed=392), R(X.P, Cn, Ho * f, Wo * f, seed=393)
    dx = torch.autograd.grad(y, x, dy)[0]
    big, small = (B, Ho * f, Wo * f, Cn), (B, Ho, Wo, Cn)
    nbig, nsmall = 4 * B * Ho * f * Wo * f * Cn, 4 * B * Ho * Wo * Cn
    with X.guarded_case([nbig, nsmall]) as pool:
        xd = X.fill_periodic(pool.take("x", big), _nhwc(x.detach()))
        yd = pool.take("y", small)
        _, names = launched(lambda: hip.avgpool_fwd(xd, yd, f))
        e = X.rel_periodic(yd, _nhwc(y.detach()))
        print("avgpool_fwd: rel %.3g, launched %s" % (e, sorted(names)))
        assert e <= TOL, e
        _unchanged("x", xd, _nhwc(x.detach()))
    for acc in (False, True):
        with X.guarded_case([nsmall, nbig]) as pool:
            dyd = X.fill_periodic(pool.take("dy", small), _nhwc(dy))
            dxd = pool.take("dx", big)
            if acc:
                X.fill_periodic(dxd, _nhwc(base))
            hip.avgpool_bwd(dyd, dxd, f, acc)
            e = X.rel_periodic(dxd, _nhwc(dx + base if acc else dx))
            print("avgpool_bwd accumulate=%d: rel %.3g" % (acc, e))
            assert e <= TOL, e
            _unchanged("dy", dyd, _nhwc(dy))


def test_up2_materialised_wgrad_extent():
    """Where LMN_SRC_UP2 is refused by size (1366 images of 256 x 256 x 12: past 0xfffffff0 bytes at the upsampled size) the engine's
    other route must be right: up2_fwd into a materialised map, then the plain 3x3 weight gradient (wgrad_lds_kernel at this extent)."""
    from lm_net_amd import hip
    B, H, W, Cn = 1366, 256, 256, 12
    xs = R(X.P, Cn, H // 2, W // 2, seed=395) + SHIFT
    dy = R(X.P, Cn, H, W, seed=396) + 0.5 * SHIFT
    up = F.interpolate(xs, scale_factor=2, mode="bilinear", align_corners=True)
    gw = lambda a, g: torch.stack([torch.nn.grad.conv2d_weight(a[j:j + 1], (Cn, Cn, 3, 3), g[j:j + 1], padding=1) for j in range(X.P)])
    pw, aw, pb, ab = gw(up, dy), gw(up.abs(), dy.abs()), dy.sum((2, 3)), dy.abs().sum((2, 3))
    nb = 4 * B * H * W * Cn
    with X.guarded_case([nb // 4, nb, nb, 4 * Cn * Cn * 9, 4 * Cn]) as pool:
        xd = X.fill_periodic(pool.take("x", (B, H // 2, W // 2, Cn)), _nhwc(xs))
        dyd = X.fill_periodic(pool.take("dy", (B, H, W, Cn)), _nhwc(dy))
        upd = pool.take("up", (B, H, W, Cn))
        dW = pool.take("dW", None, init=torch.zeros(Cn, Cn, 3, 3, device="cuda"))
        db = pool.take("db", None, init=torch.zeros(Cn, device="cuda"))
        assert not hip.conv_wgrad_up2_ok(xd, dyd, B=B, Hin=H, Win=W, Cout=Cn)
        with pytest.raises(RuntimeError, match="4294967280-byte limit"):
            hip.conv_wgrad([dict(view=xd, flags=hip.SRC_UP2)], dyd, dW, db, B=B, Hin=H, Win=W, Hout=H, Wout=W, Cout=Cn, ksize=3)
        _, names = launched(lambda: (hip.up2_fwd(xd, upd), hip.conv_wgrad([upd], dyd, dW, db, B=B, Hin=H, Win=W, Hout=H, Wout=W, Cout=Cn, ksize=3)))
        eu = X.rel_periodic(upd, _nhwc(up))
        ew = X.rel_reduced(dW, X.expected_sum(pw, B), X.expected_sum(aw, B))
        eb = X.rel_reduced(db, X.expected_sum(pb, B), X.expected_sum(ab, B))
        print("materialised UP2 route: up rel %.3g, dW rel %.3g, db rel %.3g, launched %s" % (eu, ew, eb, sorted(names)))
        _forms(names, ["up2_fwd_kernel<", WL], [W3])
        assert eu <= TOL and ew <= RTOL and eb <= RTOL, (eu, ew, eb)
        _unchanged("x", xd, _nhwc(xs)), _unchanged("dy", dyd, _nhwc(dy))


# --------------------------------------------------------------------------------------------------------------------- global attention
# gattn.hip forms every offset in 64 bits from (image, head, row) and has no limit in bytes; the image index is a grid dimension
# (65535 images at most: refused above, tests/test_extent_cpu.py).  N = 484 tokens, 12 heads of dim 31 (the widest map of check_gattn):
# qkv is 2.06 MiB per image, past 4 GiB at 1989 images.
def test_gattn_extent():
    from lm_net_amd import hip
    B, N, heads, hd = 1989, 484, 12, 31
    Cn = heads * hd
    qkv = (R(X.P, N, 3 * Cn, seed=401) * 0.7).requires_grad_(True)
    q, k, v = qkv.view(X.P, N, 3, heads, hd).permute(2, 0, 3, 1, 4).unbind(0)
    o = (torch.softmax((q @ k.transpose(-2, -1)) * hd ** -0.5, -1) @ v).transpose(1, 2).reshape(X.P, N, Cn)
    do = R(X.P, N, Cn, seed=402)
    dq = torch.autograd.grad(o, qkv, do)[0]
    with X.guarded_case([4 * B * N * 3 * Cn] * 2 + [4 * B * N * Cn] * 2 + [4 * B * heads * N] * 2) as pool:
        qd = X.fill_periodic(pool.take("qkv", (B, N, 3 * Cn)), qkv.detach())
        dod = X.fill_periodic(pool.take("dout", (B, N, Cn)), do)
        out, dqd = pool.take("out", (B, N, Cn)), pool.take("dqkv", (B, N, 3 * Cn))
        lse, delta = pool.take("lse", (B, heads, N)), pool.take("delta", (B, heads, N))
        _, names = launched(lambda: (hip.gattn_fwd(qd, out, lse, heads), hip.gattn_bwd(qd, out, dod, lse, dqd, delta, heads)))
        eo, eq = X.rel_periodic(out, o.detach()), X.rel_periodic(dqd, dq)
        print("gattn B=%d: out rel %.3g, dqkv rel %.3g, launched %s" % (B, eo, eq, sorted(names)))
        assert eo <= TOL and eq <= RTOL, (eo, eq)                            # (dqkv: 2e-4 in check_gattn as well)
        _unchanged("qkv", qd, qkv.detach()), _unchanged("dout", dod, do)


# ------------------------------------------------------------------------------ the one-launch depthwise forms (BatchNorm bookkeeping inside)
class _BN:   # the attributes hip.dw_fwd_bn reads of a BatchNorm2d
    def __init__(self, g, b, E):
        self.weight, self.bias = g.float().cuda(), b.float().cuda()
        self.running_mean, self.running_var, self.eps, self.momentum = torch.zeros(E, device="cuda"), torch.ones(E, device="cuda"), 1e-5, 0.1


def test_dw_bn_forms_extent():
    """dw_fwd_bn (finalise the batch statistics, merge the four branches, forward) and dw_bwd_bn (coefficients from the backward sums,
    backward) at 1365 images: the statistics handed in are the fp64 sums of the periodic batch, and the references form mean, rstd, A,
    shift and the coefficients from them in fp64 (lmn_dw_bwd_coef's arithmetic: T = (S1 - mu S0) rstd, c = -A T rstd / N,
    d = -A S0 / N - c mu; dgamma = T, dbeta = S0)."""
    from lm_net_amd import hip
    d, B, E = _dw_ref(False), DW_B, DW_E
    N = B * DW_H * DW_W
    # (the backward sums handed in are a twentieth of the batch's own: with the consistent ones f_b is the BatchNorm adjoint, orthogonal
    #  to 1 and to y_b, and the weight-gradient sums would cancel to 1-3 % of their absolute addends; the kernel forms its
    #  coefficients from whatever sums it is given)
    st, bst = X.expected_sum(d["stats"], B), 0.05 * X.expected_sum(d["bstats"], B)   # [4, 2, E], [5, E]
    gam, bet = [R(E, seed=411 + i).abs() + 0.5 for i in range(4)], [R(E, seed=415 + i) * 0.1 for i in range(4)]
    mean = st[:, 0] / N
    rstd = 1.0 / torch.sqrt(st[:, 1] / N - mean * mean + 1e-5)
    A = torch.stack(gam) * rstd
    shift = torch.stack(bet) - mean * A
    v = lambda c, i: c[i].view(1, E, 1, 1)
    pre = sum(v(A, i) * d["ys"][i] + v(shift, i) for i in range(4))
    T = (bst[1:] - mean * bst[0]) * rstd
    cC = -A * T * rstd / N
    cD = -A * bst[0] / N - cC * mean
    dx1, dws, dws_abs = _dw_bwd_ref(d, A, cC, cD)
    nb = 4 * B * DW_H * DW_W * E
    with X.guarded_case([nb, nb, 4 * B * E, 4 * 8 * E] + [4 * 4 * E] * 3 + [4 * w.numel() for w in d["ws"]]) as pool:
        x1 = hip.rp4(X.fill_periodic(pool.take("x1", (B, DW_H, DW_W, E)), _to_rp(d["x1"])))
        pd = hip.rp4(pool.take("pre", (B, DW_H, DW_W, E)))
        gsum = pool.take("gsum", None, init=torch.zeros(B, E, device="cuda"))
        sd = pool.take("stats", None, init=st.float().cuda())
        m, r, Ad = (pool.take(n, (4, E)) for n in ("mean", "rstd", "A"))
        wd = _dw_small(pool, d)
        bns = [_BN(gam[i], bet[i], E) for i in range(4)]
        _, names = launched(lambda: hip.dw_fwd_bn(x1, pd, gsum, sd, N, bns, wd, m, r, Ad))
        ep, eg = X.rel_periodic(pd, _to_rp(pre)), X.rel_periodic(gsum, _gelu(pre).sum((2, 3)))
        from kernel_checks import rel
        ec = max(rel(m, mean), rel(r, rstd), rel(Ad, A))
        print("dw_fwd_bn B=%d: pre rel %.3g, gsum rel %.3g, mean / rstd / A rel %.3g, launched %s" % (B, ep, eg, ec, sorted(names)))
        assert ep <= TOL and eg <= RTOL and ec <= TOL, (ep, eg, ec)
        _unchanged("x1", x1, _to_rp(d["x1"]))
    with X.guarded_case([nb] * 3 + [4 * 5 * E] + [4 * 4 * E] * 3 + [4 * E] * 8 + [4 * w.numel() for w in d["ws"]] * 2) as pool:
        per = lambda name, t: hip.rp4(X.fill_periodic(pool.take(name, (B, DW_H, DW_W, E)), _to_rp(t)))
        x1, dpre = per("x1", d["x1"]), per("dpre", d["dpre_in"])
        dxd = hip.rp4(pool.take("dx1", (B, DW_H, DW_W, E)))
        wd = _dw_small(pool, d)
        bsd = pool.take("bstats", None, init=bst.float().cuda())
        m, r, Ad = (pool.take(n, None, init=t.float().cuda()) for n, t in (("mean", mean), ("rstd", rstd), ("A", A)))
        dgs = [pool.take("dg%d" % i, None, init=torch.zeros(E, device="cuda")) for i in range(4)]
        dbs = [pool.take("db%d" % i, None, init=torch.zeros(E, device="cuda")) for i in range(4)]
        dwd = [pool.take("dw%d" % i, None, init=torch.zeros_like(w, dtype=torch.float32, device="cuda")) for i, w in enumerate(d["ws"])]
        _, names = launched(lambda: hip.dw_bwd_bn(x1, dpre, dxd, *wd, bsd, m, r, Ad, N, True, dgs, dbs, *dwd))
        ex = X.rel_periodic(dxd, _to_rp(dx1))
        ew = max(X.rel_reduced(dwd[i], X.expected_sum(dws[i], B), X.expected_sum(dws_abs[i], B)) for i in range(4))
        from kernel_checks import rel
        eg = max(max(rel(dgs[i], T[i]), rel(dbs[i], bst[0])) for i in range(4))
        print("dw_bwd_bn B=%d: dx1 rel %.3g, dW rel %.3g, dgamma / dbeta rel %.3g, launched %s" % (B, ex, ew, eg, sorted(names)))
        assert ex <= TOL and ew <= RTOL and eg <= RTOL, (ex, ew, eg)
        _unchanged("x1", x1, _to_rp(d["x1"])), _unchanged("dpre", dpre, _to_rp(d["dpre_in"]))

"""GPU: the wave mappings of wgrad3_kernel's 2 x 2-tile blocks (conv_wgrad.hip) against fp64 F.conv2d autograd.

A block whose tile set reaches past the channel count has 1 or 2 valid tiles instead of 4; the waves of the other slots take some of the
nine taps of a valid tile, over every K step, so no sum changes its order.  Channel pairs and maps (wgrad_fill_cases.py) are
the smallest that reach every mapping: sets with 2x2, 2x1, 1x2 and 1x1 valid tiles, a partly filled channel tile, one pixel tile and
partial tiles with an image change inside a block's tile range, the atomics and the two-stage reduction.

Tolerances are those of the checks that own the same comparison in kernel_checks.py: 2e-4 for dW and db in fp32 (check_conv_wgrad,
check_conv_up2), 2e-4 with bf16-representable operands in the bf16 modes and 1e-2 where the bilinear x2 sample is rounded to bf16
(check_conv3_storage)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu


def _check(c, want, tol=2e-4):
    import wgrad_fill_cases as wf
    from kernel_checks import rel
    dW, db, names = wf.run(c)
    torch.cuda.synchronize()
    w3 = sorted(n for n in names if n.startswith(("wgrad3_kernel<", "wgrad_lds_kernel<")))
    assert w3 == [want], "launched %s, expected %s alone" % (sorted(names), want)
    rW, rb = wf.reference(c)
    eW = rel(dW, rW)
    eb = rel(db, rb) if db is not None else 0.0
    print("%s: dW %.3e db %.3e (tol %.1e)" % (c, eW, eb, tol))
    assert eW <= tol and eb <= tol, "%s: dW %.3e db %.3e > %.1e" % (c, eW, eb, tol)


PAIRS = [(48, 48), (48, 32), (32, 48), (36, 72), (20, 48)]


@pytest.mark.parametrize("B,H,W", [(1, 32, 32), (2, 33, 40)])
@pytest.mark.parametrize("cout,cin", PAIRS)
def test_fp32(cout, cin, B, H, W):
    from wgrad_fill_cases import case
    _check(case(cout, cin, B, H, W), "wgrad3_kernel<2, 2, 0, false>")


@pytest.mark.parametrize("cout,cin", PAIRS)
def test_fp32_no_bias_gradient(cout, cin):
    from wgrad_fill_cases import case
    _check(case(cout, cin, 1, 32, 32, bias=False), "wgrad3_kernel<2, 2, 0, false>")


@pytest.mark.parametrize("B,H,W", [(1, 32, 32), (2, 33, 40)])
def test_two_sources(B, H, W):
    """12 + 24 channels: 1 + 2 cin tiles, the second set holds the last tile of the second source alone."""
    from wgrad_fill_cases import case
    _check(case(48, (12, 24), B, H, W), "wgrad3_kernel<2, 2, 0, false>")


def test_dropout_on_load():
    from wgrad_fill_cases import case
    _check(case(48, 48, 2, 33, 40, drop=True), "wgrad3_kernel<2, 2, 0, false>")


@pytest.mark.parametrize("cout,cin,B,h,w", [(48, 48, 1, 16, 16), (48, 32, 1, 16, 16), (32, 48, 1, 16, 16), (20, 48, 1, 16, 16), (48, 48, 2, 17, 20), (36, 72, 2, 17, 20)])
def test_up2_source(cout, cin, B, h, w):
    from wgrad_fill_cases import case
    _check(case(cout, cin, B, h, w, up=True), "wgrad3_kernel<2, 2, 0, true>")


@pytest.mark.parametrize("pm", [1, 2])
@pytest.mark.parametrize("cout,cin", PAIRS)
def test_bf16_modes(cout, cin, pm):
    from wgrad_fill_cases import case
    _check(case(cout, cin, 2, 33, 40, pm=pm), "wgrad3_kernel<2, 2, %d, false>" % pm)


@pytest.mark.parametrize("pm", [1, 2])
def test_bf16_modes_one_pixel_tile(pm):
    """B = 1, 32 x 32: one pixel tile a block at most, 8 K steps of 16 pixels (four mfma_bf16x2 pairs, no odd last step)."""
    from wgrad_fill_cases import case
    _check(case(48, 48, 1, 32, 32, pm=pm), "wgrad3_kernel<2, 2, %d, false>" % pm)


@pytest.mark.parametrize("pm", [1, 2])
def test_bf16_modes_up2_source(pm):
    from wgrad_fill_cases import case
    _check(case(48, 48, 2, 17, 20, pm=pm, up=True), "wgrad3_kernel<2, 2, %d, true>" % pm, tol=1e-2)


@pytest.mark.parametrize("c", [(48, 48, 1, 16, 16, 1), (48, 24, 1, 32, 32, 2)])
def test_lds_kernel(c):
    """The general LDS-staged kernel keeps its mapping (every wave walks all four slots of a set): 3 x 3 tiles on a 16 x 16 map, and the
    stride-2 24 -> 48 conv from 32 x 32."""
    from wgrad_fill_cases import case
    cout, cin, B, H, W, st = c
    _check(case(cout, cin, B, H, W, stride=st), "wgrad_lds_kernel<9, 2, 2, 0>")


def test_deterministic_mode_is_bit_identical():
    import wgrad_fill_cases as wf
    a, _ = wf.run_switch_cases()
    b, _ = wf.run_switch_cases()
    for c, x, y in zip(wf.SWITCH_CASES, a, b):
        assert torch.equal(x, y), "%s: two launches differ in deterministic mode" % (c,)


def test_switch(tmp_path):
    """LMN_WGRAD_FILL=0 (a child process: the switch is read once) against the default.  Both meet the reference -- with the same bits:
    a tap of a tile is summed by one wave over every K step in either mapping.  The switch is seen in the block partials: with one wave
    per slot every float of them is written, by default the floats of the slots past the channel count are not."""
    import wgrad_fill_cases as wf
    from kernel_checks import rel
    assert os.environ.get("LMN_WGRAD_FILL", "1") != "0", "this test compares the default with LMN_WGRAD_FILL=0"
    out = str(tmp_path / "fill0.pt")
    env = dict(os.environ, LMN_WGRAD_FILL="0")
    subprocess.run([sys.executable, wf.__file__, out], env=env, check=True, timeout=300)
    off, holes_off = torch.load(out)
    on, holes_on = wf.run_switch_cases()
    for c, x0, x1 in zip(wf.SWITCH_CASES, off, on):
        tol = 1e-2 if (c[5] and c[6]) else 2e-4
        rW, _ = wf.reference(c)
        e0, e1 = rel(x0, rW), rel(x1, rW)
        print("%s: switch off %.3e, default %.3e (tol %.1e)" % (c, e0, e1, tol))
        assert e0 <= tol and e1 <= tol
        assert torch.equal(x0, x1), "%s: the two wave mappings differ in their bits" % (c,)
    print("floats of the block partials left unwritten: switch off %d, default %d" % (holes_off, holes_on))
    assert holes_off == 0, "LMN_WGRAD_FILL=0: %d floats of the block partials unwritten" % holes_off
    assert holes_on > 0, "default: every float of the block partials was written -- the empty slots still have waves"

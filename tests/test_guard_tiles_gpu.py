"""GPU: the entries of include/tiles/lmnet_tiles.h inside guard bands (tests/guard.py): the guard manifest's test of these entries.
Every buffer of lmn_tile_gather and lmn_tile_blend -- the source, the gathered tiles, the tile outputs, the two window tables, the map
and the labels -- is carved from a GuardPool at its exact size, canaries flush against each."""
import numpy as np
import pytest
import torch

import tiles_ref as R
from guard import GuardPool, LaunchLog

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.mark.parametrize("H,W,pad", [(33, 47, "zero"), (20, 70, "reflect")])
def test_gather_and_blend_entries(H, W, pad):
    """33x47: the last tile of both axes pulled back by an odd amount; 20x70: the rows padded up to one tile.  Tile 32x32, stride 16,
    F = 4, C = 3, two images; the gather is issued for all entries, the blend with labels."""
    from lm_net_amd import hip
    B, ch, C, tile, stride, flips = 2, 3, 3, (32, 32), (16, 16), ("h", "v", "hv")
    p_src = hip.tile_param(B, ch, H, W, tile, stride, pad, flips)
    p_out = hip.tile_param(B, C, H, W, tile, stride, pad, flips, "softmax")
    n = B * hip.tile_entries(p_src)
    assert n == B * len(R.axis(H, 32, 16)[2]) * len(R.axis(W, 32, 16)[2]) * 4
    inputs = dict(src=torch.from_numpy(R.seeded((B, ch, H, W), 1)), z=torch.from_numpy(R.seeded((n, C, 32, 32), 2)),
                  wy=torch.from_numpy(R.window(32, "gaussian")), wx=torch.from_numpy(R.window(32, "gaussian")))
    outputs = dict(tiles=((n, ch, 32, 32), torch.float32), map=((B, C, H, W), torch.float32), labels=((B, H, W), torch.uint8))

    def run(t):
        hip.tile_gather(t["src"], p_src, 0, n, t["tiles"])
        hip.tile_blend(t["z"], p_out, t["wy"], t["wx"], t["map"], t["labels"])
        torch.cuda.synchronize()

    plain = {k: v.to(DEV) for k, v in inputs.items()}
    plain.update({k: torch.empty(s, dtype=dt, device=DEV) for k, (s, dt) in outputs.items()})
    run(plain)
    sizes = [v.numel() * v.element_size() for v in plain.values()]
    pool = GuardPool(DEV, GuardPool.size_for(sizes))
    guarded = {k: pool.take(k, None, None, init=v.to(DEV)) for k, v in inputs.items()}
    guarded.update({k: pool.take(k, s, dt) for k, (s, dt) in outputs.items()})
    with LaunchLog(pool) as log:
        run(guarded)
    pool.assert_clean("tile entries")
    pool.assert_inputs_unchanged()
    assert log.names == ["tile_gather", "tile_blend"]
    got = {e[0]: e[2] for e in pool.entries}
    assert got == {k: v.numel() * v.element_size() for k, v in plain.items()}     # exact sizes: nothing is rounded up
    assert got["labels"] == B * H * W and got["wy"] == 128 and got["tiles"] == 4 * n * ch * 1024
    for k in outputs:                                                           # bit-identical to ordinary allocations
        assert torch.equal(plain[k].view(torch.uint8), guarded[k].view(torch.uint8)), k
    # ... and the right values, so that the guarded run is the real one
    assert np.array_equal(guarded["tiles"].cpu().numpy(), R.gather(inputs["src"].numpy(), tile, stride, pad, flips))
    ref = R.blend(inputs["z"].numpy(), B, H, W, tile, stride, flips, inputs["wy"].numpy(), inputs["wx"].numpy(), "softmax")
    assert float(np.abs(guarded["map"].cpu().numpy() - ref).max()) <= R.tol("softmax", 1.0)

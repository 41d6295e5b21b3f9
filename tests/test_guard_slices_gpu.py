"""GPU: the two entries of include/slices/lmnet_slices.h that write device memory -- lmn_slices_stats, lmn_slices_gather -- inside guard
bands (tests/guard.py): the guard manifest's test of these entries.  Every buffer -- the volume and the labels, the workspace at
exactly lmn_slices_workspace bytes, the record, the table, the slice list, the parameter rows, x and y -- is carved from a GuardPool at
its exact size, canaries flush against each, and every body the entries write starts filled with junk (0xA5 bytes).  The shapes cover
the vector and the scalar route of both entries and the label-only mode."""
import numpy as np
import pytest
import torch

import slices_ref as R
from guard import LaunchLog, pools

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.mark.parametrize("shape,size,context,ldt,dtype", [
    ((1, 3, 5, 7), (6, 9), 1, torch.uint8, np.int16),            # odd everything: the scalar routes, less than one wave
    ((2, 4, 8, 16), (8, 12), 1, torch.int64, np.int16),          # 16-byte chunks in the statistics, four x per lane in the gather
    ((1, 2, 16, 16), (4, 8), 0, torch.uint8, np.uint8)])
def test_slices_entries(shape, size, context, ldt, dtype):
    """Statistics, gather and the label-only gather with every buffer at its exact size and junk in it: the same bits as with
    ordinary allocations, the record of the restatement, canaries intact, inputs untouched."""
    from lm_net_amd import hip
    from lm_net_amd.data import slice_param_row
    M, D, Hs, Ws = shape
    h, w = size
    vol, lab = R.phantom(M, D, Hs, Ws, seed=4, dtype=dtype)
    specs = [(m, k, 40.0, 400.0) for m in range(M) for k in (hip.SLICES_ZSCORE, hip.SLICES_WINDOW)]
    S, K, n = len(specs), 2 * context + 1, 3
    z = np.array([D - 1, 0, D // 2], dtype=np.int32)
    rows = np.tile(slice_param_row(size, (Hs, Ws)), (n, 1))
    back = np.tile(slice_param_row((Hs, Ws), size), (n, 1))
    ws_bytes = hip.slices_workspace(M, D, Hs, Ws)
    inputs = dict(volume=torch.from_numpy(vol), labels=torch.from_numpy(lab), z=torch.from_numpy(z), rows=torch.from_numpy(rows),
                  back=torch.from_numpy(back), zb=torch.arange(n, dtype=torch.int32))
    outputs = dict(workspace=((ws_bytes,), torch.uint8), stats=((M, 8), torch.int64), table=((S, 4), torch.float32),
                   x=((n, S * K, h, w), torch.float32), y=((n, h, w), ldt), y8=((n, h, w), torch.uint8), restored=((n, Hs, Ws), torch.uint8))
    fg, bv = [-1000 if dtype == np.int16 else 0] * M, [0.0] * M

    def run(t):
        hip.slices_stats(t["volume"], fg, 5000, 995000, specs, t["workspace"], t["stats"], t["table"])
        hip.slices_gather(t["volume"], t["labels"], t["z"], t["rows"], t["table"], [s[0] for s in specs], context, 1, hip.SLICES_EDGE_REPLICATE,
                          hip.SLICES_BORDER_REPLICATE, bv, 0, t["x"], t["y"])
        hip.slices_gather(None, t["labels"], t["z"], t["rows"], None, None, 0, 1, 0, 0, None, 0, None, t["y8"])
        hip.slices_gather(None, t["y8"], t["zb"], t["back"], None, None, 0, 1, 0, hip.SLICES_BORDER_CONSTANT, None, 255, None, t["restored"])
        torch.cuda.synchronize()

    plain, pool, guarded = pools(inputs, outputs, DEV, fill="junk")
    run(plain)
    with LaunchLog(pool) as log:
        run(guarded)
    pool.assert_clean("slices entries")
    pool.assert_inputs_unchanged()
    assert log.names == ["slices_stats", "slices_gather", "slices_gather", "slices_gather"]
    got = {e[0]: e[2] for e in pool.entries}
    assert got == {k: v.numel() * v.element_size() for k, v in plain.items()}     # exact sizes: nothing is rounded up
    assert got["workspace"] == ws_bytes and got["stats"] == 64 * M and got["table"] == 16 * S and got["x"] == 4 * n * S * K * h * w
    for name in outputs:
        if name != "workspace":
            assert torch.equal(plain[name].view(torch.uint8), guarded[name].view(torch.uint8)), name
    assert guarded["stats"].cpu().tolist() == R.record(vol, fg, (5000, 995000))
    assert torch.equal(guarded["y"].to(torch.uint8), guarded["y8"])

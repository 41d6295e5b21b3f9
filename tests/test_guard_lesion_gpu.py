"""GPU: the entry of include/lesion/lmnet_lesion.h that writes device memory, lmn_lesion_match, inside guard bands (tests/guard.py):
the guard manifest's test of this entry.  Every buffer -- the two uint8 volumes, the workspace at exactly lmn_lesion_workspace bytes,
the component records, the pair table and ctrl -- is carved from a GuardPool at its exact size, canaries flush against each, and the
scratch starts poisoned.  The shapes are two of tests/test_lesion_kernels_gpu.py: (3, 5, 70), 1050 voxels -- the second block's last
lanes take the scalar path and most of its lanes lie past the volume -- and (17, 66, 130), whose 145 860 voxels end inside a block as
well; the capacities are no multiples of anything: 1000 component records, the smallest table that holds the pairs."""
import numpy as np
import pytest
import torch

import lesion_ref as R
from guard import LaunchLog, pools

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SHAPES = [(3, 5, 70), (17, 66, 130)]


def _canonical(x):
    from lm_net_amd.metrics import _canonical_records
    ck, cs = _canonical_records(x["comp_keys"], x["comp_sizes"])
    pk, pc = _canonical_records(x["pair_keys"], x["pair_counts"])
    return [t.cpu().numpy() for t in (ck, cs, pk, pc, x["ctrl"])]


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lesion_match_entry(shape, connectivity):
    """Both labellings, the component records and the pair table with the scratch at its exact size and poisoned: the canonical
    records equal those of ordinary allocations and the restatement.  (The raw slot order depends on arrival order: not compared.)"""
    from lm_net_amd import hip
    C, mask = 4, 0b1110
    Lp, Lt = R.lesion_case(*shape, C)
    want = R.records(Lp, Lt, C, connectivity)
    M, S = 1000 if shape == SHAPES[0] else int(want[4][0]) + 3, 64
    while S < want[4][1]:
        S *= 2
    want = R.records(Lp, Lt, C, connectivity, None, M, S)
    ws_bytes = hip.lesion_workspace(*shape)
    inputs = dict(pred=torch.from_numpy(Lp), target=torch.from_numpy(Lt))
    outputs = dict(workspace=((ws_bytes,), torch.uint8), comp_keys=((M,), torch.int64), comp_sizes=((M,), torch.int32),
                   pair_keys=((S,), torch.int64), pair_counts=((S,), torch.int32), ctrl=((4,), torch.int32))

    def run(x):
        hip.lesion_match(x["pred"], x["target"], C, connectivity, mask, x["workspace"], x["comp_keys"], x["comp_sizes"], x["pair_keys"],
                         x["pair_counts"], x["ctrl"])
        torch.cuda.synchronize()

    plain, pool, guarded = pools(inputs, outputs, DEV, fill="poison")
    run(plain)
    with LaunchLog(pool) as log:
        run(guarded)
    pool.assert_clean("lesion_match entry")
    pool.assert_inputs_unchanged()
    assert log.names == ["lesion_match"]
    got = {e[0]: e[2] for e in pool.entries}
    assert got == {k: v.numel() * v.element_size() for k, v in plain.items()}     # exact sizes: nothing is rounded up
    assert got["workspace"] == ws_bytes == 4 * ((4 * Lp.size + 255) // 256 * 256) and got["comp_keys"] == 8 * M and got["pair_counts"] == 4 * S
    assert got["ctrl"] == 16 and got["pred"] == Lp.size
    a, b = _canonical(plain), _canonical(guarded)
    for x, y, w, name in zip(a, b, want, ("comp_keys", "comp_sizes", "pair_keys", "pair_counts", "ctrl")):
        assert np.array_equal(x, y), name
        assert np.array_equal(y, w), name                                         # ... the right values: the guarded run is the real one
    assert want[4][0] > 10 and want[4][1] > 5 and S >= 64

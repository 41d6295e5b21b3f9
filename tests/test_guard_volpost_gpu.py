"""GPU: the two entries of include/volpost/lmnet_volpost.h that write device memory, lmn_cc3d_label and lmn_volpost_clean, inside guard
bands (tests/guard.py): the guard manifest's tests of these entries.  Every buffer -- the uint8 volume, the roots and sizes, the
workspace at exactly lmn_volpost_workspace bytes, the cleaned volume and the statistics -- is carved from a GuardPool at its exact
size, canaries flush against each, and the scratch starts poisoned.  The shapes are two of tests/test_volpost_kernels_gpu.py:
(3, 5, 70), where x crosses a 64-wide tile and no row ends on a 4-byte boundary, and (17, 66, 130), with tile seams along both
in-plane axes; the last word of the face bitmap of either is partly used."""
import numpy as np
import pytest
import torch

import volpost_ref as R
from guard import LaunchLog, pools

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SHAPES = [(3, 5, 70), (17, 66, 130)]


@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cc3d_label_entry(shape, connectivity):
    from lm_net_amd import hip
    L = R.label_volume(R.blob_labels(shape, 4), 4)
    inputs = dict(labels=torch.from_numpy(L))
    outputs = dict(roots=(shape, torch.int32), sizes=(shape, torch.int32))

    def run(x):
        hip.cc3d_label(x["labels"], connectivity, x["roots"], x["sizes"])
        torch.cuda.synchronize()

    plain, pool, guarded = pools(inputs, outputs, DEV, fill="poison")
    run(plain)
    with LaunchLog(pool) as log:
        run(guarded)
    pool.assert_clean("cc3d_label entry")
    pool.assert_inputs_unchanged()
    assert log.names == ["cc3d_label"]
    got = {e[0]: e[2] for e in pool.entries}
    assert got == {k: v.numel() * v.element_size() for k, v in plain.items()} and got["roots"] == 4 * L.size
    roots, sizes = R.components(L, connectivity)
    for k, w in (("roots", roots), ("sizes", sizes)):
        assert torch.equal(plain[k], guarded[k])
        assert np.array_equal(guarded[k].cpu().numpy(), w), k


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_volpost_clean_entry(shape, connectivity):
    """Both labellings, two selection passes and the hole filling with the scratch at its exact size and poisoned: the result equals
    the one of ordinary allocations and the restatement."""
    from lm_net_amd import hip
    C = 4
    L = R.label_volume(R.blob_labels(shape, C, seed=1), C)
    keep, minv, mask, limit = [0, 2, 1, 0], [0, 0, 2, 3], 0b1110, 6
    ws_bytes = hip.volpost_workspace(*shape)
    inputs = dict(labels=torch.from_numpy(L))
    outputs = dict(workspace=((ws_bytes,), torch.uint8), labels_out=(shape, torch.uint8), stats=((C, 4), torch.int32))

    def run(x):
        hip.volpost_clean(x["labels"], C, connectivity, mask, keep, minv, limit, x["workspace"], x["labels_out"], x["stats"])
        torch.cuda.synchronize()

    plain, pool, guarded = pools(inputs, outputs, DEV, fill="poison")
    run(plain)
    guarded["labels_out"].fill_(0xFF)
    with LaunchLog(pool) as log:
        run(guarded)
    pool.assert_clean("volpost_clean entry")
    pool.assert_inputs_unchanged()
    assert log.names == ["volpost_clean"]
    got = {e[0]: e[2] for e in pool.entries}
    assert got == {k: v.numel() * v.element_size() for k, v in plain.items()}     # exact sizes: nothing is rounded up
    assert got["workspace"] == ws_bytes and got["stats"] == 16 * C and got["labels_out"] == L.size
    assert torch.equal(plain["labels_out"], guarded["labels_out"]) and torch.equal(plain["stats"], guarded["stats"])
    # ... and the right values, so that the guarded run is the real one
    L2, stats, info = R.clean(L, C, connectivity, classes=[1, 2, 3], keep_largest={1: 2, 2: 1}, min_volume=[0, 2, 3], fill_holes=limit)
    assert np.array_equal(guarded["labels_out"].cpu().numpy(), L2)
    assert np.array_equal(guarded["stats"].cpu().numpy(), stats)
    if shape == SHAPES[1]:
        assert stats[0, 3] > 0 and (stats[1:, 1] < stats[1:, 0]).all()             # holes were filled and components removed

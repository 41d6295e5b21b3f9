"""CPU: the precondition of the busy-stream tests (tests/busy.py), from the reference modules alone.  For every subject the
references of its three cases A, B, C differ pairwise by at least 100 times the tolerance of each compared output, exact outputs in
at least half of their elements: a launch that ran while the buffers still held case A, or a second call that accumulated on top of
the first, cannot pass as the reference of B or C.  Also the instrument's own pieces that need no device."""
import numpy as np
import pytest

import busy
import busy_cases as K


def test_every_listed_subject_exists_once():
    assert sorted(K.subjects()) == sorted(K.LOSS_NAMES + K.METER_NAMES + K.DATA_NAMES)


@pytest.mark.parametrize("name", K.LOSS_NAMES + K.METER_NAMES + K.DATA_NAMES)
def test_cases_discriminate(name):
    s = K.subjects()[name]
    refs = busy.check_discrimination(s)
    for k in K.CASES:                                               # every case is a valid input: finite references, nothing empty
        for what, a, atol in refs[k]:
            a = np.asarray(a)
            assert a.size > 0 and (a.dtype.kind in "iub" or np.isfinite(a).all()), (name, k, what)
            assert atol is None or np.all(np.asarray(atol) > 0), (name, k, what)


def test_the_detector_rejects_near_cases():
    """check_discrimination itself: two cases 50 tolerances apart, and exact outputs that differ in a third of their elements."""
    mk = lambda v: [np.full(4, v, np.float32)]
    near = busy.Subject("near", {"A": mk(0.0), "B": mk(1.0), "C": mk(1.0 + 50e-4)}, lambda a, got=None: [("x", a[0].astype(np.float64), 1e-4)])
    with pytest.raises(AssertionError, match="differs by"):
        busy.check_discrimination(near)
    third = lambda v: [np.array([v, 0, 0], np.int32)]
    few = busy.Subject("few", {"A": third(1), "B": third(2), "C": third(3)}, lambda a, got=None: [("x", a[0], None)])
    with pytest.raises(AssertionError, match="of its elements only"):
        busy.check_discrimination(few)
    with pytest.raises(AssertionError):
        busy.Subject("shapes", {"A": mk(0.0), "B": mk(1.0), "C": [np.zeros(5, np.float32)]}, None)

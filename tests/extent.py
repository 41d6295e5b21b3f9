"""Periodic batches: a call over several GiB checked against an fp64 reference of THREE images.

The per-image arithmetic of a kernel does not depend on the batch count B; what depends on it is the address arithmetic (32-bit element
and byte offsets, buffer-descriptor sizes, form switches on the operand's bytes).  So the device operand is ``tile[b % P]`` for b < B,
built on the device from a tile of P distinct fp64 images (drawn with kernel_checks.R), and

  * a per-image output is expected to be ``ref(tile)[b % P]``: compared on the device, in chunks, against the uploaded P reference
    images, scored like kernel_checks.rel (max abs error over the max abs reference; a non-finite result scores inf);
  * a batch reduction (BN sums, dW, db, drpb, dgamma / dbeta) is expected to be ``sum_j n_j * part_j`` in fp64, with n_j the number of
    images congruent to j mod P and part_j the fp64 partial of tile image j.

THE PERIOD RULE.  A wrapped or truncated offset reads 2^31 or 2^32 bytes -- or elements -- away from where it should.  If that distance
is a whole number of periods the wrapped read returns identical data and the test sees nothing.  Hence P = 3 (never a power of two),
and ``assert_period`` refuses an operand for which any of the four distances is a multiple of P * image_bytes (or P * image_elements).

REDUCED QUANTITIES are compared only when their addends do not cancel: ``rel_reduced`` takes the fp64 sum of the ABSOLUTE addends beside
the expected value and refuses a reference whose largest element is small against it (draw the data shifted, as check_ln_linear and
check_bn_shifted_stats do), so a reduction is never scored by the maximum of a near-zero reference.

Importable without a GPU: everything here is plain tensor arithmetic on the device of its arguments (tests/test_extent_cpu.py runs it
on the CPU)."""
import contextlib
import gc

import torch

P = 3
DISTANCES = (("2^31", 1 << 31), ("2^32", 1 << 32))
PEAK_LIMIT = 24 << 30           # bytes of device memory one case may hold at its peak
MIN_DEVICE = 64 << 30           # a device with less memory than this may skip the extent cases; an MI355X (288 GB) never does


def period_violations(image_elements, itemsize, period=P):
    """The distances a wrapped offset could travel without the periodic data showing it: [] when the operand is safe."""
    bad = []
    for name, d in DISTANCES:
        if d % (period * image_elements * itemsize) == 0:
            bad.append("%s bytes" % name)
        if d % (period * image_elements) == 0:
            bad.append("%s elements" % name)
    return bad


def assert_period(name, image_elements, itemsize, period=P):
    bad = period_violations(image_elements, itemsize, period)
    assert not bad, ("operand %s: %s is a whole number of periods (%d images of %d elements of %d bytes): a wrapped offset would read "
                     "identical data" % (name, " and ".join(bad), period, image_elements, itemsize))


def counts(B, period=P):
    """n_j: how many b < B are congruent to j."""
    return [(B - j + period - 1) // period for j in range(period)]


def fill_periodic(dst, tile):
    """dst[b] = tile[b % P] for every b < dst.shape[0]: whole periods by one broadcast copy on dst's device, then the tail."""
    period, B = tile.shape[0], dst.shape[0]
    assert tuple(dst.shape[1:]) == tuple(tile.shape[1:]) and dst.is_contiguous(), (tuple(dst.shape), tuple(tile.shape))
    assert_period("of shape %s" % (tuple(dst.shape),), tile[0].numel(), dst.element_size(), period)
    tile = tile.to(device=dst.device, dtype=dst.dtype)
    q = B // period
    if q:
        dst[:q * period].view(q, period, *tile.shape[1:]).copy_(tile.unsqueeze(0).expand(q, *tile.shape))
    if B - q * period:
        dst[q * period:].copy_(tile[:B - q * period])
    return dst


def expected_images(ref_tile, B):
    """The expected per-image output spelled out (for a SMALL B: the helper's own test compares it with a direct reference)."""
    return ref_tile[torch.arange(B) % ref_tile.shape[0]]


def expected_sum(parts, B):
    """sum_j n_j * parts[j] in fp64: the batch reduction of per-image partials parts [P, ...]."""
    parts = parts.double()
    n = torch.tensor(counts(B, parts.shape[0]), dtype=torch.float64, device=parts.device)
    return (parts * n.view(-1, *([1] * (parts.dim() - 1)))).sum(0)


def rel_periodic(got, ref_tile, chunk_elements=1 << 26):
    """kernel_checks.rel of got [B, ...] against ref_tile[b % P], computed on got's device in fp64 chunks of whole periods."""
    period, B = ref_tile.shape[0], got.shape[0]
    if tuple(got.shape[1:]) != tuple(ref_tile.shape[1:]):
        return float("inf")
    ref = ref_tile.to(device=got.device, dtype=torch.float64)
    step = max(1, chunk_elements // (period * ref[0].numel()))
    q, err = B // period, torch.zeros((), dtype=torch.float64, device=got.device)
    for lo in range(0, q, step):
        hi = min(q, lo + step)
        d = got[lo * period:hi * period].reshape(hi - lo, period, *ref.shape[1:]).to(torch.float64, copy=True).sub_(ref.unsqueeze(0)).abs_().max()
        err = torch.maximum(err, torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf"))))       # (max propagates NaN)
    if B - q * period:
        d = got[q * period:].to(torch.float64, copy=True).sub_(ref[:B - q * period]).abs_().max()
        err = torch.maximum(err, torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf"))))
    return float(err / (ref.abs().max() + 1e-30))


def rel_reduced(got, expected, absolute, floor=0.25):
    """Score of a batch reduction: max abs error over the max abs expected value -- after asserting that the addends did not cancel:
    `absolute` is the same reduction of the ABSOLUTE addends (fp64), and the largest expected element must reach `floor` of the largest
    absolute sum."""
    expected, absolute = expected.detach().double().cpu(), absolute.detach().double().cpu()
    assert float(expected.abs().max()) >= floor * float(absolute.abs().max()) > 0.0, (
        "reduction reference nearly cancels (max |expected| %.3g against %.3g of absolute addends): shift the data"
        % (float(expected.abs().max()), float(absolute.abs().max())))
    got = got.detach().double().cpu()
    if got.shape != expected.shape or not torch.isfinite(got).all():
        return float("inf")
    return float((got - expected).abs().max() / expected.abs().max())


def release():
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def gap_pool(device, nbytes, guard=4096):
    """A guard.GuardPool whose detector looks at the canary GAPS only (before the first tensor, between two tensors, after the last one)
    instead of keeping a byte mask as large as the pool: the same layout, the same report, half the memory -- the operands of an extent
    case are several GiB each and one case may hold 24 GiB.  Nothing is unallocated inside a pool sized by size_for, so the gaps are
    all the canary there is."""
    from guard import GRANULE, POISON, GuardPool

    class GapPool(GuardPool):
        def __init__(self):
            self.guard = int(guard)
            self.nbytes = (int(nbytes) + GRANULE - 1) // GRANULE * GRANULE
            self.buf = torch.full((self.nbytes,), POISON, dtype=torch.uint8, device=device)
            self.raw, self.ref, self.mask, self.entries, self._masked = self.buf, None, None, [], 0
            self.off, self.t, self.inputs = 0, {}, {}

        def check(self):
            self._sync()
            out, ends = [], [(None, 0)] + [(name, a + nb) for name, a, nb in self.entries]
            starts = [(name, a) for name, a, _ in self.entries] + [(None, self.nbytes)]
            for (before, lo), (after, hi) in zip(ends, starts):
                if hi <= lo:
                    continue
                bad = (self.raw[lo:hi] != POISON).nonzero().flatten()
                if bad.numel():
                    first, last = int(bad[0]) + lo, int(bad[-1]) + lo
                    if before is not None:
                        out.append((before, "after", first - lo, last - lo))
                    else:
                        out.append((after, "before", first - hi, last - hi))
            return out

    return GapPool()


@contextlib.contextmanager
def guarded_case(nbytes, device="cuda"):
    """One extent case: a guard.GuardPool (gap_pool) sized for tensors of the given byte sizes (every operand of the call is carved from this ONE
    backing buffer, so a wrapped read lands in memory the test owns and a stray store within the canaries is reported), assert_clean()
    at the end, everything released and the peak of device memory asserted.  Skips only on a device below 64 GiB."""
    import pytest
    from guard import GuardPool
    total = torch.cuda.get_device_properties(device).total_memory
    if total < MIN_DEVICE:
        pytest.skip("device memory %.0f GiB below 64 GiB: the extent cases need a large device (an MI355X must run them: 0 skips there)"
                    % (total / 2 ** 30))
    release()
    torch.cuda.reset_peak_memory_stats(device)
    pool = gap_pool(device, GuardPool.size_for(list(nbytes)))
    try:
        yield pool
        pool.assert_clean()
    finally:
        torch.cuda.synchronize(device)
        peak = torch.cuda.max_memory_allocated(device)
        pool.buf = pool.raw = pool.mask = None
        pool.t.clear(), pool.inputs.clear()
        del pool
        release()
    assert peak <= PEAK_LIMIT, "peak device memory %.1f GiB above the 24 GiB of one case" % (peak / 2 ** 30)

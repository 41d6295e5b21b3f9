"""Busy-stream instrument: do the launches of a call follow the caller's stream, and does the call return without waiting for it?

The package promises, class by class, "every launch goes to the caller's current stream" and "nothing synchronises".  A test that
lets the side stream wait for the default stream first, or whose inputs are finished before the call, cannot see a kernel, memset
or copy that went to the null stream (same bits), and torch's sync-debug mode sees torch's own synchronisations only, not a
hipStreamSynchronize or a blocking copy inside a C entry.  Here the side stream is kept BUSY while the calls are issued:

  gate(stream, ms)   enqueues work that occupies `stream` for about `ms` and touches none of the subject's tensors (torch.cuda._sleep
                     with cycles calibrated once per process by two events; a chain of matmuls where _sleep is missing) and returns
                     an event recorded behind it.
  run(subject, make_call, stream)
                     1. warms the subject three times on `stream` at the test geometry and synchronises (library load, workspaces,
                        plans, pinned staging and the per-stream deterministic scratch exist after this);
                     2. measures the host wall time t_host of two calls on the idle stream;
                     3. with the input buffers holding case A and nothing waiting on anything, enqueues on `stream`: a gate of
                        10 x t_host, device copies of case B into the buffers, call 1, device copies of case C, call 2 -- and reads
                        the gate's event.query() the moment call 2 has returned;
                     4. synchronises the stream and compares both results.

What is asserted:
  no host wait   the gate's event is not complete when call 2 returns (one subject, the host-launched training step, is documented
                 to wait for one cause; there the wait is accepted only if that cause occurred: Subject.waits).  A synchronisation anywhere in the call -- torch's, the HIP
                 runtime's, the library's -- fails this (so does a gate that was too short: the message names both causes).
  stream order   result 1 is the reference of case B and result 2 that of case C.  A launch, memset or copy on any other stream ran
                 while the buffers still held case A (a valid input whose reference differs from B's and C's by 100 tolerances:
                 tests/test_busy_cpu.py); two calls behind one gate also show a misrouted zeroing of a scratch (both memsets run
                 early, the second call accumulates on top of the first).
  exact          where the class promises exact or bit-identical results: the same bits as a plain default-stream call.
  no growth      for the subjects that promise it, torch.cuda.memory_stats()["segment.all.allocated"] does not change over steps
                 2 to 4.  This sees torch's caching allocator only: a hipMalloc inside the library is invisible to it.

A subject (tests/busy_cases.py) is data alone and importable without a GPU: three valid, in-range inputs of one geometry and the
numpy reference of each with its tolerance.  The device side (`make_call`) is given by the GPU test."""
import time

import numpy as np
import torch

GATE_FACTOR = 10              # gate = GATE_FACTOR x t_host: host time on a share of a loaded machine jitters by small multiples
GATE_LIMIT_MS = 1000.0
DISCRIMINATION = 100.0        # the references of two cases differ by at least this many tolerances

_CAL = {}


class Subject:
    """name; inputs {"A" | "B" | "C": [numpy arrays]} (same shapes and dtypes in every case); ref(arrays, got=None) -> [(what,
    numpy array, atol)] with atol None for an output that must be EQUAL, else the absolute bound on max |got - ref| (`got`: the
    device's outputs as numpy, for a reference that is evaluated on the device's own sort order); exact: bit equality with a
    default-stream call; no_growth: the class promises no device allocation after the first call of a geometry."""

    def __init__(self, name, inputs, ref, exact=False, no_growth=False):
        assert sorted(inputs) == ["A", "B", "C"]
        for k in "BC":
            assert [(a.shape, a.dtype) for a in inputs[k]] == [(a.shape, a.dtype) for a in inputs["A"]], (name, k)
        self.name, self.inputs, self.ref, self.exact, self.no_growth = name, inputs, ref, exact, no_growth
        self.waits = None         # a documented wait: callable -> a count of its documented cause; a wait is accepted only if the count rose
        self.host = None          # {case: the host-side arguments of a call on that case (e.g. augmentation parameters)}, handed to call() and ref()

    def reference(self, case, got=None):
        if self.host is None:
            return self.ref(self.inputs[case], got=got)
        return self.ref(self.inputs[case], got=got, host=self.host[case])

    def __repr__(self):
        return self.name


def distance(x, y):
    """(max |x - y|, share of differing elements) of two reference outputs."""
    x, y = np.asarray(x), np.asarray(y)
    assert x.shape == y.shape, (x.shape, y.shape)
    if x.size == 0:
        return 0.0, 0.0
    return float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()), float((x != y).mean())


def check_discrimination(subject):
    """The precondition of the stream-order assertion, from the references alone: for every compared output the references of A, B
    and C differ pairwise by at least 100 tolerances; exact outputs differ in at least half of their elements."""
    refs = {k: subject.reference(k) for k in "ABC"}
    for a, b in (("A", "B"), ("A", "C"), ("B", "C")):
        for (what, x, tx), (_, y, ty) in zip(refs[a], refs[b]):
            d, share = distance(x, y)
            if tx is None:
                assert share >= 0.5, "%s: %s of cases %s and %s differs in %.1f %% of its elements only" % (subject, what, a, b, 100 * share)
            else:
                t = max(float(np.max(tx)), float(np.max(ty)))
                assert d >= DISCRIMINATION * t > 0, "%s: %s of cases %s and %s differs by %.3e, tolerance %.3e" % (subject, what, a, b, d, t)
    return refs


# ------------------------------------------------------------------------------------------------------------------------- the gate
def _calibrate(kind):
    """(units of work per millisecond, the unit): cycles of torch.cuda._sleep, or 2048^3 fp32 matmuls into a preallocated output,
    timed once per process by two events around a few milliseconds of it, after a warm-up"""
    if kind in _CAL:
        return _CAL[kind]
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if kind == "sleep":
        n, reps = 2_000_000, 1
        unit = lambda: torch.cuda._sleep(n)
    else:
        m = torch.ones((2048, 2048), device="cuda")
        out = torch.empty_like(m)
        n, reps = 1, 32
        unit = lambda: torch.mm(m, m, out=out)
    for _ in range(3):
        unit()
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        unit()
    e.record()
    e.synchronize()
    per_ms = n * reps / max(s.elapsed_time(e), 1e-3)
    _CAL[kind] = (per_ms, unit if kind == "matmul" else None)
    return _CAL[kind]


def gate_kind():
    return "sleep" if hasattr(torch.cuda, "_sleep") else "matmul"


def gate(stream, ms, kind=None):
    """Occupy `stream` for about `ms` milliseconds with work that touches no tensor of the subject -> the event behind that work."""
    kind = kind or gate_kind()
    with torch.cuda.stream(stream):
        per_ms, unit = _calibrate(kind)
        if kind == "sleep":
            torch.cuda._sleep(max(1, int(per_ms * ms)))
        else:
            for _ in range(max(1, int(np.ceil(per_ms * ms)))):
                unit()
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


# ------------------------------------------------------------------------------------------------------------------------- the run
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.detach().cpu().numpy()


def _load(bufs, case):
    with torch.no_grad():
        for b, c in zip(bufs, case):
            b.copy_(c, non_blocking=True)


def _segments():
    return torch.cuda.memory_stats()["segment.all.allocated"]


def _compare(subject, case, got, where):
    want = subject.reference(case, got=got)
    assert len(want) == len(got), (subject, len(want), len(got))
    for (what, ref, atol), g in zip(want, got):
        assert g.shape == np.asarray(ref).shape, (subject, what, g.shape, np.asarray(ref).shape)
        d, share = distance(g, ref)
        print("busy %s %s case %s: %s max err %.3e (bound %s), %.2f %% of elements differ"
              % (subject, where, case, what, d, "equal" if atol is None else "%.3e" % np.max(atol), 100 * share))
        if atol is None:
            ok = share == 0.0 and g.dtype == np.asarray(ref).dtype
        else:
            ok = bool(np.isfinite(g).all() and np.all(np.abs(g.astype(np.float64) - ref) <= atol))
        assert ok, ("%s: %s of %s is not the reference of case %s (max err %.3e, bound %s, %.2f %% of elements differ): a launch, memset "
                    "or copy did not follow the caller's stream" % (subject, what, where, case, d, None if atol is None else np.max(atol), 100 * share))


def run(subject, make_call, stream, log=None):
    """The four steps of the module docstring.  make_call(bufs) -> call; call() -- call(subject.host[case]) where the subject has host-side
    arguments -- runs the subject once on the CURRENT stream on the device tensors `bufs` (they hold one case's arrays) and returns a
    tuple of device tensors nobody overwrites later; call.finish(outputs as numpy), if set, reduces them on the host before comparing.  -> a dict
    with t_host and the gate length in ms (also printed, and appended to `log`)."""
    assert stream != torch.cuda.default_stream()
    cases = {k: [_dev(a) for a in v] for k, v in subject.inputs.items()}
    bufs = [c.clone() for c in cases["A"]]
    call = make_call(bufs)
    go = (lambda case: call()) if subject.host is None else (lambda case: call(subject.host[case]))
    finish = getattr(call, "finish", None) or (lambda outs: outs)          # host-side reduction of the outputs, after the synchronise
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        keep = [go("A") for _ in range(3)]                                  # 1. warm
        stream.synchronize()
        del keep
        _calibrate(gate_kind())
        stream.synchronize()
        seg0 = _segments()
        t0 = time.perf_counter()                                           # 2. host time of two calls on the idle stream
        r1 = go("A")
        r2 = go("A")
        t_host = time.perf_counter() - t0
        stream.synchronize()
        del r1, r2
        gate_ms = GATE_FACTOR * t_host * 1e3
        line = "busy %s: t_host %.3f ms, gate %.2f ms" % (subject, t_host * 1e3, gate_ms)
        print(line)
        if log is not None:
            log.append(line)
        assert gate_ms <= GATE_LIMIT_MS, "%s: too slow to gate (two calls take %.1f ms of host time)" % (subject, t_host * 1e3)
        torch.cuda.synchronize()                                           # the default stream idle, nothing waiting on anything
        cause0 = subject.waits() if subject.waits else 0
        ev = gate(stream, gate_ms)                                         # 3. the buffers hold case A
        _load(bufs, cases["B"])
        t1 = time.perf_counter()
        r1 = go("B")
        t2 = time.perf_counter()
        _load(bufs, cases["C"])
        r2 = go("C")
        returned_early = not ev.query()
        t3 = time.perf_counter()
        print("busy %s: behind the gate call 1 returned after %.3f ms, call 2 after %.3f ms" % (subject, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        stream.synchronize()                                               # 4.
        seg1 = _segments()
    if subject.waits and not returned_early:                               # documented to wait, for ONE documented cause: it must be there
        assert subject.waits() > cause0, "%s: waited for the stream without its documented cause" % subject
        returned_early = True
    assert returned_early, ("%s: the gate of %.2f ms had drained when call 2 returned: the call waited for the stream, or the gate was "
                            "too short (t_host %.3f ms; behind the gate call 1 took %.3f ms of host time, call 2 %.3f ms)"
                            % (subject, gate_ms, t_host * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
    got1, got2 = finish([_host(t) for t in r1]), finish([_host(t) for t in r2])
    _compare(subject, "B", got1, "call 1")
    _compare(subject, "C", got2, "call 2")
    if subject.no_growth:
        assert seg1 == seg0, "%s: %d device segments allocated after the warm-up" % (subject, seg1 - seg0)
    if subject.exact:                                                      # the same bits as a plain default-stream call
        for case, got in (("B", got1), ("C", got2)):
            _load(bufs, cases[case])
            plain = finish([_host(t) for t in go(case)])
            torch.cuda.synchronize()
            for k, (p, g) in enumerate(zip(plain, got)):
                assert p.dtype == g.dtype and p.tobytes() == g.tobytes(), \
                    "%s: output %d of case %s differs in bits from a default-stream call" % (subject, k, case)
    return dict(t_host_ms=t_host * 1e3, gate_ms=gate_ms)

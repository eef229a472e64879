"""Helper of test_gpu_call_stream.py (no tests here): make a call on a side stream while the producer of its inputs is
still pending on that stream, and compare what a consumer queued behind the call reads.

The stream contract under test: every kernel, fill, copy and library call of an entry point is queued on the stream the caller
passed (for the wrappers: torch's current stream), in order.  A launch that went to the null stream instead would run at once,
before the producer: it would read the decoy the buffers still hold (or write before the caller's fill of its output), and
the in-stream clone of the result would differ from the expected one.

Protocol of ``run_behind_pending_work``:
  1. the expected result: ``call()`` on the default stream with ``real`` in the buffers and the device idle; the decoy's
     result the same way with ``decoy`` in the buffers.  The decoy's result must FAIL the comparison (non-vacuity), for a
     chain of wrappers (PerWrapper) in the outputs of every wrapper of the chain.
     The buffers are left holding ``decoy``; one device synchronise.
  2. on a fresh side stream: ``delay``; ``buffers[k].copy_(real[k])``; every tensor of ``scratch`` filled with 0xA5 bytes;
     ``result = call()``.
  3. ``not side.query()`` right after the call returned: everything was queued behind a producer that had not run, and the
     wrapper did not synchronise (skipped with ``blocking=True``, for entries that read back by contract).
  4. still on the side stream: every result tensor cloned, then ``decoy`` copied back into the buffers.
  5. ``side.synchronize()``, ``torch.cuda.synchronize()``; the clones are compared with the expected result.
"""
import torch

DELAY_MS = 40.0           # what one delay() aims at; not an acceptance number: step 3 asserts that it was long enough
_state = {}


def delay_cycles(device):
    """Cycles for torch.cuda._sleep that take about DELAY_MS on ``device`` (measured once per process with two events)."""
    key = torch.device(device).index or 0
    if key not in _state:
        probe, ms = 10_000, 0.0
        with torch.cuda.device(key):
            torch.cuda._sleep(1000)                       # loads the kernel
            torch.cuda.synchronize()
            while ms < 2.0 and probe < 10 ** 10:          # whatever clock _sleep counts: lengthen the probe until it is measurable
                probe *= 10
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                torch.cuda._sleep(probe)
                t1.record()
                t1.synchronize()
                ms = max(t0.elapsed_time(t1), 1e-3)
        cycles = int(probe * DELAY_MS / ms)
        _state[key] = {"cycles": cycles, "probe_ms": ms, "probe_cycles": probe}
    return _state[key]["cycles"]


def calibration(device):
    """{"cycles", "probe_ms", "probe_cycles"} of the calibration delay() uses on ``device``."""
    delay_cycles(device)
    return dict(_state[torch.device(device).index or 0])


def delay(stream):
    """Keep ``stream`` busy for about DELAY_MS: whatever is queued behind on it has not started when the host goes on."""
    cycles = delay_cycles(stream.device)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)


def tensors_of(result):
    """The tensors of a call's result, in a fixed order: the result itself, or the items of a (nested) tuple, list or dict in
    the order found.  Everything else (None, numbers, workspaces) is skipped."""
    if isinstance(result, torch.Tensor):
        return [result]
    if isinstance(result, (tuple, list)):
        return [t for item in result for t in tensors_of(item)]
    if isinstance(result, dict):
        return [t for key in result for t in tensors_of(result[key])]
    return []


def same_bits(got, expected):
    """Every tensor equal bit for bit (shape and dtype included)."""
    if len(got) != len(expected):
        return False
    for g, e in zip(got, expected):
        if g.dtype != e.dtype or g.shape != e.shape:
            return False
        if not torch.equal(g.contiguous().view(torch.uint8).reshape(-1), e.contiguous().view(torch.uint8).reshape(-1)):
            return False
    return True


def first_difference(got, expected):
    """For a failure message: the first tensor that differs and how far."""
    for i, (g, e) in enumerate(zip(got, expected)):
        if g.shape != e.shape or g.dtype != e.dtype:
            return f"tensor {i}: {tuple(g.shape)} {g.dtype} against {tuple(e.shape)} {e.dtype}"
        if not torch.equal(g.contiguous().view(torch.uint8).reshape(-1), e.contiguous().view(torch.uint8).reshape(-1)):
            gd, ed = g.double().reshape(-1), e.double().reshape(-1)
            bad = (gd != ed) | (torch.isnan(gd) != torch.isnan(ed))
            diff = torch.nan_to_num((gd - ed).abs(), nan=float("inf"))
            return (f"tensor {i} {tuple(g.shape)} {g.dtype}: {int(bad.sum())} of {gd.numel()} elements differ, "
                    f"largest difference {float(diff.max()) if diff.numel() else 0.0:.6g}")
    return f"{len(got)} tensors against {len(expected)}"


def _load(buffers, values):
    assert set(buffers) == set(values), (sorted(buffers), sorted(values))
    for k, b in buffers.items():
        v = values[k]
        assert b.shape == v.shape and b.dtype == v.dtype and b.device == v.device, f"{k}: the buffer and its value differ in layout"
        assert b.data_ptr() != v.data_ptr(), f"{k}: the buffer must be its own memory"
        b.copy_(v)


class PerWrapper(dict):
    """What a chain of wrappers returns: {wrapper name: its outputs}.  The decoy must change at least one output tensor of
    EVERY wrapper named, so that each link of the chain is tested and not only the first."""


def _groups(result):
    """[(name, number of tensors)] in the order tensors_of walks them: the wrappers of a PerWrapper, else one nameless group."""
    if isinstance(result, PerWrapper):
        return [(name, len(tensors_of(result[name]))) for name in result]
    return [("the call", len(tensors_of(result)))]


def run_behind_pending_work(call, real, decoy, buffers, scratch=(), blocking=False, between=None):
    """See the module's docstring.  ``call()`` reads ``buffers`` and returns its result tensors (nested tuples, lists, dicts),
    a chain of wrappers as a PerWrapper.  Every comparison is bit equality with the default-stream result: no kernel in csrc/
    uses float atomics, so no family needs a looser criterion.  ``scratch``: the tensors to dirty, or a function that returns
    them when the side stream gets there (workspaces are sized by the first run).  ``between``: called (on the stream in use)
    after the inputs are loaded and the scratch dirtied, before ``call`` -- for state a caller resets per run, such as
    zeroing accumulators.  Returns (got, expected)."""
    assert set(real) == set(decoy) == set(buffers)
    dev = next(iter(buffers.values())).device
    null = torch.cuda.current_stream(dev)
    assert null == torch.cuda.default_stream(dev), "start on the default stream"
    groups = []

    def on_default(values):
        _load(buffers, values)
        if between is not None:
            between()
        result = call()
        groups[:] = _groups(result)
        out = [t.clone() for t in tensors_of(result)]
        torch.cuda.synchronize(dev)
        return out

    expected = on_default(real)
    assert expected, "the call returned no tensor"
    wrong = on_default(decoy)              # leaves the decoy resident
    assert len(wrong) == len(expected) == sum(n for _, n in groups)
    at = 0
    for name, n in groups:                 # non-vacuity, per wrapper: the decoy changes at least one of its output tensors
        assert n > 0, f"{name} returned no tensor"
        assert not same_bits(wrong[at:at + n], expected[at:at + n]), f"vacuous case: the decoy's result of {name} has the real one's bits"
        at += n
    torch.cuda.synchronize(dev)

    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        delay(side)
        _load(buffers, real)
        for t in (scratch() if callable(scratch) else scratch):
            assert t.is_contiguous(), "scratch tensors are whole buffers"
            t.view(torch.uint8).fill_(0xA5)
        if between is not None:
            between()
        result = call()
        busy = not side.query()
        got = [t.clone() for t in tensors_of(result)]
        _load(buffers, decoy)
    side.synchronize()
    torch.cuda.synchronize(dev)
    if not blocking:
        assert busy, ("the side stream was idle when the call returned: the call synchronised, or the delay "
                      f"({calibration(dev)}) was shorter than the host's work")
    assert same_bits(got, expected), ("behind pending work the call gave another result than on the idle default stream: "
                                      + first_difference(got, expected)
                                      + ("; it equals the decoy's result" if same_bits(got, wrong) else ""))
    return got, expected

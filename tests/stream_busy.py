"""Helpers of test_stream_order.py: a caller's stream that is still busy when
a device entry point is called on it.

busy() enqueues a finite delay; run_busy() enqueues the delay and then the
write of the call's real input behind it, so that at the time of the call the
input buffers still hold a decoy (zeros) and only work that is ordered after
the caller's stream sees the real bytes.  Nothing here synchronises with the
host between the delay and the call.  No test lives in this file."""
import torch

DEFAULT_MS = 100.0

_cal = None  # (what the delay is made of, units per millisecond, the measurement in words)
_copy_bufs = None


def _time_ms(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def calibrate():
    """Once per process: how many torch.cuda._sleep cycles (or, without
    _sleep, 64-MiB device-to-device copies) last a millisecond.  Returns the
    figure in words, for assertion messages."""
    global _cal, _copy_bufs
    if _cal is not None:
        return _cal[2]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(1000)  # loads the kernel
            s.synchronize()
            cycles = 1_000_000
            ms = _time_ms(lambda: torch.cuda._sleep(cycles), s)
            if ms < 5.0:  # a fast counter: measure over about 10 ms
                cycles = int(cycles * 10.0 / max(ms, 1e-3))
                ms = _time_ms(lambda: torch.cuda._sleep(cycles), s)
            _cal = ("sleep", cycles / ms, f"_sleep({cycles}) took {ms:.3f} ms: {cycles / ms:.0f} cycles per ms")
        else:
            n = 64 << 20
            _copy_bufs = (torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda"))
            _copy_bufs[1].copy_(_copy_bufs[0])
            s.synchronize()
            reps = 16
            ms = _time_ms(lambda: [_copy_bufs[1].copy_(_copy_bufs[0]) for _ in range(reps)], s)
            _cal = ("copy", reps / ms, f"{reps} device copies of 64 MiB took {ms:.3f} ms: {reps / ms:.2f} copies per ms")
    s.synchronize()
    return _cal[2]


def calibration():
    """The calibrated figure in words (calibrate() must have run)."""
    return _cal[2] if _cal else "not calibrated"


def busy(stream, ms=DEFAULT_MS):
    """Enqueue a delay of about `ms` milliseconds on `stream` and return at once."""
    calibrate()
    kind, per_ms, _ = _cal
    with torch.cuda.stream(stream):
        if kind == "sleep":
            torch.cuda._sleep(int(per_ms * ms))
        else:
            for _ in range(max(1, int(per_ms * ms))):
                _copy_bufs[1].copy_(_copy_bufs[0])


class Gate:
    """An event recorded on a stream right after the input write: pending()
    while the stream has not reached it."""

    def __init__(self, stream):
        self.event = torch.cuda.Event()
        self.event.record(stream)

    def pending(self):
        return not self.event.query()


def run_busy(call, stream, staged, inp, ms=DEFAULT_MS, call_stream=None):
    """Behind a delay of `ms` on `stream`, write the real input (`staged`, a
    list of device tensors, complete and synchronised) over the decoy in `inp`
    (device to device, no host sync), record a Gate, assert that it is still
    pending, and make `call(s)` under torch.cuda.stream(s), s being
    `call_stream` or else `stream` itself.  Returns (what call returned, the
    gate).  Every tensor the call needs was allocated before."""
    busy(stream, ms)
    with torch.cuda.stream(stream):
        for dst, src in zip(inp, staged):
            dst.copy_(src, non_blocking=True)
    gate = Gate(stream)
    assert gate.pending(), f"premise: the input write is still pending at the call ({calibration()}, delay {ms} ms)"
    s = stream if call_stream is None else call_stream
    with torch.cuda.stream(s):
        result = call(s)
    return result, gate


def independent(a, b, scratch, ms=20.0):
    """True when work on stream `b` does not wait for work on stream `a`:
    streams that HIP maps onto one hardware queue run one after the other
    (GPU_MAX_HW_QUEUES, 4 by default).  `scratch`: a small device tensor."""
    busy(a, ms)
    ev = torch.cuda.Event()
    ev.record(a)
    with torch.cuda.stream(b):
        scratch.fill_(1)
    b.synchronize()
    ok = not ev.query()
    a.synchronize()
    return ok


def independent_streams(want, tries=12):
    """Up to `want` fresh non-blocking streams none of which waits for
    another (see independent()), chosen among `tries` streams of torch's pool."""
    calibrate()
    scratch = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    kept = []
    for _ in range(tries):
        s = torch.cuda.Stream()
        if any(s.cuda_stream == k.cuda_stream for k in kept):
            continue
        if all(independent(k, s, scratch) and independent(s, k, scratch) for k in kept):
            kept.append(s)
        if len(kept) == want:
            break
    torch.cuda.synchronize()
    return kept


def fetch_via(tensors, hosts, other):
    """Copy device tensors into preallocated pinned host tensors on the stream
    `other` and synchronise that stream only; returns numpy views."""
    with torch.cuda.stream(other):
        for h, t in zip(hosts, tensors):
            h.copy_(t, non_blocking=True)
    other.synchronize()
    return [h.numpy() for h in hosts]

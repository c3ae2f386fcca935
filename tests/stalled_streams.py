"""Streams that lag on purpose, for tests/test_route_streams_gpu.py: a calibrated device-side sleep (``stall``) and a factory that
remembers every torch stream made while it is armed and stalls it at birth (``StalledFactory``).  A stream that is busy sleeping
makes an ordering slip deterministic: work that should have waited for it runs early and reads what the inputs held before, work
that nobody waits for has not run when its result is read.  This is no test module: it holds no test.  It sets no environment
variable, touches no queue setting and starts no process."""
import functools

STALL_MS = 100.0                           # a choice, not a measurement: tests assert per case that the stall outlasted the call
PROBE_CYCLES = 1 << 22                     # the sleep that is timed once to find the cycles per millisecond
LOW, HIGH = 0.8, 4.0                       # the chosen count must really stall between LOW x and HIGH x the target


def _timed_sleep(torch, cycles, stream):
    """Milliseconds one torch.cuda._sleep(cycles) takes on `stream`, between a pair of events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record(stream)
        torch.cuda._sleep(int(cycles))
        b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


@functools.lru_cache(maxsize=None)
def calibrate(device_index=0, target_ms=STALL_MS):
    """-> (cycles of a `target_ms` stall, the milliseconds the probe took, the milliseconds the chosen count took).  The probe is timed
    once (after one untimed sleep, so that the first launch's set-up is not in it); the chosen count is then timed once and must lie in
    [LOW, HIGH] x target."""
    import torch
    stream = torch.cuda.Stream(torch.device('cuda', device_index))
    _timed_sleep(torch, 1 << 10, stream)
    probe_ms = _timed_sleep(torch, PROBE_CYCLES, stream)
    assert probe_ms > 0.0, probe_ms
    cycles = int(PROBE_CYCLES * target_ms / probe_ms)
    took_ms = _timed_sleep(torch, cycles, stream)
    assert LOW * target_ms <= took_ms <= HIGH * target_ms, (
        f'{cycles} cycles stall {took_ms:.1f} ms, not {target_ms} ms (the probe of {PROBE_CYCLES} cycles took {probe_ms:.3f} ms)')
    return cycles, probe_ms, took_ms


def stall(stream):
    """Enqueues the calibrated sleep on `stream` -> an event recorded right after it (``not e.query()``: the stream is still stalled)."""
    import torch
    cycles = calibrate(stream.device.index)[0]
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        e = torch.cuda.Event()
        e.record(stream)
    return e


class StalledFactory:
    """``torch.cuda.Stream`` replaced (through pytest's monkeypatch) by a function that makes the stream, remembers it and stalls it
    at birth.  Wrapping an existing handle (``stream_id=`` / ``stream_ptr=``, what torch.cuda.current_stream does) passes through
    untouched.  ``stall_all()`` stalls every remembered stream again: for objects that keep a stream across calls."""

    def __init__(self, monkeypatch):
        import torch
        self.torch, self.stream_type, self.made, self.armed = torch, torch.cuda.Stream, [], False
        calibrate()                                                          # with the real stream type, before the patch
        monkeypatch.setattr(torch.cuda, 'Stream', self._make)

    def _make(self, *args, **kwargs):
        s = self.stream_type(*args, **kwargs)
        if self.armed and 'stream_id' not in kwargs and 'stream_ptr' not in kwargs:
            self.made.append(s)
            stall(s)
        return s

    def arm(self):
        self.armed = True
        return self

    def disarm(self):
        self.armed = False

    def stall_all(self):
        return [stall(s) for s in self.made]

    def synchronize(self):
        for s in self.made:
            s.synchronize()

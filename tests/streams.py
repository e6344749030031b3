"""A deterministic adversarial schedule for two HIP streams (helper of tests/test_gpu_streams.py; nothing here is collected).

A race between two streams is lost almost never when both run freely: the stream that ought to be waited for has usually finished before
the other one starts.  `Stall` makes it lose every time: it keeps one stream busy for a chosen wall time, everything the schedule puts
behind the stall has then not started when the other stream runs, and a missing event wait or a block freed too early shows as wrong
numbers.

The stall is torch.cuda._sleep, a kernel that spins for a given number of clock ticks (the fall-back the design allowed for, a chain of
large matmuls, is not needed: _sleep spins for the requested ticks on the MI355X).  Ticks per millisecond are measured once per process
(`ticks_per_ms`), with two timing events round one _sleep.  A stall is a bounded spin -- at most CAP_S seconds -- never a wait on something
that may not come.

Its length is not fixed in advance: the larger of MIN_S and ten times the host time that enqueueing the calls of the schedule took when
the test measured it (`stall_seconds`), capped at CAP_S.  Every schedule checks its premise after its last call has been enqueued
(`Stall.assert_held`): the event recorded right behind the stall must still be pending -- "the stalled stream had not started when the
other stream was launched".  A false premise FAILS the test with that message; it neither skips nor passes.

Nothing here may fault: a stale read in these schedules reads allocated memory that holds old, unwritten or NaN floats.  `poison`
allocates NaN-filled tensors of given sizes on a given stream -- what makes a block that was handed out too early visibly wrong -- and
reports whether one of them landed inside the address ranges it was meant to hit (the reuse premise: the caching allocator hands a freed
block to the next request of the same size on the same stream).
"""
import time

import torch

MIN_S, CAP_S = 0.25, 2.0
_TICKS = {}


def ticks_per_ms(device=None):
    """clock ticks of torch.cuda._sleep per millisecond, measured once per device: one _sleep between two timing events, its length
    grown until it takes at least 20 ms (launch overhead below 1 %)"""
    dev = torch.cuda.current_device() if device is None else torch.device(device).index or 0
    if dev not in _TICKS:
        with torch.cuda.device(dev):
            ticks, ms = 1 << 20, 0.0
            while True:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                torch.cuda._sleep(ticks)
                b.record()
                b.synchronize()
                ms = a.elapsed_time(b)
                if ms >= 20.0 or ticks >= 1 << 36:
                    break
                ticks <<= 2
            assert ms >= 20.0, "torch.cuda._sleep(%d) took %.3f ms: it does not spin on this device" % (ticks, ms)
            _TICKS[dev] = ticks / ms
    return _TICKS[dev]


def stall_seconds(host_seconds):
    """the larger of MIN_S and ten times the measured host time of the schedule's calls, capped at CAP_S"""
    return min(CAP_S, max(MIN_S, 10.0 * float(host_seconds)))


def timed(fn):
    """(result, host seconds) of enqueueing fn(): no synchronisation inside the timed region"""
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


class Stall:
    """Keeps `stream` busy for stall_seconds(host_seconds) from now on and records an event right behind the spin."""

    def __init__(self, stream, host_seconds):
        self.stream = stream
        self.seconds = stall_seconds(host_seconds)
        self.host_seconds = float(host_seconds)
        ticks = int(self.seconds * 1e3 * ticks_per_ms(stream.device))
        self.t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            torch.cuda._sleep(ticks)
        self.event = torch.cuda.Event()
        self.event.record(stream)

    def assert_held(self):
        """the premise of every schedule, checked after its last call has been enqueued"""
        took = time.perf_counter() - self.t0
        assert not self.event.query(), (
            "premise false: the stalled stream had ALREADY started when the other stream was launched -- the %.3f s stall (ten times the "
            "%.4f s the calls took when measured, at least %.2f s, at most %.1f s) ran out while the schedule was being enqueued "
            "(%.3f s): something in it synchronised the host or took far longer than measured; the schedule proves nothing like this"
            % (self.seconds, self.host_seconds, MIN_S, CAP_S, took))


def span(t):
    s = t.untyped_storage()
    return s.data_ptr(), s.data_ptr() + s.nbytes()


def poison(like, stream, ranges=(), rounds=1):
    """NaN-filled tensors of the shapes and dtypes of `like`, allocated and filled on `stream` (`rounds` of them per entry, stopping early
    at the first that lands inside one of `ranges` = [(lo, hi), ...]).  Returns (the tensors -- keep them alive for as long as the
    poison must stay --, how many entries of `like` got a tensor inside `ranges`)."""
    keep, hits = [], 0
    with torch.cuda.stream(stream):
        for shape, dtype in like:
            for _ in range(rounds):
                t = torch.full(shape, float("nan"), dtype=dtype, device=stream.device)
                keep.append(t)
                if any(lo <= t.data_ptr() < hi for lo, hi in ranges):
                    hits += 1
                    break
    return keep, hits


def shapes_of(tensors):
    """[(shape of the whole storage as a flat tensor, dtype)] -- what `poison` takes -- for tensors that may be views"""
    return [((t.untyped_storage().nbytes() // t.element_size(),), t.dtype) for t in tensors]


REUSE = ("reuse premise false: no NaN tensor landed inside the freed block -- this schedule needs the caching allocator to hand a freed "
         "block to the next request of the same size on the same stream; without that the broken fake cannot be shown to be broken")

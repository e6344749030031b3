"""-m gpu: stream order.  Packed weights, results and inputs that cross from one HIP stream to another, under a schedule that makes a
missing ordering lose every time (tests/streams.py: one stream is held busy while the other runs).

bench.py's headline figure keeps two forwards in flight on two streams (parallel.InFlight); the packed weights are built with
asynchronous kernels on the stream of the call that misses and are read from both, a replaced pack is freed while the other stream may
still read it, and InFlight hands a result allocated on its private stream to a caller on another one.  Run freely, every one of these
orderings is kept by timing alone.  Here one stream is stalled behind a spin kernel, the premise -- the stalled stream had not started
when the other was launched -- is asserted in every test, and the oracle is the serial result on one stream, compared with torch.equal
(as tests/test_gpu_lifecycle.py does: every kernel has a fixed summation order, so no tolerance appears).

Section 1 proves the schedule on toy modules in plain torch (no project kernel; the convention of test_guard_host.py / test_exact_host.py:
the harness shows that it sees the fault before it is trusted).  Each broken fake must be caught, each corrected twin must pass the
identical schedule.  Section 2 runs the project under the same schedules.

Nothing here may fault: a stale read in these schedules reads allocated memory holding old, unwritten or NaN floats.  Every model is
checked before use (`check_pack_is_plain`): its eval pack holds floating-point tensors only -- no integer table from which a kernel
derives an address -- and none of them aliases a parameter.  The train path (autograd._PACKS, single-stream per model) stays out.

dtype: bf16, the benchmark's.  One exception: Mixer-B/16 in the two schedules that PACK on the stalled stream runs in fp16 -- the bf16
pack of the generated token kernel (engine.pack_token_mlp, layout 3) reads max |W2| back to the host once per block, the host then waits
out the stall and the premise is false by construction; the fp16 pack takes the same kernel family (layout 2) without the read-back."""
import contextlib
import importlib

import pytest
import torch

import streams as S
from conftest import load_pkg
from test_gpu_lifecycle import DEV, cold_model, gen, images, run, warm_model
from test_lifecycle_host import AT224, config, noise_like

pytestmark = pytest.mark.gpu
MODELS = ["mixer", "hiremlp", "vip_weighted", "mixer_b16" + AT224, "hiremlp_s" + AT224]
SIDE_MODELS = ["hiremlp", "vip_weighted", "hiremlp_s" + AT224]         # the families with a SideChain (one side stream per device)
NAN = float("nan")


def mismatches(got, want):
    """the checker: indices of the results that are not bit-equal to the serial ones"""
    assert len(got) == len(want)
    return [i for i, (g, w) in enumerate(zip(got, want)) if not torch.equal(g, w)]


# ====================================================================== 1. broken fakes that the schedule must catch
N_W = 2400          # the fakes' weight is (N_W, N_W) fp32; its bf16 pack is 11.5 MB: a request above 10 MB gets a segment of its own


def fake_weight(seed):
    return torch.randn((N_W, N_W), generator=gen(seed)).to(DEV)


def fake_input(seed):
    return torch.randn((N_W,), generator=gen(seed)).to(DEV)


class FakeNoEvent:
    """Caches w.to(bfloat16) keyed by w's version, as EngineModule._get_pack did: the conversion is asynchronous on the stream of the
    call that missed, and a hit on another stream reads the pack with nothing in between."""

    def __init__(self, w):
        self.w, self.hit = w, None

    def build(self):
        return {"version": self.w._version, "pack": self.w.to(torch.bfloat16)}

    def use(self, hit):
        return hit["pack"]

    def __call__(self, x):
        if self.hit is None or self.hit["version"] != self.w._version:
            self.hit = self.build()                     # (the old pack is freed here)
        return x + self.use(self.hit).float()           # elementwise: the same bits on any stream


class FakeWithEvent(FakeNoEvent):
    """the corrected twin: an event behind the conversion, and a stream wait for a call on another stream.  Still frees a replaced pack
    at once: the broken fake of the next schedule."""

    def build(self):
        hit = super().build()
        hit["stream"], hit["event"] = torch.cuda.current_stream(), torch.cuda.Event()
        hit["event"].record(hit["stream"])
        return hit

    def use(self, hit):
        if torch.cuda.current_stream() != hit["stream"]:
            torch.cuda.current_stream().wait_event(hit["event"])
        return hit["pack"]


FakeFreesEarly = FakeWithEvent


class FakeRecordsStream(FakeWithEvent):
    """the corrected twin of FakeFreesEarly: every stream that reads the pack is made known to the allocator"""

    def use(self, hit):
        if torch.cuda.current_stream() != hit["stream"]:
            hit["pack"].record_stream(torch.cuda.current_stream())
        return super().use(hit)


def schedule_cold(make, seed):
    """stream A is stalled and then called cold, B is called straight after.  Returns (serial, [on A, on B], the pack took the poisoned
    block)."""
    torch.cuda.empty_cache()
    w, xs = fake_weight(seed), [fake_input(seed + 1), fake_input(seed + 2)]
    ref = make(w)
    [ref(x) for x in xs]
    serial, host = S.timed(lambda: [ref(x) for x in xs])                 # warm: the pack exists
    fake = make(w)
    A, B = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    (junk,), _ = S.poison([((N_W, N_W), torch.bfloat16)], A)             # what the cold pack's block holds until the conversion has run
    at = junk.data_ptr()
    del junk
    torch.cuda.synchronize()
    stall = S.Stall(A, host)
    with torch.cuda.stream(A):
        ya = fake(xs[0])
    with torch.cuda.stream(B):
        yb = fake(xs[1])
    stall.assert_held()
    torch.cuda.synchronize()
    print("cold: stall %.3f s, host %.5f s" % (stall.seconds, host))
    return serial, [ya, yb], fake.hit["pack"].data_ptr() == at


def test_fake_no_event_is_caught():
    serial, got, reused = schedule_cold(FakeNoEvent, 200)
    assert reused, S.REUSE
    assert mismatches(got, serial) == [1], "the schedule did not catch a pack read on stream B before stream A had built it"
    assert torch.isnan(got[1]).all()


def test_fake_with_event_passes():
    serial, got, _ = schedule_cold(FakeWithEvent, 210)
    assert mismatches(got, serial) == []


def schedule_replaced(make, seed):
    """stream B is stalled with a read of the old pack queued; the weight is updated and a call on the main stream replaces the pack; NaN
    tensors of the old pack's size are allocated on the old pack's allocation stream.  Returns (old serial result of B's input, B's
    result, main-stream result, its serial result, NaN tensors that landed in the old block)."""
    torch.cuda.empty_cache()
    w, xb, xm = fake_weight(seed), fake_input(seed + 1), fake_input(seed + 2)
    fake = make(w)
    M = torch.cuda.current_stream()
    fake(xb)
    (old, _), host = S.timed(lambda: (fake(xb), fake(xm)))
    B = torch.cuda.Stream(DEV)
    where, like = [S.span(fake.hit["pack"])], S.shapes_of([fake.hit["pack"]])
    torch.cuda.synchronize()
    stall = S.Stall(B, host)
    with torch.cuda.stream(B):
        yb = fake(xb)
    w.add_(1.0)
    ym = fake(xm)
    keep, hits = S.poison(like, M, where, rounds=4)
    stall.assert_held()
    torch.cuda.synchronize()
    print("replaced: stall %.3f s, host %.5f s, %d NaN tensor(s) in the old block" % (stall.seconds, host, hits))
    return old, yb, ym, xm + w.to(torch.bfloat16).float(), hits


def test_fake_frees_early_is_caught():
    old, yb, ym, want_m, hits = schedule_replaced(FakeFreesEarly, 220)
    assert hits == 1, S.REUSE
    assert mismatches([yb], [old]) == [0], "the schedule did not catch a pack freed and overwritten under a queued reader"
    assert torch.equal(ym, want_m)


def test_fake_records_stream_passes():
    old, yb, ym, want_m, hits = schedule_replaced(FakeRecordsStream, 230)
    assert hits == 0, "the allocator handed out a block that a recorded stream still reads"
    assert mismatches([yb, ym], [old, want_m]) == []


class FakeInFlight:
    """A one-slot parallel.InFlight in plain torch: f runs on a private stream behind the stream that is current at the call; the result
    is allocated on the private stream, the input on the caller's, and nothing tells the allocator that either crosses over.  This one
    class is both FakeInFlightOut and FakeInFlightIn: the two schedules drop the result and the input."""
    record_out = record_in = False

    def __init__(self):
        self.s = torch.cuda.Stream(DEV)

    def __call__(self, x):
        cur = torch.cuda.current_stream()
        self.s.wait_stream(cur)
        with torch.cuda.stream(self.s):
            out = x + 1.0                               # (one kernel, one allocation)
        if self.record_out:
            out.record_stream(cur)
        if self.record_in:
            x.record_stream(self.s)
        return out, self.s


FakeInFlightOut = FakeInFlightIn = FakeInFlight


class FakeInFlightOutRecorded(FakeInFlight):
    record_out = True


class FakeInFlightInRecorded(FakeInFlight):
    record_in = True


def big(seed):
    return torch.randn((6 * 1024 * 1024,), generator=gen(seed)).to(DEV).to(torch.bfloat16)       # 12 MB


def schedule_out_dropped(call, x1, x2, host):
    """the caller, on stream C: wait_stream, (C is stalled here), out.float().clone(), del out.  Then the slot's next call, on another
    input, made while another stream D is current -- the slot's stream waits for the stream that is current at a call, so a next call
    made on C itself would be ordered behind the clone by that wait and hide the fault.  Returns (the clone, the second result, the
    second result took the first one's block)."""
    C, D = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(C):
        out, s = call(x1)
        C.wait_stream(s)
        stall = S.Stall(C, host)
        got = out.float().clone()
        lo, hi = S.span(out)
        del out
    with torch.cuda.stream(D):
        out2, _ = call(x2)
    reused = lo <= out2.data_ptr() < hi
    stall.assert_held()
    torch.cuda.synchronize()
    print("out dropped: stall %.3f s, host %.5f s, block reused: %s" % (stall.seconds, host, reused))
    return got, out2, reused


def fake_out_dropped(cls, seed):
    torch.cuda.empty_cache()
    x1, x2 = big(seed), big(seed + 1)
    slot = cls()
    _, host = S.timed(lambda: (slot(x1), slot(x2)))
    got, out2, reused = schedule_out_dropped(slot, x1, x2, host)
    return got, (x1 + 1.0).float(), out2, x2 + 1.0, reused


def test_fake_inflight_out_is_caught():
    got, want, out2, want2, reused = fake_out_dropped(FakeInFlightOut, 240)
    assert reused, S.REUSE
    assert mismatches([got], [want]) == [0], "the schedule did not catch a result overwritten under its consumer"
    assert torch.equal(out2, want2)


def test_fake_inflight_out_recorded_passes():
    got, want, out2, want2, reused = fake_out_dropped(FakeInFlightOutRecorded, 250)
    assert not reused, "the allocator handed out a block that a recorded stream still reads"
    assert mismatches([got, out2], [want, want2]) == []


def schedule_in_dropped(call, slot_stream, make_x, host):
    """the slot's stream is stalled; the call is made, its input dropped at once and a NaN tensor of its shape allocated on the caller's
    stream.  make_x() returns a fresh input that nothing else refers to.  Returns (result, NaN tensors that landed in the input's block)."""
    M = torch.cuda.current_stream()
    x = make_x()
    where, like = [S.span(x)], S.shapes_of([x])
    torch.cuda.synchronize()
    stall = S.Stall(slot_stream, host)
    out, _ = call(x)
    del x
    keep, hits = S.poison(like, M, where, rounds=4)
    stall.assert_held()
    torch.cuda.synchronize()
    print("input dropped: stall %.3f s, host %.5f s, %d NaN tensor(s) in the input's block" % (stall.seconds, host, hits))
    return out, hits


def fake_in_dropped(cls, seed):
    torch.cuda.empty_cache()
    slot = cls()
    want, host = S.timed(lambda: slot(big(seed))[0])
    return schedule_in_dropped(slot, slot.s, lambda: big(seed), host) + (want,)


def test_fake_inflight_in_is_caught():
    out, hits, want = fake_in_dropped(FakeInFlightIn, 260)
    assert hits == 1, S.REUSE
    assert mismatches([out], [want]) == [0], "the schedule did not catch an input overwritten before the forward had read it"


def test_fake_inflight_in_recorded_passes():
    out, hits, want = fake_in_dropped(FakeInFlightInRecorded, 270)
    assert hits == 0, "the allocator handed out a block that a recorded stream still reads"
    assert mismatches([out], [want]) == []


# ====================================================================== 2. the project under the same schedules
def mods():
    pkg = load_pkg()
    return pkg.engine, importlib.import_module(pkg.__name__ + ".parallel")


@contextlib.contextmanager
def switches():
    """the two process-wide switches InFlight sets, put back whatever the body does"""
    E, _ = mods()
    plan, side = E.GEMM_PLAN_WHOLE, E.SIDE_STREAMS
    try:
        yield E
    finally:
        torch.cuda.synchronize()
        E.set_gemm_plan(plan)
        E.set_side_streams(side)


@contextlib.contextmanager
def in_flight(model, n):
    """InFlight(model, n) inside `switches()`; ends with slots.synchronize()"""
    _, parallel = mods()
    with switches():
        slots = parallel.InFlight(lambda t: run(model, t), n, device=DEV)
        try:
            yield slots
        finally:
            slots.synchronize()
            slots.close()


def dtype_for(name, packs_under_stall=False):
    """bf16; fp16 for Mixer-B/16 where the schedule packs on the stalled stream (module docstring)"""
    return torch.float16 if packs_under_stall and name == "mixer_b16" + AT224 else torch.bfloat16


def new_state(like, seed):
    """a state that no earlier test has packed: stale memory cannot hold the right pack by coincidence"""
    g = gen(seed)
    return {k: v + noise_like(v, g) for k, v in like.items()}


def packs_of(model):
    E, _ = mods()
    hits = {id(hit): hit for e in model.modules() if isinstance(e, E.EngineModule) for hit in e._packs.values()}       # (one entry under several keys)
    return [hit[1] for hit in hits.values()]


def check_pack_is_plain(model):
    """what makes a stale read harmless, confirmed on a model that has run: every leaf of every eval pack is a floating-point tensor or a
    plain number -- no integer table from which a kernel derives an address -- engine.pack_tensors finds every tensor, and no pack
    tensor shares storage with a parameter or buffer (a forward reads packs only, so an in-place update cannot reach a queued forward).
    Returns the pack tensors."""
    E, _ = mods()
    packs = packs_of(model)
    assert packs, "the model has not run"
    leaves, stack = [], list(packs)
    while stack:
        v = stack.pop()
        if isinstance(v, dict):
            stack.extend(v.values())
        elif isinstance(v, (tuple, list)):
            stack.extend(v)
        else:
            assert v is None or torch.is_tensor(v) or isinstance(v, (int, float, bool, str)), "a pack holds a %s: not walked" % type(v).__name__
            if torch.is_tensor(v):
                leaves.append(v)
    assert leaves and all(t.is_floating_point() for t in leaves), "an eval pack holds an integer tensor: keep this model out of these schedules"
    tensors = [t for p in packs for t in E.pack_tensors(p)]
    assert {S.span(t) for t in leaves} == {S.span(t) for t in tensors}, "engine.pack_tensors misses a tensor of the pack"
    own = [S.span(t) for t in model.state_dict(keep_vars=True).values()]
    for t in tensors:
        lo, hi = S.span(t)
        assert all(b <= lo or hi <= a for a, b in own), ("a pack tensor %s %s aliases a parameter: an in-place update reaches a queued forward"
                                                         % (tuple(t.shape), t.dtype))
    return tensors


@pytest.mark.parametrize("name", MODELS)
def test_cold_model_first_call_through_in_flight(name):
    """stream A is stalled; call 1 (which packs) goes to A, call 2 (a cache hit) to B: both equal the serial results of a cold model"""
    cfg, dt = config(name), dtype_for(name, True)
    sd = new_state(cfg.sd, 300)
    xs = [images(cfg, 2, dt, seed=30 + i) for i in range(2)]
    ref = cfg.fresh(sd=sd).to(DEV)
    serial, host = S.timed(lambda: [run(ref, x) for x in xs])                # a cold model's calls: the packing is in the measured time
    serial = [o.clone() for o in serial]
    like = S.shapes_of(check_pack_is_plain(ref))
    m = cfg.fresh(sd=sd).to(DEV)
    with in_flight(m, 2) as slots:
        A = slots.streams[0]
        S.poison(like, A)                                                    # (dropped at once) what A's free blocks of the pack's sizes hold: NaN
        torch.cuda.synchronize()
        stall = S.Stall(A, host)
        got = [slots(x) for x in xs]
        stall.assert_held()
        slots.synchronize()
        print("%s: stall %.3f s, host %.5f s" % (name, stall.seconds, host))
        assert got[0][1] is A and got[1][1] is slots.streams[1]
        bad = mismatches([o for o, _ in got], serial)
        assert not bad, (name, bad, "a call read packed weights that the packing stream had not written yet (1 = the cache hit on stream B)")


@pytest.mark.parametrize("name", MODELS)
def test_load_state_dict_between_calls_without_synchronize(name):
    """a warm model in flight, load_state_dict with no synchronize, then the same schedule: both results equal a cold model on the new
    state and differ from the old ones"""
    cfg, dt = config(name), dtype_for(name, True)
    m = warm_model(cfg)
    xs = [images(cfg, 2, dt, seed=32 + i) for i in range(2)]
    with in_flight(m, 2) as slots:
        old = [slots(x)[0] for x in xs]
        slots.synchronize()
        check_pack_is_plain(m)
        _, host = S.timed(lambda: [slots(x) for x in xs])
        new = new_state(m.state_dict(), 310)
        torch.cuda.synchronize()
        A = slots.streams[0]
        stall = S.Stall(A, host)
        m.load_state_dict(new)
        got = [slots(x) for x in xs]
        stall.assert_held()
        slots.synchronize()
        print("%s: stall %.3f s, host %.5f s" % (name, stall.seconds, host))
        assert got[0][1] is A
        cold = cold_model(cfg, m)
        want = [run(cold, x) for x in xs]
        bad = mismatches([o for o, _ in got], want)
        assert not bad, (name, bad, "a call after load_state_dict did not run on the new state")
        assert mismatches([o for o, _ in got], old) == [0, 1], (name, "the update was a no-op: the case checks nothing")


@pytest.mark.parametrize("name", MODELS)
def test_pack_replaced_under_a_stalled_reader(name):
    """B is stalled with a forward on the old weights queued; the weights are updated in place, a call on A packs again and drops the
    old pack, and NaN tensors of the old pack's sizes are allocated on the stream the old pack was allocated on.  B's result is the
    serial old-weights result bit for bit, and finite."""
    cfg, dt = config(name), dtype_for(name)
    m = warm_model(cfg)
    xs = [images(cfg, 2, dt, seed=34 + i) for i in range(2)]
    M = torch.cuda.current_stream()
    old = [run(m, x).clone() for x in xs]                                    # packs on M: the old pack's allocation stream
    with in_flight(m, 2) as slots:
        [slots(x) for x in xs]
        slots.synchronize()
        _, host = S.timed(lambda: [slots(x) for x in xs])
        tensors = check_pack_is_plain(m)
        where, like = [S.span(t) for t in tensors], S.shapes_of(tensors)
        del tensors
        new = new_state(m.state_dict(), 320)
        torch.cuda.synchronize()
        B = slots.streams[0]
        stall = S.Stall(B, host)
        ob, sb = slots(xs[0])
        m.load_state_dict(new)
        oa, _ = slots(xs[1])
        keep, hits = S.poison(like, M, where, rounds=3)
        stall.assert_held()
        slots.synchronize()
        print("%s: stall %.3f s, host %.5f s, %d of %d NaN allocations landed in the old pack's blocks" % (name, stall.seconds, host, hits, len(like)))
        assert sb is B
        assert torch.isfinite(ob.float()).all(), (name, "the stalled forward read a block that had been handed out again")
        assert torch.equal(ob, old[0]), (name, "the stalled forward did not run on the weights it was called with")
        assert torch.equal(oa, run(cold_model(cfg, m), xs[1])) and not torch.equal(oa, old[1])


@pytest.mark.parametrize("name", MODELS)
def test_result_consumed_and_dropped_by_the_caller(name):
    """InFlight(model, 1): wait_stream, the caller's stream stalled, out.float().clone() queued, del out; then the slot's next call on
    another input (schedule_out_dropped).  The clone equals the serial logits of the first input."""
    cfg, dt = config(name), dtype_for(name)
    m = warm_model(cfg)
    x1, x2 = images(cfg, 2, dt, seed=36), images(cfg, 2, dt, seed=37)
    want1, want2 = run(m, x1).float().clone(), run(m, x2).clone()
    with in_flight(m, 1) as slots:
        slots(x1)
        slots.synchronize()
        _, host = S.timed(lambda: (slots(x1), slots(x2)))
        got, out2, _ = schedule_out_dropped(slots, x1, x2, host)
        slots.synchronize()
        assert torch.equal(got, want1), (name, "the result was overwritten by the slot's next forward before the caller's stream had read it")
        assert torch.equal(out2, want2)


@pytest.mark.parametrize("name", MODELS)
def test_input_dropped_right_after_the_call(name):
    """the slot is stalled, x is dropped as soon as the call returns and a NaN tensor of its shape is allocated on the caller's stream:
    the result equals serial"""
    cfg, dt = config(name), dtype_for(name)
    m = warm_model(cfg)
    want = run(m, images(cfg, 2, dt, seed=38)).clone()
    with in_flight(m, 1) as slots:
        slots(images(cfg, 2, dt, seed=38))
        slots.synchronize()
        _, host = S.timed(lambda: slots(images(cfg, 2, dt, seed=39)))
        out, _ = schedule_in_dropped(slots, slots.streams[0], lambda: images(cfg, 2, dt, seed=38), host)
        slots.synchronize()
        assert torch.equal(out, want), (name, "the input's block was handed out again before the forward had read it")


@pytest.mark.parametrize("name", SIDE_MODELS)
def test_two_plain_streams_with_side_streams_on(name):
    """no InFlight: two torch streams of the caller's, side streams on (both forwards fork to the device's ONE side stream), stream A
    stalled: both equal serial"""
    cfg, dt = config(name), dtype_for(name)
    with switches() as E:
        E.set_side_streams(True)
        m = warm_model(cfg)
        xs = [images(cfg, 2, dt, seed=40 + i) for i in range(2)]
        [run(m, x) for x in xs]
        serial, host = S.timed(lambda: [run(m, x) for x in xs])
        serial = [o.clone() for o in serial]
        check_pack_is_plain(m)
        A, B = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
        torch.cuda.synchronize()
        stall = S.Stall(A, host)
        with torch.cuda.stream(A):
            oa = run(m, xs[0])
        with torch.cuda.stream(B):
            ob = run(m, xs[1])
        stall.assert_held()
        torch.cuda.synchronize()
        print("%s: stall %.3f s, host %.5f s" % (name, stall.seconds, host))
        assert E.SIDE_STREAMS
        assert mismatches([oa, ob], serial) == [], name


@pytest.mark.parametrize("name", MODELS)
def test_three_batch_sizes_alternating_over_two_streams(name):
    """batches 1, 2, 3, 1, 2, 3 over two slots = six (batch, stream) workspaces on top of the serial ones: past the bound of four, so
    workspaces are evicted while the forwards that use them are still queued behind the stall.  All equal serial."""
    cfg, dt = config(name), dtype_for(name)
    m = warm_model(cfg)
    xs = [images(cfg, b, dt, seed=42 + i) for i, b in enumerate((1, 2, 3, 1, 2, 3))]
    [run(m, x) for x in xs[:3]]
    serial, host = S.timed(lambda: [run(m, x) for x in xs])
    serial = [o.clone() for o in serial]
    with in_flight(m, 2) as slots:
        check_pack_is_plain(m)
        torch.cuda.synchronize()
        stall = S.Stall(slots.streams[0], host)
        got = [slots(x)[0] for x in xs]
        stall.assert_held()
        slots.synchronize()
        print("%s: stall %.3f s, host %.5f s" % (name, stall.seconds, host))
        assert len(m._spaces) <= 4
        assert mismatches(got, serial) == [], name


def test_with_in_flight_restores_the_switches_on_normal_exit():
    E, parallel = mods()
    with switches():
        E.set_gemm_plan(False)
        E.set_side_streams(True)
        with parallel.InFlight(lambda t: t, 2, device=DEV) as slots:
            assert (E.GEMM_PLAN_WHOLE, E.SIDE_STREAMS) == (True, False)
            slots.synchronize()
        assert (E.GEMM_PLAN_WHOLE, E.SIDE_STREAMS) == (False, True)
        slots.close()                                   # idempotent: a second close does not put an older state back
        slots.restore_plan()
        assert (E.GEMM_PLAN_WHOLE, E.SIDE_STREAMS) == (False, True)


def test_with_in_flight_restores_the_switches_when_the_body_raises():
    E, parallel = mods()
    with switches():
        E.set_gemm_plan(False)
        E.set_side_streams(True)
        with pytest.raises(ZeroDivisionError):
            with parallel.InFlight(lambda t: t, 2, device=DEV) as slots:
                assert (E.GEMM_PLAN_WHOLE, E.SIDE_STREAMS) == (True, False)
                1 / 0
        slots.synchronize()
        assert (E.GEMM_PLAN_WHOLE, E.SIDE_STREAMS) == (False, True)
        # the last resort: an object that was never closed puts the switches back when it is collected
        parallel.InFlight(lambda t: t, 2, device=DEV)
        import gc
        gc.collect()
        assert (E.GEMM_PLAN_WHOLE, E.SIDE_STREAMS) == (False, True)

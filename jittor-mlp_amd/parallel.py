"""Data-parallel inference across the GPUs of one node: one process per GPU, weights replicated,
the batch sharded on dim 0 in equal contiguous slices, and ONE collective per forward -- an
all-gather of the (B_local, num_classes) logits (RCCL over xGMI).  Images are
independent in eval mode, so there is no exchange inside the model.  The reference has no
distributed code at all; this is new.

The message is tiny (256 x 1000 logits = 0.5-1 MB per rank), i.e. latency-bound on the xGMI mesh:
it is issued through torch.distributed (backend "nccl" == RCCL on ROCm) right behind the head GEMM,
stream-ordered (no host synchronisation), so successive forwards pipeline.

Ordering relied upon (ProcessGroupNCCL, synchronous-op form): the kernels of the forward are enqueued on
torch's current stream S of the rank's device (engine.stream()); all_gather_into_tensor records an event
on S and makes the process group's RCCL stream wait for it, enqueues ncclAllGather there, records the
collective's end event and makes S wait for that event before returning.  Everything later on S
(the next forward, a copy of the result) is therefore ordered after the gather, and the gather after the
head GEMM, with no host-side synchronisation anywhere; the result tensor is allocated on S and, in this
wrapper, only ever touched on S.  InFlight (below) is where a second stream enters: there the input and the
result cross streams and are made known to the allocator with record_stream, and the packed weights are
ordered across streams by EngineModule._get_pack (streams).
tests/test_gpu_parallel.py runs the collective path with two ranks (HIP forward + collective) and checks the
rows bit for bit; tests/test_gpu_streams.py holds the cross-stream ordering under an adversarial schedule.
"""
import torch


def shard_batch(x, rank, world):
    """Equal contiguous slice of a global batch for `rank` (dim 0 must divide evenly)."""
    n = x.shape[0]
    if n % world:
        raise ValueError("global batch %d is not divisible by %d ranks" % (n, world))
    per = n // world
    return x[rank * per:(rank + 1) * per]


class DataParallelForward:
    """Callable wrapper: local forward + all-gather of the logits in rank order.

    forward_fn : callable mapping the local shard (B_local, ...) to (B_local, num_classes)
    world      : number of ranks (1 = no collective, no process group needed)
    group      : optional torch.distributed process group (default group when None)
    force_collective : issue the all-gather for world == 1 too (a one-rank RCCL group on a single-GPU box: exercises
                 the collective and its stream ordering where no second GPU exists)
    """

    def __init__(self, forward_fn, world=1, group=None, force_collective=False):
        self.forward_fn = forward_fn
        self.world = world
        self.group = group
        self.force_collective = force_collective

    def __call__(self, x_local):
        logits = self.forward_fn(x_local)
        if self.world == 1 and not self.force_collective:
            return logits
        import torch.distributed as dist
        logits = logits.contiguous()
        shape = (self.world * logits.shape[0],) + tuple(logits.shape[1:])
        # a fresh result per call (torch's caching allocator makes this free): the caller may keep step i's logits
        # while step i+1 is already running
        out = torch.empty(shape, dtype=logits.dtype, device=logits.device)
        if dist.get_backend(self.group) == "nccl":
            dist.all_gather_into_tensor(out, logits, group=self.group)       # one ncclAllGather straight into `out`
        else:
            # gloo (CPU tests, or two ranks sharing one GPU): the list form, gathering into the row blocks of `out`
            dist.all_gather(list(out.chunk(self.world, dim=0)), logits, group=self.group)
        return out


class InFlight:
    """Keep `n` forwards in flight on one GPU (round 6): successive calls alternate over `n` HIP streams, so the next request's workgroups
    fill the CUs that the tail of the current request's persistent kernels leaves idle (every big kernel of the path is a persistent grid
    with a static tile list: a launch ends with a partly empty last round).  Each stream has its own workspace inside the model
    (EngineModule._get_space is keyed by the stream), the packed weights are shared and ordered across the streams by the model
    (EngineModule._get_pack), the kernels and hence the results are the same bits as one call after the other.
    Same-box: Mixer-B/16 at 256 images 34.65 -> 36.55 k images/s with n = 2; n = 3 adds nothing (profiles/r06_two_steps_in_flight_probe.txt).

        with InFlight(model, 2) as slots:
            out, stream = slots(x)      # enqueued, not waited for
            ...
            torch.cuda.current_stream().wait_stream(stream)   # (or stream.synchronize()) before `out` is consumed elsewhere

    What a call does for the caller: the slot's stream waits for the stream that is current at the call (x may have been produced there),
    `x` is made known to the allocator for the slot's stream and `out` for the caller's stream (record_stream), so either may be dropped as
    soon as the last use has been ENQUEUED.  What the caller still owes: a wait_stream (or synchronize) before `out` is consumed on another
    stream, a record_stream of their own if that stream is not the one the call was made on, and no write to `x` until the call has run.

    While the object is open two process-wide switches are set (the GEMM tile plan and the side streams, see __init__); close() -- also the
    end of the `with` block, and as a last resort the destructor -- puts back what the constructor found.
    """

    def __init__(self, forward_fn, n=2, device=None, throughput_plan=True):
        self.forward_fn = forward_fn
        self.streams = [torch.cuda.Stream(device=device) for _ in range(max(1, int(n)))]
        self._i = 0
        if throughput_plan and len(self.streams) > 1:
            # with several forwards sharing the chip the persistent GEMM's plan with the least TOTAL work wins over the one with the shortest
            # single launch (engine.set_gemm_plan): whole 256-row tiles.  Process-wide, same bits; close() undoes it.
            from . import engine as E
            self._old_plan = E.GEMM_PLAN_WHOLE
            E.set_gemm_plan(True)
            # ... and a model's own side stream (Hire-MLP's second branch chain) only couples the in-flight streams: issue in line
            self._old_side = E.SIDE_STREAMS
            E.set_side_streams(False)

    def close(self):
        """Put the two process-wide switches back (idempotent).  Work already enqueued is not waited for: synchronize() does that."""
        if hasattr(self, "_old_plan"):
            from . import engine as E
            old_plan, old_side = self._old_plan, self._old_side
            del self._old_plan
            E.set_gemm_plan(old_plan)
            E.set_side_streams(old_side)

    restore_plan = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:           # interpreter shutdown: the library or the module globals may be gone
            pass

    def __call__(self, x):
        s = self.streams[self._i % len(self.streams)]
        self._i += 1
        cur = torch.cuda.current_stream(x.device)
        s.wait_stream(cur)                                         # x may have been produced on the caller's stream
        with torch.cuda.stream(s):
            out = self.forward_fn(x)
        x.record_stream(s)                                         # x's block is not handed out again before the forward has read it
        for t in ((out,) if torch.is_tensor(out) and out.is_cuda else _tensors(out)):
            t.record_stream(cur)                                   # nor out's (allocated on s) before what the caller enqueues on `cur` has read it
        return out, s

    def synchronize(self):
        for s in self.streams:
            s.synchronize()


def _tensors(out):
    """the device tensors of a forward's result (a tensor, or tuples / lists / dicts of them)"""
    if torch.is_tensor(out):
        return [out] if out.is_cuda else []
    if isinstance(out, dict):
        out = list(out.values())
    if isinstance(out, (tuple, list)):
        return [t for v in out for t in _tensors(v)]
    return []

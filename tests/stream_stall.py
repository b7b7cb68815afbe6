"""A bounded busy period on a torch stream, for the ordering cases of tests/gpu_ordering_worker.py: a producer that is still
running when its consumer is issued on another stream, so that the library's events -- not the few microseconds a small
decode takes -- decide what the consumer reads.

    stall(stream)         queues TARGET_MS of spinning on `stream` (calibrated once per process, on the card)
    window_open(stream)   the stream has not drained: what was queued behind the stall has not run
    independent_pair()    two streams of which the second really overtakes the stalled first on this machine
    overtakes(a, b)       that control, for two given streams

torch is imported by the caller's process first (the workers' rule); nothing here needs it at import."""

TARGET_MS = 30.0    # one stall: an order of magnitude above the host time of the few calls a case issues inside it
REFUSED_MS = 250.0  # no stall may last longer: a case has one or two of them, the worker some seventy
FRESH_STREAMS = 8   # how many streams independent_pair() tries

_stall = None       # (kind, count, measured ms): set by the first stall


def _elapsed_ms(fn, stream):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        start.record()
        fn()
        end.record()
    end.synchronize()
    return start.elapsed_time(end)


def _spin(cycles):
    import torch
    torch.cuda._sleep(int(cycles))


_chain_tensor = None


def _chain(count):
    """The stand-in for _sleep: `count` in-place element-wise passes over 64 MiB."""
    global _chain_tensor
    import torch
    if _chain_tensor is None:
        _chain_tensor = torch.zeros(16 << 20, dtype=torch.float32, device="cuda")
    for _ in range(int(count)):
        _chain_tensor.add_(1.0)


def _calibrate(stream):
    """(kind, count, ms): how much of `kind` lasts TARGET_MS on this card, and how long a stall of that length then measured.
    The unit of _sleep's argument differs between cards and builds of torch (core cycles here, a fixed-rate counter
    there), so nothing is assumed about it: a probe is timed, scaled, and the result timed again."""
    import torch
    roads = ([("sleep", _spin, 1_000_000)] if hasattr(torch.cuda, "_sleep") else []) + [("chain", _chain, 16)]
    said = []
    for kind, fn, probe in roads:
        fn(1)   # (the first launch loads the kernel)
        torch.cuda.synchronize()
        ms = 0.0
        for _ in range(4):   # a probe of at least a millisecond, or this road does not spin as expected
            ms = _elapsed_ms(lambda: fn(probe), stream)
            if ms >= 1.0 or ms > REFUSED_MS:
                break
            probe *= 10
        if not 1.0 <= ms <= REFUSED_MS:
            said.append(f"{kind}: a probe of {probe} lasted {ms:.3f} ms")
            continue
        count = max(1, int(probe * TARGET_MS / ms))
        ms = _elapsed_ms(lambda: fn(count), stream)
        if TARGET_MS / 3 <= ms <= REFUSED_MS:
            return kind, count, ms
        said.append(f"{kind}: {count} lasted {ms:.3f} ms, not about {TARGET_MS}")
    raise AssertionError("no bounded stall on this card: " + "; ".join(said))


def stall_ms():
    """The measured length of one stall (None before the first)."""
    return _stall[2] if _stall else None


def stall_kind():
    return _stall[0] if _stall else None


def stall(stream):
    """Queues one busy period on `stream` and returns at once.  It neither faults nor hangs: a fixed number of cycles (or
    of passes over one tensor) that was measured on this card and refused above REFUSED_MS."""
    global _stall
    import torch
    if _stall is None:
        _stall = _calibrate(stream)
    with torch.cuda.stream(stream):
        (_spin if _stall[0] == "sleep" else _chain)(_stall[1])


def window_open(stream):
    """Called right after the consumer was issued: the stall on `stream` is still running, so whatever stands behind it has
    not run, and the consumer was issued into an open race window."""
    return not stream.query()


def overtakes(a, b):
    """The control: x.fill_(1) behind a stall on `a`, y.copy_(x) on `b` with no event and no wait.  True when y still reads
    zeros -- work on `b` really runs while `a` is stalled (two streams may share a hardware queue, and then it does not)."""
    import torch
    x = torch.zeros(4096, dtype=torch.float32, device="cuda")
    y = torch.full((4096,), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    stall(a)
    with torch.cuda.stream(a):
        x.fill_(1.0)
    with torch.cuda.stream(b):
        y.copy_(x)
    issued_in_time = window_open(a)
    a.synchronize()
    b.synchronize()
    torch.cuda.synchronize()
    return issued_in_time and bool((y == 0).all()) and bool((x == 1).all())


def independent_of(stalled, others=(), tries=FRESH_STREAMS):
    """A fresh stream that overtakes each of `stalled` and is overtaken by each of `others`, or an AssertionError."""
    import torch
    for _ in range(tries):
        s = torch.cuda.Stream()
        if all(overtakes(a, s) for a in stalled) and all(overtakes(s, b) for b in others):
            return s
    raise AssertionError(f"none of {tries} fresh streams runs beside the stalled ones: they share their hardware queues")


def independent_pair():
    """(A, B): two torch streams for which the control holds both ways, out of FRESH_STREAMS fresh ones at the most."""
    import torch
    seen = []
    for _ in range(FRESH_STREAMS):
        s = torch.cuda.Stream()
        for a in seen:
            if overtakes(a, s) and overtakes(s, a):
                return a, s
        seen.append(s)
    raise AssertionError(f"no two of {FRESH_STREAMS} fresh streams overtake each other: work on one does not run while the other is stalled")

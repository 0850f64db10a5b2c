"""Stale-then-fresh-behind-a-delay: does ALL of an entry point's work run on the caller's stream?

Every test of the suite but the stream tests runs on the legacy default stream, where a launch, fill or copy that forgot
its stream argument still runs in order.  On one of torch's side streams (non-blocking: no implicit ordering with the
null stream) the same mistake reads inputs that do not exist yet.  ``run_case`` makes that visible:

1. ``build(seed, device)`` makes two complete, valid input sets of the same shapes, FRESH and STALE.  They differ only
   in value arrays (positions, directions, table contents, float payloads); every array that determines an address in a
   later launch (counts, offsets, ids: every integer tensor, unless the case names it in ``varies``) is identical, so
   a mis-streamed middle launch that sees a mixture still stays inside its buffers.  All values are finite.
2. The call runs on the default stream with FRESH (-> ``want``) and with STALE (-> ``want_stale``), synchronised, and
   the two must differ, or the case could not notice anything.
3. STALE goes into the live input buffers, a sentinel byte pattern into the outputs (zeros where the contract says the
   call accumulates), and the device is synchronised.
4. On a new ``torch.cuda.Stream`` s: a device-side delay, FRESH copied into the live buffers from device staging
   tensors, the pre-zeroing again, the call.  Whatever went to another stream runs while the delay still spins: it reads
   STALE, or what it writes is overwritten later.
5. For an entry point that does not wait on the host, ``s.query()`` straight after the call must say "still busy"; a
   case whose delay had already run out FAILS as "delay too short" -- it never passes in that state.
6. ``s.synchronize()``; the outputs must equal ``want`` (bit for bit, or within the case's ``tol`` where the entry
   point's own test compares with a tolerance: the float-atomic scatter routes).

Conventions of a case's input dict: key ``out_*`` = an output buffer the call overwrites (sentinel-filled), ``acc_*`` =
a buffer the call accumulates into (zeroed, on s again), ``tmp_*`` = scratch between the entry point's own launches (left
alone), everything else a tensor = an input (live buffer, refilled with ``copy_``); non-tensor values (descriptors, handles, sizes) are taken from the FRESH build and must be equal in
both.  ``call(inputs)`` returns the tuple of output tensors.

The delay is ``torch.cuda._sleep(cycles)``, calibrated once per session with an event pair.  A case's delay is ten
times the host time its call took to issue on the default stream (measured after a warm-up call, against the code as it
stands), at least ``MIN_DELAY_MS``, at most ``MAX_DELAY_MS``.

Measured on an MI355X: ``_sleep`` runs 2.40 M cycles per millisecond.  Host issue times on the default stream: 0.24 ms
for the slowest case (the front-to-back field frame as separately bound launches: two selects, two field launches, the
finish), 0.12-0.21 ms for the one-call frames, 0.13 ms for qf_raster_intersect_wide, below 0.1 ms for everything else
-- ten times that is 2.4 ms at most, so every case runs behind the 20 ms floor and none reported an idle stream.
(DESIGN.md section 4b has the same figures and the time the tests take.)
"""
import time
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import torch

MIN_DELAY_MS = 20.0
MAX_DELAY_MS = 250.0
ISSUE_FACTOR = 10.0            # delay >= this many times the host's issue time of the call
SENTINEL_BYTE = 0x5A            # int32 0x5A5A5A5A: a positive count far above any capacity, so every `slot < K` guard rejects it
_CALIBRATION_CYCLES = 20_000_000


@dataclass
class Case:
    name: str
    build: Callable                       # (seed, device) -> dict
    call: Callable                        # (inputs dict) -> tuple of output tensors
    host_wait: bool = False               # the entry point itself waits on the host: no ``busy`` check
    tol: Optional[Tuple[float, float]] = None      # (rtol, atol) of the entry point's own test; None = bit for bit
    post: Optional[Callable] = None       # (inputs, outputs) -> outputs in a canonical form (lists in arrival order
                                          # sorted, as the entry point's own test compares them); runs after the wait
    compare: Optional[Callable] = None    # (got, want, fresh inputs) -> None or what differs: the entry point's own
                                          # test's comparison with ITS reference, for float-atomic accumulators
    varies: Tuple[str, ...] = ()          # integer inputs that differ between the sets (wholly structural inputs)
    entry_points: Tuple[str, ...] = ()    # the exported functions the case runs
    cpu_buildable: bool = True            # build(seed, "cpu") works (the safety conditions are checked without a GPU)


class StreamMismatch(AssertionError):
    pass


class DelayTooShort(AssertionError):
    pass


# ---------------------------------------------------------------------------------------------------- host-side parts
def delay_ms_for(issue_ms: float) -> float:
    return min(MAX_DELAY_MS, max(MIN_DELAY_MS, ISSUE_FACTOR * issue_ms))


def tensors(d: dict):
    return {k: v for k, v in d.items() if isinstance(v, torch.Tensor)}


def is_output(key: str) -> bool:
    """out_ (overwritten), acc_ (accumulated into) and tmp_ (scratch between the entry point's own launches: left as
    the STALE default-stream run left it, so that a mis-streamed middle launch reads a valid, stale state)."""
    return key.startswith(("out_", "acc_", "tmp_"))


def check_sets(case: Case, fresh: dict, stale: dict) -> None:
    """The safety conditions of the two input sets (module docstring, 1.); device-independent."""
    assert fresh.keys() == stale.keys(), case.name
    differs = False
    for k, a in fresh.items():
        b = stale[k]
        if not isinstance(a, torch.Tensor):
            continue
        assert isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype, (case.name, k)
        if is_output(k):
            continue
        if a.dtype.is_floating_point:
            assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), f"{case.name}: {k} not finite"
        same = same_bits(a, b)
        if not (a.dtype.is_floating_point or k in case.varies):
            assert same, f"{case.name}: structural input {k} differs between the fresh and the stale set"
        differs |= not same
    assert differs, f"{case.name}: the fresh and the stale set are the same"


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def outputs_match(case: Case, got, want, inputs=None) -> Optional[str]:
    """None, or which output differs and by how much."""
    assert len(got) == len(want), case.name
    if case.compare is not None and inputs is not None:
        return case.compare(got, want, inputs)
    for i, (g, w) in enumerate(zip(got, want)):
        if case.tol is None or not g.dtype.is_floating_point:
            if not same_bits(g, w):
                n_bad = int((g != w).sum()) if g.shape == w.shape else -1
                return f"output {i}: {n_bad} of {g.numel()} elements differ"
        else:
            rtol, atol = case.tol
            if not torch.allclose(g, w, rtol=rtol, atol=atol, equal_nan=True):
                return f"output {i}: max |diff| {float((g - w).abs().max()):.3e} beyond rtol {rtol} atol {atol}"
    return None


# ---------------------------------------------------------------------------------------------------- device parts
_cycles_per_ms = None
ISSUE_MS = {}                          # case name -> measured host issue time (ms); the stream tests print it


def cycles_per_ms() -> float:
    """``torch.cuda._sleep`` cycles per millisecond, timed once per session with an event pair."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        torch.cuda._sleep(1000)                       # loads the kernel
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(_CALIBRATION_CYCLES)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        assert ms > 0.5, f"torch.cuda._sleep({_CALIBRATION_CYCLES}) took {ms} ms: it does not delay on this device"
        _cycles_per_ms = _CALIBRATION_CYCLES / ms
    return _cycles_per_ms


def delay(ms: float) -> None:
    """Keep the current stream busy for ``ms`` milliseconds (device side; the host returns at once)."""
    torch.cuda._sleep(int(ms * cycles_per_ms()))


def _prefill(live: dict) -> None:
    for k, t in tensors(live).items():
        if k.startswith("out_"):
            t.view(torch.uint8).fill_(SENTINEL_BYTE) if t.is_contiguous() else t.fill_(0)
        elif k.startswith("acc_"):
            t.zero_()


def _rezero(live: dict) -> None:
    for k, t in tensors(live).items():
        if k.startswith("acc_"):
            t.zero_()


def _load(live: dict, src: dict) -> None:
    for k, t in tensors(live).items():
        if not is_output(k):
            t.copy_(src[k])


def _clone(case, live, outs):
    outs = tuple(o.clone() for o in outs)
    return tuple(case.post(live, outs)) if case.post is not None else outs


def run_case(case: Case, device):
    """Steps 1-6 of the module docstring.  Raises StreamMismatch / DelayTooShort; returns (issue_ms, delay_ms)."""
    fresh, stale = case.build(1, device), case.build(2, device)
    check_sets(case, fresh, stale)
    live = fresh            # the FRESH build's own tensors are the live buffers: objects built with them (modules,
    #                         handles, jobs) keep pointing at what the call reads
    staging = {k: t.clone() for k, t in tensors(fresh).items() if not is_output(k)}

    def on_default(src):
        _load(live, src)
        _prefill(live)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = case.call(live)
        issue = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        return _clone(case, live, outs), issue

    on_default(staging)                                # warm-up: code objects loaded, handles' scratch allocated
    want, issue_ms = on_default(staging)
    again, _ = on_default(staging)
    want_stale, _ = on_default(stale)
    if case.tol is None and case.compare is None:
        assert outputs_match(case, again, want) is None, f"{case.name}: not bit-reproducible on the default stream"
    assert outputs_match(case, want_stale, want) is not None, f"{case.name}: stale and fresh inputs give the same result"
    if case.host_wait:
        issue_ms = 0.0                                 # the call's own wait is no issue time; the floor applies
    ISSUE_MS[case.name] = issue_ms
    ms = delay_ms_for(issue_ms)

    _load(live, stale)
    _prefill(live)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=device)
    with torch.cuda.stream(s):
        delay(ms)
        _load(live, staging)
        _rezero(live)
        outs = case.call(live)
        busy = not s.query()
    s.synchronize()
    got = _clone(case, live, outs)
    torch.cuda.synchronize()
    if not case.host_wait and not busy:
        raise DelayTooShort(f"{case.name}: the stream was idle when the call returned (delay {ms:.0f} ms, issue "
                            f"{issue_ms:.2f} ms): delay too short, the case has no power")
    why = outputs_match(case, got, want, fresh)
    if why is not None:
        stale_like = outputs_match(case, got, want_stale) is None
        raise StreamMismatch(f"{case.name}: on a side stream behind a {ms:.0f} ms delay, {why}"
                             + (" (the result is the STALE inputs' result)" if stale_like else ""))
    return issue_ms, ms

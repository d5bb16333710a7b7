"""A stream gate: makes stream-order bugs of the device entry points deterministic where it can.

The caller's stream S (a torch.cuda.Stream(), which torch creates non-blocking) is held shut by a
device-side delay.  Behind the delay the REAL input is copied over a DECOY that the input buffer held
until then, the engine is called on S, every output is copied to pinned host memory on S, and the host
waits for the last of these copies alone.  So:
  - whatever the engine queues outside the order of S runs while the gate is shut: it reads the decoy, or
    what it writes is overwritten -- a wrong result (the decoy is a valid input), not a fault;
  - whatever is not joined back into S has not happened when the outputs are copied: they hold the sentinel;
  - a call that waits for the device does not come back while the gate is shut (Gate.shut()).
Between shutting the gate and the wait for the last copy there is no device-wide synchronise, no .cpu() and
no work on the default stream.

What it cannot make deterministic: the HIP runtime keeps books of its own on asynchronous COPIES -- a
device-to-host copy of a buffer waits for a host-to-device copy into that buffer that is pending on another
stream (measured on an MI355X under ROCm 7.0; kernels, memsets, device-to-device copies and copies of other
buffers do not wait).  So a kernel on the wrong stream is always seen; a mis-streamed copy is seen where its
order against the neighbouring calls matters (the sequences), not by the decoy.  The same runtime sets a
hardware queue up at a kernel's first launch on it and stalls the host for that, which is why a case is
warmed up on the very stream it is gated on.

Importing this module needs no GPU (torch is imported when a Gate is made).  Test infrastructure only.
"""
import time

import numpy as np

MIN_GATE_MS = 30.0
HOST_FACTOR = 20.0


def gate_ms(host_seconds):
    """The gate's length for calls whose host side took host_seconds on the warm-up pass."""
    return max(MIN_GATE_MS, HOST_FACTOR * host_seconds * 1e3)


class Buffers:
    """The device and pinned buffers of one call: d_in (the input buffer), h_real (the real input, pinned),
    d_decoy (the decoy, on the device), and outs = {name: (device buffer, pinned destination, init: a byte
    value or a device tensor)}."""

    def __init__(self, torch, real, decoy, outs):
        """real, decoy: uint8 arrays of one shape; outs: {name: (nbytes, init byte or uint8 array)}."""
        assert real.shape == decoy.shape and real.dtype == decoy.dtype == np.uint8
        self.torch = torch
        self.d_in = torch.empty(real.size, dtype=torch.uint8, device="cuda")
        self.h_real = torch.from_numpy(np.ascontiguousarray(real).ravel()).pin_memory()
        self.d_decoy = torch.from_numpy(np.ascontiguousarray(decoy).ravel()).cuda()
        self.outs = {}
        for name, (nbytes, init) in outs.items():
            d = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            h = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
            if not isinstance(init, int):
                init = torch.from_numpy(np.ascontiguousarray(init).ravel()).cuda()
            self.outs[name] = (d, h, init)

    def reset(self):
        """Set-up (default stream; the caller synchronises): the decoy in the input, every output its pattern."""
        self.d_in.copy_(self.d_decoy)
        for d, h, init in self.outs.values():
            if isinstance(init, int):
                d.fill_(init)
            else:
                d.copy_(init)
            h.fill_(0xEE)

    def queue_input(self):
        """On the current stream: the real input over the decoy."""
        self.d_in.copy_(self.h_real, non_blocking=True)

    def queue_collect(self):
        """On the current stream: every output to pinned memory, then the decoy over the input again."""
        for d, h, _ in self.outs.values():
            h.copy_(d, non_blocking=True)
        self.d_in.copy_(self.d_decoy, non_blocking=True)

    def result(self, name):
        return self.outs[name][1].numpy()


class Gate:
    """Calibrates the delay, finds a stream that is independent of the null stream (self_check), and shuts it."""

    def __init__(self, log=print):
        import torch
        self.torch = torch
        self.log = log
        self.kind = "sleep"
        self.cycles_per_ms = self._calibrate_sleep()
        if self.cycles_per_ms is None:   # torch.cuda._sleep unusable here: a chain of device-to-device copies
            self.kind = "copies"
            self._chain_a = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
            self._chain_b = torch.empty_like(self._chain_a)
            self.copies_per_ms = self._calibrate_copies()
        self.log("gate: %s, %s" % (self.kind, "%.0f cycles/ms" % self.cycles_per_ms if self.kind == "sleep"
                                   else "%.3f copies of 256 MiB per ms" % self.copies_per_ms))

    def _timed(self, fn):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def _calibrate_sleep(self):
        """Cycles per millisecond of torch.cuda._sleep, from two events (as torch's own tests do); None when
        the delay does not scale with its argument."""
        torch = self.torch
        if not hasattr(torch.cuda, "_sleep"):
            return None
        try:
            self._timed(lambda: torch.cuda._sleep(100000))
            n = 2000000
            ms = self._timed(lambda: torch.cuda._sleep(n))
            ms4 = self._timed(lambda: torch.cuda._sleep(4 * n))
        except Exception:
            return None
        if not (ms > 0.05 and 2.5 * ms < ms4 < 6.0 * ms):
            return None
        return 4 * n / ms4

    def _chain(self, n):
        for _ in range(n):
            self._chain_b.copy_(self._chain_a, non_blocking=True)

    def _calibrate_copies(self):
        self._timed(lambda: self._chain(2))
        return 16 / self._timed(lambda: self._chain(16))

    def delay(self, ms):
        """Queue a delay of about `ms` on the current stream."""
        if self.kind == "sleep":
            self.torch.cuda._sleep(int(ms * self.cycles_per_ms))
        else:
            self._chain(max(1, int(ms * self.copies_per_ms + 0.5)))

    def shut(self, stream, ms):
        """Shut `stream` for about ms: returns the event `opened`, recorded behind the delay.  While
        opened.query() is False the device has begun nothing queued on the stream since."""
        torch = self.torch
        with torch.cuda.stream(stream):
            opened = torch.cuda.Event(enable_timing=True)
            opened.shut_at = torch.cuda.Event(enable_timing=True)   # (opened.shut_at.elapsed_time(opened): how long it was shut)
            opened.shut_at.record(stream)
            self.delay(ms)
            opened.record(stream)
        return opened

    def self_check(self, tries=8):
        """A stream on which the detector works: with the gate shut and the real input queued behind it, a
        copy of the input buffer on torch's DEFAULT stream (waited for on that stream alone) reads the decoy,
        and the gate is still shut -- so the stream is independent of the null stream, and an engine operation
        on the wrong stream would be seen.  The copy goes to pinned memory directly or, where the runtime
        holds that back (below), by way of a snapshot on the device.  Returns the stream; None when none of
        `tries` passes in either form."""
        torch = self.torch
        n = 1 << 20
        real = np.full(n, 0xE1, np.uint8)
        decoy = np.full(n, 0x1D, np.uint8)
        buf = Buffers(torch, real, decoy, {})
        h_seen = torch.empty(n, dtype=torch.uint8).pin_memory()
        d_snap = torch.empty(n, dtype=torch.uint8, device="cuda")
        for k in range(tries):
            s = torch.cuda.Stream()
            # Two forms of the default stream's read.  "direct": the input buffer straight to pinned memory.
            # "snapshot": the input buffer to a second device buffer; that copy is what is waited for with the
            # gate shut, and the snapshot goes to pinned memory afterwards.  (The HIP runtime orders a
            # device-to-host copy of a buffer behind a host-to-device copy INTO that buffer that is pending on
            # another stream -- its own bookkeeping of the allocation, not stream order: kernels and
            # device-to-device copies, which are what an engine queues, are not held back.  Where it does,
            # the direct form waits for the gate and only the snapshot form can pass.)
            for form in ("direct", "snapshot"):
                buf.reset()
                h_seen.fill_(0)
                d_snap.zero_()
                torch.cuda.synchronize()
                opened = self.shut(s, MIN_GATE_MS)
                with torch.cuda.stream(s):
                    buf.queue_input()
                    done = torch.cuda.Event()
                    done.record(s)
                if form == "direct":                           # (the default stream)
                    h_seen.copy_(buf.d_in, non_blocking=True)
                else:
                    d_snap.copy_(buf.d_in, non_blocking=True)
                torch.cuda.default_stream().synchronize()
                still_shut = not opened.query()
                if form == "snapshot":
                    h_seen.copy_(d_snap, non_blocking=True)
                    torch.cuda.default_stream().synchronize()
                saw_decoy = bool((h_seen.numpy() == 0x1D).all())
                done.synchronize()
                arrived = bool((buf.d_in.cpu().numpy() == 0xE1).all())
                self.log("gate self-check, stream %d, %s read: decoy seen from the default stream %s, gate still "
                         "shut %s, real input behind the gate %s" % (k, form, saw_decoy, still_shut, arrived))
                if still_shut and saw_decoy and arrived:
                    return s
        return None


def timed_call(fn):
    """fn()'s host wall time in seconds."""
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0

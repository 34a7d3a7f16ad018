"""A caller's stream that runs late: the harness of tests/test_gpu_streams.py.

Every other GPU test calls the library on the null stream with the GPU idle, where a launch without its stream argument, a copy on
the null stream or a side stream that was never joined computes the right bits all the same.  Here one call sequence runs twice:

  plain  on the null stream, everything synchronised, fresh buffers -- its outputs are the expected bits;
  late   on S, a non-blocking torch.cuda.Stream.  Every user-visible device buffer starts as NaN (synchronised).  A stage of the
         sequence enqueues on S a calibrated spin (torch.cuda._sleep), then NaN into the stage's outputs once more, then the copies
         of the stage's real inputs; the library calls follow with S; at the end S copies the outputs aside, refills every buffer
         with NaN and is synchronised.  The set-aside outputs must equal the plain run's bit for bit.

While the spin runs nothing on S has happened yet: a kernel or copy on any other stream reads NaN (or the previous stage's data)
instead of its inputs, and what it writes early is overwritten by the poison behind the spin; a side stream that was not forked
from S behaves the same; a result fetched without waiting for S is read before it exists.  Only user-visible inputs and outputs
are poisoned -- never a workspace or a factor, nothing an in-launch wait could stall on.

The spin's length is no pass criterion: max(10 x device time of the plain run, 20 ms), at most 250 ms, per stage."""
import time

import numpy as np
import torch

NAN = float("nan")
F64 = dict(dtype=torch.float64, device="cuda")
SPIN_MIN_MS, SPIN_MAX_MS, SPIN_FACTOR = 20.0, 250.0, 10.0
PROBE_MS = 10.0          # the spin behind which a candidate for S is probed

_S = None
_CYCLES_PER_MS = None
LOG = []            # (label, plain ms, spin ms per stage, stages): printed by the tests (pytest -s), quoted in DESIGN_LOG.md


def _ticks_per_ms(S):
    """torch.cuda._sleep counts device clock ticks: two events around a known count give ticks per millisecond"""
    with torch.cuda.stream(S):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000000)
        S.synchronize()
        e0.record(); torch.cuda._sleep(10000000); e1.record(); S.synchronize()
    return 10000000 / max(e0.elapsed_time(e1), 1e-3)


def runs_beside_the_null_stream(S, ticks_per_ms):
    """does work on the null stream get ahead of a spin on S?  A process has few hardware queues (four by default) and every stream
    is bound to one of them; two streams on one queue run one behind the other, and a stream that shares the null stream's queue
    would hide exactly what this harness is for: the stray null-stream launch would wait for the spin like everything else."""
    flag = torch.zeros(1, **F64)
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    with torch.cuda.stream(S):
        torch.cuda._sleep(int(PROBE_MS * ticks_per_ms))
    flag.add_(1.0)                                          # on the null stream
    ev.record()
    t0 = time.perf_counter()
    while not ev.query() and time.perf_counter() - t0 < 0.5e-3 * PROBE_MS:
        pass
    ahead = ev.query() and not S.query()
    S.synchronize()
    torch.cuda.synchronize()
    return ahead


def stream():
    """S: one non-blocking stream for the whole process (handles keep its pointer until they are closed), taken from torch's pool
    -- the first one that does not share its hardware queue with the null stream (see runs_beside_the_null_stream)"""
    global _S, _CYCLES_PER_MS
    if _S is None:
        tried = []
        for _ in range(32):
            S = torch.cuda.Stream()
            if _CYCLES_PER_MS is None:
                _CYCLES_PER_MS = _ticks_per_ms(S)
            if runs_beside_the_null_stream(S, _CYCLES_PER_MS):
                _S = S
                break
            tried.append(S)
        assert _S is not None, "none of %d streams runs beside the null stream: no late stream can be built" % len(tried)
        print("LATE | S is stream %d of torch's pool to run beside the null stream" % (len(tried) + 1))
    return _S


def cycles_per_ms():
    stream()
    return _CYCLES_PER_MS


def spin(ms, on=None):
    S = stream() if on is None else on
    with torch.cuda.stream(S):
        torch.cuda._sleep(int(ms * cycles_per_ms()))


def spin_ms_for(plain_ms):
    return min(SPIN_MAX_MS, max(SPIN_MIN_MS, SPIN_FACTOR * plain_ms))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), **F64)


def poison(t):
    """NaN into a floating-point buffer, -1 into an index buffer (a row pointer of -1 is refused before anything is enqueued)"""
    return t.fill_(NAN if t.is_floating_point() else -1)


class Run:
    """One pass over a call sequence.  real: name -> device tensor with the true inputs (never handed to the library);
    outs: name -> shape of a pure output.  self.buf holds the buffers the library sees, self.ptr the hip_stream argument of the
    stand-alone entry points (None on the plain run), self.late tells the two passes apart."""

    def __init__(self, late, real, outs, spin_ms=0.0):
        self.late, self.real, self.spin_ms, self.stages = late, real, spin_ms, 0
        self.S = stream() if late else None
        self.ptr = self.S.cuda_stream if late else None
        self.buf = {k: poison(torch.empty_like(t)) for k, t in real.items()}
        self.buf.update({k: torch.full(tuple(int(d) for d in np.atleast_1d(shape)), NAN, **F64) for k, shape in outs.items()})
        torch.cuda.synchronize()

    def __getitem__(self, name):
        return self.buf[name]

    def stage(self, inputs=(), outputs=()):
        """the real inputs of the next calls arrive -- late: behind a spin on S, together with fresh poison in their outputs"""
        self.stages += 1
        if self.late:
            with torch.cuda.stream(self.S):
                torch.cuda._sleep(int(self.spin_ms * cycles_per_ms()))
                for k in outputs:
                    poison(self.buf[k])
                for k in inputs:
                    self.buf[k].copy_(self.real[k], non_blocking=True)
            assert not self.S.query(), "the spin of %.0f ms was over before the calls were made" % self.spin_ms
        else:
            for k in inputs:
                self.buf[k].copy_(self.real[k])
            torch.cuda.synchronize()

    def still_busy(self, what):
        """after calls the header documents as not waiting for the GPU: S must still be inside the stage's spin"""
        if self.late:
            assert not self.S.query(), "%s waited for the stream" % what

    def finish(self, names):
        if not self.late:
            torch.cuda.synchronize()
            return {k: self.buf[k].clone() for k in names}
        with torch.cuda.stream(self.S):
            aside = {k: self.buf[k].clone() for k in names}
            for t in self.buf.values():
                poison(t)                                       # trailing poison: nothing may still be reading or writing
        self.S.synchronize()
        torch.cuda.synchronize()
        return aside


def run_plain(seq, real, outs, names):
    """(device outputs, host values, device milliseconds) of the sequence on the null stream"""
    r = Run(False, real, outs)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    host = seq(r)
    e1.record()
    torch.cuda.synchronize()
    return r.finish(names), host, e0.elapsed_time(e1)


def run_late(seq, real, outs, names, plain_ms, label=""):
    r = Run(True, real, outs, spin_ms_for(plain_ms))
    host = seq(r)
    out = r.finish(names)
    LOG.append((label, plain_ms, r.spin_ms, r.stages))
    print("LATE | %s | plain %.3f ms | spin %.1f ms x %d stages | %.0f ticks/ms" % (label, plain_ms, r.spin_ms, r.stages, cycles_per_ms()))
    return out, host


def _bits(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if isinstance(x, (float, np.floating)):
        x = np.float64(x)
    a = np.ascontiguousarray(x)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def differences(want, got):
    """names whose bits differ; want / got: (device dict, host dict or None)"""
    bad = []
    for k, t in want[0].items():
        g = got[0][k]
        if not (torch.equal(t.view(torch.int64), g.view(torch.int64)) if t.dtype == torch.float64 else torch.equal(t, g)):
            bad.append(k)
    for k, v in (want[1] or {}).items():
        g = got[1][k]
        if isinstance(v, (tuple, list)):
            same = len(v) == len(g) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(v, g))
        else:
            same = np.array_equal(_bits(v), _bits(g))
        if not same:
            bad.append("host:" + k)
    return bad


def assert_same_bits(want, got, label):
    bad = differences(want, got)
    assert not bad, "%s: the late stream's results differ from the null-stream run in %s" % (label, bad)


def compare(seq, real, outs, names, label):
    """plain run, late run, bit comparison: for sequences that need nothing in between (stand-alone entry points)"""
    dv, host, ms = run_plain(seq, real, outs, names)
    got = run_late(seq, real, outs, names, ms, label)
    assert_same_bits((dv, host), got, label)
    return (dv, host), got

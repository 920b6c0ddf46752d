"""The harness of tests/test_gpu_stream_order.py: a caller's stream that is BUSY while the library is called on it.

Every other GPU test passes torch's default stream, uploads its input before the call and reads the output behind a device-wide wait;
a missing stream-side wait inside the library is invisible to it.  Here the caller's stream is a side stream with bounded work queued
on it (BusyStream.fill), the input reaches the device buffer by a copy queued BEHIND that work, the output leaves by a copy queued
behind the call, both buffers are NaN before and after, and every host array the headers call "reusable on return" is overwritten the
moment the call returns (scribble).

The premise -- the caller's stream was still busy when the call returned -- is a condition of every scenario that must not block, not
an assumption: PremiseError if it does not hold.  It is the test of asynchrony itself and is never confused with a DataMismatch.

Host-only at import (torch is imported where a stream is made), so tests/test_cpu_stream_order.py checks the sizing rule, the
scribbler and the header scan without a device.
"""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("ohs_hip.h", "ohs_scene.h", "ohs_scene2.h")

# ---- sizing ------------------------------------------------------------------------------------------------------------------------
# The filler is 10 x the host time the scenario took to enqueue on the quiet twin: launch-side jitter of several-fold is normal on a
# shared machine.  Never below FLOOR_S: the enqueue time is measured around the calls alone, and between two of them the busy run
# also queues its copies and scribbles its rows -- a scheduler time slice or a collection of Python's garbage in there costs
# milliseconds whatever the calls cost.  Never above CAP_S, so that one scenario's filler stays under half a second.
JITTER = 10.0
FLOOR_S = 0.05
CAP_S = 0.5
FILL_FLOATS = 1 << 26           # one filler unit: one fill of 256 MiB (33-34 us of device time on an MI355X)


def filler_seconds(enqueue_s):
    """how long the caller's stream is kept busy for a scenario whose calls took enqueue_s of host time on the quiet twin"""
    assert enqueue_s >= 0.0 and math.isfinite(enqueue_s), enqueue_s
    return min(CAP_S, max(FLOOR_S, JITTER * float(enqueue_s)))


def filler_units(seconds, unit_s):
    """fills of FILL_FLOATS floats that keep a stream busy for `seconds`, one fill measured at unit_s of device time"""
    assert 0.0 < seconds <= CAP_S and unit_s > 0.0, (seconds, unit_s)
    return max(1, int(math.ceil(seconds / unit_s)))


# ---- poison and scribble -------------------------------------------------------------------------------------------------------------
BAD_INDEX = 0xFFFFFFFF          # above every table, set and direction count the library accepts (<= 2^24, 65536)


def scribble(rows):
    """Overwrite the caller's row arrays in place with entries no call accepts: 0xFFFFFFFF for indices, NaN for gains and weights (a
    NaN weight is refused, a NaN gain makes every sample NaN).  rows: {name: array or None}; the arrays are the very memory the call
    was given."""
    for name, a in rows.items():
        if a is None:
            continue
        assert isinstance(a, np.ndarray) and a.flags.c_contiguous and a.flags.writeable, name
        if a.dtype == np.uint32:
            a[...] = BAD_INDEX
        elif a.dtype == np.float32:
            a[...] = np.nan
        else:
            raise TypeError(f"{name}: rows are uint32 or float32, not {a.dtype}")


def row_arrays(rows):
    """fresh, writable, contiguous copies of a call's rows in the dtypes the C entry points read: what the wrappers pass on WITHOUT
    a copy of their own (np.ascontiguousarray of such an array is the array), so that scribbling them reaches the memory the library
    was handed"""
    out = {}
    for name, a in rows.items():
        if a is None:
            out[name] = None
            continue
        a = np.asarray(a)
        out[name] = np.array(a, dtype=np.float32 if a.dtype.kind == "f" else np.uint32, order="C", copy=True)
    return out


# ---- what the sources say --------------------------------------------------------------------------------------------------------------
def staging_slots():
    """kSchedSlots of csrc/api_internal.h: the scheduled calls in flight before the next one waits on the host"""
    with open(os.path.join(ROOT, "open_headstage_amd", "csrc", "api_internal.h")) as f:
        m = re.search(r"\bkSchedSlots\s*=\s*(\d+)\s*;", f.read())
    assert m, "kSchedSlots not found in csrc/api_internal.h"
    return int(m.group(1))


def async_entry_points(include_dir=None):
    """every prototype of the three headers with a `void *hip_stream` parameter, and ohs_node_batch_process (its stream is the
    slot's own, ohs_node_batch_stream) -> sorted names"""
    include_dir = include_dir or os.path.join(ROOT, "include")
    names = set()
    for h in HEADERS:
        with open(os.path.join(include_dir, h)) as f:
            text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
        for m in re.finditer(r"\b(ohs_\w+)\s*\(([^;{}]*?)\)\s*;", text):
            if re.search(r"\bvoid\s*\*\s*hip_stream\b", m.group(2)):
                names.add(m.group(1))
    names.add("ohs_node_batch_process")
    return sorted(names)


# ---- the two ways a scenario fails --------------------------------------------------------------------------------------------------------
class PremiseError(AssertionError):
    """the caller's stream was idle when a call that must not block returned"""


class DataMismatch(AssertionError):
    """a busy run's output, or its launch record, differs from the quiet twin's"""


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        raise DataMismatch(f"{what}: shape {got.shape} against the twin's {want.shape}")
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if bad.size:
        raise DataMismatch(f"{what}: {len(bad)} of {got.size} samples differ from the quiet twin's bits, {int(np.isnan(got).sum())} of them "
                           f"NaN; first at {bad[0].tolist()} ({got[tuple(bad[0])]!r} against {want[tuple(bad[0])]!r}), last at {bad[-1].tolist()}")


# ---- the stream ------------------------------------------------------------------------------------------------------------------------
_unit = {}


def _filler_tensor():
    import torch
    if "t" not in _unit:
        _unit["t"] = torch.empty(FILL_FLOATS, device="cuda")
    return _unit["t"]


def unit_seconds():
    """device time of one filler unit, measured once per process with events on a side stream"""
    import torch
    if "s" not in _unit:
        big, st, n = _filler_tensor(), torch.cuda.Stream(), 50
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            for _ in range(5):
                big.fill_(0.0)
            a.record(st)
            for _ in range(n):
                big.fill_(0.0)
            b.record(st)
        b.synchronize()
        _unit["s"] = a.elapsed_time(b) * 1e-3 / n
        assert _unit["s"] > 0.0
        print(f"busy stream: one filler unit ({FILL_FLOATS * 4 >> 20} MiB filled) takes {_unit['s'] * 1e6:.1f} us of device time")
    return _unit["s"]


class BusyStream:
    """One side stream of the caller's (never the default stream; `stream`: one the library owns, wrapped by the test) and bounded
    work queued on it with no host dependency: fills of one large tensor, nothing that waits for a flag."""

    def __init__(self, stream=None):
        import torch
        self.stream = torch.cuda.Stream() if stream is None else stream
        self.busy_done = torch.cuda.Event()
        self.seconds = self.units = 0

    @property
    def handle(self):
        return self.stream.cuda_stream

    def fill(self, seconds):
        import torch
        unit, big = unit_seconds(), _filler_tensor()
        self.seconds, self.units = seconds, filler_units(seconds, unit)
        with torch.cuda.stream(self.stream):
            for _ in range(self.units):
                big.fill_(1.0)
        self.busy_done.record(self.stream)

    def still_busy(self):
        return not self.busy_done.query()

    def premise(self, returned_late):
        """right after a call that must not block has returned"""
        if not self.still_busy():
            raise PremiseError(f"premise: the caller's stream was idle when the call returned -- {returned_late} returned only after "
                               f"{self.units} filler units ({self.seconds * 1e3:.1f} ms of device work) had run out: it waited for its "
                               f"stream, or the host was held up for that long")

    def drained(self, what):
        """right after a call the headers say waits for the device"""
        assert self.busy_done.query(), f"{what} returned while the work queued in front of it was still running: it did not wait"

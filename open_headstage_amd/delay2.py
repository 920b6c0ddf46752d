"""Object distance with air absorption over libohs_delay2.so (include/ohs_delay2.h): delay.py's stage with a short symmetric FIR per
object fused into it.

A source at 80 m is not one at 2 m turned down: the air dulls its treble.  FilteredObjectDelay takes, beside ObjectDelay's delay and
gain, five taps per object, stream and segment -- the centre and one side of a 9-tap symmetric filter, reached at the segment's last
frame and moving linearly per sample in between --, applied to the four interpolation nodes inside the delay kernel.  The library
carries no acoustics: air_absorption_taps turns distances into taps, render_with_distance_air queues the stage and
TrackedSceneProcessor.process_xyz on one stream.  Rows whose taps are the identity cost what ObjectDelay costs and have its bits.
The library is a tenth one with a loader and a prototype table of its own.  There is no fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._ffi import OHS_OK, fp
from .batch import _n_segs
from .delay import CARRY, FRESH, ObjectDelay, distance_rows
from .dsp import BLOCK_SIZE
from .lookup import dp
from .scene import vp, vpp

HERE = os.path.dirname(os.path.abspath(__file__))
DELAY2_LIB_PATH = os.path.join(HERE, "libohs_delay2.so")
FIR_RADIUS = 4
FIR_TAPS = FIR_RADIUS + 1
IDENTITY_TAPS = np.array([1.0, 0.0, 0.0, 0.0, 0.0], np.float32)

_ull = C.POINTER(C.c_ulonglong)
_process_args = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, dp, fp]
# name -> (restype, argtypes): the complete export list of include/ohs_delay2.h
DELAY2_PROTOTYPES = {
    "ohs_delay2_create": (C.c_int, [C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, vpp]),
    "ohs_delay2_destroy": (None, [vp]),
    "ohs_delay2_status_string": (C.c_char_p, [C.c_int]),
    "ohs_delay2_last_error": (C.c_char_p, []),
    "ohs_delay2_process": (C.c_int, _process_args + [C.c_size_t, C.c_int, vp]),
    "ohs_delay2_process_filtered": (C.c_int, _process_args + [fp, C.c_size_t, C.c_int, vp]),
    "ohs_delay2_reset": (C.c_int, [vp]),
    "ohs_delay2_sync": (C.c_int, [vp, vp]),
    "ohs_delay2_last_launch": (C.c_int, [vp, C.POINTER(C.c_uint), C.POINTER(C.c_uint), _ull, _ull, _ull]),
    "ohs_delay2_carried": (C.c_int, [vp, C.POINTER(C.c_size_t), dp, fp, fp]),
}

_lib = None


def delay2_lib() -> C.CDLL:
    """libohs_delay2.so, loaded beside the other libraries.  There is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(DELAY2_LIB_PATH):
            raise ImportError(f"{DELAY2_LIB_PATH} not found: build it with `python -m open_headstage_amd.build` (hipcc, gfx950)")
        try:
            import torch  # noqa: F401  (one HIP runtime per process: torch's first, see _ffi._load)
        except ImportError:
            pass
        L = C.CDLL(DELAY2_LIB_PATH)
        for name, (res, args) in DELAY2_PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class FilteredObjectDelayError(RuntimeError):
    def __init__(self, status: int, detail: str, text: str | None = None):
        self.status = status
        text = delay2_lib().ohs_delay2_status_string(status).decode() if text is None else text
        super().__init__(f"{text} ({status}): {detail}")


def delay2_check(status: int) -> None:
    if status != OHS_OK:
        raise FilteredObjectDelayError(status, delay2_lib().ohs_delay2_last_error().decode(errors="replace"))


def air_absorption_taps(r_m, fs: float = 48000.0, k: float = 1.6e-9):
    """Distances in metres -> the five taps FilteredObjectDelay.process takes, r_m's shape + (5,), f32; numpy f64 with sums in a fixed
    order.  k is the absorption in dB per metre per Hz^2 (1.6e-9: about 0.16 dB/m at 10 kHz), the classical f^2 law.
    b = min(0.25, r * k * (ln 10 / 20) * fs^2 / (16 pi^2)); the 9 taps are [b, 1 - 2b, b] convolved with itself four times, whose
    response (1 - 4 b sin^2(w / 2))^4 follows -k f^2 r dB where w is small, is positive and falls monotonically up to fs / 2, and
    sums to 1 at DC.  b = 0.25 ([1, 2, 1] / 4 four times, a null at fs / 2) is reached near 93 m at 48 kHz: beyond, the filter no
    longer changes.  r = 0 gives exactly (1, +0, +0, +0, +0), the row that takes the plain pass."""
    r = np.asarray(r_m, np.float64)
    if not (fs > 0 and k >= 0):
        raise ValueError("fs is positive and k is not negative")
    if not (np.isfinite(r).all() and (r >= 0).all()):
        raise ValueError("distances are finite and not negative")
    b = np.minimum(np.float64(0.25), r * (np.float64(k) * (np.log(10.0) / 20.0) * np.float64(fs) ** 2 / (16.0 * np.pi ** 2)))
    taps = np.zeros(r.shape + (2 * FIR_RADIUS + 1,), np.float64)
    taps[..., FIR_RADIUS] = 1.0
    side, mid = b[..., None], (1.0 - 2.0 * b)[..., None]
    for _ in range(FIR_RADIUS):                 # (zeros beyond the ends: the filter has grown to 2 * pass + 1 taps)
        lower = np.concatenate([taps[..., 1:], np.zeros_like(taps[..., :1])], -1)
        upper = np.concatenate([np.zeros_like(taps[..., :1]), taps[..., :-1]], -1)
        taps = (side * lower + mid * taps) + side * upper
    return np.ascontiguousarray(taps[..., FIR_RADIUS:].astype(np.float32) + np.float32(0.0))


class FilteredObjectDelay:
    """ohs_delay2_create's handle: the last max_delay + 6 input frames and the last (delay, gain, taps) per stream and object."""

    def __init__(self, n_streams: int, max_objects: int, max_delay: int = 8192, device: int = 0):
        self._h = None
        self.n_streams, self.max_objects, self.max_delay, self.device = int(n_streams), int(max_objects), int(max_delay), int(device)
        self._carried = False
        L = delay2_lib()
        h = C.c_void_p()
        delay2_check(L.ohs_delay2_create(self.device, self.n_streams, self.max_objects, self.max_delay, C.byref(h)))
        self._h = h
        self._destroy = L.ohs_delay2_destroy

    def process_ptr(self, d_in: int, d_out: int, n_blocks: int, in_stream_stride: int, in_channel_stride: int, out_stream_stride: int,
                    out_channel_stride: int, n_objects: int, seg_blocks: int, delay, gains=None, row_stream_stride: int = 0,
                    carry=None, hip_stream: int = 0, fir=None) -> None:
        """ohs_delay2_process_filtered, or with fir None ohs_delay2_process.  delay: f64 at [(s * row_stream_stride + k) * K + c];
        gains: f32 likewise or None (1.0); fir: f32, five per entry of that layout, or None; carry as ObjectDelay.process_ptr's."""
        delay = np.ascontiguousarray(delay, np.float64)
        g = None if gains is None else np.ascontiguousarray(gains, np.float32)
        h = None if fir is None else np.ascontiguousarray(fir, np.float32)
        n_segs = _n_segs(n_blocks, seg_blocks)
        need = ((self.n_streams - 1) * int(row_stream_stride) + n_segs) * int(n_objects)
        if delay.size < need or (g is not None and g.size < need) or (h is not None and h.size < need * FIR_TAPS):
            raise ValueError(f"rows: {need} entries are read, got {delay.size}" + ("" if g is None else f" and {g.size}") +
                             ("" if h is None else f" and {h.size} taps"))
        if carry is None:
            carry = self._carried
        L = delay2_lib()
        head = (self._h, C.c_void_p(d_in), C.c_void_p(d_out), int(n_blocks), int(in_stream_stride), int(in_channel_stride),
                int(out_stream_stride), int(out_channel_stride), int(n_objects), int(seg_blocks), delay.ctypes.data_as(dp),
                None if g is None else g.ctypes.data_as(fp))
        tail = (int(row_stream_stride), CARRY if carry else FRESH, C.c_void_p(hip_stream) if hip_stream else None)
        if h is None:
            delay2_check(L.ohs_delay2_process(*head, *tail))
        else:
            delay2_check(L.ohs_delay2_process_filtered(*head, h.ctypes.data_as(fp), *tail))
        if n_blocks:
            self._carried = True

    def _rows(self, a, n_segs, K, dtype, what, inner=()):
        """[K] (one row, held), [segs][K] (one row per segment for all streams) or [streams][segs][K], each with `inner` behind it
        -> (array, row stream stride)"""
        a = np.ascontiguousarray(a, dtype)
        if a.shape == (K,) + inner:
            return np.ascontiguousarray(np.broadcast_to(a, (n_segs, K) + inner)), 0
        if a.shape == (n_segs, K) + inner:
            return a, 0
        if a.shape == (self.n_streams, n_segs, K) + inner:
            return a, n_segs
        raise ValueError(f"{what} {a.shape}: expected [{K}], [{n_segs}][{K}] or [{self.n_streams}][{n_segs}][{K}]" +
                         (f", each with {list(inner)} behind it" if inner else ""))

    def process(self, x, delay, seg_blocks: int, gains=None, fir=None, carry=None, out=None, hip_stream: int | None = None):
        """x: contiguous float32 device tensor [streams, >= K, frames] -> [streams, K, frames], K from delay's last dimension.  delay
        (f64, frames) and gains (f32, or None: 1.0): [K], [segs][K] or [streams][segs][K]; fir (f32, or None: the unfiltered call):
        [K][5], [segs][K][5] or [streams][segs][K][5]."""
        import torch
        K = int(np.shape(delay)[-1])
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()):
            raise TypeError("x must be a contiguous float32 CUDA tensor [streams, channels, frames]")
        S, ch, frames = x.shape
        if S != self.n_streams or frames % BLOCK_SIZE or ch < K:
            raise ValueError(f"expected [{self.n_streams}, >= {K}, k*{BLOCK_SIZE}], got {tuple(x.shape)}")
        if x.device.index != self.device:
            raise ValueError("tensor is on a different device than the FilteredObjectDelay")
        if out is None:
            out = torch.empty((S, K, frames), dtype=x.dtype, device=x.device)
        elif tuple(out.shape) != (S, K, frames) or out.dtype != x.dtype or not out.is_contiguous() or out.device != x.device:
            raise ValueError("out must be a contiguous [streams, K, frames] tensor on x's device")
        if hip_stream is None:
            hip_stream = torch.cuda.current_stream(x.device).cuda_stream
        n_segs = _n_segs(frames // BLOCK_SIZE, seg_blocks)
        rows = {"delay": self._rows(delay, n_segs, K, np.float64, "delay")}
        if gains is not None:
            rows["gains"] = self._rows(gains, n_segs, K, np.float32, "gains")
        if fir is not None:
            rows["fir"] = self._rows(fir, n_segs, K, np.float32, "fir", (FIR_TAPS,))
        stride = max(st for _, st in rows.values())
        if any(st != stride for _, st in rows.values()):        # (one layout for all)
            rows = {name: (np.ascontiguousarray(np.broadcast_to(a, (self.n_streams,) + a.shape[-(3 if name == "fir" else 2):])), stride)
                    for name, (a, _) in rows.items()}
        get = lambda name: rows[name][0] if name in rows else None      # noqa: E731
        self.process_ptr(x.data_ptr(), out.data_ptr(), frames // BLOCK_SIZE, ch * frames, frames, K * frames, frames, K, seg_blocks,
                         get("delay"), get("gains"), stride, carry, hip_stream, fir=get("fir"))
        return out

    def sync(self, hip_stream: int = 0) -> None:
        delay2_check(delay2_lib().ohs_delay2_sync(self._h, C.c_void_p(hip_stream) if hip_stream else None))

    def reset(self) -> None:
        """the history is zeroed and the carry dropped (waits for the device)"""
        delay2_check(delay2_lib().ohs_delay2_reset(self._h))
        self._carried = False

    def last_launch(self):
        """(frames of a tile, the widest window a tile stages in LDS, tiles staged in LDS, tiles gathered from global memory, tiles
        that took the filtered pass) of the most recent call (waits for it)"""
        t, w, a, b, f = C.c_uint(), C.c_uint(), C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
        delay2_check(delay2_lib().ohs_delay2_last_launch(self._h, C.byref(t), C.byref(w), C.byref(a), C.byref(b), C.byref(f)))
        return int(t.value), int(w.value), int(a.value), int(b.value), int(f.value)

    def carried(self):
        """(delay [streams][K] f64, gain [streams][K] f32, taps [streams][K][5] f32) the handle holds in front of a carry=True call,
        or None"""
        k = C.c_size_t()
        n = self.n_streams * self.max_objects
        d, g, h = np.empty(n, np.float64), np.empty(n, np.float32), np.empty(n * FIR_TAPS, np.float32)
        delay2_check(delay2_lib().ohs_delay2_carried(self._h, C.byref(k), d.ctypes.data_as(dp), g.ctypes.data_as(fp), h.ctypes.data_as(fp)))
        if not k.value:
            return None
        n = self.n_streams * int(k.value)
        return (d[:n].reshape(self.n_streams, -1).copy(), g[:n].reshape(self.n_streams, -1).copy(),
                h[:n * FIR_TAPS].reshape(self.n_streams, -1, FIR_TAPS).copy())

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and getattr(self, "_destroy", None) is not None:
            self._destroy(h)


def render_with_distance_air(tr, dl2, x, src, rot, seg_blocks: int, gains=None, carry=None, crossfade: bool = True, fs: float = 48000.0,
                             c: float = 343.0, ref_m: float = 1.0, min_m: float = 0.1, k: float = 1.6e-9, listener=None, out=None,
                             hip_stream: int | None = None):
    """delay.render_with_distance with the air between source and listener: distance_rows(src ...) and air_absorption_taps of the same
    r -> dl2.process(x, delay, seg_blocks, gains=the distance gains, fir=the taps) -> tr.process_xyz(that, src - listener, rot,
    seg_blocks, gains), both queued on ONE stream with no wait between them.  tr: a TrackedSceneProcessor, dl2: a
    FilteredObjectDelay of the same streams.  A source nearer than 5 frames (3.6 cm at 48 kHz) is the call's to refuse."""
    import torch
    delay, dist_gain = distance_rows(src, fs, c, ref_m, min_m, listener)
    v = np.asarray(src, np.float64)
    if listener is not None:
        v = v - np.asarray(listener, np.float64)
    r = np.maximum(np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]), np.float64(min_m))    # distance_rows' r
    taps = air_absorption_taps(r, fs, k)
    if hip_stream is None:
        hip_stream = torch.cuda.current_stream(x.device).cuda_stream
    # the buffer between the two stays with dl2: the scene call reads it on hip_stream after this function has returned
    K, between = int(delay.shape[-1]), getattr(dl2, "_between", None)
    if between is None or tuple(between.shape) != (x.shape[0], K, x.shape[2]) or between.device != x.device:
        between = dl2._between = torch.empty((x.shape[0], K, x.shape[2]), dtype=torch.float32, device=x.device)
    dl2.process(x, delay, seg_blocks, gains=dist_gain, fir=taps, carry=carry, out=between, hip_stream=hip_stream)
    return tr.process_xyz(between, v, rot, seg_blocks, gains=gains, carry=carry, crossfade=crossfade, out=out, hip_stream=hip_stream)

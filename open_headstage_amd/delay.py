"""Object distance over libohs_delay.so (include/ohs_delay.h): a propagation delay and a gain per object, in front of a scene call.

The scene calls render where a source is; ObjectDelay adds how far away it is.  Per object, stream and segment it takes a delay in
frames and a gain, both reached at the segment's last frame and moving linearly per sample in between -- a source that flies past
has its Doppler shift --, and writes [streams, K, frames] on the device, which a scene call on the same stream reads as its input.
distance_rows turns positions into those rows, render_with_distance queues the stage and TrackedSceneProcessor.process_xyz on one
stream.  The library is a ninth one with a loader and a prototype table of its own.  There is no fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._ffi import OHS_OK, fp
from .batch import _n_segs
from .dsp import BLOCK_SIZE
from .lookup import dp
from .scene import vp, vpp

HERE = os.path.dirname(os.path.abspath(__file__))
DELAY_LIB_PATH = os.path.join(HERE, "libohs_delay.so")
MAX_OBJECTS = 64
MAX_DELAY = 65536
FRESH, CARRY = 0, 1

_ull = C.POINTER(C.c_ulonglong)
# name -> (restype, argtypes): the complete export list of include/ohs_delay.h
DELAY_PROTOTYPES = {
    "ohs_delay_create": (C.c_int, [C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, vpp]),
    "ohs_delay_destroy": (None, [vp]),
    "ohs_delay_status_string": (C.c_char_p, [C.c_int]),
    "ohs_delay_last_error": (C.c_char_p, []),
    "ohs_delay_process": (C.c_int, [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, dp, fp,
                                    C.c_size_t, C.c_int, vp]),
    "ohs_delay_reset": (C.c_int, [vp]),
    "ohs_delay_sync": (C.c_int, [vp, vp]),
    "ohs_delay_last_launch": (C.c_int, [vp, C.POINTER(C.c_uint), C.POINTER(C.c_uint), _ull, _ull]),
    "ohs_delay_carried": (C.c_int, [vp, C.POINTER(C.c_size_t), dp, fp]),
}

_lib = None


def delay_lib() -> C.CDLL:
    """libohs_delay.so, loaded beside the other libraries.  There is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(DELAY_LIB_PATH):
            raise ImportError(f"{DELAY_LIB_PATH} not found: build it with `python -m open_headstage_amd.build` (hipcc, gfx950)")
        try:
            import torch  # noqa: F401  (one HIP runtime per process: torch's first, see _ffi._load)
        except ImportError:
            pass
        L = C.CDLL(DELAY_LIB_PATH)
        for name, (res, args) in DELAY_PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class ObjectDelayError(RuntimeError):
    def __init__(self, status: int, detail: str, text: str | None = None):
        self.status = status
        text = delay_lib().ohs_delay_status_string(status).decode() if text is None else text
        super().__init__(f"{text} ({status}): {detail}")


def delay_check(status: int) -> None:
    if status != OHS_OK:
        raise ObjectDelayError(status, delay_lib().ohs_delay_last_error().decode(errors="replace"))


def distance_rows(src, fs: float = 48000.0, c: float = 343.0, ref_m: float = 1.0, min_m: float = 0.1, listener=None):
    """Positions in metres -> (delay, gain) for ObjectDelay.process, numpy f64 throughout: r = sqrt((x^2 + y^2) + z^2) of src - listener,
    floored at min_m; delay = max(1, r * (fs / c)) frames (f64); gain = (float)(ref_m / r) (f32).  src: [K][3], [segs][K][3] or
    [streams][segs][K][3], as TrackedSceneProcessor.process_xyz takes it; the rows have src's leading shape.  A delay above the
    handle's max_delay is the call's to refuse."""
    v = np.asarray(src, np.float64)
    if v.ndim < 2 or v.ndim > 4 or v.shape[-1] != 3:
        raise ValueError(f"expected src [K][3], [segs][K][3] or [streams][segs][K][3], got {v.shape}")
    if not (fs > 0 and c > 0 and ref_m > 0 and min_m > 0):
        raise ValueError("fs, c, ref_m and min_m are positive")
    if listener is not None:
        v = v - np.asarray(listener, np.float64)
    r = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    r = np.maximum(r, np.float64(min_m))
    delay = np.maximum(np.float64(1.0), r * (np.float64(fs) / np.float64(c)))
    return delay, (np.float64(ref_m) / r).astype(np.float32)


class ObjectDelay:
    """ohs_delay_create's handle: the last max_delay + 2 input frames and the last (delay, gain) per stream and object."""

    def __init__(self, n_streams: int, max_objects: int, max_delay: int = 8192, device: int = 0):
        self._h = None
        self.n_streams, self.max_objects, self.max_delay, self.device = int(n_streams), int(max_objects), int(max_delay), int(device)
        self._carried = False
        L = delay_lib()
        h = C.c_void_p()
        delay_check(L.ohs_delay_create(self.device, self.n_streams, self.max_objects, self.max_delay, C.byref(h)))
        self._h = h
        self._destroy = L.ohs_delay_destroy

    def process_ptr(self, d_in: int, d_out: int, n_blocks: int, in_stream_stride: int, in_channel_stride: int, out_stream_stride: int,
                    out_channel_stride: int, n_objects: int, seg_blocks: int, delay, gains=None, row_stream_stride: int = 0,
                    carry=None, hip_stream: int = 0) -> None:
        """ohs_delay_process.  delay: f64 at [(s * row_stream_stride + k) * K + c]; gains: f32 likewise or None (1.0); carry: True --
        the previous call's last (delay, gain) and the history stand in front of the call --, False, or None: True when the handle
        carries them."""
        delay = np.ascontiguousarray(delay, np.float64)
        g = None if gains is None else np.ascontiguousarray(gains, np.float32)
        n_segs = _n_segs(n_blocks, seg_blocks)
        need = ((self.n_streams - 1) * int(row_stream_stride) + n_segs) * int(n_objects)
        if delay.size < need or (g is not None and g.size < need):
            raise ValueError(f"rows: {need} entries are read, got {delay.size}" + ("" if g is None else f" and {g.size}"))
        if carry is None:
            carry = self._carried
        delay_check(delay_lib().ohs_delay_process(
            self._h, C.c_void_p(d_in), C.c_void_p(d_out), int(n_blocks), int(in_stream_stride), int(in_channel_stride),
            int(out_stream_stride), int(out_channel_stride), int(n_objects), int(seg_blocks), delay.ctypes.data_as(dp),
            None if g is None else g.ctypes.data_as(fp), int(row_stream_stride), CARRY if carry else FRESH,
            C.c_void_p(hip_stream) if hip_stream else None))
        if n_blocks:
            self._carried = True

    def _rows(self, a, n_segs, K, dtype, what):
        """[K] (one row, held), [segs][K] (one row per segment for all streams) or [streams][segs][K] -> (array, row stream stride)"""
        a = np.ascontiguousarray(a, dtype)
        if a.ndim == 1 and a.shape[0] == K:
            return np.ascontiguousarray(np.broadcast_to(a, (n_segs, K))), 0
        if a.ndim == 2 and a.shape == (n_segs, K):
            return a, 0
        if a.ndim == 3 and a.shape == (self.n_streams, n_segs, K):
            return a, n_segs
        raise ValueError(f"{what} {a.shape}: expected [{K}], [{n_segs}][{K}] or [{self.n_streams}][{n_segs}][{K}]")

    def process(self, x, delay, seg_blocks: int, gains=None, carry=None, out=None, hip_stream: int | None = None):
        """x: contiguous float32 device tensor [streams, >= K, frames] -> [streams, K, frames], K from delay's last dimension.  delay
        (f64, frames) and gains (f32, or None: 1.0): [K], [segs][K] or [streams][segs][K]."""
        import torch
        K = int(np.shape(delay)[-1])
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()):
            raise TypeError("x must be a contiguous float32 CUDA tensor [streams, channels, frames]")
        S, ch, frames = x.shape
        if S != self.n_streams or frames % BLOCK_SIZE or ch < K:
            raise ValueError(f"expected [{self.n_streams}, >= {K}, k*{BLOCK_SIZE}], got {tuple(x.shape)}")
        if x.device.index != self.device:
            raise ValueError("tensor is on a different device than the ObjectDelay")
        if out is None:
            out = torch.empty((S, K, frames), dtype=x.dtype, device=x.device)
        elif tuple(out.shape) != (S, K, frames) or out.dtype != x.dtype or not out.is_contiguous() or out.device != x.device:
            raise ValueError("out must be a contiguous [streams, K, frames] tensor on x's device")
        if hip_stream is None:
            hip_stream = torch.cuda.current_stream(x.device).cuda_stream
        n_segs = _n_segs(frames // BLOCK_SIZE, seg_blocks)
        d, stride = self._rows(delay, n_segs, K, np.float64, "delay")
        g = None
        if gains is not None:
            g, g_stride = self._rows(gains, n_segs, K, np.float32, "gains")
            if g_stride != stride:          # (one layout for both)
                d = np.ascontiguousarray(np.broadcast_to(d, (self.n_streams, n_segs, K)))
                g = np.ascontiguousarray(np.broadcast_to(g, (self.n_streams, n_segs, K)))
                stride = n_segs
        self.process_ptr(x.data_ptr(), out.data_ptr(), frames // BLOCK_SIZE, ch * frames, frames, K * frames, frames, K, seg_blocks, d, g,
                         stride, carry, hip_stream)
        return out

    def sync(self, hip_stream: int = 0) -> None:
        delay_check(delay_lib().ohs_delay_sync(self._h, C.c_void_p(hip_stream) if hip_stream else None))

    def reset(self) -> None:
        """the history is zeroed and the carry dropped (waits for the device)"""
        delay_check(delay_lib().ohs_delay_reset(self._h))
        self._carried = False

    def last_launch(self):
        """(frames of a tile, the widest window a tile stages in LDS, tiles staged in LDS, tiles gathered from global memory) of the most
        recent call (waits for it)"""
        t, w, a, b = C.c_uint(), C.c_uint(), C.c_ulonglong(), C.c_ulonglong()
        delay_check(delay_lib().ohs_delay_last_launch(self._h, C.byref(t), C.byref(w), C.byref(a), C.byref(b)))
        return int(t.value), int(w.value), int(a.value), int(b.value)

    def carried(self):
        """(delay [streams][K] f64, gain [streams][K] f32) the handle holds in front of a carry=True call, or None"""
        k = C.c_size_t()
        d, g = np.empty(self.n_streams * self.max_objects, np.float64), np.empty(self.n_streams * self.max_objects, np.float32)
        delay_check(delay_lib().ohs_delay_carried(self._h, C.byref(k), d.ctypes.data_as(dp), g.ctypes.data_as(fp)))
        if not k.value:
            return None
        n = self.n_streams * int(k.value)
        return d[:n].reshape(self.n_streams, -1).copy(), g[:n].reshape(self.n_streams, -1).copy()

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and getattr(self, "_destroy", None) is not None:
            self._destroy(h)


def render_with_distance(tr, dl, x, src, rot, seg_blocks: int, gains=None, carry=None, crossfade: bool = True, fs: float = 48000.0,
                         c: float = 343.0, ref_m: float = 1.0, min_m: float = 0.1, listener=None, out=None, hip_stream: int | None = None):
    """Positions in metres in, two ears out: distance_rows(src ...) -> dl.process(x, delay, seg_blocks, gains=the distance gains) ->
    tr.process_xyz(that, src - listener, rot, seg_blocks, gains), both queued on ONE stream with no wait between them.  tr: a
    TrackedSceneProcessor, dl: an ObjectDelay of the same streams; gains: process_xyz's object gains, beside the distance law's.
    carry: both handles', None: each continues if it carries."""
    import torch
    delay, dist_gain = distance_rows(src, fs, c, ref_m, min_m, listener)
    if hip_stream is None:
        hip_stream = torch.cuda.current_stream(x.device).cuda_stream
    v = np.asarray(src, np.float64)
    if listener is not None:
        v = v - np.asarray(listener, np.float64)
    # the buffer between the two stays with dl: the scene call reads it on hip_stream after this function has returned
    K, between = int(delay.shape[-1]), getattr(dl, "_between", None)
    if between is None or tuple(between.shape) != (x.shape[0], K, x.shape[2]) or between.device != x.device:
        between = dl._between = torch.empty((x.shape[0], K, x.shape[2]), dtype=torch.float32, device=x.device)
    dl.process(x, delay, seg_blocks, gains=dist_gain, carry=carry, out=between, hip_stream=hip_stream)
    return tr.process_xyz(between, v, rot, seg_blocks, gains=gains, carry=carry, crossfade=crossfade, out=out, hip_stream=hip_stream)

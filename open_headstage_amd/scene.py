"""Object scenes over libohs_scene.so (include/ohs_scene.h): K independently moving sources per stream -> two ears in one kernel.

A scene handle lives in a library of its own beside libohs_hip.so -- the header of that one is frozen --, so this module has
its own loader and its own prototype table (SCENE_PROTOTYPES); `_ffi.PROTOTYPES` stays the 119 entries of ohs_hip.h.  Audio is
exchanged as device tensors [stream, object, frame] -> [stream, 2, frame]; torch only owns the memory and the streams.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._ffi import OHS_OK, fp
from .batch import _layout_io, _n_segs
from .dsp import BLOCK_SIZE

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE_LIB_PATH = os.path.join(HERE, "libohs_scene.so")
MAX_OBJECTS = 64
SWITCH_RING_OUT, SWITCH_CROSSFADE = 0, 1

vp, vpp, u32p = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)

# name -> (restype, argtypes): the complete export list of include/ohs_scene.h
SCENE_PROTOTYPES = {
    "ohs_scene_create": (C.c_int, [C.c_int, C.c_size_t, C.c_size_t, vpp]),
    "ohs_scene_destroy": (None, [vp]),
    "ohs_scene_status_string": (C.c_char_p, [C.c_int]),
    "ohs_scene_last_error": (C.c_char_p, []),
    "ohs_scene_set_direction_irs": (C.c_int, [vp, C.c_size_t, fp, C.c_size_t]),
    "ohs_scene_process": (C.c_int, [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                    u32p, fp, C.c_size_t, u32p, fp, C.c_int, vp]),
    "ohs_scene_set_gain": (C.c_int, [vp, C.c_float]),
    "ohs_scene_set_eq_band_coeffs": (C.c_int, [vp, C.c_size_t, fp, C.c_int]),
    "ohs_scene_set_eq_enabled": (C.c_int, [vp, C.c_int]),
    "ohs_scene_set_flush_denormals": (C.c_int, [vp, C.c_int]),
    "ohs_scene_reset": (C.c_int, [vp]),
    "ohs_scene_sync": (C.c_int, [vp, vp]),
    "ohs_scene_last_launch": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]),
}

_lib = None


def scene_lib() -> C.CDLL:
    """libohs_scene.so, loaded beside the product library: a copy of the code with its own state.  There is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(SCENE_LIB_PATH):
            raise ImportError(f"{SCENE_LIB_PATH} not found: build it with `python -m open_headstage_amd.build` (hipcc, gfx950)")
        try:
            import torch  # noqa: F401  (one HIP runtime per process: torch's first, see _ffi._load)
        except ImportError:
            pass
        L = C.CDLL(SCENE_LIB_PATH)
        for name, (res, args) in SCENE_PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class SceneError(RuntimeError):
    def __init__(self, status: int, detail: str, text: str | None = None):
        self.status = status
        text = scene_lib().ohs_scene_status_string(status).decode() if text is None else text
        super().__init__(f"{text} ({status}): {detail}")


def _check_status(L: C.CDLL, prefix: str, status: int) -> None:
    """the one place a status of either scene library becomes a SceneError: that library's last error and status string"""
    if status != OHS_OK:
        raise SceneError(status, getattr(L, prefix + "last_error")().decode(errors="replace"),
                         getattr(L, prefix + "status_string")(status).decode())


def scene_check(status: int) -> None:
    """Public: for callers that use scene_lib()'s entries directly.  The classes check through their own library (_check)."""
    _check_status(scene_lib(), "ohs_scene_", status)


# -- host helpers: where the objects are, seen from the head -----------------------------------------------------------
def rotate_sources(az, el, yaw, pitch=0.0, roll=0.0):
    """Source directions in the room -> directions seen from a turned head, all in the plugin's degrees (azimuth positive to the
    RIGHT, elevation up; yaw positive to the right, pitch positive nose up, roll positive right ear down).  Arrays broadcast
    against each other; -> (az', el') as float32.  With pitch = roll = 0 this is the yaw rule of ohs_sofa_layout_yaw_irs in its
    own f32 arithmetic: az - yaw wrapped into [-180, 180), el unchanged."""
    az, el, yaw, pitch, roll = np.broadcast_arrays(*(np.asarray(v, np.float32) for v in (az, el, yaw, pitch, roll)))
    d = (az - yaw).astype(np.float32)
    az_y = (d - np.float32(360.0) * np.floor((d + np.float32(180.0)) / np.float32(360.0))).astype(np.float32)
    flat = (pitch == 0) & (roll == 0)
    if flat.all():
        return az_y, el.astype(np.float32).copy()
    # x front, y right, z up; the head's axes in the room are the columns of Rz(yaw) Ry(pitch) Rx(roll), the source seen from
    # the head is that matrix transposed times the source
    a, e = np.radians(az.astype(np.float64)), np.radians(el.astype(np.float64))
    v = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], -1)
    y, p, r = (np.radians(t.astype(np.float64)) for t in (yaw, pitch, roll))
    cy, sy, cp, sp, cr, sr = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    one, zero = np.ones_like(cy), np.zeros_like(cy)
    Rz = np.stack([np.stack([cy, -sy, zero], -1), np.stack([sy, cy, zero], -1), np.stack([zero, zero, one], -1)], -2)
    Ry = np.stack([np.stack([cp, zero, -sp], -1), np.stack([zero, one, zero], -1), np.stack([sp, zero, cp], -1)], -2)
    Rx = np.stack([np.stack([one, zero, zero], -1), np.stack([zero, cr, sr], -1), np.stack([zero, -sr, cr], -1)], -2)
    R = Rz @ Ry @ Rx
    h = np.einsum("...ji,...j->...i", R, v)
    az2 = np.degrees(np.arctan2(h[..., 1], h[..., 0])).astype(np.float32)
    el2 = np.degrees(np.arcsin(np.clip(h[..., 2], -1.0, 1.0))).astype(np.float32)
    az2 = np.where(az2 >= 180.0, az2 - np.float32(360.0), az2).astype(np.float32)
    return np.where(flat, az_y, az2).astype(np.float32), np.where(flat, el, el2).astype(np.float32)


def _xyz(a, e, r):
    """(azimuth, elevation in degrees, radius), f32 -> Cartesian f64 [..., 3]"""
    a, e = np.radians(np.asarray(a, np.float32).astype(np.float64)), np.radians(np.asarray(e, np.float32).astype(np.float64))
    r = np.asarray(r, np.float32).astype(np.float64)
    return np.stack([r * np.cos(e) * np.cos(a), r * np.cos(e) * np.sin(a), r * np.sin(e) + 0.0 * a], -1)


def nearest_directions(positions, az, el, radius_m: float = 1.0) -> np.ndarray:
    """The measurement nearest to each query in Cartesian space -- what ohs_sofa_nearest answers for a file opened without
    interpolation (the first of equally near ones).  positions: [M][3] (azimuth, elevation, radius) as MySofa.position gives
    them, SOFA degrees (azimuth positive to the LEFT; a plugin azimuth is its negative); az, el: queries in the same degrees,
    any shape -> uint32 indices of that shape."""
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    p = _xyz(pos[:, 0], pos[:, 1], pos[:, 2]).astype(np.float32).astype(np.float64)     # (the handle keeps f32 coordinates)
    azq, elq = np.broadcast_arrays(np.asarray(az, np.float32), np.asarray(el, np.float32))
    q = _xyz(azq.ravel(), elq.ravel(), np.float32(radius_m))
    out = np.empty(q.shape[0], np.uint32)
    for i0 in range(0, q.shape[0], 4096):       # (slices: M x queries distances at a time)
        d = p[None, :, :] - q[i0:i0 + 4096, None, :]
        out[i0:i0 + 4096] = np.argmin(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2], axis=1)
    return out.reshape(azq.shape)


def _object_rows(a, n_streams, n_segs, K, what, dtype):
    """rows per object -> (contiguous array, idx_stride for the C call): [>= n_segs][K] is one row for all streams (stride 0),
    [n_streams][>= n_segs][K] a row per stream (stride = the row's segments)."""
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.ndim == 2 and a.shape[0] >= n_segs and a.shape[1] == K:
        return a, 0
    if a.ndim == 3 and a.shape[0] == n_streams and a.shape[1] >= n_segs and a.shape[2] == K:
        return a, int(a.shape[1])
    raise ValueError(f"{what}: expected [{n_streams}][>= {n_segs}][{K}] or [>= {n_segs}][{K}], got {a.shape}")


class SceneProcessor:
    # the library an instance talks to and the prefix of its entries: a subclass on another library with the same surface under
    # another prefix (scene2.BlendSceneProcessor) overrides the two
    _prefix = "ohs_scene_"
    _loader = staticmethod(scene_lib)

    def _fn(self, name: str):
        return getattr(self._loader(), self._prefix + name)

    def _check(self, status: int) -> None:
        _check_status(self._loader(), self._prefix, status)

    def __init__(self, n_streams: int, num_bands: int = 10, device: int = 0):
        self.n_streams, self.num_bands, self.device = int(n_streams), int(num_bands), int(device)
        self.n_directions = 0
        self._h = None
        h = C.c_void_p()
        self._check(self._fn("create")(self.device, self.n_streams, self.num_bands, C.byref(h)))
        self._h = h
        self._destroy = self._fn("destroy")

    # -- the direction table ------------------------------------------------------------------
    def set_directions(self, irs) -> None:
        """irs [n_dirs][2][len]: direction d -> left ear irs[d][0], right ear irs[d][1]; len <= 512, n_dirs <= 65536.  Replaces any
        earlier table and zeroes the overlap; an empty array frees it (ohs_scene_set_direction_irs)."""
        a = np.ascontiguousarray(irs, dtype=np.float32)
        if a.size == 0:
            self._check(self._fn("set_direction_irs")(self._h, 0, None, 0))
            self.n_directions = 0
            return
        if a.ndim != 3 or a.shape[1] != 2:
            raise ValueError(f"expected irs [n_dirs][2][len], got {a.shape}")
        self.n_directions = 0
        self._check(self._fn("set_direction_irs")(self._h, a.shape[0], a.ctypes.data_as(fp), a.shape[2]))
        self.n_directions = int(a.shape[0])

    def set_directions_from_sofa(self, sofa, fs: float = 0.0) -> np.ndarray:
        """Every measurement of the file as one direction, in the file's order; -> their positions [M][3] (azimuth, elevation,
        radius in SOFA degrees, what nearest_directions takes).  Built with sofa.layout_irs at the measurements' own angles, 16 at
        a time, so a direction's pair has the bits a layout channel at that angle has."""
        from .sofa import layout_irs
        M = sofa.num_measurements
        pos = np.stack([sofa.position(m) for m in range(M)]).astype(np.float32)
        groups = [layout_irs(sofa, -pos[m0:m0 + 16, 0], pos[m0:m0 + 16, 1], float(pos[m0, 2]), fs) for m0 in range(0, M, 16)]
        ln = max(g.shape[2] for g in groups)
        if ln > BLOCK_SIZE:
            raise ValueError(f"a response of {ln} taps: a direction holds one-partition responses (<= {BLOCK_SIZE} taps)")
        irs = np.zeros((M, 2, ln), np.float32)
        for i, g in enumerate(groups):
            irs[16 * i:16 * i + g.shape[0], :, :g.shape[2]] = g
        self.set_directions(irs)
        return pos

    # -- the call -----------------------------------------------------------------------------
    def process_ptr(self, d_in: int, d_out: int, n_blocks: int, in_stream_stride: int, in_channel_stride: int, out_stream_stride: int,
                    out_channel_stride: int, n_objects: int, seg_blocks: int, idx, gains=None, prev_idx=None, prev_gains=None,
                    crossfade: bool = True, hip_stream: int = 0) -> None:
        """ohs_scene_process.  idx: [n_segs][K] for all streams or [n_streams][n_segs][K] direction indices; gains: the same shape,
        or None (1.0); prev_idx / prev_gains: what stood in front of the call's first block, [K] beside shared rows, [n_streams][K]
        beside rows per stream, or None: no boundary there (read when crossfade only)."""
        K, n_segs = int(n_objects), _n_segs(n_blocks, seg_blocks)
        if idx is None:
            raise ValueError("idx is required")
        a, stride = _object_rows(idx, self.n_streams, n_segs, K, "idx", np.uint32)
        g = None
        if gains is not None:
            g, gs = _object_rows(gains, self.n_streams, n_segs, K, "gains", np.float32)
            if gs != stride:
                raise ValueError("gains must have idx's shape")
        n_prev = (self.n_streams if stride else 1) * K

        def prev(v, dtype, what):
            if v is None:
                return None
            v = np.ascontiguousarray(v, dtype=dtype).reshape(-1)
            if v.size != n_prev:
                raise ValueError(f"{what}: expected {n_prev} entries, got {v.size}")
            return v
        pi, pg = prev(prev_idx, np.uint32, "prev_idx"), prev(prev_gains, np.float32, "prev_gains")
        self._check(self._fn("process")(
            self._h, C.c_void_p(d_in), C.c_void_p(d_out), int(n_blocks), int(in_stream_stride), int(in_channel_stride),
            int(out_stream_stride), int(out_channel_stride), K, int(seg_blocks), a.ctypes.data_as(u32p),
            None if g is None else g.ctypes.data_as(fp), stride, None if pi is None else pi.ctypes.data_as(u32p),
            None if pg is None else pg.ctypes.data_as(fp), SWITCH_CROSSFADE if crossfade else SWITCH_RING_OUT,
            C.c_void_p(hip_stream) if hip_stream else None))

    def process(self, x, idx, seg_blocks: int, gains=None, prev_idx=None, prev_gains=None, crossfade: bool = True, out=None,
                hip_stream: int | None = None):
        """x: contiguous float32 device tensor [streams, >= K, frames], frames a multiple of 512 -> [streams, 2, frames]:
        gain * sum over objects of conv(h[dir][ear], x[:, c] * gains[c]), a direction and a gain per object, stream and segment of
        seg_blocks * 512 frames, then the handle's EQ if it is enabled.  K is idx's last dimension; channels of x beyond K are never
        read.  crossfade: a pair of objects in which a direction or a gain changes fades over the segment's first block (False: the
        old response's tail rings out)."""
        K = int(np.shape(idx)[-1])
        out, hip_stream, frames = _layout_io(self, x, K, out, hip_stream)
        self.process_ptr(x.data_ptr(), out.data_ptr(), frames // BLOCK_SIZE, x.shape[1] * frames, frames, 2 * frames, frames, K,
                         seg_blocks, idx, gains, prev_idx, prev_gains, crossfade, hip_stream)
        return out

    # -- the chain behind the renderer --------------------------------------------------------------
    def set_gain(self, gain: float) -> None:
        self._check(self._fn("set_gain")(self._h, float(gain)))

    def set_band_coeffs(self, band_idx: int, coeffs, enabled: bool) -> None:
        c = np.ascontiguousarray(coeffs, dtype=np.float32).ravel()
        if c.size != 5:
            raise ValueError("coeffs must be [b0, b1, b2, a1, a2]")
        self._check(self._fn("set_eq_band_coeffs")(self._h, int(band_idx), c.ctypes.data_as(fp), int(bool(enabled))))

    def set_eq_enabled(self, eq_enable: bool) -> None:
        self._check(self._fn("set_eq_enabled")(self._h, int(bool(eq_enable))))

    def set_flush_denormals(self, mode: int) -> None:
        self._check(self._fn("set_flush_denormals")(self._h, int(mode)))

    def reset(self) -> None:
        self._check(self._fn("reset")(self._h))

    def sync(self, hip_stream: int = 0) -> None:
        self._check(self._fn("sync")(self._h, C.c_void_p(hip_stream) if hip_stream else None))

    def last_launch(self):
        """(pairs of objects, block ranges per stream, passes through old directions) of the most recent launch; zeros: none yet"""
        p, r, f = C.c_int(), C.c_int(), C.c_ulonglong()
        self._check(self._fn("last_launch")(self._h, C.byref(p), C.byref(r), C.byref(f)))
        return int(p.value), int(r.value), int(f.value)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and getattr(self, "_destroy", None) is not None:
            self._destroy(h)

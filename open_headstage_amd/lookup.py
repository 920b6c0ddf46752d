"""Rows for the scene calls, found on the device: libohs_lookup.so (include/ohs_lookup.h).

scene.nearest_directions and scene2.bracket_directions are the definition of a scene's rows, and brute force in numpy: hundreds of
microseconds per query.  DirectionLookup answers the same questions with k_lookup, a call for all queries: `.nearest` and `.bracket`
take what the two helpers take, `.rows` takes sources in the room and a head pose per stream and segment and returns what
SceneProcessor.process / BlendSceneProcessor.process read.  Angles become coordinates here, in numpy (scene._xyz): the library has
no trigonometry.  The library is a fourth one with a loader and a prototype table of its own.  There is no fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._ffi import OHS_OK, fp
from .scene import _xyz, u32p, vp, vpp

HERE = os.path.dirname(os.path.abspath(__file__))
LOOKUP_LIB_PATH = os.path.join(HERE, "libohs_lookup.so")
MAX_OBJECTS = 64
MAX_DIRECTIONS = 65536

dp = C.POINTER(C.c_double)

# name -> (restype, argtypes): the complete export list of include/ohs_lookup.h
LOOKUP_PROTOTYPES = {
    "ohs_lookup_create": (C.c_int, [C.c_int, C.c_size_t, fp, vpp]),
    "ohs_lookup_destroy": (None, [vp]),
    "ohs_lookup_status_string": (C.c_char_p, [C.c_int]),
    "ohs_lookup_last_error": (C.c_char_p, []),
    "ohs_lookup_points": (C.c_int, [vp, C.c_size_t, dp, u32p, u32p, fp]),
    "ohs_lookup_rows": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_size_t, dp, C.c_size_t, C.c_size_t, dp, C.c_size_t, u32p, u32p, fp]),
    "ohs_lookup_last_launch": (C.c_int, [vp, C.POINTER(C.c_uint), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
}

_lib = None


def lookup_lib() -> C.CDLL:
    """libohs_lookup.so, loaded beside the other libraries.  There is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LOOKUP_LIB_PATH):
            raise ImportError(f"{LOOKUP_LIB_PATH} not found: build it with `python -m open_headstage_amd.build` (hipcc, gfx950)")
        try:
            import torch  # noqa: F401  (one HIP runtime per process: torch's first, see _ffi._load)
        except ImportError:
            pass
        L = C.CDLL(LOOKUP_LIB_PATH)
        for name, (res, args) in LOOKUP_PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class DirectionLookupError(RuntimeError):
    def __init__(self, status: int, detail: str, text: str | None = None):
        self.status = status
        text = lookup_lib().ohs_lookup_status_string(status).decode() if text is None else text
        super().__init__(f"{text} ({status}): {detail}")


def lookup_check(status: int) -> None:
    if status != OHS_OK:
        raise DirectionLookupError(status, lookup_lib().ohs_lookup_last_error().decode(errors="replace"))


def table_xyz(positions) -> np.ndarray:
    """positions [M][3] (azimuth, elevation in SOFA degrees, radius) -> the f32 Cartesian table the helpers search"""
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    return np.ascontiguousarray(_xyz(pos[:, 0], pos[:, 1], pos[:, 2]).astype(np.float32))


def pose_matrices(yaw, pitch=0.0, roll=0.0) -> np.ndarray:
    """Head poses in the plugin's degrees -> [...][3][3] f64: scene.rotate_sources' Rz(yaw) Ry(pitch) Rx(roll), built as it builds
    it, with the middle column negated -- R^T v is then the source seen from the head with its y axis to the LEFT, SOFA's frame
    (the negation is exact)."""
    yaw, pitch, roll = np.broadcast_arrays(*(np.asarray(v, np.float32) for v in (yaw, pitch, roll)))
    y, p, r = (np.radians(t.astype(np.float64)) for t in (yaw, pitch, roll))
    cy, sy, cp, sp, cr, sr = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    one, zero = np.ones_like(cy), np.zeros_like(cy)
    Rz = np.stack([np.stack([cy, -sy, zero], -1), np.stack([sy, cy, zero], -1), np.stack([zero, zero, one], -1)], -2)
    Ry = np.stack([np.stack([cp, zero, -sp], -1), np.stack([zero, one, zero], -1), np.stack([sp, zero, cp], -1)], -2)
    Rx = np.stack([np.stack([one, zero, zero], -1), np.stack([zero, cr, sr], -1), np.stack([zero, -sr, cr], -1)], -2)
    R = np.ascontiguousarray(Rz @ Ry @ Rx)
    R[..., :, 1] = -R[..., :, 1]
    return R


def rows_host_half(src_az, src_el, yaw, pitch=0.0, roll=0.0, radius_m: float = 1.0):
    """What DirectionLookup.rows hands to ohs_lookup_rows: -> (v, src_stream_stride, src_seg_stride, R, rot_stream_stride, n_streams,
    n_segs, K).  v: the sources' plugin-frame coordinates, f64, [..][K][3]; R: pose_matrices, [segs][3][3] or [streams][segs][3][3].
    Sources are [K], [streams][K], [segs][K] or [streams][segs][K], poses [segs] or [streams][segs]; two-dimensional sources whose
    first dimension is the number of segments are [segs][K], also where that is the number of streams as well."""
    az, el = np.broadcast_arrays(np.asarray(src_az, np.float32), np.asarray(src_el, np.float32))
    R = pose_matrices(yaw, pitch, roll)
    if R.ndim not in (3, 4) or az.ndim < 1 or az.ndim > 3:
        raise ValueError(f"poses are [segs] or [streams][segs], sources [K] up to [streams][segs][K]; got {R.shape[:-2]} and {az.shape}")
    n_segs, K = int(R.shape[-3]), int(az.shape[-1])
    S = int(R.shape[0]) if R.ndim == 4 else None
    sss = sks = 0
    if az.ndim == 3:
        if az.shape[1] != n_segs or (S is not None and az.shape[0] != S):
            raise ValueError(f"sources {az.shape} beside poses {R.shape[:-2]}")
        S, sss, sks = int(az.shape[0]), n_segs, 1
    elif az.ndim == 2:
        if az.shape[0] == n_segs:
            sks = 1
        elif S is None or az.shape[0] == S:
            S, sss = int(az.shape[0]), 1
        else:
            raise ValueError(f"sources {az.shape} beside poses {R.shape[:-2]}")
    S = 1 if S is None else S
    v = np.ascontiguousarray(_xyz(az, el, np.float32(radius_m)))
    return v, sss, sks, R, (n_segs if R.ndim == 4 else 0), S, n_segs, K


class DirectionLookup:
    """The measurements of a table (positions [M][3] as SceneProcessor.set_directions_from_sofa returns them) on the device."""

    def __init__(self, positions, device: int = 0, xyz=None):
        """xyz: the table's Cartesian coordinates [M][3] themselves, f32, instead of positions (positions None)"""
        self._h = None
        xyz = table_xyz(positions) if xyz is None else np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self.n_directions, self.device = int(xyz.shape[0]), int(device)
        L = lookup_lib()
        h = C.c_void_p()
        lookup_check(L.ohs_lookup_create(self.device, self.n_directions, xyz.ctypes.data_as(fp), C.byref(h)))
        self._h = h
        self._destroy = L.ohs_lookup_destroy

    def points(self, q, blend: bool = True):
        """ohs_lookup_points on q [..][3], f64 Cartesian in the table's frame -> (idx0, idx1, w) or idx0, of q's leading shape"""
        q = np.ascontiguousarray(q, np.float64)
        if q.ndim < 1 or q.shape[-1] != 3:
            raise ValueError(f"expected q [..][3], got {q.shape}")
        shape, n = q.shape[:-1], q.size // 3
        i0 = np.empty(n, np.uint32)
        i1, w = (np.empty(n, np.uint32), np.empty(n, np.float32)) if blend else (None, None)
        lookup_check(lookup_lib().ohs_lookup_points(self._h, n, q.ctypes.data_as(dp), i0.ctypes.data_as(u32p),
                                                    None if i1 is None else i1.ctypes.data_as(u32p),
                                                    None if w is None else w.ctypes.data_as(fp)))
        return (i0.reshape(shape), i1.reshape(shape), w.reshape(shape)) if blend else i0.reshape(shape)

    def _queries(self, az, el, radius_m):
        azq, elq = np.broadcast_arrays(np.asarray(az, np.float32), np.asarray(el, np.float32))
        return _xyz(azq.ravel(), elq.ravel(), np.float32(radius_m)), azq.shape

    def nearest(self, az, el, radius_m: float = 1.0) -> np.ndarray:
        """scene.nearest_directions(positions, az, el, radius_m), index for index"""
        q, shape = self._queries(az, el, radius_m)
        return self.points(q, blend=False).reshape(shape)

    def bracket(self, az, el, radius_m: float = 1.0):
        """scene2.bracket_directions(positions, az, el, radius_m): the same chord wherever one chord is clearly the nearest (the
        helper's sums have no promised order; include/ohs_lookup.h writes this one's out)"""
        q, shape = self._queries(az, el, radius_m)
        i0, i1, w = self.points(q)
        return i0.reshape(shape), i1.reshape(shape), w.reshape(shape)

    def rows(self, src_az, src_el, yaw, pitch=0.0, roll=0.0, radius_m: float = 1.0, blend: bool = True):
        """Sources in the room and head poses, everything in the plugin's degrees as scene.rotate_sources takes them -> the rows of a
        scene call, [streams][segs][K]: (idx0, idx1, w) for BlendSceneProcessor.process, or with blend=False idx0 for
        SceneProcessor.process.  Sources: [K], [streams][K], [segs][K] or [streams][segs][K]; poses: [segs] or [streams][segs]."""
        v, sss, sks, R, rss, S, n_segs, K = rows_host_half(src_az, src_el, yaw, pitch, roll, radius_m)
        n = S * n_segs * K
        i0 = np.empty(n, np.uint32)
        i1, w = (np.empty(n, np.uint32), np.empty(n, np.float32)) if blend else (None, None)
        lookup_check(lookup_lib().ohs_lookup_rows(self._h, S, n_segs, K, v.ctypes.data_as(dp), sss, sks, R.ctypes.data_as(dp), rss,
                                                  i0.ctypes.data_as(u32p), None if i1 is None else i1.ctypes.data_as(u32p),
                                                  None if w is None else w.ctypes.data_as(fp)))
        shape = (S, n_segs, K)
        return (i0.reshape(shape), i1.reshape(shape), w.reshape(shape)) if blend else i0.reshape(shape)

    def last_launch(self):
        """(table points the kernel stages at a time, queries per chunk, chunks of the most recent call)"""
        t, q, c = C.c_uint(), C.c_size_t(), C.c_size_t()
        lookup_check(lookup_lib().ohs_lookup_last_launch(self._h, C.byref(t), C.byref(q), C.byref(c)))
        return int(t.value), int(q.value), int(c.value)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and getattr(self, "_destroy", None) is not None:
            self._destroy(h)

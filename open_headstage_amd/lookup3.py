"""Three-direction rows for the scene calls, found on the device: libohs_lookup3.so (include/ohs_lookup3.h).

scene3.triangle_directions is the definition of the rows TriSceneProcessor.process reads -- three indices and two weights per object,
stream and segment over a triangle mesh of the measurements -- and brute force in numpy over every triangle.  TriangleLookup answers
the same question with k_lookup_tri, a call for all queries, bit for bit: `.triangle` takes what the helper takes, `.rows` takes
sources in the room and a head pose per stream and segment (lookup.rows_host_half).  Angles become coordinates here, in numpy
(scene._xyz): the library has no trigonometry.  The library is a sixth one with a loader and a prototype table of its own.  There is
no fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._ffi import OHS_OK, fp
from .lookup import dp, rows_host_half, table_xyz
from .scene import _xyz, u32p, vp, vpp

HERE = os.path.dirname(os.path.abspath(__file__))
LOOKUP3_LIB_PATH = os.path.join(HERE, "libohs_lookup3.so")
MAX_OBJECTS = 64
MAX_DIRECTIONS = 65536
MAX_TRIANGLES = 131072

szp = C.POINTER(C.c_size_t)
_OUT = [u32p, u32p, u32p, fp, fp, u32p]     # idx0, idx1, idx2, w1, w2, tri

# name -> (restype, argtypes): the complete export list of include/ohs_lookup3.h
LOOKUP3_PROTOTYPES = {
    "ohs_lookup3_create": (C.c_int, [C.c_int, C.c_size_t, fp, C.c_size_t, u32p, vpp]),
    "ohs_lookup3_destroy": (None, [vp]),
    "ohs_lookup3_status_string": (C.c_char_p, [C.c_int]),
    "ohs_lookup3_last_error": (C.c_char_p, []),
    "ohs_lookup3_points": (C.c_int, [vp, C.c_size_t, dp] + _OUT),
    "ohs_lookup3_rows": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_size_t, dp, C.c_size_t, C.c_size_t, dp, C.c_size_t] + _OUT),
    "ohs_lookup3_last_launch": (C.c_int, [vp, C.POINTER(C.c_uint), szp, szp]),
    "ohs_lookup3_mesh": (C.c_int, [vp, szp, szp]),
}

_lib = None


def lookup3_lib() -> C.CDLL:
    """libohs_lookup3.so, loaded beside the other libraries.  There is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LOOKUP3_LIB_PATH):
            raise ImportError(f"{LOOKUP3_LIB_PATH} not found: build it with `python -m open_headstage_amd.build` (hipcc, gfx950)")
        try:
            import torch  # noqa: F401  (one HIP runtime per process: torch's first, see _ffi._load)
        except ImportError:
            pass
        L = C.CDLL(LOOKUP3_LIB_PATH)
        for name, (res, args) in LOOKUP3_PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class TriangleLookupError(RuntimeError):
    def __init__(self, status: int, detail: str, text: str | None = None):
        self.status = status
        text = lookup3_lib().ohs_lookup3_status_string(status).decode() if text is None else text
        super().__init__(f"{text} ({status}): {detail}")


def lookup3_check(status: int) -> None:
    if status != OHS_OK:
        raise TriangleLookupError(status, lookup3_lib().ohs_lookup3_last_error().decode(errors="replace"))


def octahedron_mesh(levels: int = 0):
    """A closed triangle mesh over the sphere without scipy: the octahedron with every face cut into 4^levels triangles and the points
    pushed out to radius 1 -> (positions [M][3] (azimuth, elevation in SOFA degrees, radius) f32, triangles [T][3] uint32), M =
    4 n^2 + 2 and T = 8 n^2 with n = 2^levels.  The points are the integer triples (i, j, k) with |i| + |j| + |k| = n, numbered in
    the order the faces meet them."""
    n = 1 << int(levels)
    index, tris = {}, []

    def point(sign, a, b):
        key = (sign[0] * a, sign[1] * b, sign[2] * (n - a - b))
        return index.setdefault(key, len(index))
    for sign in [(sx, sy, sz) for sz in (1, -1) for sy in (1, -1) for sx in (1, -1)]:
        for a in range(n):
            for b in range(n - a):
                tris.append([point(sign, a, b), point(sign, a + 1, b), point(sign, a, b + 1)])
                if a + b < n - 1:
                    tris.append([point(sign, a + 1, b), point(sign, a + 1, b + 1), point(sign, a, b + 1)])
    p = np.array(list(index), np.float64)
    p /= np.sqrt((p * p).sum(1))[:, None]
    pos = np.stack([np.degrees(np.arctan2(p[:, 1], p[:, 0])) % 360.0, np.degrees(np.arcsin(np.clip(p[:, 2], -1.0, 1.0))), np.ones(len(p))], 1)
    return pos.astype(np.float32), np.array(tris, np.uint32)


class TriangleLookup:
    """The measurements of a table (positions [M][3] as SceneProcessor.set_directions_from_sofa returns them) and a triangle mesh
    over them (triangles [T][3], as scene3.triangulate_directions makes them) on the device."""

    def __init__(self, positions, triangles, device: int = 0, xyz=None):
        """xyz: the table's Cartesian coordinates [M][3] themselves, f32, instead of positions (positions None)"""
        self._h = None
        xyz = table_xyz(positions) if xyz is None else np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        tri = np.asarray(triangles)
        if tri.ndim != 2 or tri.shape[1] != 3 or tri.shape[0] == 0:
            raise ValueError(f"triangles: expected [T][3] with T >= 1, got {tri.shape}")
        if not np.issubdtype(tri.dtype, np.integer) or tri.min() < 0 or tri.max() >= xyz.shape[0]:
            raise ValueError(f"triangles: integer indices into the {xyz.shape[0]} positions expected")
        tri = np.ascontiguousarray(tri, np.uint32)
        self.n_directions, self.n_triangles, self.device = int(xyz.shape[0]), int(tri.shape[0]), int(device)
        L = lookup3_lib()
        h = C.c_void_p()
        lookup3_check(L.ohs_lookup3_create(self.device, self.n_directions, xyz.ctypes.data_as(fp), self.n_triangles,
                                           tri.ctypes.data_as(u32p), C.byref(h)))
        self._h = h
        self._destroy = L.ohs_lookup3_destroy

    @staticmethod
    def _outputs(n, return_triangle):
        arrays = [np.empty(n, np.uint32) for _ in range(3)] + [np.empty(n, np.float32) for _ in range(2)]
        if return_triangle:
            arrays.append(np.empty(n, np.uint32))
        ptrs = [a.ctypes.data_as(t) for a, t in zip(arrays, _OUT)] + ([] if return_triangle else [None])
        return arrays, ptrs

    def points(self, q, return_triangle: bool = False):
        """ohs_lookup3_points on q [..][3], f64 Cartesian in the table's frame -> (idx0, idx1, idx2, w1, w2), of q's leading shape;
        return_triangle appends the winning triangle's index"""
        q = np.ascontiguousarray(q, np.float64)
        if q.ndim < 1 or q.shape[-1] != 3:
            raise ValueError(f"expected q [..][3], got {q.shape}")
        shape, n = q.shape[:-1], q.size // 3
        arrays, ptrs = self._outputs(n, return_triangle)
        lookup3_check(lookup3_lib().ohs_lookup3_points(self._h, n, q.ctypes.data_as(dp), *ptrs))
        return tuple(a.reshape(shape) for a in arrays)

    def triangle(self, az, el, radius_m: float = 1.0, return_triangle: bool = False):
        """scene3.triangle_directions(positions, triangles, az, el, radius_m), bit for bit"""
        azq, elq = np.broadcast_arrays(np.asarray(az, np.float32), np.asarray(el, np.float32))
        out = self.points(_xyz(azq.ravel(), elq.ravel(), np.float32(radius_m)), return_triangle)
        return tuple(a.reshape(azq.shape) for a in out)

    def rows(self, src_az, src_el, yaw, pitch=0.0, roll=0.0, radius_m: float = 1.0, return_triangle: bool = False):
        """Sources in the room and head poses, everything in the plugin's degrees as scene.rotate_sources takes them -> the rows of
        TriSceneProcessor.process, [streams][segs][K]: (idx0, idx1, idx2, w1, w2) for its idx, idx1, idx2, weights, weights2.
        Sources: [K], [streams][K], [segs][K] or [streams][segs][K]; poses: [segs] or [streams][segs]."""
        v, sss, sks, R, rss, S, n_segs, K = rows_host_half(src_az, src_el, yaw, pitch, roll, radius_m)
        arrays, ptrs = self._outputs(S * n_segs * K, return_triangle)
        lookup3_check(lookup3_lib().ohs_lookup3_rows(self._h, S, n_segs, K, v.ctypes.data_as(dp), sss, sks, R.ctypes.data_as(dp), rss, *ptrs))
        return tuple(a.reshape((S, n_segs, K)) for a in arrays)

    def last_launch(self):
        """(triangles the kernel stages at a time, queries per chunk, chunks of the most recent call)"""
        t, q, c = C.c_uint(), C.c_size_t(), C.c_size_t()
        lookup3_check(lookup3_lib().ohs_lookup3_last_launch(self._h, C.byref(t), C.byref(q), C.byref(c)))
        return int(t.value), int(q.value), int(c.value)

    def mesh(self):
        """(directions, triangles) of the handle"""
        m, t = C.c_size_t(), C.c_size_t()
        lookup3_check(lookup3_lib().ohs_lookup3_mesh(self._h, C.byref(m), C.byref(t)))
        return int(m.value), int(t.value)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and getattr(self, "_destroy", None) is not None:
            self._destroy(h)

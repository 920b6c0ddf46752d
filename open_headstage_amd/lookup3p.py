"""Three-direction rows for the scene calls at any mesh size: libohs_lookup3p.so (include/ohs_lookup3p.h).

TriangleLookup (lookup3.py) walks every triangle of the mesh for every query.  PrunedTriangleLookup answers the same questions with
the same bits -- idx0, idx1, idx2, w1, w2 and the winning triangle -- from a cube-map index over directions built at create: pass 1
(k_lookup_tri_cells) walks only the triangles whose reach covers the query's cell, a certificate decides whether that answer is the
full walk's, and pass 2 (k_lookup_tri_rest) gives the queries it does not cover -- the origin, queries on a corner or an edge, queries
outside an open mesh -- the full walk.  No answer depends on the grid.  The library is a seventh one with a loader and a prototype
table of its own.  There is no fallback to TriangleLookup or to numpy.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._ffi import OHS_OK, fp
from .lookup import dp, rows_host_half, table_xyz
from .lookup3 import _OUT, szp
from .scene import _xyz, u32p, vp, vpp

HERE = os.path.dirname(os.path.abspath(__file__))
LOOKUP3P_LIB_PATH = os.path.join(HERE, "libohs_lookup3p.so")
MAX_GRID = 256

# name -> (restype, argtypes): the complete export list of include/ohs_lookup3p.h
LOOKUP3P_PROTOTYPES = {
    "ohs_lookup3p_create": (C.c_int, [C.c_int, C.c_size_t, fp, C.c_size_t, u32p, C.c_uint, vpp]),
    "ohs_lookup3p_destroy": (None, [vp]),
    "ohs_lookup3p_status_string": (C.c_char_p, [C.c_int]),
    "ohs_lookup3p_last_error": (C.c_char_p, []),
    "ohs_lookup3p_points": (C.c_int, [vp, C.c_size_t, dp] + _OUT),
    "ohs_lookup3p_rows": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.c_size_t, dp, C.c_size_t, C.c_size_t, dp, C.c_size_t] + _OUT),
    "ohs_lookup3p_last_launch": (C.c_int, [vp, szp, szp, C.POINTER(C.c_uint64)]),
    "ohs_lookup3p_index": (C.c_int, [vp, C.POINTER(C.c_uint), szp, szp, szp, szp]),
    "ohs_lookup3p_mesh": (C.c_int, [vp, szp, szp]),
}

_lib = None


def lookup3p_lib() -> C.CDLL:
    """libohs_lookup3p.so, loaded beside the other libraries.  There is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LOOKUP3P_LIB_PATH):
            raise ImportError(f"{LOOKUP3P_LIB_PATH} not found: build it with `python -m open_headstage_amd.build` (hipcc, gfx950)")
        try:
            import torch  # noqa: F401  (one HIP runtime per process: torch's first, see _ffi._load)
        except ImportError:
            pass
        L = C.CDLL(LOOKUP3P_LIB_PATH)
        for name, (res, args) in LOOKUP3P_PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class PrunedTriangleLookupError(RuntimeError):
    def __init__(self, status: int, detail: str, text: str | None = None):
        self.status = status
        text = lookup3p_lib().ohs_lookup3p_status_string(status).decode() if text is None else text
        super().__init__(f"{text} ({status}): {detail}")


def lookup3p_check(status: int) -> None:
    if status != OHS_OK:
        raise PrunedTriangleLookupError(status, lookup3p_lib().ohs_lookup3p_last_error().decode(errors="replace"))


class PrunedTriangleLookup:
    """TriangleLookup's table and mesh on the device, with an index over directions.  grid: the cube map's cells per face edge, 1 ..
    256, or 0 for the library's choice (about one cell per triangle)."""

    def __init__(self, positions, triangles, device: int = 0, grid: int = 0, xyz=None):
        """xyz: the table's Cartesian coordinates [M][3] themselves, f32, instead of positions (positions None)"""
        self._h = None
        xyz = table_xyz(positions) if xyz is None else np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        tri = np.asarray(triangles)
        if tri.ndim != 2 or tri.shape[1] != 3 or tri.shape[0] == 0:
            raise ValueError(f"triangles: expected [T][3] with T >= 1, got {tri.shape}")
        if not np.issubdtype(tri.dtype, np.integer) or tri.min() < 0 or tri.max() >= xyz.shape[0]:
            raise ValueError(f"triangles: integer indices into the {xyz.shape[0]} positions expected")
        if not 0 <= int(grid) <= MAX_GRID:
            raise ValueError(f"grid: 0 (the library's choice) or 1 .. {MAX_GRID} expected, got {grid}")
        tri = np.ascontiguousarray(tri, np.uint32)
        self.n_directions, self.n_triangles, self.device = int(xyz.shape[0]), int(tri.shape[0]), int(device)
        L = lookup3p_lib()
        h = C.c_void_p()
        lookup3p_check(L.ohs_lookup3p_create(self.device, self.n_directions, xyz.ctypes.data_as(fp), self.n_triangles,
                                             tri.ctypes.data_as(u32p), int(grid), C.byref(h)))
        self._h = h
        self._destroy = L.ohs_lookup3p_destroy

    @staticmethod
    def _outputs(n, return_triangle):
        arrays = [np.empty(n, np.uint32) for _ in range(3)] + [np.empty(n, np.float32) for _ in range(2)]
        if return_triangle:
            arrays.append(np.empty(n, np.uint32))
        ptrs = [a.ctypes.data_as(t) for a, t in zip(arrays, _OUT)] + ([] if return_triangle else [None])
        return arrays, ptrs

    def points(self, q, return_triangle: bool = False):
        """ohs_lookup3p_points on q [..][3], f64 Cartesian in the table's frame -> (idx0, idx1, idx2, w1, w2), of q's leading shape;
        return_triangle appends the winning triangle's index"""
        q = np.ascontiguousarray(q, np.float64)
        if q.ndim < 1 or q.shape[-1] != 3:
            raise ValueError(f"expected q [..][3], got {q.shape}")
        shape, n = q.shape[:-1], q.size // 3
        arrays, ptrs = self._outputs(n, return_triangle)
        lookup3p_check(lookup3p_lib().ohs_lookup3p_points(self._h, n, q.ctypes.data_as(dp), *ptrs))
        return tuple(a.reshape(shape) for a in arrays)

    def triangle(self, az, el, radius_m: float = 1.0, return_triangle: bool = False):
        """scene3.triangle_directions(positions, triangles, az, el, radius_m), bit for bit"""
        azq, elq = np.broadcast_arrays(np.asarray(az, np.float32), np.asarray(el, np.float32))
        out = self.points(_xyz(azq.ravel(), elq.ravel(), np.float32(radius_m)), return_triangle)
        return tuple(a.reshape(azq.shape) for a in out)

    def rows(self, src_az, src_el, yaw, pitch=0.0, roll=0.0, radius_m: float = 1.0, return_triangle: bool = False):
        """TriangleLookup.rows: sources in the room and head poses in the plugin's degrees -> the rows of TriSceneProcessor.process,
        [streams][segs][K]"""
        v, sss, sks, R, rss, S, n_segs, K = rows_host_half(src_az, src_el, yaw, pitch, roll, radius_m)
        arrays, ptrs = self._outputs(S * n_segs * K, return_triangle)
        lookup3p_check(lookup3p_lib().ohs_lookup3p_rows(self._h, S, n_segs, K, v.ctypes.data_as(dp), sss, sks, R.ctypes.data_as(dp), rss, *ptrs))
        return tuple(a.reshape((S, n_segs, K)) for a in arrays)

    def last_launch(self):
        """(queries per chunk, chunks of the most recent call, how many of its queries pass 2 answered)"""
        q, c, f = C.c_size_t(), C.c_size_t(), C.c_uint64()
        lookup3p_check(lookup3p_lib().ohs_lookup3p_last_launch(self._h, C.byref(q), C.byref(c), C.byref(f)))
        return int(q.value), int(c.value), int(f.value)

    def index(self):
        """(G, cells = 6 G^2, entries of all cells' lists, the longest cell's list, the length of the everywhere list)"""
        g, cells, entries, longest, every = C.c_uint(), C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        lookup3p_check(lookup3p_lib().ohs_lookup3p_index(self._h, C.byref(g), C.byref(cells), C.byref(entries), C.byref(longest), C.byref(every)))
        return int(g.value), int(cells.value), int(entries.value), int(longest.value), int(every.value)

    def mesh(self):
        """(directions, triangles) of the handle"""
        m, t = C.c_size_t(), C.c_size_t()
        lookup3p_check(lookup3p_lib().ohs_lookup3p_mesh(self._h, C.byref(m), C.byref(t)))
        return int(m.value), int(t.value)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and getattr(self, "_destroy", None) is not None:
            self._destroy(h)

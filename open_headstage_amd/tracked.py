"""The tracked scene call over libohs_tracked.so (include/ohs_tracked.h): sources and head poses in, two ears out, the rows on the device.

TrackedSceneProcessor is what PrunedTriangleLookup.rows followed by TriSceneProcessor.process computes, bit for bit, as ONE asynchronous
call: the lookup's passes write the rows where the scene kernel reads them, k_scene_rows_seal does the scene call's host scan on the
device, and the last segment's rows stay on the handle as what stands in front of the next call.  The library is an eighth one with a
loader and a prototype table of its own.  There is no fallback to the two-call path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._ffi import fp
from .batch import _layout_io, _n_segs
from .dsp import BLOCK_SIZE
from .lookup import dp, rows_host_half, table_xyz
from .scene import SWITCH_CROSSFADE, SWITCH_RING_OUT, SceneProcessor, u32p, vp, vpp

HERE = os.path.dirname(os.path.abspath(__file__))
TRACKED_LIB_PATH = os.path.join(HERE, "libohs_tracked.so")
MAX_GRID = 256
FRESH, CARRY = 0, 1

_ull = C.POINTER(C.c_ulonglong)
# name -> (restype, argtypes): the complete export list of include/ohs_tracked.h
TRACKED_PROTOTYPES = {
    "ohs_tracked_create": (C.c_int, [C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, fp, C.c_size_t, u32p, C.c_uint, vpp]),
    "ohs_tracked_destroy": (None, [vp]),
    "ohs_tracked_status_string": (C.c_char_p, [C.c_int]),
    "ohs_tracked_last_error": (C.c_char_p, []),
    "ohs_tracked_set_direction_irs": (C.c_int, [vp, C.c_size_t, fp, C.c_size_t]),
    "ohs_tracked_set_gain": (C.c_int, [vp, C.c_float]),
    "ohs_tracked_set_eq_band_coeffs": (C.c_int, [vp, C.c_size_t, fp, C.c_int]),
    "ohs_tracked_set_eq_enabled": (C.c_int, [vp, C.c_int]),
    "ohs_tracked_set_flush_denormals": (C.c_int, [vp, C.c_int]),
    "ohs_tracked_reset": (C.c_int, [vp]),
    "ohs_tracked_sync": (C.c_int, [vp, vp]),
    "ohs_tracked_process": (C.c_int, [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                      dp, C.c_size_t, C.c_size_t, dp, C.c_size_t, fp, C.c_int, C.c_int, vp]),
    "ohs_tracked_last_launch": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), _ull, _ull, _ull, _ull]),
    "ohs_tracked_rows": (C.c_int, [vp, u32p, u32p, u32p, fp, fp]),
}

_lib = None


def tracked_lib() -> C.CDLL:
    """libohs_tracked.so, loaded beside the other libraries: a copy of the code with its own state.  There is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(TRACKED_LIB_PATH):
            raise ImportError(f"{TRACKED_LIB_PATH} not found: build it with `python -m open_headstage_amd.build` (hipcc, gfx950)")
        try:
            import torch  # noqa: F401  (one HIP runtime per process: torch's first, see _ffi._load)
        except ImportError:
            pass
        L = C.CDLL(TRACKED_LIB_PATH)
        for name, (res, args) in TRACKED_PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class TrackedSceneProcessor(SceneProcessor):
    """TriSceneProcessor's handle and PrunedTriangleLookup's table and mesh in one.  positions: [M][3] (azimuth, elevation in SOFA
    degrees, radius), as set_directions_from_sofa returns them -- row i of the direction table is measurement i; triangles: [T][3]
    indices into them; grid: the lookup's cells per cube-face edge, 0 for the library's choice.  set_directions,
    set_directions_from_sofa and the chain's setters are SceneProcessor's."""
    _prefix = "ohs_tracked_"
    _loader = staticmethod(tracked_lib)

    def __init__(self, n_streams: int, positions, triangles, grid: int = 0, num_bands: int = 10, device: int = 0, xyz=None):
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
        self.n_streams, self.num_bands, self.device = int(n_streams), int(num_bands), int(device)
        self.n_directions = 0
        self.n_mesh_directions, self.n_triangles = int(xyz.shape[0]), int(tri.shape[0])
        self._shape = None      # (streams, segments, K) of the most recent call
        self._carried = False   # the handle holds that call's last segment
        h = C.c_void_p()
        self._check(self._fn("create")(self.device, self.n_streams, self.num_bands, self.n_mesh_directions, xyz.ctypes.data_as(fp),
                                       self.n_triangles, tri.ctypes.data_as(u32p), int(grid), C.byref(h)))
        self._h = h
        self._destroy = self._fn("destroy")

    # -- the call -----------------------------------------------------------------------------
    def process_ptr(self, d_in: int, d_out: int, n_blocks: int, in_stream_stride: int, in_channel_stride: int, out_stream_stride: int,
                    out_channel_stride: int, n_objects: int, seg_blocks: int, src, src_stream_stride: int, src_seg_stride: int, rot=None,
                    rot_stream_stride: int = 0, gains=None, crossfade: bool = True, carry=None, hip_stream: int = 0) -> None:
        """ohs_tracked_process.  src: f64 [..][K][3] with ohs_lookup3p_rows' strides (in entries of K sources); rot: f64 3 x 3 per
        (stream and) segment or None; gains: f32 [streams][segs][K] or None (1.0); carry: True -- the handle's carried rows stand in
        front of the call --, False, or None: True when rows are carried."""
        K, n_segs = int(n_objects), _n_segs(n_blocks, seg_blocks)
        src = np.ascontiguousarray(src, np.float64)
        rot = None if rot is None else np.ascontiguousarray(rot, np.float64)
        g = None
        if gains is not None:
            g = np.ascontiguousarray(gains, np.float32)
            if g.shape != (self.n_streams, n_segs, K):
                raise ValueError(f"gains: expected [{self.n_streams}][{n_segs}][{K}], got {g.shape}")
        if carry is None:
            carry = self._carried
        self._check(self._fn("process")(
            self._h, C.c_void_p(d_in), C.c_void_p(d_out), int(n_blocks), int(in_stream_stride), int(in_channel_stride),
            int(out_stream_stride), int(out_channel_stride), K, int(seg_blocks), src.ctypes.data_as(dp), int(src_stream_stride),
            int(src_seg_stride), None if rot is None else rot.ctypes.data_as(dp), int(rot_stream_stride),
            None if g is None else g.ctypes.data_as(fp), SWITCH_CROSSFADE if crossfade else SWITCH_RING_OUT, CARRY if carry else FRESH,
            C.c_void_p(hip_stream) if hip_stream else None))
        if n_blocks:
            self._shape, self._carried = (self.n_streams, n_segs, K), True

    def process_xyz(self, x, src, rot, seg_blocks: int, gains=None, carry=None, crossfade: bool = True, out=None,
                    hip_stream: int | None = None, src_stream_stride: int | None = None, src_seg_stride: int | None = None,
                    rot_stream_stride: int | None = None):
        """x: contiguous float32 device tensor [streams, >= K, frames] -> [streams, 2, frames].  src: Cartesian f64 in the table's
        frame, [K][3], [segs][K][3] or [streams][segs][K][3]; rot: [segs][3][3], [streams][segs][3][3] or None (q = rot^T src, as
        ohs_lookup3p_rows forms it).  The strides follow from the shapes unless given."""
        src = np.ascontiguousarray(src, np.float64)
        if src.ndim < 2 or src.shape[-1] != 3:
            raise ValueError(f"expected src [..][K][3], got {src.shape}")
        K = int(src.shape[-2])
        out, hip_stream, frames = _layout_io(self, x, K, out, hip_stream)
        n_segs = _n_segs(frames // BLOCK_SIZE, seg_blocks)
        if src_stream_stride is None and src_seg_stride is None:
            if src.ndim == 2:
                src_stream_stride = src_seg_stride = 0
            elif src.ndim == 3 and src.shape[0] == n_segs:
                src_stream_stride, src_seg_stride = 0, 1
            elif src.ndim == 4 and src.shape[:2] == (self.n_streams, n_segs):
                src_stream_stride, src_seg_stride = n_segs, 1
            else:
                raise ValueError(f"src {src.shape}: expected [K][3], [{n_segs}][K][3] or [{self.n_streams}][{n_segs}][K][3]")
        if rot is not None and rot_stream_stride is None:
            rot = np.ascontiguousarray(rot, np.float64)
            if rot.shape == (n_segs, 3, 3):
                rot_stream_stride = 0
            elif rot.shape == (self.n_streams, n_segs, 3, 3):
                rot_stream_stride = n_segs
            else:
                raise ValueError(f"rot {rot.shape}: expected [{n_segs}][3][3] or [{self.n_streams}][{n_segs}][3][3]")
        self.process_ptr(x.data_ptr(), out.data_ptr(), frames // BLOCK_SIZE, x.shape[1] * frames, frames, 2 * frames, frames, K,
                         seg_blocks, src, src_stream_stride or 0, src_seg_stride or 0, rot, rot_stream_stride or 0, gains, crossfade,
                         carry, hip_stream)
        return out

    def process(self, x, src_az, src_el, yaw, pitch=0.0, roll=0.0, seg_blocks: int = 1, gains=None, carry=None, crossfade: bool = True,
                radius_m: float = 1.0, out=None, hip_stream: int | None = None):
        """Sources in the room and head poses in the plugin's degrees, PrunedTriangleLookup.rows' conventions and shapes (sources [K],
        [streams][K], [segs][K] or [streams][segs][K]; poses [segs] or [streams][segs]) -> what TriSceneProcessor.process renders from
        those rows: gain * sum over objects of conv(((1 - w1) - w2) h[idx0] + w1 h[idx1] + w2 h[idx2], x[:, c] * gains[c]), then the
        handle's EQ if it is enabled.  carry=None: the rows the handle carries stand in front of the call, if it carries any."""
        v, sss, sks, R, rss, S, n_segs, K = rows_host_half(src_az, src_el, yaw, pitch, roll, radius_m)
        out, hip_stream, frames = _layout_io(self, x, K, out, hip_stream)
        if n_segs != _n_segs(frames // BLOCK_SIZE, seg_blocks) or S not in (1, self.n_streams):
            raise ValueError(f"poses for {n_segs} segments of {S} streams beside {frames // BLOCK_SIZE} blocks in segments of {seg_blocks} "
                             f"on {self.n_streams} streams")
        if S == 1 and self.n_streams > 1:       # (one row of sources and poses for all streams)
            sss = rss = 0
        self.process_ptr(x.data_ptr(), out.data_ptr(), frames // BLOCK_SIZE, x.shape[1] * frames, frames, 2 * frames, frames, K,
                         seg_blocks, v, sss, sks, R, rss, gains, crossfade, carry, hip_stream)
        return out

    # -- what was rendered ----------------------------------------------------------------------
    def rows(self):
        """(idx0, idx1, idx2, w1, w2) of the most recent call, [streams][segs][K] each, copied from the device (waits for the call)"""
        if self._shape is None:
            raise RuntimeError("no call has been made on this handle")
        n = int(np.prod(self._shape))
        arrays = [np.empty(n, np.uint32) for _ in range(3)] + [np.empty(n, np.float32) for _ in range(2)]
        self._check(self._fn("rows")(self._h, *[a.ctypes.data_as(t) for a, t in zip(arrays, (u32p, u32p, u32p, fp, fp))]))
        return tuple(a.reshape(self._shape) for a in arrays)

    def last_launch(self):
        """(pairs of objects, block ranges per stream, passes through old directions, passes that loaded four table rows, passes that
        loaded six, queries the lookup's pass 2 answered) of the most recent call (waits for it); zeros: none yet"""
        p, r = C.c_int(), C.c_int()
        f, b, t, q = C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
        self._check(self._fn("last_launch")(self._h, C.byref(p), C.byref(r), C.byref(f), C.byref(b), C.byref(t), C.byref(q)))
        return int(p.value), int(r.value), int(f.value), int(b.value), int(t.value), int(q.value)

    def reset(self) -> None:
        """SceneProcessor.reset, and the carried rows are dropped"""
        super().reset()
        self._carried = False

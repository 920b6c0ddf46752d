"""Blended object scenes over libohs_scene2.so (include/ohs_scene2.h): every object between TWO measured directions, in one kernel.

libohs_scene2.so is a superset of libohs_scene.so in a library of its own -- ohs_scene.h is frozen as ohs_hip.h is --, so this module
has its own loader and prototype table (SCENE2_PROTOTYPES); `scene.SCENE_PROTOTYPES` stays the thirteen entries of ohs_scene.h.
BlendSceneProcessor is a SceneProcessor on the new library: the same methods, `process` with a second index and a weight per object,
`last_launch` with a fourth figure.  bracket_directions finds the two indices and the weight for a source position.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._ffi import fp
from .batch import _layout_io, _n_segs
from .dsp import BLOCK_SIZE
from .scene import (SCENE_PROTOTYPES, SWITCH_CROSSFADE, SWITCH_RING_OUT, SceneProcessor, _object_rows, _xyz, nearest_directions,
                    u32p, vp)

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE2_LIB_PATH = os.path.join(HERE, "libohs_scene2.so")

# name -> (restype, argtypes): the complete export list of include/ohs_scene2.h -- ohs_scene.h's thirteen under the new prefix, the
# launch record with a fourth out-parameter, and the blended call
SCENE2_PROTOTYPES = {name.replace("ohs_scene_", "ohs_scene2_", 1): proto for name, proto in SCENE_PROTOTYPES.items()}
SCENE2_PROTOTYPES["ohs_scene2_last_launch"] = (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_ulonglong),
                                                         C.POINTER(C.c_ulonglong)])
SCENE2_PROTOTYPES["ohs_scene2_process_blended"] = (C.c_int, SCENE_PROTOTYPES["ohs_scene_process"][1] + [u32p, fp, u32p, fp])

_lib = None


def scene2_lib() -> C.CDLL:
    """libohs_scene2.so, loaded beside the other two libraries: a copy of the code with its own state.  There is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(SCENE2_LIB_PATH):
            raise ImportError(f"{SCENE2_LIB_PATH} not found: build it with `python -m open_headstage_amd.build` (hipcc, gfx950)")
        try:
            import torch  # noqa: F401  (one HIP runtime per process: torch's first, see _ffi._load)
        except ImportError:
            pass
        L = C.CDLL(SCENE2_LIB_PATH)
        for name, (res, args) in SCENE2_PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def bracket_directions(positions, az, el, radius_m: float = 1.0):
    """The two measurements a source stands between, and how far along: -> (idx0, idx1, w), uint32, uint32, float32, of the queries'
    shape.  idx0 is nearest_directions' answer.  idx1 is the OTHER measurement whose chord [p0, p1] passes nearest to the query (the
    first of equally near ones), w the query's projection onto that chord, clamped to [0, 1]: the source is rendered through
    (1 - w) h[idx0] + w h[idx1].  This is one-dimensional interpolation along the best chord -- exact in position for a source on a
    measured ring, where the chord is the one to the ring neighbour on the query's side; it is no triangulation, and off the rings
    the elevation comes from whichever neighbour the chord names.  A table of one direction gives idx1 = idx0, w = 0.
    positions, az, el, radius_m: as nearest_directions takes them (SOFA degrees)."""
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    p = _xyz(pos[:, 0], pos[:, 1], pos[:, 2]).astype(np.float32).astype(np.float64)      # (nearest_directions' coordinates)
    azq, elq = np.broadcast_arrays(np.asarray(az, np.float32), np.asarray(el, np.float32))
    idx0 = nearest_directions(positions, az, el, radius_m).reshape(-1)
    # (the queries in the precision the measurements are kept in: a query ON a measurement is that point, and w is 0 exactly)
    q = _xyz(azq.ravel(), elq.ravel(), np.float32(radius_m)).astype(np.float32).astype(np.float64)
    idx1 = idx0.copy()
    w = np.zeros(q.shape[0], np.float32)
    if p.shape[0] > 1:
        step = max(1, (1 << 19) // p.shape[0])                          # (slices of about 2^19 chords: a few tens of MB of f64)
        for lo in range(0, q.shape[0], step):
            qs = q[lo:lo + step]
            p0 = p[idx0[lo:lo + step]]                                  # [n][3]
            chord = p[None, :, :] - p0[:, None, :]                      # [n][M][3]
            len2 = np.einsum("nmj,nmj->nm", chord, chord)
            ok = len2 > 0.0                                             # (not idx0 itself, nor a duplicate of it)
            t = np.einsum("nmj,nj->nm", chord, qs - p0) / np.where(ok, len2, 1.0)
            t = np.where(ok, np.clip(t, 0.0, 1.0), 0.0)
            off = p0[:, None, :] + t[:, :, None] * chord - qs[:, None, :]
            d2 = np.where(ok, np.einsum("nmj,nmj->nm", off, off), np.inf)
            j = np.argmin(d2, axis=1)                                   # (ties: the first)
            rows = np.arange(qs.shape[0])
            found = np.isfinite(d2[rows, j])                            # (none: every measurement is a duplicate of idx0)
            idx1[lo:lo + step] = np.where(found, j, idx0[lo:lo + step])
            w[lo:lo + step] = np.where(found, t[rows, j], 0.0).astype(np.float32)
    return idx0.reshape(azq.shape).astype(np.uint32), idx1.reshape(azq.shape).astype(np.uint32), w.reshape(azq.shape)


def _scene_rows(n_streams, K, n_segs, idx, rows, prevs):
    """The rows of a scene call as the C entries read them, for this module's call and scene3's.  idx: [n_segs][K] for all streams or
    [n_streams][n_segs][K]; rows: (value or None, dtype, name) each, of idx's shape; prevs: the same for what stood in front of the
    call's first block, [K] beside shared rows, [n_streams][K] beside rows per stream.
    -> (idx array, idx_stride, [row arrays or None], [prev arrays or None]); the arrays live as long as the caller holds them."""
    if idx is None:
        raise ValueError("idx is required")
    a, stride = _object_rows(idx, n_streams, n_segs, K, "idx", np.uint32)
    out = []
    for v, dtype, what in rows:
        if v is not None:
            v, rs = _object_rows(v, n_streams, n_segs, K, what, dtype)
            if rs != stride:
                raise ValueError(f"{what} must have idx's shape")
        out.append(v)
    n_prev = (n_streams if stride else 1) * K
    front = []
    for v, dtype, what in prevs:
        if v is not None:
            v = np.ascontiguousarray(v, dtype=dtype).reshape(-1)
            if v.size != n_prev:
                raise ValueError(f"{what}: expected {n_prev} entries, got {v.size}")
        front.append(v)
    return a, stride, out, front


def _ptr(v, t):
    return None if v is None else v.ctypes.data_as(t)


class BlendSceneProcessor(SceneProcessor):
    """A SceneProcessor on libohs_scene2.so: every method of it, and two directions with a weight per object."""
    _prefix = "ohs_scene2_"
    _loader = staticmethod(scene2_lib)

    def process_ptr(self, d_in: int, d_out: int, n_blocks: int, in_stream_stride: int, in_channel_stride: int, out_stream_stride: int,
                    out_channel_stride: int, n_objects: int, seg_blocks: int, idx, gains=None, prev_idx=None, prev_gains=None,
                    crossfade: bool = True, hip_stream: int = 0, idx1=None, weights=None, prev_idx1=None, prev_weights=None) -> None:
        """ohs_scene2_process_blended.  idx, gains, prev_idx, prev_gains: as SceneProcessor.process_ptr takes them.  idx1, weights:
        the second direction and its share in [0, 1], idx's shape, both or neither (neither: the one-direction call);
        prev_idx1 / prev_weights: what stood in front of the call's first block, prev_idx's shape, or None: no boundary there."""
        if idx1 is None and weights is None:
            return super().process_ptr(d_in, d_out, n_blocks, in_stream_stride, in_channel_stride, out_stream_stride, out_channel_stride,
                                       n_objects, seg_blocks, idx, gains, prev_idx, prev_gains, crossfade, hip_stream)
        K, u32, f32 = int(n_objects), np.uint32, np.float32
        a, stride, (g, a1, w), (pi, pg, pi1, pw) = _scene_rows(
            self.n_streams, K, _n_segs(n_blocks, seg_blocks), idx, [(gains, f32, "gains"), (idx1, u32, "idx1"), (weights, f32, "weights")],
            [(prev_idx, u32, "prev_idx"), (prev_gains, f32, "prev_gains"), (prev_idx1, u32, "prev_idx1"), (prev_weights, f32, "prev_weights")])
        self._check(self._fn("process_blended")(
            self._h, C.c_void_p(d_in), C.c_void_p(d_out), int(n_blocks), int(in_stream_stride), int(in_channel_stride),
            int(out_stream_stride), int(out_channel_stride), K, int(seg_blocks), _ptr(a, u32p), _ptr(g, fp), stride, _ptr(pi, u32p), _ptr(pg, fp),
            SWITCH_CROSSFADE if crossfade else SWITCH_RING_OUT, C.c_void_p(hip_stream) if hip_stream else None, _ptr(a1, u32p), _ptr(w, fp),
            _ptr(pi1, u32p), _ptr(pw, fp)))

    def process(self, x, idx, seg_blocks: int, gains=None, prev_idx=None, prev_gains=None, crossfade: bool = True, idx1=None,
                weights=None, prev_idx1=None, prev_weights=None, out=None, hip_stream: int | None = None):
        """SceneProcessor.process with every object between two directions: gain * sum over objects of
        conv((1 - w) h[idx] + w h[idx1], x[:, c] * gains[c]), then the handle's EQ if it is enabled.  idx1 / weights None: the
        one-direction call.  A pair of objects whose weights are all +0.0 has that call's bits."""
        K = int(np.shape(idx)[-1])
        out, hip_stream, frames = _layout_io(self, x, K, out, hip_stream)
        self.process_ptr(x.data_ptr(), out.data_ptr(), frames // BLOCK_SIZE, x.shape[1] * frames, frames, 2 * frames, frames, K,
                         seg_blocks, idx, gains, prev_idx, prev_gains, crossfade, hip_stream, idx1, weights, prev_idx1, prev_weights)
        return out

    def last_launch(self):
        """(pairs of objects, block ranges per stream, passes through old directions, passes that loaded four table rows) of the most
        recent launch; zeros: none yet"""
        p, r, f, b = C.c_int(), C.c_int(), C.c_ulonglong(), C.c_ulonglong()
        self._check(self._fn("last_launch")(self._h, C.byref(p), C.byref(r), C.byref(f), C.byref(b)))
        return int(p.value), int(r.value), int(f.value), int(b.value)

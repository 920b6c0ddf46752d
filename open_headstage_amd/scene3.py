"""Object scenes over libohs_scene3.so (include/ohs_scene3.h): every object inside a TRIANGLE of three measured directions, in one kernel.

libohs_scene3.so is a superset of libohs_scene2.so in a library of its own -- the older headers are frozen --, so this module has its
own loader and prototype table (SCENE3_PROTOTYPES); `scene2.SCENE2_PROTOTYPES` stays the fourteen entries of ohs_scene2.h.
TriSceneProcessor is a BlendSceneProcessor on the new library: the same methods, `process` with a third index and a second weight per
object, `last_launch` with a fifth figure.  triangle_directions finds the three indices and the two weights for a source position over a
triangle mesh of the measurements -- it DEFINES those rows --, triangulate_directions makes such a mesh where scipy is installed.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._ffi import fp
from .batch import _layout_io, _n_segs
from .dsp import BLOCK_SIZE
from .scene import SCENE_PROTOTYPES, SWITCH_CROSSFADE, SWITCH_RING_OUT, _xyz, u32p, vp
from .scene2 import BlendSceneProcessor, _ptr, _scene_rows

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE3_LIB_PATH = os.path.join(HERE, "libohs_scene3.so")

# name -> (restype, argtypes): the complete export list of include/ohs_scene3.h -- ohs_scene.h's thirteen under the new prefix, the
# launch record with a fifth out-parameter, the two-direction call and the three-direction call
SCENE3_PROTOTYPES = {name.replace("ohs_scene_", "ohs_scene3_", 1): proto for name, proto in SCENE_PROTOTYPES.items()}
SCENE3_PROTOTYPES["ohs_scene3_last_launch"] = (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_ulonglong),
                                                         C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)])
SCENE3_PROTOTYPES["ohs_scene3_process_blended"] = (C.c_int, SCENE_PROTOTYPES["ohs_scene_process"][1] + [u32p, fp, u32p, fp])
SCENE3_PROTOTYPES["ohs_scene3_process_blended3"] = (C.c_int, SCENE_PROTOTYPES["ohs_scene_process"][1] + [u32p, fp, u32p, fp] +
                                                    [u32p, fp, u32p, fp])

_lib = None


def scene3_lib() -> C.CDLL:
    """libohs_scene3.so, loaded beside the other libraries: a copy of the code with its own state.  There is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(SCENE3_LIB_PATH):
            raise ImportError(f"{SCENE3_LIB_PATH} not found: build it with `python -m open_headstage_amd.build` (hipcc, gfx950)")
        try:
            import torch  # noqa: F401  (one HIP runtime per process: torch's first, see _ffi._load)
        except ImportError:
            pass
        L = C.CDLL(SCENE3_LIB_PATH)
        for name, (res, args) in SCENE3_PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _triangle_inverses(p, tri):
    """the inverse of every triangle's vertex matrix [a b c] (columns), [T][3][3] f64: row 0 = (b x c) / det, row 1 = (c x a) / det,
    row 2 = (a x b) / det, det = (a0 (b x c)0 + a1 (b x c)1) + a2 (b x c)2 -- every product and sum written out, in this order"""
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]

    def cross(u, v):
        return [u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]]
    bc, ca, ab = cross(b, c), cross(c, a), cross(a, b)
    det = (a[:, 0] * bc[0] + a[:, 1] * bc[1]) + a[:, 2] * bc[2]

    def norm(u):
        return np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])
    bad = ~(np.abs(det) > 1e-9 * (norm(a) * norm(b) * norm(c)))       # (not-a-number counts as singular)
    if bad.any():
        t = int(np.flatnonzero(bad)[0])
        raise ValueError(f"triangle {t} {tuple(int(v) for v in tri[t])} is singular: its three directions lie in one plane through the origin")
    inv = np.empty((tri.shape[0], 3, 3), np.float64)
    for i, row in enumerate((bc, ca, ab)):
        for j in range(3):
            inv[:, i, j] = row[j] / det
    return inv


def triangle_directions(positions, triangles, az, el, radius_m: float = 1.0):
    """The triangle of measurements a source stands in, and its barycentric share of each corner (VBAP over a triangulated sphere):
    -> (idx0, idx1, idx2, w1, w2), uint32 x 3 and float32 x 2, of the queries' shape.  The source is rendered through
    ((1 - w1) - w2) h[idx0] + w1 h[idx1] + w2 h[idx2] (TriSceneProcessor.process).  This function is the DEFINITION of those rows:
    elementwise f64 with a fixed order of every sum, so that another implementation can be held to it bit for bit.
      1. the measurements' and the queries' Cartesian coordinates are rounded to f32 and widened (bracket_directions' coordinates);
      2. per triangle (a, b, c) the inverse of its vertex matrix (_triangle_inverses); a singular triangle is refused;
      3. the query's gains over that triangle, g[i] = (inv[i][0] q0 + inv[i][1] q1) + inv[i][2] q2;
      4. the triangle with the largest min(g) wins, the first of equals (inside a triangle every gain is >= 0);
      5. negative gains are set to 0 (an open mesh: no triangle may contain the query; just outside the rim the rim's edge answers), and
         so is a gain of at most 2^-20 of the triangle's largest, compared as g <= 2^-20 max(g) in f64 -- what a query ON a corner or
         an edge keeps of the third corner once coordinates are f32: each of the twelve coordinates of the query and the corners is
         off by up to 2^-25 of the radius, which over a triangle whose corners stand 15 degrees apart or more (height >= 1/4) is a
         gain of up to 12 * 2^-25 * 4 < 2^-20 (a grid of 30 x 30 degrees shows up to 2^-22.2); on a finer mesh such a query may keep
         a third weight near 1e-6, which is rendered correctly, through six rows.  2^-20 is below the renderer's own 1e-6 bar.  If
         nothing is left (every gain <= 0: the query faces away from the best triangle of an open mesh), the corner with the
         largest gain, the first of equals, takes it all;
      6. weights g / ((g0 + g1) + g2);
      7. the three corners in the order of descending weight, equal weights by ascending index;
      8. w1, w2: the second and the third weight as float32, a zero of either sign written +0.0 -- a query on a measurement takes
         the kernel's plain pass, a query on an edge its four-row pass.  w1 <= 1/2 and w2 <= 1/3, so the f32 sum passes the C check.
    positions: [M][3] (azimuth, elevation, radius) in SOFA degrees, as nearest_directions takes them; triangles: [T][3] indices into
    positions (triangulate_directions makes them); az, el, radius_m: the queries, in the same degrees."""
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    p = _xyz(pos[:, 0], pos[:, 1], pos[:, 2]).astype(np.float32).astype(np.float64)
    tri = np.asarray(triangles)
    if tri.ndim != 2 or tri.shape[1] != 3 or tri.shape[0] == 0:
        raise ValueError(f"triangles: expected [T][3] with T >= 1, got {tri.shape}")
    if not np.issubdtype(tri.dtype, np.integer) or tri.min() < 0 or tri.max() >= p.shape[0]:
        raise ValueError(f"triangles: integer indices into the {p.shape[0]} positions expected")
    tri = tri.astype(np.int64)
    inv = _triangle_inverses(p, tri)
    azq, elq = np.broadcast_arrays(np.asarray(az, np.float32), np.asarray(el, np.float32))
    q = _xyz(azq.ravel(), elq.ravel(), np.float32(radius_m)).astype(np.float32).astype(np.float64)
    n = q.shape[0]
    idx = np.empty((n, 3), np.uint32)
    wts = np.empty((n, 3), np.float64)
    step = max(1, (1 << 19) // tri.shape[0])                            # (slices of about 2^19 triangles: a few tens of MB of f64)
    for lo in range(0, n, step):
        qs = q[lo:lo + step]
        q0, q1, q2 = qs[:, None, 0], qs[:, None, 1], qs[:, None, 2]     # [n][1] against [T]
        g = np.stack([(inv[None, :, i, 0] * q0 + inv[None, :, i, 1] * q1) + inv[None, :, i, 2] * q2 for i in range(3)], -1)    # [n][T][3]
        t = np.argmax(np.minimum(np.minimum(g[..., 0], g[..., 1]), g[..., 2]), axis=1)      # (ties: the first)
        rows = np.arange(qs.shape[0])
        gt = g[rows, t]                                                 # [n][3]
        gc = np.where(gt > np.max(gt, axis=1)[:, None] * 2.0 ** -20, gt, 0.0)     # (drops every negative gain beside a positive one)
        gc = np.where(gc < 0.0, 0.0, gc)
        s = (gc[:, 0] + gc[:, 1]) + gc[:, 2]
        none = ~(s > 0.0)
        if none.any():
            top = np.argmax(gt, axis=1)
            gc = np.where(none[:, None], (np.arange(3)[None, :] == top[:, None]).astype(np.float64), gc)
            s = np.where(none, 1.0, s)
        w = gc / s[:, None]
        v = tri[t]                                                      # [n][3]
        order = np.lexsort((v, -w), axis=1)                             # by descending weight, then by ascending index
        idx[lo:lo + step] = np.take_along_axis(v, order, 1)
        wts[lo:lo + step] = np.take_along_axis(w, order, 1)
    w1 = wts[:, 1].astype(np.float32) + np.float32(0.0)                 # (-0.0 + 0.0 = +0.0)
    w2 = wts[:, 2].astype(np.float32) + np.float32(0.0)
    sh = azq.shape
    return idx[:, 0].reshape(sh).copy(), idx[:, 1].reshape(sh).copy(), idx[:, 2].reshape(sh).copy(), w1.reshape(sh), w2.reshape(sh)


def triangulate_directions(positions) -> np.ndarray:
    """A triangle mesh over the measurements for triangle_directions: the convex hull of their unit vectors, [T][3] uint32, every row
    ascending and the rows in ascending order.  A convenience, not part of the definition of the rows -- any mesh will do there.
    Needs scipy (scipy.spatial.ConvexHull); the package does not require it, and without it this function raises ImportError."""
    try:
        from scipy.spatial import ConvexHull
    except ImportError as e:
        raise ImportError("triangulate_directions needs scipy (scipy.spatial.ConvexHull), which is not installed: install scipy, or hand "
                          "triangle_directions a mesh of your own ([T][3] indices into positions)") from e
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    p = _xyz(pos[:, 0], pos[:, 1], np.float32(1.0)).astype(np.float32).astype(np.float64)
    hull = ConvexHull(p, qhull_options="Qt")        # (Qt: triangulated output, also where four measurements share a plane)
    tri = np.sort(np.asarray(hull.simplices, np.int64), axis=1)
    tri = tri[np.lexsort((tri[:, 2], tri[:, 1], tri[:, 0]))]
    return tri.astype(np.uint32)


class TriSceneProcessor(BlendSceneProcessor):
    """A BlendSceneProcessor on libohs_scene3.so: every method of it, and three directions with two weights per object."""
    _prefix = "ohs_scene3_"
    _loader = staticmethod(scene3_lib)

    def process_ptr(self, d_in: int, d_out: int, n_blocks: int, in_stream_stride: int, in_channel_stride: int, out_stream_stride: int,
                    out_channel_stride: int, n_objects: int, seg_blocks: int, idx, gains=None, prev_idx=None, prev_gains=None,
                    crossfade: bool = True, hip_stream: int = 0, idx1=None, weights=None, prev_idx1=None, prev_weights=None,
                    idx2=None, weights2=None, prev_idx2=None, prev_weights2=None) -> None:
        """ohs_scene3_process_blended3.  Everything up to prev_weights: as BlendSceneProcessor.process_ptr takes it (weights is w1).
        idx2, weights2: the third direction and its share, idx's shape, both or neither (neither: the parent's call on this
        library); w1 >= 0, w2 >= 0, w1 + w2 <= 1.  prev_idx2 / prev_weights2: what stood in front of the call's first block,
        prev_idx's shape, or None: no boundary there."""
        if idx2 is None and weights2 is None:
            return super().process_ptr(d_in, d_out, n_blocks, in_stream_stride, in_channel_stride, out_stream_stride, out_channel_stride,
                                       n_objects, seg_blocks, idx, gains, prev_idx, prev_gains, crossfade, hip_stream, idx1, weights,
                                       prev_idx1, prev_weights)
        K, u32, f32 = int(n_objects), np.uint32, np.float32
        a, stride, (g, a1, w, a2, w2), (pi, pg, pi1, pw, pi2, pw2) = _scene_rows(
            self.n_streams, K, _n_segs(n_blocks, seg_blocks), idx,
            [(gains, f32, "gains"), (idx1, u32, "idx1"), (weights, f32, "weights"), (idx2, u32, "idx2"), (weights2, f32, "weights2")],
            [(prev_idx, u32, "prev_idx"), (prev_gains, f32, "prev_gains"), (prev_idx1, u32, "prev_idx1"), (prev_weights, f32, "prev_weights"),
             (prev_idx2, u32, "prev_idx2"), (prev_weights2, f32, "prev_weights2")])
        self._check(self._fn("process_blended3")(
            self._h, C.c_void_p(d_in), C.c_void_p(d_out), int(n_blocks), int(in_stream_stride), int(in_channel_stride),
            int(out_stream_stride), int(out_channel_stride), K, int(seg_blocks), _ptr(a, u32p), _ptr(g, fp), stride, _ptr(pi, u32p), _ptr(pg, fp),
            SWITCH_CROSSFADE if crossfade else SWITCH_RING_OUT, C.c_void_p(hip_stream) if hip_stream else None, _ptr(a1, u32p), _ptr(w, fp),
            _ptr(pi1, u32p), _ptr(pw, fp), _ptr(a2, u32p), _ptr(w2, fp), _ptr(pi2, u32p), _ptr(pw2, fp)))

    def process(self, x, idx, seg_blocks: int, gains=None, prev_idx=None, prev_gains=None, crossfade: bool = True, idx1=None,
                weights=None, prev_idx1=None, prev_weights=None, idx2=None, weights2=None, prev_idx2=None, prev_weights2=None,
                out=None, hip_stream: int | None = None):
        """BlendSceneProcessor.process with every object inside a triangle of directions: gain * sum over objects of
        conv(((1 - w1) - w2) h[idx] + w1 h[idx1] + w2 h[idx2], x[:, c] * gains[c]), then the handle's EQ if it is enabled.
        idx2 / weights2 None: the parent's call.  A pair of objects whose w2 are all +0.0 has the two-direction call's bits, one
        whose w1 are +0.0 as well the one-direction call's."""
        K = int(np.shape(idx)[-1])
        out, hip_stream, frames = _layout_io(self, x, K, out, hip_stream)
        self.process_ptr(x.data_ptr(), out.data_ptr(), frames // BLOCK_SIZE, x.shape[1] * frames, frames, 2 * frames, frames, K,
                         seg_blocks, idx, gains, prev_idx, prev_gains, crossfade, hip_stream, idx1, weights, prev_idx1, prev_weights,
                         idx2, weights2, prev_idx2, prev_weights2)
        return out

    def last_launch(self):
        """(pairs of objects, block ranges per stream, passes through old directions, passes that loaded four table rows, passes that
        loaded six) of the most recent launch; zeros: none yet"""
        p, r, f, b, t = C.c_int(), C.c_int(), C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
        self._check(self._fn("last_launch")(self._h, C.byref(p), C.byref(r), C.byref(f), C.byref(b), C.byref(t)))
        return int(p.value), int(r.value), int(f.value), int(b.value), int(t.value)

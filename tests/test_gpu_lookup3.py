"""libohs_lookup3.so on the device (k_lookup_tri) against tests/lookup3_model.py: every query, bit for bit -- idx0, idx1, idx2, w1, w2 and
the winning triangle's index.

The model is include/ohs_lookup3.h's arithmetic in elementwise numpy (tests/test_cpu_lookup3.py ties it to scene3.triangle_directions,
the definition of the rows, bit for bit).  TT and Q below are the kernel's tile of triangles and the chunk of queries, read from
ohs_lookup3_last_launch: the sizes around them are where the walk over tiles and the cut into chunks can go wrong.  Meshes are random
overlapping triangles over a random unit table (lookup3_model.random_soup) unless a test builds its own: several triangles then contain
a query, and which of them wins is a real contest."""
import ctypes as C

import numpy as np
import pytest

from tests import lookup3_model as l3

pytestmark = pytest.mark.gpu

SENT_U, SENT_F = np.uint32(0xDEADBEEF), np.float32(-7.25)
INV = 1
OCTA_XYZ = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
OCTA_TRI = np.array([[r, (r + 1) % 4, p] for p in (4, 5) for r in range(4)], np.uint32)


def _lookup(xyz, tris):
    import open_headstage_amd as ohs
    return ohs.TriangleLookup(None, tris, xyz=xyz)


def _sizes(lk):
    TT, Q, _ = lk.last_launch()
    assert TT >= 66 and Q >= 258
    return TT, Q


def assert_model_bits(xyz, tris, q, got, what="", model=None):
    """got: (idx0, idx1, idx2, w1, w2, tri); model: l3.lookup3(xyz, tris, q) where the caller has it already
    (tests/test_gpu_lookup_chunks.py)"""
    m = l3.lookup3(xyz, tris, q) if model is None else model
    got = [np.asarray(g).reshape(-1) for g in got]
    bad = np.flatnonzero(~l3.same_rows(got[:5], m) | (got[5] != m["tri"]))
    assert bad.size == 0, (what, bad[:8], [g[bad[:8]] for g in got], [m[k][bad[:8]] for k in l3.FIELDS + ("tri",)])
    assert (l3.bits(got[3]) != 0x80000000).all() and (l3.bits(got[4]) != 0x80000000).all(), what      # (a zero is +0.0)
    return m


def c_arrays(n, extra=5):
    return [np.full(n + extra, SENT_U) for _ in range(3)] + [np.full(n + extra, SENT_F) for _ in range(2)] + [np.full(n + extra, SENT_U)]


def untouched(arrays, lo=0):
    return all((l3.bits(a[lo:]) == l3.bits(SENT_F)).all() if a.dtype == np.float32 else (a[lo:] == SENT_U).all() for a in arrays)


def _ptrs(arrays):
    from open_headstage_amd import lookup3
    return [None if a is None else a.ctypes.data_as(t) for a, t in zip(arrays, lookup3._OUT)]


def c_points(lk, q, arrays):
    from open_headstage_amd import lookup, lookup3
    q = None if q is None else np.ascontiguousarray(q, np.float64)
    n = 1 if q is None else q.size // 3
    return lookup3.lookup3_lib().ohs_lookup3_points(lk._h, n, None if q is None else q.ctypes.data_as(lookup.dp), *_ptrs(arrays))


def c_rows(lk, S, segs, K, src, sss, sks, rot, rss, arrays):
    from open_headstage_amd import lookup, lookup3
    p = lambda a: None if a is None else a.ctypes.data_as(lookup.dp)      # noqa: E731
    return lookup3.lookup3_lib().ohs_lookup3_rows(lk._h, S, segs, K, p(src), sss, sks, p(rot), rss, *_ptrs(arrays))


# ---- mesh sizes around the tile --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["1", "2", "63", "64", "65", "TT-1", "TT", "TT+1", "2*TT+1"])
def test_mesh_sizes(size):
    TT, _ = _sizes(_lookup(OCTA_XYZ, OCTA_TRI))
    T = eval(size, {"TT": TT})
    xyz, tris = l3.random_soup(max(3, min(120, 3 * T)), T, seed=300 + T)
    q = l3.soup_queries(xyz, tris, 600, seed=T)
    often = np.bincount(l3.lookup3(xyz, tris, q)["tri"]).argmax()       # the triangle that wins most often goes last: the walk's tail
    tris[[often, T - 1]] = tris[[T - 1, often]]
    lk = _lookup(xyz, tris)
    assert lk.mesh() == (len(xyz), T)
    m = assert_model_bits(xyz, tris, q, lk.points(q, return_triangle=True), f"T = {T}")
    assert lk.last_launch() == (TT, _sizes(lk)[1], 1)
    assert (m["tri"] == T - 1).any()
    if T > 2 * TT:
        assert len(set(m["tri"] // TT)) == 3            # (winners in every tile)
    if T >= 63:
        assert (m["w2"] > 0).sum() > 100 and (m["m_next"] > 0).sum() > 100      # (a contest: the runner-up contains the query too)
    five = lk.points(q)
    assert len(five) == 5 and l3.same_rows(five, m).all()


# ---- query counts around the wave, the workgroup and the chunk ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_query_counts(n):
    xyz, tris = l3.random_soup(30, 65, seed=65)
    lk = _lookup(xyz, tris)
    q = l3.soup_queries(xyz, tris, 600, seed=n)[:n]
    out = c_arrays(n)
    assert c_points(lk, q, out) == 0
    assert_model_bits(xyz, tris, q, [a[:n] for a in out], f"n = {n}")
    assert untouched(out, n) and lk.last_launch()[2] == 1
    # tri == NULL: the five others are written all the same
    out = c_arrays(n)
    assert c_points(lk, q, out[:5] + [None]) == 0
    assert l3.same_rows([a[:n] for a in out[:5]], l3.lookup3(xyz, tris, q)).all() and untouched(out[:5], n) and untouched(out[5:])


def test_one_query_more_than_a_chunk():
    lk = _lookup(OCTA_XYZ, OCTA_TRI)
    _, Q = _sizes(lk)
    n = Q + 1
    rng = np.random.default_rng(12)
    q = rng.standard_normal((n, 3))
    q[::7] = OCTA_XYZ[rng.integers(0, 6, len(q[::7]))]
    q[3::7] = (OCTA_XYZ[rng.integers(0, 6, len(q[3::7]))] + OCTA_XYZ[rng.integers(0, 6, len(q[3::7]))]) / 2      # (the origin among them)
    out = c_arrays(n)
    assert c_points(lk, q, out) == 0
    assert lk.last_launch()[2] == 2
    assert_model_bits(OCTA_XYZ, OCTA_TRI, q, [a[:n] for a in out], "Q + 1 queries")
    assert untouched(out, n)
    # the buffers have grown to a chunk: a small call behind it is right, and an empty one touches nothing
    assert_model_bits(OCTA_XYZ, OCTA_TRI, q[:7], lk.points(q[:7], return_triangle=True), "a small call behind a large one")
    assert c_points(lk, np.zeros((0, 3)), [None] * 6) == 0 and lk.last_launch()[2] == 0


# ---- ties across the seams ---------------------------------------------------------------------------------------------------------
def test_a_triangle_stored_again_on_both_sides_of_a_tile_boundary():
    """a closed mesh, so that inside a triangle nothing else comes near; one triangle at index 3 and again, its corners rotated, at
    TT and 2 TT.  The triangle is one whose inverse has the same bits from all three rotations (the determinant's sum is taken in
    another order in each), so the three entries tie exactly and the first must win."""
    from open_headstage_amd import lookup, lookup3
    TT, _ = _sizes(_lookup(OCTA_XYZ, OCTA_TRI))
    pos, mesh = lookup3.octahedron_mesh(5)              # 2 048 triangles: enough for any tile up to 1 023
    xyz = lookup.table_xyz(pos)
    assert len(mesh) >= 2 * TT + 1
    inv = [l3.inverses(xyz, np.roll(mesh, r, axis=1))[0] for r in range(3)]
    exact = np.flatnonzero((inv[1] == np.roll(inv[0], 1, axis=1)).all((1, 2)) & (inv[2] == np.roll(inv[0], 2, axis=1)).all((1, 2)))
    assert exact.size > 0
    j = int(exact[0])
    rest = np.delete(mesh, j, axis=0)[:2 * TT - 2]
    one = mesh[j:j + 1]
    tris = np.ascontiguousarray(np.concatenate([rest[:3], one, rest[3:TT - 1], np.roll(one, 1, axis=1), rest[TT - 1:], np.roll(one, 2, axis=1)]))
    assert len(tris) == 2 * TT + 1 and all(set(tris[i]) == set(one[0]) for i in (3, TT, 2 * TT))
    lk = _lookup(xyz, tris)
    rng = np.random.default_rng(5)
    P = xyz[one[0]].astype(np.float64)
    q = (rng.dirichlet([2.0, 2.0, 2.0], 200) @ P) * rng.choice([0.5, 1.0, 3.0], (200, 1))
    got = lk.points(q, return_triangle=True)
    m = assert_model_bits(xyz, tris, q, got, "copies across tiles")
    assert (m["m_next"] == m["m_best"]).all() and (m["m_best"] > 0).all()       # the model: a tie inside the triangle
    assert (got[5] == 3).all()
    alone = _lookup(xyz, np.ascontiguousarray(tris[:TT]))
    assert l3.same_rows(alone.points(q), m).all()                               # the same five rows as without the copies


def test_the_full_size_mesh():
    """131 072 triangles: the octahedron's eight, over and over -- every query ties 16 384 times and the first eight must win"""
    T = 131072
    tris = np.ascontiguousarray(np.tile(OCTA_TRI, (T // 8, 1)))
    lk = _lookup(OCTA_XYZ, tris)
    assert lk.mesh() == (6, T)
    rng = np.random.default_rng(64)
    q = rng.standard_normal((64, 3))
    got = lk.points(q, return_triangle=True)
    assert (got[5] < 8).all() and len(set(got[5])) == 8
    small = l3.lookup3(OCTA_XYZ, OCTA_TRI, q)
    assert l3.same_rows(got[:5], small).all() and (got[5] == small["tri"]).all()
    assert_model_bits(OCTA_XYZ, tris, q[:16], [g[:16] for g in got], "T = 131072")


def test_the_largest_table():
    """65 536 rows, and the 258 points of a closed mesh of 512 triangles scattered over them, rows 0 and 65 535 among them"""
    from open_headstage_amd import lookup, lookup3
    pos, mesh = lookup3.octahedron_mesh(3)
    rng = np.random.default_rng(65536)
    xyz = rng.standard_normal((65536, 3)).astype(np.float32)
    at = np.concatenate([[0, 65535], 1 + rng.choice(65534, len(pos) - 2, replace=False)]).astype(np.uint32)
    xyz[at] = lookup.table_xyz(pos)
    tris = np.ascontiguousarray(at[mesh])
    lk = _lookup(xyz, tris)
    assert lk.mesh() == (65536, 512)
    q = np.concatenate([l3.soup_queries(xyz, tris, 500, seed=6), xyz[[0, 65535]].astype(np.float64)])
    got = lk.points(q, return_triangle=True)
    assert_model_bits(xyz, tris, q, got, "M = 65536")
    assert got[0][-2] == 0 and got[0][-1] == 65535 and len(set(got[0] // 4096)) > 10


# ---- rows ----------------------------------------------------------------------------------------------------------------------------
def _rows_inputs(S, segs, K, src_shape, pose_shape, seed):
    rng = np.random.default_rng(seed)
    dims = {"K": (K,), "SK": (S, K), "gK": (segs, K), "SgK": (S, segs, K)}[src_shape]
    pdims = {"g": (segs,), "Sg": (S, segs)}[pose_shape]
    az, el = rng.uniform(-180, 180, dims).astype(np.float32), rng.uniform(-80, 80, dims).astype(np.float32)
    yaw, pitch, roll = (rng.uniform(-r, r, pdims).astype(np.float32) for r in (180, 40, 30))
    return az, el, yaw, pitch, roll


@pytest.mark.parametrize("K", [1, 6, 64])
@pytest.mark.parametrize("src_shape,pose_shape", [("K", "g"), ("SK", "g"), ("gK", "g"), ("gK", "Sg"), ("SgK", "Sg"), ("K", "Sg"), ("SK", "Sg"),
                                                  ("SgK", "g")])
def test_rows(K, src_shape, pose_shape):
    from open_headstage_amd import lookup
    S, segs = 3, 5
    xyz, tris = l3.random_soup(40, 130, seed=13)
    lk = _lookup(xyz, tris)
    az, el, yaw, pitch, roll = _rows_inputs(S, segs, K, src_shape, pose_shape, seed=K)
    v, sss, sks, R, rss, S_, segs_, K_ = lookup.rows_host_half(az, el, yaw, pitch, roll, 1.5)
    S_want = S if ("S" in src_shape or "S" in pose_shape) else 1
    assert (S_, segs_, K_) == (S_want, segs, K)
    q = l3.rows_queries(v, sss, sks, R, rss, S_, segs, K).reshape(-1, 3)
    got = lk.rows(az, el, yaw, pitch, roll, 1.5, return_triangle=True)
    assert len(got) == 6 and all(g.shape == (S_, segs, K) for g in got)
    assert [g.dtype for g in got] == [np.uint32] * 3 + [np.float32] * 2 + [np.uint32]
    m = assert_model_bits(xyz, tris, q, got, f"rows {src_shape} {pose_shape} K = {K}")
    five = lk.rows(az, el, yaw, pitch, roll, 1.5)
    assert len(five) == 5 and l3.same_rows(five, m).all()
    # rot == NULL: q = v
    n = S_ * segs * K
    out = c_arrays(n)
    assert c_rows(lk, S_, segs, K, v, sss, sks, None, 0, out) == 0
    assert_model_bits(xyz, tris, l3.rows_queries(v, sss, sks, None, 0, S_, segs, K).reshape(-1, 3), [a[:n] for a in out], "rot NULL")
    assert untouched(out, n)


def test_rows_with_wide_strides_never_read_the_gaps():
    S, segs, K = 3, 5, 6
    xyz, tris = l3.random_soup(40, 130, seed=14)
    lk = _lookup(xyz, tris)
    rng = np.random.default_rng(15)
    src = np.full((S, 7, 2, K, 3), np.nan)          # stream stride 14, segment stride 2
    src[:, :segs, 0] = rng.standard_normal((S, segs, K, 3))
    rot = np.full((S, 8, 3, 3), np.inf)             # stream stride 8
    rot[:, :segs] = np.linalg.qr(rng.standard_normal((S, segs, 3, 3)))[0]
    n = S * segs * K
    out = c_arrays(n)
    assert c_rows(lk, S, segs, K, src, 14, 2, rot, 8, out) == 0
    q = l3.pose(rot[:, :segs, None], src[:, :segs, 0]).reshape(-1, 3)
    assert_model_bits(xyz, tris, q, [a[:n] for a in out], "wide strides")
    # shared both ways: one set of sources for every stream and segment (both strides 0), a pose per segment (stride 0)
    out = c_arrays(n)
    assert c_rows(lk, S, segs, K, src[0, 0, 0], 0, 0, rot[1], 0, out) == 0
    q = l3.pose(rot[1, :segs, None], np.broadcast_to(src[0, 0, 0], (S, segs, K, 3))).reshape(-1, 3)
    assert_model_bits(xyz, tris, q, [a[:n] for a in out], "strides of 0")


def test_rows_of_more_than_a_chunk():
    """sources per stream, poses per segment, shared the other way: the parts of both that a chunk stages change from chunk to chunk"""
    from open_headstage_amd import lookup
    lk = _lookup(OCTA_XYZ, OCTA_TRI)
    _, Q = _sizes(lk)
    K, segs = 6, 500
    S = Q // (K * segs) + 2
    az, el, yaw, pitch, roll = _rows_inputs(S, segs, K, "SK", "g", seed=77)
    v, sss, sks, R, rss, S_, _, _ = lookup.rows_host_half(az, el, yaw, pitch, roll)
    got = lk.rows(az, el, yaw, pitch, roll, return_triangle=True)
    assert lk.last_launch()[2] == 2 and S_ == S
    assert_model_bits(OCTA_XYZ, OCTA_TRI, l3.rows_queries(v, sss, sks, R, rss, S, segs, K).reshape(-1, 3), got, "two chunks of rows")
    # and everything per stream and segment
    az, el, yaw, pitch, roll = _rows_inputs(S, segs, K, "SgK", "Sg", seed=78)
    v, sss, sks, R, rss, _, _, _ = lookup.rows_host_half(az, el, yaw, pitch, roll)
    got = lk.rows(az, el, yaw, pitch, roll, return_triangle=True)
    assert_model_bits(OCTA_XYZ, OCTA_TRI, l3.rows_queries(v, sss, sks, R, rss, S, segs, K).reshape(-1, 3), got, "two chunks, all per stream")


# ---- the Python surface against the helper -----------------------------------------------------------------------------------------
def test_triangle_against_the_helper():
    from open_headstage_amd import TriangleLookup, lookup3, scene3
    from tests.test_cpu_lookup3 import mesh_queries
    from tests.test_cpu_scene_blend3 import grid_mesh
    for pos, tri in (grid_mesh(), lookup3.octahedron_mesh(3)):
        az, el = mesh_queries(pos, tri, 1000, seed=len(tri) + 1)
        az, el = az[:len(az) // 4 * 4].reshape(4, -1), el[:len(el) // 4 * 4].reshape(4, -1)
        lk = TriangleLookup(pos, tri)
        assert lk.mesh() == (len(pos), len(tri))
        for radius in (1.0, 1.75):
            got = lk.triangle(az, el, radius)
            want = scene3.triangle_directions(pos, tri, az, el, radius)
            assert all(g.shape == az.shape and g.dtype == w.dtype for g, w in zip(got, want))
            for g, w in zip(got, want):
                assert (np.ascontiguousarray(g).view(np.uint32) == np.ascontiguousarray(w).view(np.uint32)).all()
        assert (got[4] > 0).sum() > 500 and (l3.bits(got[3]) == 0).sum() >= 60


def test_rows_into_a_three_direction_scene_call():
    """S = 3, K = 5, 4 segments: TriSceneProcessor.process on TriangleLookup.rows' output against the same call on
    triangle_directions' rows for the same head-relative directions, bit for bit"""
    import torch

    import open_headstage_amd as ohs
    from open_headstage_amd import lookup3
    from tests.test_cpu_layout import make_input, make_layout
    S, K, blocks, seg = 3, 5, 4, 1
    pos, tri = lookup3.octahedron_mesh(2)
    n_dirs = len(pos)
    rng = np.random.default_rng(66)
    src_az, src_el = rng.uniform(-180, 180, (blocks, K)).astype(np.float32), rng.uniform(-60, 60, (blocks, K)).astype(np.float32)
    src_az[0, 0], src_el[0, 0] = 0.0, 0.0
    yaw, pitch, roll = (rng.uniform(-r, r, (S, blocks, 1)).astype(np.float32) for r in (180, 30, 20))
    yaw[0, 0], pitch[0, 0], roll[0, 0] = 90.0, 0.0, 0.0
    az, el = ohs.rotate_sources(src_az[None], src_el[None], yaw, pitch, roll)            # [S][blocks][K], seen from each head
    want = ohs.triangle_directions(pos, tri, -az, el)
    lk = ohs.TriangleLookup(pos, tri)
    got = lk.rows(az, el, np.zeros(blocks, np.float32))
    for g, w in zip(got, want):
        assert g.shape == (S, blocks, K) and (np.ascontiguousarray(g).view(np.uint32) == np.ascontiguousarray(w).view(np.uint32)).all()
    assert (got[4] > 0).sum() > 0 and len(set(got[0].reshape(-1))) > 8
    dirs = make_layout(n_dirs, 512)
    x = torch.from_numpy(make_input(S, K, blocks, seed=660)).cuda()
    outs, launches = [], []
    for i0, i1, i2, w1, w2 in (got, want):
        sc = ohs.TriSceneProcessor(S, num_bands=10)
        sc.set_directions(dirs)
        y = sc.process(x, i0, seg, idx1=i1, weights=w1, idx2=i2, weights2=w2)
        torch.cuda.synchronize()
        outs.append(y.cpu().numpy())
        launches.append(sc.last_launch())
        assert sc.last_launch()[4] > 0
    assert launches[0] == launches[1]
    assert np.abs(outs[0]).max() > 0 and (outs[0].view(np.uint32) == outs[1].view(np.uint32)).all()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_create_refuses_a_bad_mesh_on_the_device():
    from open_headstage_amd import TriangleLookupError, lookup, lookup3
    for xyz, tris, text in ((OCTA_XYZ, np.array([[0, 1, 6]], np.uint32), "names direction 6 of 6"),
                            (OCTA_XYZ, np.concatenate([OCTA_TRI, [[0, 2, 1]]]).astype(np.uint32), "triangle 8 (0, 2, 1) is singular"),
                            (np.where(np.arange(18).reshape(6, 3) == 4, np.float32(np.nan), OCTA_XYZ), OCTA_TRI, "xyz[4] is not finite")):
        h = C.c_void_p(1)
        xyz = np.ascontiguousarray(xyz, np.float32)
        st = lookup3.lookup3_lib().ohs_lookup3_create(0, len(xyz), xyz.ctypes.data_as(lookup.fp), len(tris), tris.ctypes.data_as(lookup.u32p), C.byref(h))
        assert st == INV and not h.value and text.encode() in lookup3.lookup3_lib().ohs_lookup3_last_error(), text
    with pytest.raises(TriangleLookupError, match="singular"):
        _lookup(OCTA_XYZ, np.array([[0, 2, 4]], np.uint32))


def test_refusals_leave_the_outputs_and_the_handle():
    from open_headstage_amd import TriangleLookupError, lookup3
    xyz, tris = l3.random_soup(40, 130, seed=21)
    lk = _lookup(xyz, tris)
    L = lookup3.lookup3_lib()
    q = l3.soup_queries(xyz, tris, 60, seed=22)[:40]
    assert_model_bits(xyz, tris, q, lk.points(q, return_triangle=True))
    before = lk.last_launch()
    bad = q.copy()
    bad[33, 1] = np.nan
    out = c_arrays(40)
    assert c_points(lk, bad, out) == INV and untouched(out)
    assert b"finite" in L.ohs_lookup3_last_error()
    for v in (np.inf, 2e15, -1.0000001e15):
        bad[33, 1] = v
        assert c_points(lk, bad, out) == INV and untouched(out), v
    for j in range(5):                                  # each of the five required outputs
        assert c_points(lk, q, out[:j] + [None] + out[j + 1:]) == INV and untouched(out), j
        assert b"NULL" in L.ohs_lookup3_last_error()
    assert c_points(lk, None, out) == INV and untouched(out)
    S, segs, K = 3, 5, 6
    rng = np.random.default_rng(23)
    src = rng.standard_normal((S, segs, K, 3))
    rot = np.linalg.qr(rng.standard_normal((S, segs, 3, 3)))[0]
    n = S * segs * K
    out = c_arrays(n)
    rot_bad = rot.copy()
    rot_bad[2, 4, 1, 1] = np.inf
    assert c_rows(lk, S, segs, K, src, segs, 1, rot_bad, segs, out) == INV and untouched(out)
    rot_bad[2, 4, 1, 1] = 1.1e15
    assert c_rows(lk, S, segs, K, src, segs, 1, rot_bad, segs, out) == INV and untouched(out)
    src_bad = src.copy()
    src_bad[2, 4, 5, 2] = -np.inf
    assert c_rows(lk, S, segs, K, src_bad, segs, 1, rot, segs, out) == INV and untouched(out)
    src_bad[2, 4, 5, 2] = -1.1e15                       # (the last element of the last chunk: checked before the first runs)
    assert c_rows(lk, S, segs, K, src_bad, segs, 1, rot, segs, out) == INV and untouched(out)
    assert c_rows(lk, S, segs, K, src, segs - 1, 1, rot, segs, out) == INV and untouched(out)       # a short stride
    assert b"stride" in L.ohs_lookup3_last_error()
    assert c_rows(lk, S, segs, K, src, segs, 1, rot, segs - 1, out) == INV and untouched(out)
    assert c_rows(lk, S, segs, 0, src, segs, 1, rot, segs, out) == INV and untouched(out)
    assert c_rows(lk, S, segs, 65, src, segs, 1, rot, segs, out) == INV and untouched(out)
    assert c_rows(lk, S, segs, K, None, segs, 1, rot, segs, out) == INV and untouched(out)
    for j in range(5):
        assert c_rows(lk, S, segs, K, src, segs, 1, rot, segs, out[:j] + [None] + out[j + 1:]) == INV and untouched(out), j
    assert c_rows(lk, 0, segs, K, src, segs, 1, rot, segs, out) == 0 and untouched(out)
    with pytest.raises(TriangleLookupError) as e:
        lk.points(bad)
    assert e.value.status == INV
    # 1e15 itself is taken: the f32 rounding of the posed query stays finite
    big = src.copy()
    big[0, 0, 0] = (1e15, -1e15, 1e15)
    assert c_rows(lk, S, segs, K, big, segs, 1, rot, segs, out) == 0
    assert_model_bits(xyz, tris, l3.pose(rot[:, :, None], big).reshape(-1, 3), [a[:n] for a in out], "a source at the limit")
    # the handle is as it was: the record of the last launch, and the next valid calls
    assert c_points(lk, bad, c_arrays(40)) == INV and lk.last_launch()[:2] == before[:2]
    assert_model_bits(xyz, tris, q, lk.points(q, return_triangle=True), "after the refusals")
    assert lk.last_launch() == before
    out = c_arrays(n)
    assert c_rows(lk, S, segs, K, src, segs, 1, rot, segs, out) == 0 and untouched(out, n)
    assert_model_bits(xyz, tris, l3.pose(rot[:, :, None], src).reshape(-1, 3), [a[:n] for a in out], "rows after the refusals")

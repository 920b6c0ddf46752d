"""libohs_lookup3p.so on the device (k_lookup_tri_cells, k_lookup_tri_rest) against tests/lookup3_model.py and tests/lookup3p_model.py:
every query, bit for bit -- idx0, idx1, idx2, w1, w2 and the winning triangle's index are the unpruned walk's -- and the number of
queries pass 2 answered is the number the model predicts from the mesh and the queries alone, at every grid.

The meshes and the query mix are tests/test_cpu_lookup3p.py's (closed, open, overlapping soups, every triangle twice, a needle; random
directions, measurements, edge midpoints, centroids, the origin, the cube map's seams, -0.0, radii from an f32 subnormal to 1e15).  Q is
the chunk of queries, read from ohs_lookup3p_last_launch."""
import ctypes as C

import numpy as np
import pytest

from tests import lookup3_model as l3
from tests import lookup3p_model as l3p
from tests.test_cpu_lookup3p import meshes, mixed_queries, seam_queries
from tests.test_gpu_lookup3 import OCTA_TRI, OCTA_XYZ, _rows_inputs, c_arrays, untouched

pytestmark = pytest.mark.gpu

INV = 1
GRIDS = (1, 3, 16, 0)


def _lookup(xyz, tris, grid=0):
    import open_headstage_amd as ohs
    return ohs.PrunedTriangleLookup(None, tris, xyz=xyz, grid=grid)


def _ptrs(arrays):
    from open_headstage_amd import lookup3
    return [None if a is None else a.ctypes.data_as(t) for a, t in zip(arrays, lookup3._OUT)]


def c_points(lk, q, arrays):
    from open_headstage_amd import lookup, lookup3p
    q = None if q is None else np.ascontiguousarray(q, np.float64)
    n = 1 if q is None else q.size // 3
    return lookup3p.lookup3p_lib().ohs_lookup3p_points(lk._h, n, None if q is None else q.ctypes.data_as(lookup.dp), *_ptrs(arrays))


def c_rows(lk, S, segs, K, src, sss, sks, rot, rss, arrays):
    from open_headstage_amd import lookup, lookup3p
    p = lambda a: None if a is None else a.ctypes.data_as(lookup.dp)      # noqa: E731
    return lookup3p.lookup3p_lib().ohs_lookup3p_rows(lk._h, S, segs, K, p(src), sss, sks, p(rot), rss, *_ptrs(arrays))


def assert_bits(m, rest, got, what=""):
    """got: (idx0, idx1, idx2, w1, w2, tri) against the model's rows m"""
    got = [np.asarray(g).reshape(-1) for g in got]
    bad = np.flatnonzero(~l3.same_rows(got[:5], m) | (got[5] != m["tri"]))
    assert bad.size == 0, (what, bad[:8], rest[bad[:8]], [g[bad[:8]] for g in got], [m[k][bad[:8]] for k in l3.FIELDS + ("tri",)])
    assert (l3.bits(got[3]) != 0x80000000).all() and (l3.bits(got[4]) != 0x80000000).all(), what      # (a zero is +0.0)


def assert_model(lk, xyz, tris, q, got, what="", model=None):
    """the rows against the model, and the call's fallback count against the model's; -> (m, rest)"""
    q = np.asarray(q).reshape(-1, 3)
    m = l3.lookup3(xyz, tris, q) if model is None else model
    rest = l3p.falls_back(xyz, tris, q, m)
    assert_bits(m, rest, got, what)
    assert lk.last_launch()[2] == int(rest.sum()), (what, lk.last_launch(), int(rest.sum()))
    return m, rest


# ---- the CPU list's meshes at four grids: one set of queries and one model per mesh ---------------------------------------------------
@pytest.fixture(scope="module")
def mesh_models():
    out = {}
    for name, (xyz, tris) in meshes().items():
        q = np.concatenate([l3.soup_queries(xyz, tris, 300, seed=len(tris))] + [seam_queries(G, seed=G) for G in (1, 3, 16, l3p.choose_grid(len(tris)))])
        out[name] = (xyz, tris, q, l3.lookup3(xyz, tris, q))
    return out


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name", ["octahedron0", "octahedron1", "octahedron3", "octahedron5", "open_grid", "soup40", "soup12", "twice", "needle"])
def test_meshes_at_every_grid(mesh_models, name, grid):
    xyz, tris, q, m = mesh_models[name]
    lk = _lookup(xyz, tris, grid)
    G, cells, entries, longest, everywhere = lk.index()
    assert G == (grid or l3p.choose_grid(len(tris))) and cells == 6 * G * G and lk.mesh() == (len(xyz), len(tris))
    assert entries <= 64 * len(tris) and longest <= len(tris) and everywhere <= len(tris) and (entries > 0 or everywhere == len(tris))
    _, rest = assert_model(lk, xyz, tris, q, lk.points(q, return_triangle=True), f"{name} at grid {grid}", m)
    assert 0 < rest.sum() < len(q)
    five = lk.points(q)
    assert len(five) == 5 and l3.same_rows(five, m).all()
    if name == "twice":
        assert (m["tri"] % 2 == 0).all()            # the lower of the two copies, in pass 1 and in pass 2 alike
    if name in ("soup40", "soup12") and grid == 1:
        assert 0.25 * len(tris) < everywhere < 0.75 * len(tris)


# ---- query counts around the wave, the workgroup and the chunk ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_query_counts(n):
    xyz, tris = meshes()["octahedron3"]
    lk = _lookup(xyz, tris)
    q = mixed_queries(xyz, tris, 0, 300, seed=n)[:n] if n > 1 else xyz[:1].astype(np.float64)        # (n = 1: a measurement, for pass 2)
    out = c_arrays(n)
    assert c_points(lk, q, out) == 0
    assert_model(lk, xyz, tris, q, [a[:n] for a in out], f"n = {n}")
    assert untouched(out, n) and lk.last_launch()[1] == 1
    out = c_arrays(n)
    assert c_points(lk, q, out[:5] + [None]) == 0           # tri == NULL: the five others are written all the same
    assert l3.same_rows([a[:n] for a in out[:5]], l3.lookup3(xyz, tris, q)).all() and untouched(out[:5], n) and untouched(out[5:])


def test_one_query_more_than_a_chunk():
    """2^18 + 1 queries over the level-2 mesh of 128 triangles: 8 191 distinct queries repeated (the model is computed once per distinct
    query), so that every workgroup of both chunks sees certified and uncertified lanes at shifting places"""
    from open_headstage_amd import lookup, lookup3
    pos, tris = lookup3.octahedron_mesh(2)
    xyz = lookup.table_xyz(pos)
    assert len(tris) == 128
    lk = _lookup(xyz, tris)
    Q = lk.last_launch()[0]
    assert Q == 1 << 18 and lk.last_launch()[1:] == (0, 0)
    base = mixed_queries(xyz, tris, 0, 12000, seed=18)[:8191]
    assert len(base) == 8191
    mb = l3.lookup3(xyz, tris, base)
    n = Q + 1
    at = np.arange(n) % len(base)
    q = np.ascontiguousarray(base[at])
    m = {k: v[at] for k, v in mb.items()}
    out = c_arrays(n)
    assert c_points(lk, q, out) == 0
    assert lk.last_launch()[:2] == (Q, 2)
    _, rest = assert_model(lk, xyz, tris, q, [a[:n] for a in out], "Q + 1 queries", m)
    assert untouched(out, n) and 1000 < rest.sum() < n - 1000
    # the buffers have grown to a chunk: a small call behind it is right, and an empty one touches nothing
    assert_model(lk, xyz, tris, q[:7], lk.points(q[:7], return_triangle=True), "a small call behind a large one")
    assert c_points(lk, np.zeros((0, 3)), [None] * 6) == 0 and lk.last_launch() == (Q, 0, 0)


# ---- who answers: pass 1, pass 2, and both within a wave ---------------------------------------------------------------------------
def test_all_fall_back_none_fall_back_and_alternating():
    xyz, tris = meshes()["octahedron3"]
    lk = _lookup(xyz, tris)
    rng = np.random.default_rng(3)
    P = xyz.astype(np.float64)
    n = 1000
    t = tris[rng.integers(0, len(tris), n)].astype(np.int64)
    cen = ((P[t[:, 0]] + P[t[:, 1]]) + P[t[:, 2]]) / 3
    on = P[rng.integers(0, len(P), n)]
    _, rest = assert_model(lk, xyz, tris, on, lk.points(on, return_triangle=True), "every query on a measurement")
    assert rest.all() and lk.last_launch()[2] == n
    _, rest = assert_model(lk, xyz, tris, cen, lk.points(cen, return_triangle=True), "centroids only")
    assert not rest.any() and lk.last_launch()[2] == 0
    lane = np.where((np.arange(n) % 2 == 0)[:, None], on, cen)
    _, rest = assert_model(lk, xyz, tris, lane, lk.points(lane, return_triangle=True), "alternating lane by lane")
    assert (rest == (np.arange(n) % 2 == 0)).all()
    wave = np.where(((np.arange(n) // 64) % 2 == 0)[:, None], on, cen)
    _, rest = assert_model(lk, xyz, tris, wave, lk.points(wave, return_triangle=True), "alternating wave by wave")
    assert (rest == ((np.arange(n) // 64) % 2 == 0)).all()


def test_a_triangle_stored_again_beyond_pass_2s_tile():
    """a closed mesh of 2 048 triangles with the triangle at index 3 stored again, bit for bit, at 3 + 256 and 3 + 512: inside it
    pass 1 meets all three on the cell's list, on its corners and edges pass 2 meets them in three tiles; the lowest index wins"""
    from open_headstage_amd import lookup, lookup3
    pos, mesh = lookup3.octahedron_mesh(4)
    xyz = lookup.table_xyz(pos)
    tris = mesh.copy()
    tris[3 + 256], tris[3 + 512] = tris[3], tris[3]
    lk = _lookup(xyz, tris)
    rng = np.random.default_rng(5)
    P = xyz[tris[3]].astype(np.float64)
    inside = (rng.dirichlet([2.0, 2.0, 2.0], 200) @ P) * rng.choice([0.5, 1.0, 3.0], (200, 1))
    edge = np.concatenate([P, (P + np.roll(P, 1, axis=0)) / 2, 2.0 * P])
    q = np.concatenate([inside, edge])
    got = lk.points(q, return_triangle=True)
    m, rest = assert_model(lk, xyz, tris, q, got, "copies at + 256 and + 512")
    assert (m["m_next"][:200] == m["m_best"][:200]).all() and not rest[:200].any() and (got[5][:200] == 3).all()
    assert rest[200:].sum() >= 6 and not np.isin(got[5], [3 + 256, 3 + 512]).any()


# ---- the limits ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def level6():
    from open_headstage_amd import lookup, lookup3
    pos, tris = lookup3.octahedron_mesh(6)
    assert pos.shape == (16386, 3) and tris.shape == (32768, 3)
    return lookup.table_xyz(pos), tris


def test_the_full_size_mesh(level6):
    """131 072 triangles: the level-6 mesh stored four times, 257 queries.  The first copy holds the lowest indices, the inverses and
    so B are the one mesh's: the answers are the one mesh's model's; the model over all 131 072 is held on the first 32 queries."""
    xyz, one = level6
    tris = np.ascontiguousarray(np.tile(one, (4, 1)))
    lk = _lookup(xyz, tris)
    assert lk.mesh() == (16386, 131072) and lk.index()[0] == 148
    q = mixed_queries(xyz, one, 1, 400, seed=66)[:257]
    got = lk.points(q, return_triangle=True)
    m = l3.lookup3(xyz, one, q)
    _, rest = assert_model(lk, xyz, one, q, got, "T = 131072 against the one mesh", m)
    assert 0 < rest.sum() < 257 and (got[5] < 32768).all()
    full = l3.lookup3(xyz, tris, q[:32])
    assert l3.same_rows([g[:32] for g in got[:5]], full).all() and (got[5][:32] == full["tri"]).all()
    assert (l3p.falls_back(xyz, tris, q[:32], full) == rest[:32]).all()


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
    q = np.concatenate([mixed_queries(xyz, tris, 0, 500, seed=6), xyz[[0, 65535]].astype(np.float64)])
    got = lk.points(q, return_triangle=True)
    assert_model(lk, xyz, tris, q, got, "M = 65536")
    assert got[0][-2] == 0 and got[0][-1] == 65535 and len(set(got[0] // 4096)) > 10


def test_device_against_device_on_the_level_6_mesh(level6):
    """4 096 mixed queries over 32 768 triangles: libohs_lookup3p.so against libohs_lookup3.so on the same inputs"""
    import open_headstage_amd as ohs
    xyz, tris = level6
    q = mixed_queries(xyz, tris, 0, 6000, seed=4096)[:4096]
    assert len(q) == 4096
    brute = ohs.TriangleLookup(None, tris, xyz=xyz).points(q, return_triangle=True)
    lk = _lookup(xyz, tris)
    got = lk.points(q, return_triangle=True)
    for name, g, b in zip(l3.FIELDS + ("tri",), got, brute):
        assert (np.ascontiguousarray(g).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all(), name
    G, cells, entries, longest, everywhere = lk.index()
    print(f"level 6: G = {G}, {entries} entries, longest list {longest}, everywhere {everywhere}; {lk.last_launch()[2]} of 4096 to pass 2")
    assert G == 74 and everywhere == 0 and 0 < lk.last_launch()[2] < 2048


# ---- rows --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows_mesh():
    xyz, tris = l3.random_soup(40, 130, seed=13)
    return xyz, tris, _lookup(xyz, tris)


@pytest.mark.parametrize("K", [1, 6, 64])
@pytest.mark.parametrize("src_shape,pose_shape", [("K", "g"), ("SK", "g"), ("gK", "g"), ("gK", "Sg"), ("SgK", "Sg"), ("K", "Sg"), ("SK", "Sg"),
                                                  ("SgK", "g")])
def test_rows(rows_mesh, K, src_shape, pose_shape):
    from open_headstage_amd import lookup
    S, segs = 3, 5
    xyz, tris, lk = rows_mesh
    az, el, yaw, pitch, roll = _rows_inputs(S, segs, K, src_shape, pose_shape, seed=K)
    v, sss, sks, R, rss, S_, segs_, K_ = lookup.rows_host_half(az, el, yaw, pitch, roll, 1.5)
    assert (S_, segs_, K_) == (S if ("S" in src_shape or "S" in pose_shape) else 1, segs, K)
    q = l3.rows_queries(v, sss, sks, R, rss, S_, segs, K).reshape(-1, 3)
    got = lk.rows(az, el, yaw, pitch, roll, 1.5, return_triangle=True)
    assert len(got) == 6 and all(g.shape == (S_, segs, K) for g in got)
    assert [g.dtype for g in got] == [np.uint32] * 3 + [np.float32] * 2 + [np.uint32]
    m, _ = assert_model(lk, xyz, tris, q, got, f"rows {src_shape} {pose_shape} K = {K}")
    five = lk.rows(az, el, yaw, pitch, roll, 1.5)
    assert len(five) == 5 and l3.same_rows(five, m).all()
    # rot == NULL: q = v
    n = S_ * segs * K
    out = c_arrays(n)
    assert c_rows(lk, S_, segs, K, v, sss, sks, None, 0, out) == 0
    assert_model(lk, xyz, tris, l3.rows_queries(v, sss, sks, None, 0, S_, segs, K).reshape(-1, 3), [a[:n] for a in out], "rot NULL")
    assert untouched(out, n)


def test_rows_on_a_closed_mesh_with_sources_on_measurements():
    """the level-3 mesh, K = 6: half the sources on measurements with identity poses (pass 2), half anywhere under real poses"""
    xyz, tris = meshes()["octahedron3"]
    lk = _lookup(xyz, tris)
    S, segs, K = 4, 5, 6
    rng = np.random.default_rng(36)
    src = rng.standard_normal((S, segs, K, 3))
    src[::2] = xyz[rng.integers(0, len(xyz), (S // 2, segs, K))]
    rot = np.linalg.qr(rng.standard_normal((S, segs, 3, 3)))[0]
    rot[::2] = np.eye(3)
    n = S * segs * K
    out = c_arrays(n)
    assert c_rows(lk, S, segs, K, src, segs, 1, rot, segs, out) == 0
    _, rest = assert_model(lk, xyz, tris, l3.pose(rot[:, :, None], src).reshape(-1, 3), [a[:n] for a in out], "rows, half on measurements")
    assert rest.reshape(S, -1)[::2].all() and not rest.reshape(S, -1)[1::2].any() and untouched(out, n)


def test_rows_with_wide_strides_never_read_the_gaps(rows_mesh):
    S, segs, K = 3, 5, 6
    xyz, tris, lk = rows_mesh
    rng = np.random.default_rng(15)
    src = np.full((S, 7, 2, K, 3), np.nan)          # stream stride 14, segment stride 2
    src[:, :segs, 0] = rng.standard_normal((S, segs, K, 3))
    rot = np.full((S, 8, 3, 3), np.inf)             # stream stride 8
    rot[:, :segs] = np.linalg.qr(rng.standard_normal((S, segs, 3, 3)))[0]
    n = S * segs * K
    out = c_arrays(n)
    assert c_rows(lk, S, segs, K, src, 14, 2, rot, 8, out) == 0
    q = l3.pose(rot[:, :segs, None], src[:, :segs, 0]).reshape(-1, 3)
    assert_model(lk, xyz, tris, q, [a[:n] for a in out], "wide strides")
    # shared both ways: one set of sources for every stream and segment (both strides 0), a pose per segment (stride 0)
    out = c_arrays(n)
    assert c_rows(lk, S, segs, K, src[0, 0, 0], 0, 0, rot[1], 0, out) == 0
    q = l3.pose(rot[1, :segs, None], np.broadcast_to(src[0, 0, 0], (S, segs, K, 3))).reshape(-1, 3)
    assert_model(lk, xyz, tris, q, [a[:n] for a in out], "strides of 0")
    assert untouched(out, n)


def test_rows_into_a_three_direction_scene_call():
    """S = 3, K = 5, 4 segments: TriSceneProcessor.process on PrunedTriangleLookup.rows' output against the same call on
    TriangleLookup.rows' output: the same rows, the same output bits, the same launch record"""
    import torch

    import open_headstage_amd as ohs
    from open_headstage_amd import lookup3
    from tests.test_cpu_layout import make_input, make_layout
    S, K, blocks, seg = 3, 5, 4, 1
    pos, tri = lookup3.octahedron_mesh(2)
    rng = np.random.default_rng(66)
    src_az, src_el = rng.uniform(-180, 180, (blocks, K)).astype(np.float32), rng.uniform(-60, 60, (blocks, K)).astype(np.float32)
    src_az[0, 0], src_el[0, 0] = 0.0, 0.0
    yaw, pitch, roll = (rng.uniform(-r, r, (S, blocks)).astype(np.float32) for r in (180, 30, 20))
    yaw[0, 0], pitch[0, 0], roll[0, 0] = 90.0, 0.0, 0.0
    want = ohs.TriangleLookup(pos, tri).rows(src_az, src_el, yaw, pitch, roll)
    lk = ohs.PrunedTriangleLookup(pos, tri)
    got = lk.rows(src_az, src_el, yaw, pitch, roll)
    for g, w in zip(got, want):
        assert g.shape == (S, blocks, K) and (np.ascontiguousarray(g).view(np.uint32) == np.ascontiguousarray(w).view(np.uint32)).all()
    assert (got[4] > 0).sum() > 0 and len(set(got[0].reshape(-1))) > 8
    dirs = make_layout(len(pos), 512)
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
def test_create_refuses_a_bad_mesh_and_a_wide_grid_on_the_device():
    from open_headstage_amd import PrunedTriangleLookupError, lookup, lookup3p
    L = lookup3p.lookup3p_lib()
    for xyz, tris, grid, text in ((OCTA_XYZ, np.array([[0, 1, 6]], np.uint32), 0, "names direction 6 of 6"),
                                  (OCTA_XYZ, np.concatenate([OCTA_TRI, [[0, 2, 1]]]).astype(np.uint32), 0, "triangle 8 (0, 2, 1) is singular"),
                                  (np.where(np.arange(18).reshape(6, 3) == 4, np.float32(np.nan), OCTA_XYZ), OCTA_TRI, 0, "xyz[4] is not finite"),
                                  (OCTA_XYZ, OCTA_TRI, 257, "grid 257 is outside 0 .. 256")):
        h = C.c_void_p(1)
        xyz = np.ascontiguousarray(xyz, np.float32)
        st = L.ohs_lookup3p_create(0, len(xyz), xyz.ctypes.data_as(lookup.fp), len(tris), tris.ctypes.data_as(lookup.u32p), grid, C.byref(h))
        assert st == INV and not h.value and text.encode() in L.ohs_lookup3p_last_error(), text
    with pytest.raises(PrunedTriangleLookupError, match="singular"):
        _lookup(OCTA_XYZ, np.array([[0, 2, 4]], np.uint32))
    assert _lookup(OCTA_XYZ, OCTA_TRI, 256).index()[:2] == (256, 6 * 256 * 256)


def test_refusals_leave_the_outputs_and_the_handle(rows_mesh):
    from open_headstage_amd import PrunedTriangleLookupError, lookup3p
    xyz, tris, _ = rows_mesh
    lk = _lookup(xyz, tris, 3)
    L = lookup3p.lookup3p_lib()
    q = np.concatenate([l3.soup_queries(xyz, tris, 60, seed=22)[:39], np.zeros((1, 3))])
    assert_model(lk, xyz, tris, q, lk.points(q, return_triangle=True))
    before = lk.last_launch()
    assert before[1] == 1 and before[2] >= 1
    bad = q.copy()
    bad[33, 1] = np.nan
    out = c_arrays(40)
    assert c_points(lk, bad, out) == INV and untouched(out) and lk.last_launch() == before
    assert b"finite" in L.ohs_lookup3p_last_error()
    for v in (np.inf, 2e15, -1.0000001e15):
        bad[33, 1] = v
        assert c_points(lk, bad, out) == INV and untouched(out), v
    for j in range(5):                                  # each of the five required outputs
        assert c_points(lk, q, out[:j] + [None] + out[j + 1:]) == INV and untouched(out), j
        assert b"NULL" in L.ohs_lookup3p_last_error()
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
    assert b"stride" in L.ohs_lookup3p_last_error()
    assert c_rows(lk, S, segs, K, src, segs, 1, rot, segs - 1, out) == INV and untouched(out)
    assert c_rows(lk, S, segs, 0, src, segs, 1, rot, segs, out) == INV and untouched(out)
    assert c_rows(lk, S, segs, 65, src, segs, 1, rot, segs, out) == INV and untouched(out)
    assert c_rows(lk, S, segs, K, None, segs, 1, rot, segs, out) == INV and untouched(out)
    for j in range(5):
        assert c_rows(lk, S, segs, K, src, segs, 1, rot, segs, out[:j] + [None] + out[j + 1:]) == INV and untouched(out), j
    assert lk.last_launch() == before                   # unchanged by every refused call
    with pytest.raises(PrunedTriangleLookupError) as e:
        lk.points(bad)
    assert e.value.status == INV
    assert c_rows(lk, 0, segs, K, src, segs, 1, rot, segs, out) == 0 and untouched(out) and lk.last_launch() == (before[0], 0, 0)
    # 1e15 itself is taken: the f32 rounding of the posed query stays finite
    big = src.copy()
    big[0, 0, 0] = (1e15, -1e15, 1e15)
    assert c_rows(lk, S, segs, K, big, segs, 1, rot, segs, out) == 0
    assert_model(lk, xyz, tris, l3.pose(rot[:, :, None], big).reshape(-1, 3), [a[:n] for a in out], "a source at the limit")
    # the handle is as it was: the next valid calls, and their record
    assert_model(lk, xyz, tris, q, lk.points(q, return_triangle=True), "after the refusals")
    assert lk.last_launch() == before
    out = c_arrays(n)
    assert c_rows(lk, S, segs, K, src, segs, 1, rot, segs, out) == 0 and untouched(out, n)
    assert_model(lk, xyz, tris, l3.pose(rot[:, :, None], src).reshape(-1, 3), [a[:n] for a in out], "rows after the refusals")
    assert L.ohs_lookup3p_last_launch(lk._h, None, None, None) == INV and L.ohs_lookup3p_index(lk._h, None, None, None, None, None) == INV
    assert L.ohs_lookup3p_mesh(lk._h, None, None) == INV

"""libohs_lookup.so on the device (k_lookup) against tests/lookup_model.py: every query, bit for bit -- idx0, idx1 and w.

The model is include/ohs_lookup.h's arithmetic in elementwise numpy (tests/test_cpu_lookup.py ties it to the host helpers that define a
scene's rows).  T and Q below are the kernel's tile of table points and the chunk of queries, read from ohs_lookup_last_launch: the sizes
around them are where the walk over tiles and the cut into chunks can go wrong.  Tables are random points near the unit sphere unless a
test builds its own."""
import ctypes as C

import numpy as np
import pytest

from tests import lookup_model as lm

pytestmark = pytest.mark.gpu

SENT_U, SENT_F = np.uint32(0xDEADBEEF), np.float32(-7.25)
INV = 1


def unit_table(M, seed):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((M, 3))
    return (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)


def mixed_queries(xyz, n, seed):
    """n queries: random ones at several radii, some ON table points, some on chord midpoints"""
    rng = np.random.default_rng(seed)
    P = xyz.astype(np.float64)
    q = rng.standard_normal((n, 3)) * rng.choice([0.5, 1.0, 1.0, 3.0], (n, 1))
    on = rng.random(n) < 0.15
    q[on] = P[rng.integers(0, len(P), int(on.sum()))]
    mid = ~on & (rng.random(n) < 0.15)
    q[mid] = (P[rng.integers(0, len(P), int(mid.sum()))] + P[rng.integers(0, len(P), int(mid.sum()))]) / 2
    return q


def _lookup(xyz):
    import open_headstage_amd as ohs
    return ohs.DirectionLookup(None, xyz=xyz)


def _sizes(lk):
    T, Q, _ = lk.last_launch()
    assert T >= 66 and Q >= 66
    return T, Q


def assert_model_bits(xyz, q, got, blend, what="", model=None):
    """model: lm.lookup(xyz, q, blend) where the caller has it already (tests/test_gpu_lookup_chunks.py)"""
    m = lm.lookup(xyz, q, blend) if model is None else model
    if blend:
        i0, i1, w = (np.asarray(v).reshape(-1) for v in got)
        bad = np.flatnonzero((i0 != m["idx0"]) | (i1 != m["idx1"]) | (lm.bits(w) != lm.bits(m["w"])))
        assert bad.size == 0, (what, bad[:8], i0[bad[:8]], m["idx0"][bad[:8]], i1[bad[:8]], m["idx1"][bad[:8]], w[bad[:8]], m["w"][bad[:8]])
        assert (lm.bits(w) != 0x80000000).all(), what          # (a zero is +0.0)
    else:
        i0 = np.asarray(got).reshape(-1)
        bad = np.flatnonzero(i0 != m["idx0"])
        assert bad.size == 0, (what, bad[:8], i0[bad[:8]], m["idx0"][bad[:8]])
    return m


def c_arrays(n, extra=5):
    return np.full(n + extra, SENT_U), np.full(n + extra, SENT_U), np.full(n + extra, SENT_F)


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def c_points(lk, q, i0, i1, w):
    from open_headstage_amd import lookup
    q = np.ascontiguousarray(q, np.float64)
    return lookup.lookup_lib().ohs_lookup_points(lk._h, q.size // 3, _ptr(q, lookup.dp), _ptr(i0, lookup.u32p), _ptr(i1, lookup.u32p),
                                                 _ptr(w, lookup.fp))


def c_rows(lk, S, segs, K, src, sss, sks, rot, rss, i0, i1, w):
    from open_headstage_amd import lookup
    return lookup.lookup_lib().ohs_lookup_rows(lk._h, S, segs, K, _ptr(src, lookup.dp), sss, sks, _ptr(rot, lookup.dp), rss,
                                               _ptr(i0, lookup.u32p), _ptr(i1, lookup.u32p), _ptr(w, lookup.fp))


# ---- table sizes around the tile -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["1", "2", "63", "64", "65", "T-1", "T", "T+1", "2*T+1"])
def test_table_sizes(size):
    probe = _lookup(unit_table(1, 0))
    T, _ = _sizes(probe)
    M = eval(size, {"T": T})
    xyz = unit_table(M, seed=100 + M)
    lk = _lookup(xyz)
    q = mixed_queries(xyz, 130, seed=M)
    assert_model_bits(xyz, q, lk.points(q), True, f"M = {M}")
    assert_model_bits(xyz, q, lk.points(q, blend=False), False, f"M = {M}, nearest only")
    assert lk.last_launch()[2] == 1


def test_the_largest_table():
    M = 65536
    xyz = unit_table(M, seed=65536)
    lk = _lookup(xyz)
    q = mixed_queries(xyz, 256, seed=6)
    assert_model_bits(xyz, q, lk.points(q, blend=False), False, "M = 65536, nearest only")
    m = assert_model_bits(xyz, q[:128], lk.points(q[:128]), True, "M = 65536")
    assert len(set(m["idx0"] // 1024)) > 20         # (answers all over the table)


# ---- query counts around the wave and the chunk ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_query_counts(n):
    xyz = unit_table(65, seed=65)
    lk = _lookup(xyz)
    q = mixed_queries(xyz, n, seed=n)
    i0, i1, w = c_arrays(n)
    assert c_points(lk, q, i0, i1, w) == 0
    assert_model_bits(xyz, q, (i0[:n], i1[:n], w[:n]), True, f"n = {n}")
    assert (i0[n:] == SENT_U).all() and (i1[n:] == SENT_U).all() and (lm.bits(w[n:]) == lm.bits(SENT_F)).all()
    assert lk.last_launch()[2] == 1


def test_one_query_more_than_a_chunk():
    xyz = unit_table(65, seed=66)
    lk = _lookup(xyz)
    _, Q = _sizes(lk)
    n = Q + 1
    q = mixed_queries(xyz, n, seed=12)
    i0, i1, w = c_arrays(n)
    assert c_points(lk, q, i0, i1, w) == 0
    assert lk.last_launch()[2] == 2
    assert_model_bits(xyz, q, (i0[:n], i1[:n], w[:n]), True, "Q + 1 queries")
    assert (i0[n:] == SENT_U).all() and (i1[n:] == SENT_U).all() and (lm.bits(w[n:]) == lm.bits(SENT_F)).all()
    # the buffers have grown to a chunk: a small call behind it is right, and an empty one touches nothing
    assert_model_bits(xyz, q[:7], lk.points(q[:7]), True, "a small call behind a large one")
    assert c_points(lk, np.zeros((0, 3)), None, None, None) == 0 and lk.last_launch()[2] == 0


# ---- ties across the seams ---------------------------------------------------------------------------------------------------------
def test_a_point_stored_on_both_sides_of_a_tile_boundary():
    probe = _lookup(unit_table(1, 0))
    T, _ = _sizes(probe)
    xyz = unit_table(2 * T + 1, seed=9)
    lo, hi, hi2 = 3, T, 2 * T
    xyz[hi] = xyz[lo]
    xyz[hi2] = xyz[lo]
    lk = _lookup(xyz)
    P = xyz[lo].astype(np.float64)
    q = np.stack([P, P * 1.0009765625, P * 0.99])        # on it, and two the copies are equally far from
    i0, i1, w = lk.points(q)
    m = assert_model_bits(xyz, q, (i0, i1, w), True, "copies across tiles")
    assert (m["idx0"] == lo).all() and (m["d_next"] == m["d_best"]).all()       # the model: a tie, the lower index
    assert (i0 == lo).all()
    assert not np.isin(i1, [lo, hi, hi2]).any()                                  # the copies of idx0 are no chord (L > 0)
    assert lm.bits(w)[0] == 0
    # the second stage's own tie: the query on P[lo] is at O = 0 from every chord, the first point that is no copy is taken
    assert i1[0] == 0


def test_one_point_65_times():
    xyz = np.repeat(unit_table(1, 5), 65, axis=0)
    lk = _lookup(xyz)
    q = mixed_queries(xyz, 70, seed=65)
    i0, i1, w = lk.points(q)
    assert_model_bits(xyz, q, (i0, i1, w), True, "one point 65 times")
    assert (i0 == 0).all() and (i1 == 0).all() and (lm.bits(w) == 0).all()


# ---- where the queries are -----------------------------------------------------------------------------------------------------------
def test_queries_on_points_on_midpoints_far_out_and_at_the_origin():
    xyz = unit_table(200, seed=200)
    lk = _lookup(xyz)
    P = xyz.astype(np.float64)
    rng = np.random.default_rng(4)
    a, b = rng.integers(0, 200, 64), rng.integers(0, 200, 64)
    d = rng.standard_normal((64, 3))
    q = np.concatenate([P, (P[a] + P[b]) / 2, 10.0 * d / np.linalg.norm(d, axis=1, keepdims=True), np.zeros((3, 3))])
    i0, i1, w = lk.points(q)
    assert_model_bits(xyz, q, (i0, i1, w), True, "special queries")
    assert (i0[:200] == np.arange(200)).all() and (lm.bits(w[:200]) == 0).all()
    assert (w[200:264] > 0).any() and (w >= 0).all() and (w <= 1).all()


# ---- rows ----------------------------------------------------------------------------------------------------------------------------
def _rows_inputs(S, segs, K, src_shape, pose_shape, seed):
    rng = np.random.default_rng(seed)
    dims = {"K": (K,), "SK": (S, K), "gK": (segs, K), "SgK": (S, segs, K)}[src_shape]
    pdims = {"g": (segs,), "Sg": (S, segs)}[pose_shape]
    az, el = rng.uniform(-180, 180, dims).astype(np.float32), rng.uniform(-80, 80, dims).astype(np.float32)
    yaw, pitch, roll = (rng.uniform(-r, r, pdims).astype(np.float32) for r in (180, 40, 30))
    return az, el, yaw, pitch, roll


@pytest.mark.parametrize("K", [1, 6, 64])
@pytest.mark.parametrize("src_shape,pose_shape", [("K", "g"), ("SK", "g"), ("gK", "Sg"), ("SgK", "Sg"), ("K", "Sg"), ("SgK", "g")])
def test_rows(K, src_shape, pose_shape):
    from open_headstage_amd import lookup
    S, segs = 3, 5
    xyz = unit_table(130, seed=13)
    lk = _lookup(xyz)
    az, el, yaw, pitch, roll = _rows_inputs(S, segs, K, src_shape, pose_shape, seed=K)
    v, sss, sks, R, rss, S_, segs_, K_ = lookup.rows_host_half(az, el, yaw, pitch, roll, 1.5)
    S_want = S if ("S" in src_shape or "S" in pose_shape) else 1
    assert (S_, segs_, K_) == (S_want, segs, K)
    q = lm.rows_queries(v, sss, sks, R, rss, S_, segs, K).reshape(-1, 3)
    i0, i1, w = lk.rows(az, el, yaw, pitch, roll, 1.5)
    assert i0.shape == i1.shape == w.shape == (S_, segs, K) and i0.dtype == i1.dtype == np.uint32 and w.dtype == np.float32
    assert_model_bits(xyz, q, (i0, i1, w), True, f"rows {src_shape} {pose_shape} K = {K}")
    only = lk.rows(az, el, yaw, pitch, roll, 1.5, blend=False)
    assert only.shape == (S_, segs, K) and (only == i0).all()
    # without a pose: q = v
    n = S_ * segs * K
    a0, a1, aw = c_arrays(n)
    assert c_rows(lk, S_, segs, K, v, sss, sks, None, 0, a0, a1, aw) == 0
    assert_model_bits(xyz, lm.rows_queries(v, sss, sks, None, 0, S_, segs, K).reshape(-1, 3), (a0[:n], a1[:n], aw[:n]), True, "rot NULL")
    assert (a0[n:] == SENT_U).all() and (a1[n:] == SENT_U).all() and (lm.bits(aw[n:]) == lm.bits(SENT_F)).all()
    # nearest only: nothing but idx0 is written
    b0, b1, bw = c_arrays(n)
    assert c_rows(lk, S_, segs, K, v, sss, sks, R, rss, b0, None, None) == 0
    assert (b0[:n] == i0.reshape(-1)).all() and (b0[n:] == SENT_U).all()


def test_rows_with_wide_strides_never_read_the_gaps():
    S, segs, K = 3, 5, 6
    xyz = unit_table(130, seed=14)
    lk = _lookup(xyz)
    rng = np.random.default_rng(15)
    src = np.full((S, 7, 2, K, 3), np.nan)          # stream stride 14, segment stride 2
    src[:, :segs, 0] = rng.standard_normal((S, segs, K, 3))
    rot = np.full((S, 8, 3, 3), np.inf)             # stream stride 8
    rot[:, :segs] = np.linalg.qr(rng.standard_normal((S, segs, 3, 3)))[0]
    n = S * segs * K
    i0, i1, w = c_arrays(n)
    assert c_rows(lk, S, segs, K, src, 14, 2, rot, 8, i0, i1, w) == 0
    q = lm.pose(rot[:, :segs, None], src[:, :segs, 0]).reshape(-1, 3)
    assert_model_bits(xyz, q, (i0[:n], i1[:n], w[:n]), True, "wide strides")


def test_rows_of_more_than_a_chunk():
    """sources per stream, poses per segment, shared the other way: the parts of both that a chunk stages change from chunk to chunk"""
    from open_headstage_amd import lookup
    xyz = unit_table(3, seed=3)
    lk = _lookup(xyz)
    _, Q = _sizes(lk)
    K, segs = 6, 500
    S = Q // (K * segs) + 2
    az, el, yaw, pitch, roll = _rows_inputs(S, segs, K, "SK", "g", seed=77)
    v, sss, sks, R, rss, S_, _, _ = lookup.rows_host_half(az, el, yaw, pitch, roll)
    i0, i1, w = lk.rows(az, el, yaw, pitch, roll)
    assert lk.last_launch()[2] == 2 and S_ == S
    assert_model_bits(xyz, lm.rows_queries(v, sss, sks, R, rss, S, segs, K).reshape(-1, 3), (i0, i1, w), True, "two chunks of rows")
    # and everything per stream and segment
    az, el, yaw, pitch, roll = _rows_inputs(S, segs, K, "SgK", "Sg", seed=78)
    v, sss, sks, R, rss, _, _, _ = lookup.rows_host_half(az, el, yaw, pitch, roll)
    got = lk.rows(az, el, yaw, pitch, roll, blend=False)
    assert_model_bits(xyz, lm.rows_queries(v, sss, sks, R, rss, S, segs, K).reshape(-1, 3), got, False, "two chunks of rows, all per stream")


# ---- the Python surface against the helpers ----------------------------------------------------------------------------------------
def test_nearest_and_bracket_against_the_helpers():
    from open_headstage_amd import DirectionLookup, scene, scene2
    from tests.test_cpu_lookup import MAX_UNCLEAR, judge_bracket, random_queries, ring_grid_table
    pos = ring_grid_table()
    lk = DirectionLookup(pos)
    az, el = random_queries(2048, seed=8)
    az, el = az.reshape(32, 64), el.reshape(32, 64)
    got = lk.nearest(az, el, 1.25)
    assert got.shape == (32, 64) and got.dtype == np.uint32
    assert (got == scene.nearest_directions(pos, az, el, 1.25)).all()
    i0, i1, w = lk.bracket(az, el)
    assert i0.shape == i1.shape == w.shape == (32, 64) and w.dtype == np.float32
    unclear = judge_bracket(pos, az, el, (i0, i1, w), "DirectionLookup.bracket against the model")
    h0, h1, hw = scene2.bracket_directions(pos, az, el)
    from tests.test_cpu_lookup import CLEAR, model_for
    m, _ = model_for(pos, az, el)
    clear = (m["o_next"] - m["o_best"] > CLEAR * m["o_best"]).reshape(32, 64)
    assert (i0 == h0).all() and (i1[clear] == h1[clear]).all() and (lm.bits(w[clear]) == lm.bits(hw[clear])).all()
    assert unclear <= MAX_UNCLEAR


def test_rows_into_a_blended_scene_call():
    """S = 3, K = 3, 4 blocks, 64 directions: BlendSceneProcessor.process on DirectionLookup.rows' output against the same call on the
    helpers' rows for the same head-relative directions, bit for bit"""
    import torch

    import open_headstage_amd as ohs
    from tests.test_cpu_layout import make_input, make_layout
    from tests.test_cpu_lookup import sphere_table
    S, K, blocks, seg, n_dirs = 3, 3, 4, 1, 64
    pos = sphere_table(n_dirs, seed=64)
    rng = np.random.default_rng(64)
    src_az, src_el = rng.uniform(-180, 180, (blocks, K)).astype(np.float32), rng.uniform(-60, 60, (blocks, K)).astype(np.float32)
    yaw, pitch, roll = (rng.uniform(-r, r, (S, blocks, 1)).astype(np.float32) for r in (180, 30, 20))
    az, el = ohs.rotate_sources(src_az[None], src_el[None], yaw, pitch, roll)            # [S][blocks][K], seen from each head
    h0, h1, hw = ohs.bracket_directions(pos, -az, el)
    lk = ohs.DirectionLookup(pos)
    i0, i1, w = lk.rows(az, el, np.zeros(blocks, np.float32))
    assert (i0 == h0).all() and (i1 == h1).all() and (lm.bits(w) == lm.bits(hw)).all()
    assert (w > 0).any() and len(set(i0.reshape(-1))) > 8
    dirs = make_layout(n_dirs, 512)
    x = torch.from_numpy(make_input(S, K, blocks, seed=640)).cuda()
    outs = []
    for rows in ((i0, i1, w), (h0, h1, hw)):
        sc = ohs.BlendSceneProcessor(S, num_bands=10)
        sc.set_directions(dirs)
        y = sc.process(x, rows[0], seg, idx1=rows[1], weights=rows[2])
        torch.cuda.synchronize()
        outs.append(y.cpu().numpy())
        assert sc.last_launch()[3] > 0
    assert np.abs(outs[0]).max() > 0 and (outs[0].view(np.uint32) == outs[1].view(np.uint32)).all()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_and_the_handle():
    from open_headstage_amd import DirectionLookupError, lookup
    xyz = unit_table(130, seed=21)
    lk = _lookup(xyz)
    L = lookup.lookup_lib()
    q = mixed_queries(xyz, 40, seed=22)
    assert_model_bits(xyz, q, lk.points(q), True)
    before = lk.last_launch()

    def untouched(i0, i1, w):
        return (i0 == SENT_U).all() and (i1 == SENT_U).all() and (lm.bits(w) == lm.bits(SENT_F)).all()
    bad = q.copy()
    bad[33, 1] = np.nan
    i0, i1, w = c_arrays(40)
    assert c_points(lk, bad, i0, i1, w) == INV and untouched(i0, i1, w)
    assert b"finite" in L.ohs_lookup_last_error()
    bad[33, 1] = 2e100
    assert c_points(lk, bad, i0, i1, w) == INV and untouched(i0, i1, w)
    assert c_points(lk, q, i0, None, w) == INV and c_points(lk, q, i0, i1, None) == INV and untouched(i0, i1, w)
    assert c_points(lk, q, None, i1, w) == INV and untouched(i0, i1, w)
    S, segs, K = 3, 5, 6
    rng = np.random.default_rng(23)
    src = rng.standard_normal((S, segs, K, 3))
    rot = np.linalg.qr(rng.standard_normal((S, segs, 3, 3)))[0]
    n = S * segs * K
    i0, i1, w = c_arrays(n)
    rot_bad = rot.copy()
    rot_bad[2, 4, 1, 1] = np.inf
    assert c_rows(lk, S, segs, K, src, segs, 1, rot_bad, segs, i0, i1, w) == INV and untouched(i0, i1, w)
    src_bad = src.copy()
    src_bad[2, 4, 5, 2] = -np.inf
    assert c_rows(lk, S, segs, K, src_bad, segs, 1, rot, segs, i0, i1, w) == INV and untouched(i0, i1, w)
    assert c_rows(lk, S, segs, K, src, segs - 1, 1, rot, segs, i0, i1, w) == INV and untouched(i0, i1, w)       # a short stride
    assert b"stride" in L.ohs_lookup_last_error()
    assert c_rows(lk, S, segs, K, src, segs, 1, rot, segs - 1, i0, i1, w) == INV and untouched(i0, i1, w)
    assert c_rows(lk, S, segs, 0, src, segs, 1, rot, segs, i0, i1, w) == INV and untouched(i0, i1, w)
    assert c_rows(lk, S, segs, 65, src, segs, 1, rot, segs, i0, i1, w) == INV and untouched(i0, i1, w)
    assert c_rows(lk, S, segs, K, None, segs, 1, rot, segs, i0, i1, w) == INV and untouched(i0, i1, w)
    assert c_rows(lk, 0, segs, K, src, segs, 1, rot, segs, i0, i1, w) == 0 and untouched(i0, i1, w)
    with pytest.raises(DirectionLookupError) as e:
        lk.points(bad)
    assert e.value.status == INV
    # the handle is as it was: the record of the last launch, and the next valid calls
    assert c_points(lk, bad, i0, i1, w) == INV and lk.last_launch()[:2] == before[:2]
    assert_model_bits(xyz, q, lk.points(q), True, "after the refusals")
    assert lk.last_launch() == before
    assert c_rows(lk, S, segs, K, src, segs, 1, rot, segs, i0, i1, w) == 0
    assert_model_bits(xyz, lm.pose(rot[:, :, None], src).reshape(-1, 3), (i0[:n], i1[:n], w[:n]), True, "rows after the refusals")

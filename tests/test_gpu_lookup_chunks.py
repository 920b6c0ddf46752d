"""Rows across chunk cuts on the device, for libohs_lookup.so, libohs_lookup3.so and libohs_lookup3p.so alike: every branch of the
staging with a base that is not zero, a chunk that is neither first nor last, and one handle driven through a long mixed sequence.

Every call is made at the C level with explicit src and rot arrays, so every stride form is reachable; every answer is compared bit for
bit -- by lookup_chunks.hold_answers, which names the first wrong (chunk, stream, segment, object), and by the library's existing checker
(assert_model_bits, assert_model) on the same arrays.  libohs_lookup.so is held to tests/lookup_model.py over a table of 30 points, the
two triangle libraries to tests/lookup3_model.py over the level-1 octahedron mesh of 32 triangles, tri included, and the pruned one's
count of queries answered by pass 2 to lookup3p_model.falls_back summed over the call.  Sources and poses come from a palette
(tests/lookup_chunks.py), so the model is computed for 168 pairs and indexed out; nothing is sampled.  Q is the chunk of queries, read
from last_launch.

SHAPE A, S = 3, segs = 30000, K = 6: 540 000 queries in three chunks; chunk 1 starts at object 4 of a group in mid-stream and spans two
streams, chunk 2 lies inside one stream (tests/test_cpu_lookup_chunks.py holds the shapes to this).  Five stride forms:
(a) sources and poses per stream and segment, (b) sources per segment only, (c) poses per segment only, (d) sources per stream only and
no poses, (e) wide strides with NaN in every gap of the sources and Inf in every gap of the poses.
SHAPE B, K = 64, segs = 1, S = Q / 64 + 3: the cut falls between groups, sources and poses per stream with s_lo = 4 096.
SHAPE C, K = 1, segs = 1, S = Q + 5: one object per stream, s_lo = Q."""
import numpy as np
import pytest

from tests import lookup3_model as l3
from tests import lookup3p_model as l3p
from tests import lookup_chunks as lc
from tests import lookup_model as lm
from tests import test_gpu_lookup as g2
from tests import test_gpu_lookup3 as g3
from tests import test_gpu_lookup3p as g3p

pytestmark = pytest.mark.gpu

LIBS = ("lookup", "lookup3", "lookup3p")
U, F = np.uint32, np.float32


class Device:
    """the adapter of tests/lookup_chunks.py over one handle of one library"""

    def __init__(self, world, grid=0):
        import open_headstage_amd as ohs
        self.w = w = world
        self.name, self.want, self.pq = w["name"], w["want"], w["pq"]
        self.rest = w["rest"] if self.name == "lookup3p" else None
        if self.name == "lookup":
            self.lk, self.dtypes, self.optional = ohs.DirectionLookup(None, xyz=w["xyz"]), [U, U, F], (1, 2)
        elif self.name == "lookup3":
            self.lk, self.dtypes, self.optional = ohs.TriangleLookup(None, w["tris"], xyz=w["xyz"]), [U] * 3 + [F] * 2 + [U], (5,)
        else:
            self.lk = ohs.PrunedTriangleLookup(None, w["tris"], xyz=w["xyz"], grid=grid)
            self.dtypes, self.optional = [U] * 3 + [F] * 2 + [U], (5,)
        self.Q = self.lk.last_launch()[0 if self.name == "lookup3p" else 1]
        assert self.Q >= 258 and self.launch() == (0, None if self.rest is None else 0)

    def launch(self):
        rec = self.lk.last_launch()
        return (rec[1], rec[2]) if self.name == "lookup3p" else (rec[2], None)

    def rows(self, case, arrays):
        c = case
        args = (self.lk, c["S"], c["segs"], c["K"], c["src"], c["sss"], c["sks"], c["rot"], c["rss"])
        if self.name == "lookup":
            return g2.c_rows(*args, *arrays)
        return (g3 if self.name == "lookup3" else g3p).c_rows(*args, arrays)

    def points(self, q, pair, arrays):
        if self.name == "lookup":
            return g2.c_points(self.lk, q, *arrays)
        return (g3 if self.name == "lookup3" else g3p).c_points(self.lk, q, arrays)

    def existing(self, got, pair, what):
        n, w = len(pair), self.w
        if n == 0 or any(g is None for g in got):
            return
        q, m = self.pq[pair], {k: v[pair] for k, v in w["m"].items() if v is not None}
        got = [g[:n] for g in got]
        if self.name == "lookup":
            g2.assert_model_bits(w["xyz"], q, got, True, what, model=m)
        elif self.name == "lookup3":
            g3.assert_model_bits(w["xyz"], w["tris"], q, got, what, model=m)
        else:
            g3p.assert_model(self.lk, w["xyz"], w["tris"], q, got, what, model=m)


@pytest.fixture(scope="module")
def worlds():
    """per library: the table (and mesh), the palette over it, the model of the palette's pairs; and the cases made so far"""
    from open_headstage_amd import lookup, lookup3
    pos, tris = lookup3.octahedron_mesh(1)
    xyz3 = lookup.table_xyz(pos)
    assert len(tris) == 32
    pal3 = lc.palette(xyz3, tris, seed=5)
    pq3 = lc.pair_queries(pal3[0], pal3[1])
    m3 = l3.lookup3(xyz3, tris, pq3)
    three = dict(xyz=xyz3, tris=tris, pal=pal3, pq=pq3, m=m3, want=lc.model_planes(m3, l3.FIELDS + ("tri",)), rest=l3p.falls_back(xyz3, tris, pq3, m3))
    xyz2 = g2.unit_table(30, seed=30)
    pal2 = lc.palette(xyz2, None, seed=6)
    pq2 = lc.pair_queries(pal2[0], pal2[1])
    m2 = lm.lookup(xyz2, pq2)
    two = dict(xyz=xyz2, tris=None, pal=pal2, pq=pq2, m=m2, want=lc.model_planes(m2, ("idx0", "idx1", "w")), rest=None)
    cases3 = {}
    return {"lookup": dict(two, name="lookup", cases={}), "lookup3": dict(three, name="lookup3", cases=cases3),
            "lookup3p": dict(three, name="lookup3p", cases=cases3)}


def _case(world, key, make):
    """cases are made once per palette and left unchanged (the two triangle libraries share theirs)"""
    if key not in world["cases"]:
        world["cases"][key] = make()
    return world["cases"][key]


def _same_bits(a, b, n):
    return all((lc.bits(x[:n]) == lc.bits(y[:n])).all() for x, y in zip(a, b))


# ---- shape A -------------------------------------------------------------------------------------------------------------------------
def _shape_a(world, form, grid=0):
    ad = Device(world, grid)
    case = _case(world, "A" + form, lambda: lc.shape_a(world["pal"], form))
    n = len(case["pair"])
    assert n == 540000 and n > 2 * ad.Q
    out = lc.hold_rows(ad, case, f"{ad.name}, shape A ({form})")
    assert ad.launch()[0] == 3
    if ad.rest is not None:
        assert all(c >= 100 for c in lc.hold_launch(ad, case["pair"], "shape A"))
    if form == "e":
        # the same sources and poses stored densely: the same bits
        dense = _case(world, "Aa", lambda: lc.shape_a(world["pal"], "a"))
        assert (dense["pair"] == case["pair"]).all() and np.isnan(case["src"]).sum() > 0 and np.isinf(case["rot"]).sum() > 0
        assert _same_bits(out, lc.hold_rows(ad, dense, f"{ad.name}, shape A dense"), n)
    if ad.name == "lookup3p" and form in "ad":
        five = lc.hold_rows(ad, case, f"{ad.name}, shape A ({form}), tri NULL", null=True)
        assert _same_bits(out[:5], five[:5], n) and ad.launch()[0] == 3
    return ad


@pytest.mark.parametrize("name", LIBS)
def test_shape_a_per_stream_and_segment(worlds, name):
    _shape_a(worlds[name], "a")


@pytest.mark.parametrize("name", LIBS)
def test_shape_a_sources_per_segment_only(worlds, name):
    _shape_a(worlds[name], "b")


@pytest.mark.parametrize("name", LIBS)
def test_shape_a_poses_per_segment_only(worlds, name):
    _shape_a(worlds[name], "c")


@pytest.mark.parametrize("name", LIBS)
def test_shape_a_sources_per_stream_only_and_no_poses(worlds, name):
    _shape_a(worlds[name], "d")


@pytest.mark.parametrize("name", LIBS)
def test_shape_a_wide_strides_with_unreadable_gaps(worlds, name):
    _shape_a(worlds[name], "e")


def test_shape_a_pruned_at_grid_16(worlds):
    ad = _shape_a(worlds["lookup3p"], "a", grid=16)
    assert ad.lk.index()[0] == 16


# ---- shapes B and C ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LIBS)
def test_shape_b_the_cut_between_groups_of_64(worlds, name):
    ad = Device(worlds[name])
    case = _case(worlds[name], "B", lambda: lc.shape_b(worlds[name]["pal"], ad.Q))
    assert case["S"] == ad.Q // 64 + 3 and (case["sss"], case["sks"], case["rss"]) == (1, 0, 1)
    lc.hold_rows(ad, case, f"{name}, shape B")
    assert ad.launch()[0] == 2


@pytest.mark.parametrize("name", LIBS)
def test_shape_c_one_object_per_stream(worlds, name):
    ad = Device(worlds[name])
    case = _case(worlds[name], "C", lambda: lc.shape_c(worlds[name]["pal"], ad.Q))
    assert case["S"] == ad.Q + 5 and case["K"] == 1
    lc.hold_rows(ad, case, f"{name}, shape C")
    assert ad.launch()[0] == 2


# ---- one handle, many calls ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed", [("lookup", 1), ("lookup3", 2), ("lookup3p", 3)])
def test_one_handle_many_calls(worlds, name, seed):
    ad = Device(worlds[name])
    ops = lc.draw_sequence(seed)
    assert lc.run_sequence(ad, worlds[name]["pal"], ops) == 16
    print(f"{name}: {len(ops)} operations on one handle, {sum(lc.is_large(op) for op in ops)} of more than a chunk")


# ---- the widest grid ---------------------------------------------------------------------------------------------------------------------
def test_the_widest_grid_is_queried():
    """the level-6 mesh at grid = 256: some triangles on the everywhere list, the others in cell lists, pass 1 walks both merged"""
    import open_headstage_amd as ohs
    from tests.test_cpu_lookup3p import widest_grid_case
    xyz, tris, q, G = widest_grid_case()
    lk = ohs.PrunedTriangleLookup(None, tris, xyz=xyz, grid=G)
    grid, cells, entries, longest, everywhere = lk.index()
    assert (grid, cells) == (256, 6 * 256 * 256) and 0 < everywhere < len(tris) and entries > 0 and longest > 0
    got = lk.points(q, return_triangle=True)
    _, rest = g3p.assert_model(lk, xyz, tris, q, got, "level 6 at grid 256")
    assert 0 < rest.sum() < len(q) and lk.last_launch()[1] == 1
    brute = ohs.TriangleLookup(None, tris, xyz=xyz).points(q, return_triangle=True)
    for field, g, b in zip(l3.FIELDS + ("tri",), got, brute):
        assert (lc.bits(g) == lc.bits(b)).all(), field
    print(f"level 6 at grid 256: {entries} entries, longest list {longest}, everywhere {everywhere}; {int(rest.sum())} of {len(q)} to pass 2")

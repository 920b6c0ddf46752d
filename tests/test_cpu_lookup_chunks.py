"""tests/lookup_chunks.py held to what it names, without a GPU: the shapes of tests/test_gpu_lookup_chunks.py cut where that file says
they are cut, the staging equal to the direct formula for every one of them, both kinds of query in every chunk for the pruned library,
six numpy libraries each wrong in one way each reported by the checker the GPU file uses -- with the first wrong (chunk, stream,
segment, object) named --, and the one-handle sequence's generator.

The numpy libraries and the checker work on the palette's pairs (lookup_chunks.py): the model here is lookup3_model.lookup3 over the
level-1 octahedron mesh for the 168 pairs of the palette, as the GPU file computes it."""
import os
import re

import numpy as np
import pytest

from tests import lookup3_model as l3
from tests import lookup3p_model as l3p
from tests import lookup_chunks as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = lc.CHUNK
FORMS_A = "abcde"
DTYPES3 = [np.uint32] * 3 + [np.float32] * 2 + [np.uint32]


@pytest.fixture(scope="module")
def world():
    """the level-1 mesh, the palette over it, the model per pair"""
    from open_headstage_amd import lookup, lookup3
    pos, tris = lookup3.octahedron_mesh(1)
    xyz = lookup.table_xyz(pos)
    assert len(tris) == 32
    pal = lc.palette(xyz, tris, seed=5)
    pq = lc.pair_queries(pal[0], pal[1])
    m = l3.lookup3(xyz, tris, pq)
    return dict(xyz=xyz, tris=tris, pal=pal, pq=pq, m=m, want=lc.model_planes(m, l3.FIELDS + ("tri",)), rest=l3p.falls_back(xyz, tris, pq, m))


@pytest.fixture(scope="module")
def cases(world):
    pal = world["pal"]
    out = {f"A({f})": lc.shape_a(pal, f) for f in FORMS_A}
    out.update(B=lc.shape_b(pal), C=lc.shape_c(pal), big=lc.big_rows(pal))
    return out


def _library(world, fault=None, Q_=Q):
    return lc.NumpyLibrary(world["want"], world["rest"], DTYPES3, (5,), len(world["pal"][1]), Q_, fault)


def _plan(c):
    return lc.chunk_plan(c["S"], c["segs"], c["K"], c["sss"], c["sks"], c["rss"], c["rot"] is not None)


def test_the_chunk_is_the_libraries():
    for name in ("lookup", "lookup3", "lookup3p"):
        text = open(os.path.join(ROOT, "open_headstage_amd", "csrc", name + "_internal.h")).read()
        assert re.search(r"CHUNK_QUERIES = size_t\(1\) << 18;", text), name


def test_the_palette(world):
    points, poses, n_meas = world["pal"]
    T = world["xyz"].astype(np.float64)
    assert len(points) == 24 and len(poses) == 6 and n_meas == 8 and len(world["pq"]) == 24 * 7
    assert all((T == p).all(1).any() for p in points[:n_meas]) and not any((T == p).all(1).any() for p in points[n_meas:])
    assert (poses[0] == np.eye(3)).all() and np.abs(poses @ np.swapaxes(poses, 1, 2) - np.eye(3)).max() < 1e-14
    rest = world["rest"].reshape(24, 7)
    # a measurement without a pose or under the identity is exactly on a corner: pass 2's; every centroid and random direction is pass 1's
    assert rest[:n_meas, :2].all() and not rest[13:].any() and 16 <= rest.sum() < 80
    assert (world["pq"].reshape(24, 7, 3)[:, 0] == points).all() and (world["pq"].reshape(24, 7, 3)[:, 1] == points).all()


@pytest.mark.parametrize("form", FORMS_A)
def test_shape_a_is_cut_where_the_gpu_file_says(cases, form):
    c = cases[f"A({form})"]
    plan = _plan(c)
    assert (c["S"], c["segs"], c["K"]) == (3, 30000, 6) and len(c["pair"]) == 540000 and len(plan) == 3
    assert [p["at"] for p in plan] == [0, Q, 2 * Q] and [p["nq"] for p in plan] == [Q, Q, 540000 - 2 * Q]
    assert plan[1]["c"] == 4                                                        # chunk 1 starts inside a group
    assert plan[1]["lo"] == (1, 13690) and plan[1]["hi"] == (2, 27381)              # ... and spans two streams, from mid-stream
    assert plan[2]["lo"] == (2, 27381) and plan[2]["hi"] == (2, 29999) and plan[2]["c"] == 2        # chunk 2: inside one stream
    wide = form == "e"
    assert (c["sss"], c["sks"], c["rss"]) == {"a": (30000, 1, 30000), "b": (0, 1, 30000), "c": (30000, 1, 0), "d": (1, 0, 0),
                                              "e": (60002, 2, 30002)}[form]
    assert (c["rot"] is None) == (form == "d")
    if wide:
        assert np.isnan(c["src"]).any(axis=(1, 2)).sum() == len(c["src"]) - 90000 and np.isinf(c["rot"]).any(axis=(1, 2)).sum() == len(c["rot"]) - 90000


def test_every_branch_of_range_is_taken_with_a_base_that_is_not_zero(world, cases):
    """over shape A's forms: 'stream and segment' (a), 'stream' (d) and 'segment, one stream' (b, c) with lo > 0; 'segment, every
    stream' and 'shared' have lo = 0 by construction and are taken in a chunk whose g0 is not 0"""
    seen, late = set(), set()
    for f in FORMS_A + "BC":
        c = cases[f"A({f})"] if f in FORMS_A else cases[f]
        for p in _plan(c)[1:]:
            for r in (p["src"], p["rot"]):
                if r is not None:
                    late.add(r[2])
                    if r[0] > 0:
                        seen.add(r[2])
    assert seen == set(lc.BRANCHES[:3]) and lc.BRANCHES[3] in late
    shared = lc.rows_case(world["pal"], 3, 5, 6, "g", 1)
    assert _plan(shared)[0]["src"] == (0, 0, lc.BRANCHES[4])
    b, cc = _plan(cases["B"]), _plan(cases["C"])
    assert len(b) == 2 and b[1]["c"] == 0 and b[1]["src"][:2] == (4096, 4098) and b[1]["rot"][:2] == (4096, 4098)   # the cut between groups
    assert len(cc) == 2 and cc[1]["src"] == (Q, Q + 4, lc.BRANCHES[1]) and cases["C"]["S"] < 1 << 24
    big = _plan(cases["big"])
    assert len(big) == 2 and cases["big"]["K"] == 1 and (cases["big"]["K"] * 3 + 9) * 8 == 96


@pytest.mark.parametrize("name", [f"A({f})" for f in FORMS_A] + ["B", "C", "big"])
def test_the_staging_gives_the_direct_formula(world, cases, name):
    c = cases[name]
    v, r = lc.staged_queries(c["src"], c["rot"], c["S"], c["segs"], c["K"], c["sss"], c["sks"], c["rss"])
    q = v if r is None else lc.pose(r.reshape(-1, 3, 3), v)
    direct = lc.case_queries(c)
    assert q.shape == direct.shape and (q.view(np.uint64) == direct.view(np.uint64)).all()
    assert (lc.staged_pairs(c, 6) == c["pair"]).all()
    assert (world["pq"][c["pair"]].view(np.uint64) == direct.view(np.uint64)).all()         # the palette's model is the call's


@pytest.mark.parametrize("K", lc.SMALL_K)
@pytest.mark.parametrize("form", lc.SMALL_FORMS)
def test_the_small_rows_of_the_sequence_too(world, K, form):
    c = lc.rows_case(world["pal"], 3, 5, K, form, seed=K)
    v, r = lc.staged_queries(c["src"], c["rot"], c["S"], c["segs"], c["K"], c["sss"], c["sks"], c["rss"], Q=37)      # (cuts everywhere)
    q = v if r is None else lc.pose(r.reshape(-1, 3, 3), v)
    assert (q.view(np.uint64) == lc.case_queries(c).view(np.uint64)).all() and (lc.staged_pairs(c, 6, Q=37) == c["pair"]).all()


@pytest.mark.parametrize("name", [f"A({f})" for f in FORMS_A] + ["B", "C", "big"])
def test_both_passes_have_work_in_every_chunk(world, cases, name):
    """at least 100 queries for pass 2 and at least 100 certified in every chunk of shape A and in every full chunk of the others.
    (The last chunks of B and C are 192 and 5 queries long -- 100 of each kind cannot be in them; B's has both kinds.)"""
    pair = cases[name]["pair"]
    for at in range(0, len(pair), Q):
        rest = world["rest"][pair[at:at + Q]]
        if name.startswith("A") or len(rest) == Q:
            assert rest.sum() >= 100 and (~rest).sum() >= 100, (name, at, int(rest.sum()), len(rest))
        elif len(rest) >= 100:
            assert rest.any() and not rest.all(), (name, at)


# ---- the numpy libraries ---------------------------------------------------------------------------------------------------------------
def test_the_right_numpy_library_passes_every_shape(world, cases):
    ad = _library(world)
    for name, c in cases.items():
        lc.hold_rows(ad, c, name, null=name in ("A(a)", "A(d)"))
    assert ad.launch()[0] == 2


def _report(world, cases, fault, name):
    """the checker's words on the library wrong in `fault`, or None where it passes"""
    try:
        lc.hold_rows(_library(world, fault), cases[name], name)
    except AssertionError as e:
        return str(e)
    return None


def _where(text):
    m = re.search(r"chunk (\d+), stream (\d+), segment (\d+), object (\d+)", text)
    assert m, text
    return tuple(int(v) for v in m.groups())


def test_src_base_not_subtracted_is_reported(world, cases):
    for f in "ade":
        assert _where(_report(world, cases, "src base", f"A({f})"))[:3] == (1, 1, 13690), f    # the first group of chunk 1
    assert _where(_report(world, cases, "src base", "A(b)"))[:3] == (2, 2, 27381)      # (b)'s chunk 1 stages every segment: its base is 0
    assert _where(_report(world, cases, "src base", "B")) == (1, 4096, 0, 0)
    assert _where(_report(world, cases, "src base", "C")) == (1, Q, 0, 0)


def test_rot_base_from_the_sources_is_reported(world, cases):
    """(a) has one base for both and cannot tell; (b) and (c) have different branches for the two"""
    assert _report(world, cases, "rot base", "A(a)") is None
    for f in "bc":
        chunk, s, k, _ = _where(_report(world, cases, "rot base", f"A({f})"))
        assert chunk == 1 and (s, k) >= (1, 13690), f
    assert _where(_report(world, cases, "rot base", "A(b)"))[:3] == (1, 1, 13690)


def test_one_stream_staged_from_segment_0_is_reported(world, cases):
    for f in "bc":
        chunk, s, k, _ = _where(_report(world, cases, "segment zero", f"A({f})"))
        assert (chunk, s) == (2, 2) and 27381 <= k <= 27383, f                  # chunk 2 is the one inside one stream
    assert _report(world, cases, "segment zero", "A(a)") is None and _report(world, cases, "segment zero", "A(d)") is None


def test_g0_truncated_to_the_chunk_is_reported(world, cases):
    for name in [f"A({f})" for f in FORMS_A] + ["B", "C", "big"]:
        assert _where(_report(world, cases, "g0", name))[0] == 1, name


def test_the_fallback_count_of_the_last_chunk_only_is_reported(world, cases):
    for name in ("A(a)", "A(d)", "B", "C"):
        text = _report(world, cases, "last fallback", name)
        assert "the launch record" in text and "chunk by chunk" in text, name
        per = [int(v) for v in re.search(r"chunk by chunk: \[([0-9, ]+)\]", text).group(1).split(",")]
        assert len(per) == len(_plan(cases[name])) and f"({len(per)}, {per[-1]})" in text and min(per) >= (100 if name.startswith("A") else 1)


def test_planes_copied_at_the_first_cap_are_reported_by_the_sequence(world):
    """the sequence on a right library passes; on one that copies the planes down from where they lay before the output staging grew it
    fails at the first large call, with the place and the sequence so far"""
    ops = lc.draw_sequence(3)
    assert lc.run_sequence(_library(world), world["pal"], ops) == 16
    with pytest.raises(AssertionError) as e:
        lc.run_sequence(_library(world, "first cap"), world["pal"], ops)
    text = str(e.value)
    assert text.startswith("operation 1: big rows; the sequence so far:") and "chunk 0, stream 0, segment 0, object 0 (planes [" in text
    # and three of the other faults, which the sequence's rows of more than a chunk meet as well
    for fault in ("src base", "g0", "last fallback"):
        with pytest.raises(AssertionError, match="the sequence so far"):
            lc.run_sequence(_library(world, fault), world["pal"], ops)


# ---- the sequence's generator ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_sequence_contains_what_its_docstring_names(seed):
    ops = lc.draw_sequence(seed)
    assert ops == lc.draw_sequence(seed) and len(ops) == 16 and all(op is not None for op in ops)
    large = [i for i, op in enumerate(ops) if lc.is_large(op)]
    kinds = [ops[i][0] for i in large]
    assert kinds == ["big rows", "points", "shape b", "points", "big rows"]
    assert all(lc.is_small_served(ops[i + 1]) for i in large) and lc.is_small_served(ops[0])
    first_points = next(i for i in large if ops[i][0] == "points")
    assert ops.index(("big rows",)) < first_points                                           # input staging first ...
    later = [i for i in large if i > first_points]
    assert [ops[i][0] for i in later][-2:] == ["points", "big rows"]                          # ... and the reverse order later
    for want in (("empty", "points"), ("empty", "rows"), ("refused", "nan"), ("refused", "stride")):
        assert ops.count(want) == 1
    assert sum(1 for op in ops if op[0] in ("points", "rows") and op[-2] is True) == 1        # the optional outputs NULL, once
    assert all(op[1] in lc.SMALL_N for op in ops if op[0] == "points" and not lc.is_large(op))
    assert all(op[1] in lc.SMALL_K and op[2] in lc.SMALL_FORMS for op in ops if op[0] == "rows")

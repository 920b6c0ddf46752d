"""The direction lookup (libohs_lookup.so, include/ohs_lookup.h), the part that needs no GPU.

* tests/lookup_model.py -- the header's arithmetic in elementwise numpy -- against the two host helpers that define a scene's rows:
  scene.nearest_directions index for index, scene2.bracket_directions wherever one chord is clearly the nearest (that helper sums through
  einsum, whose order numpy does not promise), and everywhere by the distance of the chord it names;
* the pose path of DirectionLookup.rows -- its host half pushed through the model -- against rotate_sources -> nearest_directions;
* csrc/lookup_body.hpp compiled for the host (tests/lookup_host_check.cpp) against the model, bit for bit;
* the header's names, libohs_lookup.so's dynamic symbols and LOOKUP_PROTOTYPES are one list of seven, every entry refuses NULL; the other
  three libraries export what they exported;
* k_lookup was built without scratch, and the build is current."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import lookup_model as lm
from tests.test_cpu_layout import ring_sofa  # noqa: F401
from tests.test_cpu_scene import _dynamic_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "open_headstage_amd")
CLEAR = 1e-9        # a chord is clearly the nearest when the runner-up's O exceeds the best by more than this, relative
NEAR = 1e-12        # everywhere: the helper's chord is within this of the model's best O, relative
MAX_UNCLEAR = 0.01


# ---- tables and queries --------------------------------------------------------------------------------------------------------
def sphere_table(M=1024, seed=11):
    rng = np.random.default_rng(seed)
    az = rng.uniform(0.0, 360.0, M)
    el = np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, M)))
    return np.stack([az, el, np.ones(M)], 1).astype(np.float32)


def ring_grid_table(pole_copies=0):
    az, el = np.meshgrid(np.arange(0.0, 360.0, 5.0), np.arange(-45.0, 75.1, 15.0))
    pos = np.stack([az.ravel(), el.ravel(), np.ones(az.size)], 1)
    if pole_copies:
        paz = np.arange(pole_copies) * (360.0 / pole_copies)
        pos = np.concatenate([pos, np.stack([paz, np.full(pole_copies, 90.0), np.ones(pole_copies)], 1)])
    return pos.astype(np.float32)


def random_queries(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-360.0, 360.0, n).astype(np.float32), np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n))).astype(np.float32)


def model_for(pos, az, el, radius=1.0, blend=True):
    from open_headstage_amd import lookup, scene
    q = scene._xyz(np.asarray(az, np.float32).ravel(), np.asarray(el, np.float32).ravel(), np.float32(radius))
    return lm.lookup(lookup.table_xyz(pos), q, blend), q


def judge_bracket(pos, az, el, got, what, radius=1.0, by_margin=True):
    """(idx0, idx1, w) `got` against the model under the margin rule, and the model's unclear share; -> that share"""
    from open_headstage_amd import lookup
    m, q = model_for(pos, az, el, radius)
    i0, i1, w = (np.asarray(v).reshape(-1) for v in got)
    assert (i0 == m["idx0"]).all(), what
    clear = m["o_next"] - m["o_best"] > CLEAR * m["o_best"]
    Oh = lm.chord_offset(lookup.table_xyz(pos), q, i0, i1)
    has = np.isfinite(m["o_best"])
    assert (np.abs(Oh[has] - m["o_best"][has]) <= NEAR * m["o_best"][has]).all(), what
    assert (i1[~has] == i0[~has]).all() and (lm.bits(w[~has]) == 0).all(), what
    same = (i1 == m["idx1"]) & (lm.bits(w) == lm.bits(m["w"]))
    unclear = 1.0 - clear.mean()
    print(f"{what}: {len(i0)} queries, unclear {100 * unclear:.3f} %, equal in index and w's bits {100 * same.mean():.3f} %")
    if by_margin:
        assert same[clear].all(), (what, np.flatnonzero(clear & ~same)[:8])
    return unclear


# ---- 1. the model against the helpers ------------------------------------------------------------------------------------------
def _ring_fixture_positions(sofa):
    return np.stack([sofa.position(m) for m in range(sofa.num_measurements)]).astype(np.float32)


@pytest.mark.parametrize("table", ["sphere", "ring_grid", "ring_fixture"])
def test_model_against_the_helpers(table, ring_sofa):  # noqa: F811
    from open_headstage_amd import scene, scene2
    pos = {"sphere": sphere_table, "ring_grid": ring_grid_table, "ring_fixture": lambda: _ring_fixture_positions(ring_sofa)}[table]()
    az, el = random_queries(4096, seed=len(pos))
    m, _ = model_for(pos, az, el)
    assert (m["idx0"] == scene.nearest_directions(pos, az, el)).all()
    unclear = judge_bracket(pos, az, el, (m["idx0"], m["idx1"], m["w"]), f"{table}: the model against itself")
    unclear_h = judge_bracket(pos, az, el, scene2.bracket_directions(pos, az, el), f"{table}: bracket_directions against the model")
    assert unclear == unclear_h <= MAX_UNCLEAR, unclear
    # every measurement itself: that measurement, the first other point, w = +0.0
    mm, _ = model_for(pos, pos[:, 0], pos[:, 1], pos[0, 2])
    h0, h1, hw = scene2.bracket_directions(pos, pos[:, 0], pos[:, 1], float(pos[0, 2]))
    assert (mm["idx0"] == np.arange(len(pos))).all() and (h0 == mm["idx0"]).all()
    assert (lm.bits(mm["w"]) == 0).all() and (hw == 0).all()
    assert (mm["idx1"] == h1).all() and (mm["idx1"] != mm["idx0"]).all()
    assert (mm["o_best"] == 0).all()


def test_a_duplicated_pole_is_judged_by_distance():
    """648 ring points and the pole 72 times: near-ties in a few percent of the queries, where einsum and left-to-right sums already
    disagree; the helper's chord is as near as the model's everywhere, and idx0 is the helper's"""
    from open_headstage_amd import scene, scene2
    pos = ring_grid_table(pole_copies=72)
    assert len(pos) == 720
    az, el = random_queries(4096, seed=72)
    m, _ = model_for(pos, az, el)
    assert (m["idx0"] == scene.nearest_directions(pos, az, el)).all()
    unclear = judge_bracket(pos, az, el, scene2.bracket_directions(pos, az, el), "duplicated pole", by_margin=False)
    assert unclear < 0.10, unclear
    # a query on the pole: the first copy, then the first point that is no copy of it
    mm, _ = model_for(pos, [0.0], [90.0])
    assert mm["idx0"][0] == 648 and mm["idx1"][0] == 0 and lm.bits(mm["w"])[0] == 0


# ---- 2. the pose path ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flat", [True, False])
def test_pose_path_against_rotate_sources(flat):
    from open_headstage_amd import lookup, scene
    pos = sphere_table()
    S, segs, K, radius = 4, 96, 8, 1.0
    rng = np.random.default_rng(7 + flat)
    src_az = rng.uniform(-180.0, 180.0, (S, segs, K)).astype(np.float32)
    src_el = rng.uniform(-60.0, 80.0, (S, segs, K)).astype(np.float32)
    yaw = rng.uniform(-180.0, 180.0, (S, segs)).astype(np.float32)
    pitch = np.zeros((S, segs), np.float32) if flat else rng.uniform(-40.0, 40.0, (S, segs)).astype(np.float32)
    roll = np.zeros((S, segs), np.float32) if flat else rng.uniform(-30.0, 30.0, (S, segs)).astype(np.float32)
    v, sss, sks, R, rss, S_, segs_, K_ = lookup.rows_host_half(src_az, src_el, yaw, pitch, roll, radius)
    assert (S_, segs_, K_, sss, sks, rss) == (S, segs, K, segs, 1, segs)
    q = lm.rows_queries(v, sss, sks, R, rss, S, segs, K)
    m = lm.lookup(lookup.table_xyz(pos), q.reshape(-1, 3), blend=False)
    az2, el2 = scene.rotate_sources(src_az, src_el, yaw[..., None], pitch[..., None], roll[..., None])
    want = scene.nearest_directions(pos, -az2, el2, radius).reshape(-1)
    delta = radius * 2.0 ** -20        # the chain rounds its angles to f32: a query moves by at most this
    clear = np.sqrt(m["d_next"]) - np.sqrt(m["d_best"]) > 2 * delta
    unclear = 1.0 - clear.mean()
    print(f"{'flat' if flat else 'pitch and roll'}: {clear.size} queries, unclear {100 * unclear:.4f} %, "
          f"equal {100 * (m['idx0'] == want).mean():.4f} %")
    assert (m["idx0"][clear] == want[clear]).all()
    assert unclear <= MAX_UNCLEAR, unclear
    # the flip is a negated middle column of rotate_sources' matrix, and with no pose at all R is diag(1, -1, 1)
    assert np.array_equal(lookup.pose_matrices(0.0), np.diag([1.0, -1.0, 1.0]))


def test_rows_host_half_shapes():
    from open_headstage_amd import lookup
    S, segs, K = 3, 5, 6
    az = np.zeros((S, segs, K), np.float32)
    for src, want in [(az[0, 0], (1, 0, 0)), (az[:, 0], (S, 1, 0)), (az[0], (1, 0, 1)), (az, (S, segs, 1))]:
        for yaw, rss in [(np.zeros(segs), 0), (np.zeros((S, segs)), segs)]:
            v, sss, sks, R, r, S_, segs_, K_ = lookup.rows_host_half(src, src, yaw)
            assert (sss, sks, r, segs_, K_) == (want[1], want[2], rss, segs, K), (src.shape, yaw.shape)
            assert S_ == (S if (rss or want[0] == S) else 1)
            assert v.dtype == np.float64 and R.dtype == np.float64 and v.flags.c_contiguous and R.flags.c_contiguous
    with pytest.raises(ValueError):
        lookup.rows_host_half(np.zeros((4, K)), np.zeros((4, K)), np.zeros((S, segs)))


# ---- 3. lookup_body.hpp on the host --------------------------------------------------------------------------------------------
def host_cases():
    """(xyz32 [M][3], q [n][3]) pairs: random tables of 1 .. 200 points, some with copies of points; queries anywhere, on points, on
    chord midpoints, far out and at the origin"""
    rng = np.random.default_rng(33)
    cases = []
    for i in range(40):
        M = [1, 2, 3, 63, 64, 65, 200][i % 7]
        xyz = rng.standard_normal((M, 3))
        xyz = (xyz / np.linalg.norm(xyz, axis=1, keepdims=True)).astype(np.float32)
        if i % 3 == 1 and M > 2:
            xyz[rng.integers(0, M, M // 2)] = xyz[rng.integers(0, M, M // 2)]       # copies
        if i % 5 == 4:
            xyz[:] = xyz[0]                                                         # one point M times
        P = xyz.astype(np.float64)
        a, b = rng.integers(0, M, 16), rng.integers(0, M, 16)
        q = np.concatenate([rng.standard_normal((32, 3)), P[a], (P[a] + P[b]) / 2, 10.0 * rng.standard_normal((8, 3)), np.zeros((1, 3))])
        cases.append((xyz, q))
    return cases


def test_lookup_body_on_the_host_has_the_models_bits(tmp_path):
    from open_headstage_amd import build
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc()))), "llvm", "bin", "clang++")
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "lookup_host_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tests", "lookup_host_check.cpp"), "-o", exe], check=True)
    cases = host_cases()
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.uint32(len(cases)).tobytes())
        for xyz, q in cases:
            f.write(np.array([len(xyz), len(q)], np.uint32).tobytes() + xyz.tobytes() + np.ascontiguousarray(q, np.float64).tobytes())
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    got = np.fromfile(tmp_path / "out.bin", np.uint32).reshape(-1, 3)
    assert len(got) == sum(len(q) for _, q in cases) >= 2000
    at = ties = blended = 0
    for xyz, q in cases:
        m = lm.lookup(xyz, q)
        g = got[at:at + len(q)]
        at += len(q)
        assert (g[:, 0] == m["idx0"]).all() and (g[:, 1] == m["idx1"]).all() and (g[:, 2] == lm.bits(m["w"])).all(), len(xyz)
        ties += int((m["d_next"] == m["d_best"]).sum())
        blended += int((m["w"] > 0).sum())
    assert ties > 0 and blended > 1000, (ties, blended)


# ---- 4. the surface ------------------------------------------------------------------------------------------------------------
ENTRIES = ["ohs_lookup_create", "ohs_lookup_destroy", "ohs_lookup_last_error", "ohs_lookup_last_launch", "ohs_lookup_points",
           "ohs_lookup_rows", "ohs_lookup_status_string"]


def test_header_library_and_prototypes_are_one_list_of_seven():
    from open_headstage_amd import _ffi, lookup, scene, scene2
    hdr = open(os.path.join(ROOT, "include", "ohs_lookup.h")).read()
    declared = sorted(set(re.findall(r"\b(ohs_lookup_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == ENTRIES == sorted(lookup.LOOKUP_PROTOTYPES)
    assert declared == _dynamic_symbols(os.path.join(PKG, "libohs_lookup.so"))
    emap = open(os.path.join(PKG, "csrc", "lookup_exports.map")).read()
    assert "global: ohs_lookup_*;" in emap and "local: *;" in emap
    # the other three libraries are what they were
    assert len(_dynamic_symbols(os.path.join(PKG, "libohs_hip.so"))) == 119 and len(_ffi.PROTOTYPES) == 119
    assert _dynamic_symbols(os.path.join(PKG, "libohs_scene.so")) == sorted(scene.SCENE_PROTOTYPES) and len(scene.SCENE_PROTOTYPES) == 13
    assert _dynamic_symbols(os.path.join(PKG, "libohs_scene2.so")) == sorted(scene2.SCENE2_PROTOTYPES) and len(scene2.SCENE2_PROTOTYPES) == 14
    doc = open(os.path.join(ROOT, "SCENES.md")).read()
    for name in declared:
        assert re.search(r"\bfn " + name + r"\(", doc), f"{name} is not listed in SCENES.md"
    assert "ohs_lookup_" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # it needs none of the product's code: no undefined ohs symbol, no dependency on the other libraries
    undefined = subprocess.run(["nm", "-D", "--undefined-only", os.path.join(PKG, "libohs_lookup.so")], check=True, capture_output=True,
                               text=True).stdout
    assert "ohs" not in undefined


def test_every_entry_refuses_null():
    import ctypes as C

    import open_headstage_amd as ohs
    from open_headstage_amd import _ffi, lookup
    L = lookup.lookup_lib()
    INV = _ffi.OHS_ERR_INVALID_ARG
    xyz = np.zeros(3, np.float32)
    h = C.c_void_p()
    assert L.ohs_lookup_create(0, 1, xyz.ctypes.data_as(lookup.fp), None) == INV
    assert L.ohs_lookup_create(0, 1, None, C.byref(h)) == INV and not h.value
    assert b"NULL" in L.ohs_lookup_last_error()
    assert L.ohs_lookup_create(0, 0, xyz.ctypes.data_as(lookup.fp), C.byref(h)) == INV and not h.value
    assert L.ohs_lookup_create(0, 65537, xyz.ctypes.data_as(lookup.fp), C.byref(h)) == INV and not h.value
    L.ohs_lookup_destroy(None)
    assert L.ohs_lookup_points(None, 1, None, None, None, None) == INV
    assert b"NULL" in L.ohs_lookup_last_error()
    assert L.ohs_lookup_rows(None, 1, 1, 1, None, 0, 0, None, 0, None, None, None) == INV
    assert L.ohs_lookup_last_launch(None, None, None, None) == INV
    assert L.ohs_lookup_status_string(INV) == _ffi.lib().ohs_status_string(INV)
    for s in (0, 2, 3, 6, 99):
        assert L.ohs_lookup_status_string(s) == _ffi.lib().ohs_status_string(s), s
    assert issubclass(ohs.DirectionLookupError, RuntimeError) and callable(ohs.DirectionLookup)


# ---- 5. the kernels' resources -------------------------------------------------------------------------------------------------
def test_kernel_resources():
    from open_headstage_amd import build
    res = build.resources()
    fields = ("vgprs", "agprs", "sgprs", "scratch_bytes_per_lane", "lds_bytes", "occupancy_waves_per_simd")
    # as built: no scratch, a tile of 1 024 points in f64
    assert {f: res["k_lookup<0>"][f] for f in fields} == \
        {"vgprs": 43, "agprs": 0, "sgprs": 38, "scratch_bytes_per_lane": 0, "lds_bytes": 24576, "occupancy_waves_per_simd": 6}
    assert {f: res["k_lookup<1>"][f] for f in fields} == \
        {"vgprs": 50, "agprs": 0, "sgprs": 45, "scratch_bytes_per_lane": 0, "lds_bytes": 24576, "occupancy_waves_per_simd": 6}
    assert build.is_current() and os.path.exists(build.LOOKUP_LIB)

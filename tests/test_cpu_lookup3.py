"""The three-direction lookup (libohs_lookup3.so, include/ohs_lookup3.h), the part that needs no GPU.

* tests/lookup3_model.py -- the header's arithmetic in elementwise numpy over Cartesian queries -- against scene3.triangle_directions,
  the definition of the rows: index for index and bit for bit, on closed and open meshes, on random queries, every measurement, the
  Cartesian midpoint of every edge and every centroid;
* csrc/lookup3_body.hpp compiled for the host (tests/lookup3_host_check.cpp) against the model, bit for bit, triangle index included;
* the header's names, libohs_lookup3.so's dynamic symbols and LOOKUP3_PROTOTYPES are one list of eight, every entry refuses NULL, and
  what ohs_lookup3_create refuses before it looks for a device it refuses here; the five older libraries export what they exported;
* k_lookup_tri was built without scratch and AGPRs, k_lookup keeps its figures, and the build is current."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import lookup3_model as l3
from tests.test_cpu_scene import _dynamic_symbols
from tests.test_cpu_scene_blend3 import OCTA_POS, OCTA_TRI, _cart, _sph, grid_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "open_headstage_amd")


# ---- 1. the model against the helper --------------------------------------------------------------------------------------------
def _mesh(name):
    from open_headstage_amd import lookup3, scene3
    if name == "octahedron":
        return OCTA_POS, OCTA_TRI
    if name == "grid":
        return grid_mesh()
    if name == "subdivided":
        return lookup3.octahedron_mesh(3)
    pytest.importorskip("scipy")
    rng = np.random.default_rng(1024)
    pos = np.stack([rng.uniform(0, 360, 1024), np.degrees(np.arcsin(rng.uniform(-1, 1, 1024))), np.ones(1024)], 1).astype(np.float32)
    return pos, scene3.triangulate_directions(pos)


def mesh_queries(pos, tri, n_random, seed):
    """(az, el) f32: random directions, every measurement, the Cartesian midpoint of every edge, every centroid"""
    rng = np.random.default_rng(seed)
    p = _cart(pos[:, 0], pos[:, 1])
    edges = sorted({tuple(sorted((int(t[a]), int(t[b])))) for t in tri for a, b in ((0, 1), (1, 2), (0, 2))})
    ea, eb = np.array(edges).T
    maz, mel = _sph((p[ea] + p[eb]) / 2)
    caz, cel = _sph(p[tri[:, 0]] + p[tri[:, 1]] + p[tri[:, 2]])
    az = np.concatenate([rng.uniform(-360.0, 360.0, n_random), pos[:, 0], maz, caz])
    el = np.concatenate([np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n_random))), pos[:, 1], mel, cel])
    return az.astype(np.float32), el.astype(np.float32)


@pytest.mark.parametrize("mesh,radius", [("octahedron", 1.0), ("octahedron", 2.5), ("grid", 1.0), ("grid", 2.5), ("subdivided", 1.0),
                                         ("subdivided", 2.5), ("hull", 1.0)])
def test_model_against_triangle_directions(mesh, radius):
    from open_headstage_amd import lookup, scene, scene3
    pos, tri = _mesh(mesh)
    az, el = mesh_queries(pos, tri, 3000, seed=len(tri))
    want = scene3.triangle_directions(pos, tri, az, el, radius)
    m = l3.lookup3(lookup.table_xyz(pos), tri, scene._xyz(az, el, np.float32(radius)))
    same = l3.same_rows(want, m)
    assert same.all(), (mesh, np.flatnonzero(~same)[:8])
    # the winner is the triangle the row names
    assert (np.sort(np.stack([m["idx0"], m["idx1"], m["idx2"]], 1), 1) == np.sort(tri[m["tri"]], 1)).all()
    three, on_point, on_edge = (m["w2"] > 0).sum(), (l3.bits(m["w1"]) == 0).sum(), ((l3.bits(m["w2"]) == 0) & (m["w1"] > 0)).sum()
    print(f"{mesh} at radius {radius}: {len(az)} queries over {len(tri)} triangles; w2 > 0 in {three}, w1 == +0.0 in {on_point}, "
          f"w2 == +0.0 < w1 in {on_edge}; ties for the best min(g) in {(m['m_next'] == m['m_best']).sum()}")
    assert not (l3.bits(m["w1"]) == 0x80000000).any() and not (l3.bits(m["w2"]) == 0x80000000).any()
    if mesh in ("grid", "subdivided"):
        assert three >= 1000 and on_point >= 100 and on_edge >= 100, (three, on_point, on_edge)
    if mesh == "grid":          # an open mesh: some random queries stand outside every triangle
        assert (m["m_best"] < 0).sum() >= 100


# ---- 2. lookup3_body.hpp on the host ---------------------------------------------------------------------------------------------
def host_cases():
    """(xyz32 [M][3], tris [T][3], q [n][3]) triples: random soups of 1 .. 300 overlapping triangles, some with triangles stored again
    (corners rotated); two real meshes; one triangle alone with queries behind it; every set of queries ends at the origin"""
    from open_headstage_amd import lookup, lookup3
    rng = np.random.default_rng(35)
    cases = []
    for i, T in enumerate([1, 2, 3, 63, 64, 65, 300] * 3):
        xyz, tris = l3.random_soup(max(3, min(40, 3 * T)), T, seed=100 + i)
        if i % 3 == 1 and T > 2:
            tris[rng.integers(0, T, T // 3)] = np.roll(tris[rng.integers(0, T, T // 3)], 1, axis=1)     # copies, corners rotated
        cases.append((xyz, tris, l3.soup_queries(xyz, tris, 120, seed=i)))
    for pos, tri in (grid_mesh(), lookup3.octahedron_mesh(2)):
        xyz = lookup.table_xyz(pos)
        cases.append((xyz, tri, l3.soup_queries(xyz, tri, 600, seed=len(tri))))
    xyz = lookup.table_xyz(OCTA_POS)
    behind = -np.abs(rng.standard_normal((64, 3)))          # the triangle (0, 1, 4) spans the octant x, y, z >= 0
    cases.append((xyz, OCTA_TRI[:1], np.concatenate([behind, np.zeros((1, 3))])))
    return cases


def test_lookup3_body_on_the_host_has_the_models_bits(tmp_path):
    from open_headstage_amd import build
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc()))), "llvm", "bin", "clang++")
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "lookup3_host_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tests", "lookup3_host_check.cpp"), "-o", exe], check=True)
    cases = host_cases()
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.uint32(len(cases)).tobytes())
        for xyz, tris, q in cases:
            f.write(np.array([len(xyz), len(tris), len(q)], np.uint32).tobytes() + xyz.tobytes() + np.ascontiguousarray(tris, np.uint32).tobytes() +
                    np.ascontiguousarray(q, np.float64).tobytes())
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    got = np.fromfile(tmp_path / "out.bin", np.uint32).reshape(-1, 6)
    assert len(got) == sum(len(q) for _, _, q in cases) >= 3000
    at = ties = three = fallback = 0
    for xyz, tris, q in cases:
        m = l3.lookup3(xyz, tris, q)
        g = got[at:at + len(q)]
        at += len(q)
        same = l3.same_rows([g[:, 0], g[:, 1], g[:, 2], g[:, 3].view(np.float32), g[:, 4].view(np.float32)], m)
        assert same.all() and (g[:, 5] == m["tri"]).all(), (len(tris), np.flatnonzero(~same)[:8])
        ties += int((m["m_next"] == m["m_best"]).sum())
        three += int((m["w2"] > 0).sum())
        fallback += int((m["m_best"] <= 0).sum())
    assert ties > 100 and three > 1000 and fallback > 64, (ties, three, fallback)
    # the last case: behind the only triangle every gain is negative and one corner takes it all; at the origin corner 0 does
    assert (l3.bits(m["w1"]) == 0).all() and (l3.bits(m["w2"]) == 0).all() and m["idx0"][-1] == 0


def test_the_model_marks_singular_triangles():
    """three directions in one plane through the origin, and a triangle naming a point twice (ohs_lookup3_create's refusals are
    below)"""
    from open_headstage_amd import lookup
    xyz = lookup.table_xyz(OCTA_POS)
    for flat in ([0, 2, 1], [0, 0, 4]):
        assert l3.inverses(xyz, [flat])[1].all()
    assert not l3.inverses(xyz, OCTA_TRI)[1].any()


# ---- 3. the surface ------------------------------------------------------------------------------------------------------------
ENTRIES = ["ohs_lookup3_create", "ohs_lookup3_destroy", "ohs_lookup3_last_error", "ohs_lookup3_last_launch", "ohs_lookup3_mesh",
           "ohs_lookup3_points", "ohs_lookup3_rows", "ohs_lookup3_status_string"]


def test_header_library_and_prototypes_are_one_list_of_eight():
    from open_headstage_amd import _ffi, lookup, lookup3, scene, scene2, scene3
    hdr = open(os.path.join(ROOT, "include", "ohs_lookup3.h")).read()
    declared = sorted(set(re.findall(r"\b(ohs_lookup3_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == ENTRIES == sorted(lookup3.LOOKUP3_PROTOTYPES)
    assert declared == _dynamic_symbols(os.path.join(PKG, "libohs_lookup3.so"))
    emap = open(os.path.join(PKG, "csrc", "lookup3_exports.map")).read()
    assert "global: ohs_lookup3_*;" in emap and "local: *;" in emap
    # the five older libraries are what they were
    assert len(_dynamic_symbols(os.path.join(PKG, "libohs_hip.so"))) == 119 and len(_ffi.PROTOTYPES) == 119
    assert _dynamic_symbols(os.path.join(PKG, "libohs_scene.so")) == sorted(scene.SCENE_PROTOTYPES) and len(scene.SCENE_PROTOTYPES) == 13
    assert _dynamic_symbols(os.path.join(PKG, "libohs_scene2.so")) == sorted(scene2.SCENE2_PROTOTYPES) and len(scene2.SCENE2_PROTOTYPES) == 14
    assert _dynamic_symbols(os.path.join(PKG, "libohs_scene3.so")) == sorted(scene3.SCENE3_PROTOTYPES) and len(scene3.SCENE3_PROTOTYPES) == 15
    assert _dynamic_symbols(os.path.join(PKG, "libohs_lookup.so")) == sorted(lookup.LOOKUP_PROTOTYPES) and len(lookup.LOOKUP_PROTOTYPES) == 7
    doc = open(os.path.join(ROOT, "SCENES.md")).read()
    for name in declared:
        assert re.search(r"\bfn " + name + r"\(", doc), f"{name} is not listed in SCENES.md"
    assert "ohs_lookup3_" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # it needs none of the product's code and none of libohs_lookup.so's: no undefined ohs symbol
    undefined = subprocess.run(["nm", "-D", "--undefined-only", os.path.join(PKG, "libohs_lookup3.so")], check=True, capture_output=True,
                               text=True).stdout
    assert "ohs" not in undefined


def test_every_entry_refuses_null_and_create_refuses_a_bad_mesh():
    import open_headstage_amd as ohs
    from open_headstage_amd import _ffi, lookup, lookup3
    L = lookup3.lookup3_lib()
    INV = _ffi.OHS_ERR_INVALID_ARG
    fp, u32p = lookup.fp, lookup.u32p
    xyz = lookup.table_xyz(OCTA_POS)
    tri = np.ascontiguousarray(OCTA_TRI, np.uint32)
    h = C.c_void_p()

    def create(n_dirs, x, n_tris, t, out=h):
        return L.ohs_lookup3_create(0, n_dirs, None if x is None else x.ctypes.data_as(fp), n_tris, None if t is None else t.ctypes.data_as(u32p),
                                    None if out is None else C.byref(out))
    assert create(6, xyz, 8, tri, None) == INV
    for args in ((6, None, 8, tri), (6, xyz, 8, None)):
        assert create(*args) == INV and not h.value and b"NULL" in L.ohs_lookup3_last_error()
    for args in ((0, xyz, 8, tri), (65537, xyz, 8, tri), (6, xyz, 0, tri), (6, xyz, 131073, tri)):
        assert create(*args) == INV and not h.value and b"outside" in L.ohs_lookup3_last_error()
    bad = xyz.copy()
    bad[3, 1] = np.inf
    assert create(6, bad, 8, tri) == INV and b"xyz[10] is not finite" in L.ohs_lookup3_last_error()
    assert create(5, xyz, 8, tri) == INV and b"triangle 4 names direction 5 of 5" in L.ohs_lookup3_last_error()
    flat = np.concatenate([tri[:2], np.array([[0, 2, 1]], np.uint32), np.array([[1, 1, 4]], np.uint32)])
    assert create(6, xyz, 4, flat) == INV and not h.value
    assert b"triangle 2 (0, 2, 1) is singular" in L.ohs_lookup3_last_error()
    L.ohs_lookup3_destroy(None)
    assert L.ohs_lookup3_points(None, 1, None, None, None, None, None, None, None) == INV and b"NULL" in L.ohs_lookup3_last_error()
    assert L.ohs_lookup3_rows(None, 1, 1, 1, None, 0, 0, None, 0, None, None, None, None, None, None) == INV
    assert L.ohs_lookup3_last_launch(None, None, None, None) == INV
    assert L.ohs_lookup3_mesh(None, None, None) == INV
    for s in (0, 1, 2, 3, 6, 99):
        assert L.ohs_lookup3_status_string(s) == _ffi.lib().ohs_status_string(s), s
    assert issubclass(ohs.TriangleLookupError, RuntimeError) and callable(ohs.TriangleLookup)
    with pytest.raises(ValueError):
        ohs.TriangleLookup(OCTA_POS, np.array([[0, 1, 6]], np.uint32))


def test_octahedron_mesh():
    from open_headstage_amd import lookup, lookup3
    for levels, M, T in ((0, 6, 8), (3, 258, 512), (4, 1026, 2048)):
        pos, tri = lookup3.octahedron_mesh(levels)
        assert pos.shape == (M, 3) and tri.shape == (T, 3) and pos.dtype == np.float32 and tri.dtype == np.uint32
        assert not l3.inverses(lookup.table_xyz(pos), tri)[1].any()
        edges = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [0, 2]]]), 1)
        assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()       # closed: every edge has two triangles


# ---- 4. the kernels' resources -------------------------------------------------------------------------------------------------
def test_kernel_resources():
    from open_headstage_amd import build
    res = build.resources()
    fields = ("vgprs", "agprs", "sgprs", "scratch_bytes_per_lane", "lds_bytes", "occupancy_waves_per_simd")
    k = res["k_lookup_tri"]
    assert k["scratch_bytes_per_lane"] == 0 and k["agprs"] == 0, k
    # as built: a tile of 256 triangles' inverses in f64
    assert {f: k[f] for f in fields} == \
        {"vgprs": 94, "agprs": 0, "sgprs": 53, "scratch_bytes_per_lane": 0, "lds_bytes": 18432, "occupancy_waves_per_simd": 5}
    src = open(os.path.join(PKG, "csrc", "lookup3_kernels.hip")).read() + open(os.path.join(PKG, "csrc", "lookup3_body.hpp")).read()
    assert "asm" not in src
    # the two-direction lookup's kernels are what tests/test_cpu_lookup.py pins
    assert {f: res["k_lookup<0>"][f] for f in fields} == \
        {"vgprs": 43, "agprs": 0, "sgprs": 38, "scratch_bytes_per_lane": 0, "lds_bytes": 24576, "occupancy_waves_per_simd": 6}
    assert {f: res["k_lookup<1>"][f] for f in fields} == \
        {"vgprs": 50, "agprs": 0, "sgprs": 45, "scratch_bytes_per_lane": 0, "lds_bytes": 24576, "occupancy_waves_per_simd": 6}
    assert build.is_current() and os.path.exists(build.LOOKUP3_LIB)
    assert os.path.basename(build.LOOKUP3_LIB) == "libohs_lookup3.so" and len(build.LOOKUP3_UNITS) == 2
    assert all("-ffp-contract=off" in flags for _, flags in build.LOOKUP3_UNITS)

"""The pruned three-direction lookup (libohs_lookup3p.so, include/ohs_lookup3p.h), the part that needs no GPU.

* the header's names, csrc/lookup3p_exports.map, LOOKUP3P_PROTOTYPES and the library's dynamic symbols are one list of nine; the
  library has no undefined ohs symbol; the six older libraries export what they exported;
* every entry refuses NULL, ohs_lookup3p_create refuses a bad mesh in ohs_lookup3_create's words and a grid of 257;
* k_lookup_tri_cells and k_lookup_tri_rest were built without scratch and AGPRs, without inline assembly, with -ffp-contract=off;
* csrc/lookup3p_body.hpp compiled for the host (tests/lookup3p_host_check.cpp): the index it builds and the answers of pass 1, the
  certificate and pass 2 against tests/lookup3p_model.py and tests/lookup3_model.py -- (1) rows, tri and the fallback flags for every
  query, (2) every list strictly ascending and every triangle on one, (3) for every query strictly inside a triangle, the model's
  winner on the query's lists: the conservative property itself;
* the same program once more under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import lookup3_model as l3
from tests import lookup3p_model as l3p
from tests.test_cpu_scene import _dynamic_symbols
from tests.test_cpu_scene_blend3 import OCTA_POS, OCTA_TRI, grid_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "open_headstage_amd")
GRIDS = (1, 2, 3, 7, 16, 0)


# ---- meshes and queries (tests/test_gpu_lookup3p.py uses them too) ------------------------------------------------------------------
def needle_mesh():
    """the octahedron and a seventh point just off the great circle through points 0 and 1: the triangle (0, 1, 6) has |det| = 1.4e-8
    |a| |b| |c|, just above create's 1e-9 line; its inverse's entries are near 1e8 and set B"""
    from open_headstage_amd import lookup
    xyz = np.concatenate([lookup.table_xyz(OCTA_POS), np.array([[np.sqrt(0.5), np.sqrt(0.5), 1.4e-8]], np.float32)])
    tris = np.concatenate([OCTA_TRI, np.array([[0, 1, 6]], np.uint32)]).astype(np.uint32)
    inv, singular = l3.inverses(xyz, tris)
    assert not singular.any() and 1e7 < np.abs(inv[-1]).max() < 1e9
    return xyz, np.ascontiguousarray(tris)


def meshes():
    """name -> (xyz32 [M][3], tris [T][3] uint32)"""
    from open_headstage_amd import lookup, lookup3
    out = {}
    for level in (0, 1, 3, 5):
        pos, tri = lookup3.octahedron_mesh(level)
        out[f"octahedron{level}"] = (lookup.table_xyz(pos), tri)
    pos, tri = grid_mesh()
    out["open_grid"] = (lookup.table_xyz(pos), np.ascontiguousarray(tri, np.uint32))
    out["soup40"] = l3.random_soup(40, 300, seed=40300)
    out["soup12"] = l3.random_soup(12, 64, seed=1264)
    xyz, tri = out["octahedron3"]
    out["twice"] = (xyz, np.ascontiguousarray(np.repeat(tri, 2, axis=0)))          # every triangle stored twice, side by side
    out["needle"] = needle_mesh()
    return out


def seam_queries(G, seed):
    """the cube map's seams at grid G: |q0| = |q1| and |q0| = |q1| = |q2| in every sign, the six axes, u or v exactly on a cell
    boundary on every face, coordinates of -0.0, and directions at radii of 1e-40 (a subnormal in f32), 1e-30 and 1e15"""
    rng = np.random.default_rng(seed)
    q = []
    signs = [(a, b, c) for a in (1.0, -1.0) for b in (1.0, -1.0) for c in (1.0, -1.0)]
    for s in signs:
        q.append(s)
        for w in (0.3, -0.0, 0.999):
            q += [(s[0], s[1], w * s[2]), (s[0], w * s[1], s[2]), (w * s[0], s[1], s[2])]
    for axis in range(3):
        for sign in (1.0, -1.0):
            e = [0.0, 0.0, 0.0]
            e[axis] = sign
            q.append(tuple(e))
            e = [-0.0, -0.0, -0.0]
            e[axis] = sign * 2.5
            q.append(tuple(e))
            for k in range(G + 1):
                uk = 2.0 * k / G - 1.0
                for other in (0.123, -0.77, uk):
                    for radius in (1.0, 0.75):
                        p = [0.0, 0.0, 0.0]
                        p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = sign * radius, uk * radius, other * radius
                        q.append(tuple(p))
                        p[(axis + 1) % 3], p[(axis + 2) % 3] = other * radius, uk * radius
                        q.append(tuple(p))
    q.append((-0.0, -0.0, -0.0))
    r = rng.standard_normal((36, 3))
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    q = np.concatenate([np.array(q, np.float64), r[:12] * 1e-40, r[12:24] * 1e-30, r[24:] * 1e15])
    assert np.abs(q).max() <= 1e15
    return np.ascontiguousarray(q)


def mixed_queries(xyz, tris, G, n, seed):
    """lookup3_model.soup_queries (random directions, on points, on edge midpoints, on centroids, the origin) and the seams of grid G
    (0: the library's choice for this mesh)"""
    return np.ascontiguousarray(np.concatenate([l3.soup_queries(xyz, tris, n, seed), seam_queries(G or l3p.choose_grid(len(tris)), seed + 1)]))


def widest_grid_case():
    """the level-6 octahedron mesh (32 768 triangles) at grid = 256, the widest: about 1 000 queries -- 400 of mixed_queries and a
    seeded sample of 600 of the 18 500 seams of that grid -> (xyz, tris, q, 256).  tests/test_gpu_lookup_chunks.py runs the same on
    the device."""
    from open_headstage_amd import lookup, lookup3
    pos, tris = lookup3.octahedron_mesh(6)
    xyz = lookup.table_xyz(pos)
    seams = seam_queries(256, seed=257)
    pick = np.sort(np.random.default_rng(256).choice(len(seams), 600, replace=False))
    q = np.concatenate([mixed_queries(xyz, tris, 256, 400, seed=6)[:400], seams[pick]])
    return xyz, tris, np.ascontiguousarray(q), 256


# ---- 1. the surface --------------------------------------------------------------------------------------------------------------
ENTRIES = ["ohs_lookup3p_create", "ohs_lookup3p_destroy", "ohs_lookup3p_index", "ohs_lookup3p_last_error", "ohs_lookup3p_last_launch",
           "ohs_lookup3p_mesh", "ohs_lookup3p_points", "ohs_lookup3p_rows", "ohs_lookup3p_status_string"]


def test_header_map_prototypes_and_library_are_one_list_of_nine():
    from open_headstage_amd import _ffi, lookup, lookup3, lookup3p, scene, scene2, scene3
    hdr = open(os.path.join(ROOT, "include", "ohs_lookup3p.h")).read()
    declared = sorted(set(re.findall(r"\b(ohs_lookup3p_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == ENTRIES == sorted(lookup3p.LOOKUP3P_PROTOTYPES) and len(declared) == 9
    lib = os.path.join(PKG, "libohs_lookup3p.so")
    assert declared == _dynamic_symbols(lib)
    emap = open(os.path.join(PKG, "csrc", "lookup3p_exports.map")).read()
    assert "global: ohs_lookup3p_*;" in emap and "local: *;" in emap
    undefined = subprocess.run(["nm", "-D", "--undefined-only", lib], check=True, capture_output=True, text=True).stdout
    assert "ohs" not in undefined
    # the six older libraries are what they were
    assert len(_dynamic_symbols(os.path.join(PKG, "libohs_hip.so"))) == 119 and len(_ffi.PROTOTYPES) == 119
    assert _dynamic_symbols(os.path.join(PKG, "libohs_scene.so")) == sorted(scene.SCENE_PROTOTYPES) and len(scene.SCENE_PROTOTYPES) == 13
    assert _dynamic_symbols(os.path.join(PKG, "libohs_scene2.so")) == sorted(scene2.SCENE2_PROTOTYPES) and len(scene2.SCENE2_PROTOTYPES) == 14
    assert _dynamic_symbols(os.path.join(PKG, "libohs_scene3.so")) == sorted(scene3.SCENE3_PROTOTYPES) and len(scene3.SCENE3_PROTOTYPES) == 15
    assert _dynamic_symbols(os.path.join(PKG, "libohs_lookup.so")) == sorted(lookup.LOOKUP_PROTOTYPES) and len(lookup.LOOKUP_PROTOTYPES) == 7
    assert _dynamic_symbols(os.path.join(PKG, "libohs_lookup3.so")) == sorted(lookup3.LOOKUP3_PROTOTYPES) and len(lookup3.LOOKUP3_PROTOTYPES) == 8
    doc = open(os.path.join(ROOT, "SCENES.md")).read()
    for name in declared:
        assert re.search(r"\bfn " + name + r"\(", doc), f"{name} is not listed in SCENES.md"
    assert "ohs_lookup3p_" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_every_entry_refuses_null_and_create_refuses_a_bad_mesh_and_a_grid_of_257():
    import open_headstage_amd as ohs
    from open_headstage_amd import _ffi, lookup, lookup3, lookup3p
    L, L3 = lookup3p.lookup3p_lib(), lookup3.lookup3_lib()
    INV = _ffi.OHS_ERR_INVALID_ARG
    fp, u32p = lookup.fp, lookup.u32p
    xyz = lookup.table_xyz(OCTA_POS)
    tri = np.ascontiguousarray(OCTA_TRI, np.uint32)
    h, h3 = C.c_void_p(), C.c_void_p()

    def create(n_dirs, x, n_tris, t, out=h, grid=0):
        return L.ohs_lookup3p_create(0, n_dirs, None if x is None else x.ctypes.data_as(fp), n_tris, None if t is None else t.ctypes.data_as(u32p),
                                     grid, None if out is None else C.byref(out))

    def create3(n_dirs, x, n_tris, t):
        return L3.ohs_lookup3_create(0, n_dirs, None if x is None else x.ctypes.data_as(fp), n_tris, None if t is None else t.ctypes.data_as(u32p),
                                     C.byref(h3))
    assert create(6, xyz, 8, tri, None) == INV and b"out is NULL" in L.ohs_lookup3p_last_error()
    bad = xyz.copy()
    bad[3, 1] = np.inf
    flat = np.concatenate([tri[:2], np.array([[0, 2, 1]], np.uint32), np.array([[1, 1, 4]], np.uint32)])
    for args, text in (((6, None, 8, tri), b"NULL"), ((6, xyz, 8, None), b"NULL"), ((0, xyz, 8, tri), b"outside"), ((65537, xyz, 8, tri), b"outside"),
                       ((6, xyz, 0, tri), b"outside"), ((6, xyz, 131073, tri), b"outside"), ((6, bad, 8, tri), b"xyz[10] is not finite"),
                       ((5, xyz, 8, tri), b"triangle 4 names direction 5 of 5"), ((6, xyz, 4, flat), b"triangle 2 (0, 2, 1) is singular")):
        assert create(*args) == INV and not h.value and text in L.ohs_lookup3p_last_error(), args
        assert create3(*args) == INV and L3.ohs_lookup3_last_error() == L.ohs_lookup3p_last_error()         # the same words
    for grid in (257, 1 << 20):
        assert create(6, xyz, 8, tri, grid=grid) == INV and not h.value and f"grid {grid} is outside 0 .. 256".encode() in L.ohs_lookup3p_last_error()
    L.ohs_lookup3p_destroy(None)
    assert L.ohs_lookup3p_points(None, 1, None, None, None, None, None, None, None) == INV and b"NULL" in L.ohs_lookup3p_last_error()
    assert L.ohs_lookup3p_rows(None, 1, 1, 1, None, 0, 0, None, 0, None, None, None, None, None, None) == INV
    assert L.ohs_lookup3p_last_launch(None, None, None, None) == INV
    assert L.ohs_lookup3p_index(None, None, None, None, None, None) == INV
    assert L.ohs_lookup3p_mesh(None, None, None) == INV
    for s in (0, 1, 2, 3, 6, 99):
        assert L.ohs_lookup3p_status_string(s) == _ffi.lib().ohs_status_string(s), s
    assert issubclass(ohs.PrunedTriangleLookupError, RuntimeError) and callable(ohs.PrunedTriangleLookup)
    assert not issubclass(ohs.PrunedTriangleLookupError, ohs.TriangleLookupError)
    assert "PrunedTriangleLookup" in ohs.__all__ and "PrunedTriangleLookupError" in ohs.__all__
    for name in ("points", "triangle", "rows", "mesh", "index", "last_launch"):
        assert callable(getattr(ohs.PrunedTriangleLookup, name)), name
    with pytest.raises(ValueError):
        ohs.PrunedTriangleLookup(OCTA_POS, np.array([[0, 1, 6]], np.uint32))
    with pytest.raises(ValueError):
        ohs.PrunedTriangleLookup(OCTA_POS, OCTA_TRI, grid=257)


# ---- 2. the kernels' resources -----------------------------------------------------------------------------------------------------
def test_kernel_resources():
    from open_headstage_amd import build
    res = build.resources()
    fields = ("vgprs", "agprs", "sgprs", "scratch_bytes_per_lane", "lds_bytes", "occupancy_waves_per_simd")
    for name in ("k_lookup_tri_cells", "k_lookup_tri_rest"):
        assert res[name]["scratch_bytes_per_lane"] == 0 and res[name]["agprs"] == 0, (name, res[name])
    # as built: pass 1 gathers from global memory and holds no LDS; pass 2 stages 256 triangles' inverses in rows of ten f64
    assert {f: res["k_lookup_tri_cells"][f] for f in fields} == \
        {"vgprs": 42, "agprs": 0, "sgprs": 66, "scratch_bytes_per_lane": 0, "lds_bytes": 0, "occupancy_waves_per_simd": 8}
    assert {f: res["k_lookup_tri_rest"][f] for f in fields} == \
        {"vgprs": 89, "agprs": 0, "sgprs": 55, "scratch_bytes_per_lane": 0, "lds_bytes": 20480, "occupancy_waves_per_simd": 5}
    for f in ("lookup3p_kernels.hip", "api_lookup3p.hip", "lookup3p_body.hpp", "lookup3p_internal.h"):
        assert "asm" not in open(os.path.join(PKG, "csrc", f)).read(), f
    assert build.is_current() and os.path.exists(build.LOOKUP3P_LIB)
    assert os.path.basename(build.LOOKUP3P_LIB) == "libohs_lookup3p.so" and len(build.LOOKUP3P_UNITS) == 2
    assert all("-ffp-contract=off" in flags for _, flags in build.LOOKUP3P_UNITS)
    assert not {u for u, _ in build.LOOKUP3P_UNITS} & {u for u, _ in build.LOOKUP3_UNITS + build.LOOKUP_UNITS + build._units()}
    # the units depend on the two older bodies as they are, and the product's units on none of the new headers
    deps = [os.path.basename(d) for d in build._deps("lookup3p_kernels.hip")]
    assert {"lookup3p_body.hpp", "lookup3p_internal.h", "lookup3_body.hpp", "lookup_body.hpp", "ohs_lookup3p.h"} <= set(deps)
    assert not {"lookup3p_body.hpp", "lookup3p_internal.h"} & {os.path.basename(d) for d in build._deps("api_core.hip")}


# ---- 3. lookup3p_body.hpp on the host ------------------------------------------------------------------------------------------------
def _cxx():
    from open_headstage_amd import build
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc()))), "llvm", "bin", "clang++")
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx, "no host C++ compiler"
    return cxx


def _compile(exe, extra=()):
    return subprocess.run([_cxx(), "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-I", os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tests", "lookup3p_host_check.cpp"), "-o", exe], capture_output=True, text=True)


def _run(exe, cases, tmp_path, env=None):
    """cases: (xyz, tris, q, grid) -> per case dict(G, everywhere, cell_start, cell_tris, rows [n][8] uint32)"""
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.uint32(len(cases)).tobytes())
        for xyz, tris, q, grid in cases:
            f.write(np.array([len(xyz), len(tris), len(q), grid], np.uint32).tobytes() + np.ascontiguousarray(xyz, np.float32).tobytes() +
                    np.ascontiguousarray(tris, np.uint32).tobytes() + np.ascontiguousarray(q, np.float64).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = np.fromfile(tmp_path / "out.bin", np.uint32)
    out, at = [], 0
    for xyz, tris, q, grid in cases:
        G, cells, E = (int(v) for v in got[at:at + 3])
        at += 3
        every = got[at:at + E]
        at += E
        start = got[at:at + cells + 1]
        at += cells + 1
        ctris = got[at:at + int(start[-1])]
        at += int(start[-1])
        rows = got[at:at + 8 * len(q)].reshape(-1, 8)
        at += 8 * len(q)
        out.append(dict(G=G, cells=cells, everywhere=every, cell_start=start, cell_tris=ctris, rows=rows))
    assert at == len(got)
    return out


def _hold_to_the_model(case, got, what):
    """the three checks; -> (queries, fallbacks, candidates walked by pass 1)"""
    xyz, tris, q, grid = case
    T = len(tris)
    m = l3.lookup3(xyz, tris, q)
    g = got["rows"]
    G = got["G"]
    assert G == (grid or l3p.choose_grid(T)) and got["cells"] == 6 * G * G, what
    # (1) rows, tri and the fallback flags, for every query
    same = l3.same_rows([g[:, 0], g[:, 1], g[:, 2], g[:, 3].view(np.float32), g[:, 4].view(np.float32)], m)
    assert same.all() and (g[:, 5] == m["tri"]).all(), (what, np.flatnonzero(~same | (g[:, 5] != m["tri"]))[:8])
    want_rest = l3p.falls_back(xyz, tris, q, m)
    assert (g[:, 6] == want_rest).all(), (what, np.flatnonzero(g[:, 6] != want_rest)[:8])
    cells = l3p.cell(q, G)
    assert (g[:, 7] == cells).all(), (what, np.flatnonzero(g[:, 7] != cells)[:8])
    # (2) every list strictly ascending, every triangle on at least one
    start, ctris, every = got["cell_start"].astype(np.int64), got["cell_tris"].astype(np.int64), got["everywhere"].astype(np.int64)
    assert start[0] == 0 and (np.diff(start) >= 0).all() and start[-1] == len(ctris), what
    inner = np.ones(len(ctris), bool)
    inner[start[:-1][start[:-1] < len(ctris)]] = False             # (the first entry of each list has no predecessor in it)
    assert (np.diff(ctris)[inner[1:]] > 0).all() and (np.diff(every) > 0).all(), what
    assert (ctris < T).all() and (every < T).all() and not np.intersect1d(ctris, every).size, what
    assert np.array_equal(np.union1d(ctris, every), np.arange(T)), what
    # (3) the conservative property: a query strictly inside a triangle finds the model's winner on its lists
    on_every = np.zeros(T, bool)
    on_every[every] = True
    walked = 0
    for i in np.flatnonzero(m["m_best"] > 0):
        mine = ctris[start[cells[i]]:start[cells[i] + 1]]
        assert on_every[m["tri"][i]] or m["tri"][i] in mine, (what, i, q[i], int(m["tri"][i]), int(cells[i]))
    walked = int((start[cells.astype(np.int64) + 1] - start[cells.astype(np.int64)]).sum()) + len(every) * len(q)
    return len(q), int(want_rest.sum()), walked


@pytest.fixture(scope="module")
def host_cases():
    cases, names = [], []
    for name, (xyz, tris) in meshes().items():
        for G in GRIDS:
            cases.append((xyz, tris, mixed_queries(xyz, tris, G, 360, seed=len(tris) + G), G))
            names.append(f"{name} at G = {G}")
    return cases, names


def test_lookup3p_body_on_the_host(tmp_path, host_cases):
    cases, names = host_cases
    exe = str(tmp_path / "lookup3p_host_check")
    r = _compile(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    got = _run(exe, cases, tmp_path)
    assert len(cases) == 9 * 6
    total = rest = 0
    for case, g, name in zip(cases, got, names):
        n, fb, walked = _hold_to_the_model(case, g, name)
        total, rest = total + n, rest + fb
        print(f"{name}: {len(case[1])} triangles, G = {g['G']}, {len(g['cell_tris'])} entries, longest list {int(np.diff(g['cell_start']).max())}, "
              f"everywhere {len(g['everywhere'])}; {n} queries, {fb} to pass 2, {walked / n:.1f} candidates per query in pass 1")
    assert total > 20000 and 0 < rest < total
    by_name = dict(zip(names, got))
    # about half of a random soup's triangles have no cap below 90 degrees; a closed mesh of small triangles has none such
    for name, T in (("soup40 at G = 3", 300), ("soup12 at G = 3", 64)):
        assert 0.25 * T < len(by_name[name]["everywhere"]) < 0.75 * T, (name, len(by_name[name]["everywhere"]))
    assert len(by_name["octahedron5 at G = 0"]["everywhere"]) == 0 and by_name["octahedron5 at G = 0"]["G"] == 37
    assert len(by_name["octahedron0 at G = 16"]["everywhere"]) == 8       # (each cap would touch more than 64 cells)


def test_the_widest_grid_on_the_host(tmp_path):
    """level 6 at G = 256, one case more for the host program: the three checks of _hold_to_the_model, the conservative property
    included, where some triangles lie on the everywhere list and the others in cell lists"""
    exe = str(tmp_path / "lookup3p_host_check")
    assert _compile(exe).returncode == 0
    case = widest_grid_case()
    assert len(case[1]) == 32768 and len(case[2]) == 1000
    got, = _run(exe, [case], tmp_path)
    n, fb, walked = _hold_to_the_model(case, got, "level 6 at G = 256")
    entries, everywhere, longest = len(got["cell_tris"]), len(got["everywhere"]), int(np.diff(got["cell_start"]).max())
    print(f"level 6 at G = 256: {entries} entries, longest list {longest}, everywhere {everywhere}; {n} queries, {fb} to pass 2, "
          f"{walked / n:.1f} candidates per query in pass 1")
    assert got["G"] == 256 and (everywhere, entries, longest) == (6728, 953688, 8)         # as built: both lists are walked, merged
    assert 0 < fb < n


def test_the_fallback_set_is_the_same_at_every_grid(tmp_path):
    """one set of queries per mesh at every G: rows, tri and flags equal across grids, not only equal to the model"""
    exe = str(tmp_path / "lookup3p_host_check")
    assert _compile(exe).returncode == 0
    cases = []
    for name, (xyz, tris) in meshes().items():
        if name in ("octahedron3", "soup40", "needle", "open_grid"):
            q = mixed_queries(xyz, tris, 7, 300, seed=7)
            cases += [(xyz, tris, q, G) for G in GRIDS]
    got = _run(exe, cases, tmp_path)
    for i in range(0, len(cases), len(GRIDS)):
        for g in got[i + 1:i + len(GRIDS)]:
            assert np.array_equal(g["rows"][:, :7], got[i]["rows"][:, :7])
        assert 0 < got[i]["rows"][:, 6].sum() < len(got[i]["rows"])


def test_the_host_program_under_the_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined, on the level-3 mesh and the two soups.  A stand-alone program: nothing
    is preloaded and Python loads none of it.  Skips where the sanitizers' runtime is not installed."""
    exe = str(tmp_path / "lookup3p_host_check_san")
    r = _compile(exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))
    if r.returncode != 0:
        pytest.skip("the address / undefined-behaviour sanitizers' runtime is not installed: " + r.stderr.strip()[-200:])
    all_meshes = meshes()
    cases = []
    for name in ("octahedron3", "soup40", "soup12"):
        xyz, tris = all_meshes[name]
        for G in (1, 7, 0):
            cases.append((xyz, tris, mixed_queries(xyz, tris, G, 200, seed=G), G))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    got = _run(exe, cases, tmp_path, env=env)
    for case, g in zip(cases, got):
        _hold_to_the_model(case, g, "under the sanitizers")

"""The tracked scene call (libohs_tracked.so, include/ohs_tracked.h), the part that needs no GPU.

* the header's names, csrc/tracked_exports.map, TRACKED_PROTOTYPES and the library's dynamic symbols are one list of fourteen; the
  library has no undefined ohs symbol; the seven older libraries export what they exported;
* every entry refuses NULL, ohs_tracked_create refuses a bad mesh in ohs_lookup3p_create's words;
* k_scene_rows_seal was built without scratch, AGPRs or LDS and without inline assembly, the scene kernels' figures are where they were;
* csrc/scene_rows_body.hpp compiled for the host (tests/scene_rows_host_check.cpp) against tests/tracked_model.py: the planes in front
  of the call under FRESH and CARRY, the carry and the three counts, on random rows at K = 1, 2, 5, 63, 64, one and three segments, a
  ragged last segment, weights of +0.0 in every combination; the model's two restatements -- the elementwise one and the host scan of
  api_batch.hip -- against each other;
* three mutants of the header, each caught;
* the same program once more under the address and undefined-behaviour sanitizers."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import tracked_model as tm
from tests.test_cpu_scene import _dynamic_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "open_headstage_amd")
BODY = os.path.join(PKG, "csrc", "scene_rows_body.hpp")

ENTRIES = ["ohs_tracked_create", "ohs_tracked_destroy", "ohs_tracked_last_error", "ohs_tracked_last_launch", "ohs_tracked_process",
           "ohs_tracked_reset", "ohs_tracked_rows", "ohs_tracked_set_direction_irs", "ohs_tracked_set_eq_band_coeffs",
           "ohs_tracked_set_eq_enabled", "ohs_tracked_set_flush_denormals", "ohs_tracked_set_gain", "ohs_tracked_status_string",
           "ohs_tracked_sync"]


# ---- 1. the surface --------------------------------------------------------------------------------------------------------------
def test_header_map_prototypes_and_library_are_one_list_of_fourteen():
    from open_headstage_amd import _ffi, lookup, lookup3, lookup3p, scene, scene2, scene3, tracked
    hdr = open(os.path.join(ROOT, "include", "ohs_tracked.h")).read()
    declared = sorted(set(re.findall(r"\b(ohs_tracked_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == ENTRIES == sorted(tracked.TRACKED_PROTOTYPES) and len(declared) == 14
    lib = os.path.join(PKG, "libohs_tracked.so")
    assert declared == _dynamic_symbols(lib)
    emap = open(os.path.join(PKG, "csrc", "tracked_exports.map")).read()
    assert "global: ohs_tracked_*;" in emap and "local: *;" in emap
    undefined = subprocess.run(["nm", "-D", "--undefined-only", lib], check=True, capture_output=True, text=True).stdout
    assert "ohs" not in undefined
    # the seven older libraries and their headers are what they were
    assert len(_dynamic_symbols(os.path.join(PKG, "libohs_hip.so"))) == 119 and len(_ffi.PROTOTYPES) == 119
    for name, protos, n in (("scene", scene.SCENE_PROTOTYPES, 13), ("scene2", scene2.SCENE2_PROTOTYPES, 14), ("scene3", scene3.SCENE3_PROTOTYPES, 15),
                            ("lookup", lookup.LOOKUP_PROTOTYPES, 7), ("lookup3", lookup3.LOOKUP3_PROTOTYPES, 8),
                            ("lookup3p", lookup3p.LOOKUP3P_PROTOTYPES, 9)):
        assert _dynamic_symbols(os.path.join(PKG, f"libohs_{name}.so")) == sorted(protos) and len(protos) == n, name
        older = open(os.path.join(ROOT, "include", f"ohs_{name}.h")).read()
        assert sorted(set(re.findall(r"\b(ohs_" + name + r"_[a-z0-9_]+)\s*\(", older))) == sorted(protos), name
        assert "ohs_tracked" not in older, name
    assert len(set(re.findall(r"\b(ohs_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "ohs_hip.h")).read()))) == 119
    doc = open(os.path.join(ROOT, "SCENES.md")).read()
    for name in declared:
        assert re.search(r"\bfn " + name + r"\(", doc), f"{name} is not listed in SCENES.md"
    assert "ohs_tracked_" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_every_entry_refuses_null_and_create_refuses_a_bad_mesh():
    import open_headstage_amd as ohs
    from open_headstage_amd import _ffi, lookup, lookup3p, tracked
    from tests.test_cpu_scene_blend3 import OCTA_POS, OCTA_TRI
    L, LP = tracked.tracked_lib(), lookup3p.lookup3p_lib()
    INV = _ffi.OHS_ERR_INVALID_ARG
    fp, u32p = lookup.fp, lookup.u32p
    xyz = lookup.table_xyz(OCTA_POS)
    tri = np.ascontiguousarray(OCTA_TRI, np.uint32)
    h, hp = C.c_void_p(), C.c_void_p()

    def create(n_dirs, x, n_tris, t, out=h, grid=0):
        return L.ohs_tracked_create(0, 2, 10, n_dirs, None if x is None else x.ctypes.data_as(fp), n_tris,
                                    None if t is None else t.ctypes.data_as(u32p), grid, None if out is None else C.byref(out))

    def create_p(n_dirs, x, n_tris, t, grid=0):
        return LP.ohs_lookup3p_create(0, n_dirs, None if x is None else x.ctypes.data_as(fp), n_tris,
                                      None if t is None else t.ctypes.data_as(u32p), grid, C.byref(hp))
    assert create(6, xyz, 8, tri, None) == INV and b"out is NULL" in L.ohs_tracked_last_error()
    bad = xyz.copy()
    bad[3, 1] = np.inf
    flat = np.concatenate([tri[:2], np.array([[0, 2, 1]], np.uint32), np.array([[1, 1, 4]], np.uint32)])
    for args, text in (((6, None, 8, tri), b"NULL"), ((6, xyz, 8, None), b"NULL"), ((0, xyz, 8, tri), b"outside"), ((65537, xyz, 8, tri), b"outside"),
                       ((6, xyz, 0, tri), b"outside"), ((6, xyz, 131073, tri), b"outside"), ((6, bad, 8, tri), b"xyz[10] is not finite"),
                       ((5, xyz, 8, tri), b"triangle 4 names direction 5 of 5"), ((6, xyz, 4, flat), b"triangle 2 (0, 2, 1) is singular")):
        assert create(*args) == INV and not h.value and text in L.ohs_tracked_last_error(), args
        assert create_p(*args) == INV and LP.ohs_lookup3p_last_error() == L.ohs_tracked_last_error()        # the same words
    assert create(6, xyz, 8, tri, grid=257) == INV and not h.value and b"grid 257 is outside 0 .. 256" in L.ohs_tracked_last_error()
    L.ohs_tracked_destroy(None)
    assert L.ohs_tracked_process(None, None, None, 1, 0, 0, 0, 0, 1, 1, None, 0, 0, None, 0, None, 1, 0, None) == INV
    assert b"NULL" in L.ohs_tracked_last_error()
    assert L.ohs_tracked_last_launch(None, None, None, None, None, None, None) == INV
    assert L.ohs_tracked_rows(None, None, None, None, None, None) == INV
    assert L.ohs_tracked_set_direction_irs(None, 0, None, 0) == INV and L.ohs_tracked_set_gain(None, 1.0) == INV
    assert L.ohs_tracked_set_eq_band_coeffs(None, 0, None, 0) == INV and L.ohs_tracked_set_eq_enabled(None, 0) == INV
    assert L.ohs_tracked_set_flush_denormals(None, 0) == INV and L.ohs_tracked_reset(None) == INV and L.ohs_tracked_sync(None, None) == INV
    for s in (0, 1, 2, 3, 6, 99):
        assert L.ohs_tracked_status_string(s) == _ffi.lib().ohs_status_string(s), s
    assert callable(ohs.TrackedSceneProcessor) and "TrackedSceneProcessor" in ohs.__all__ and issubclass(ohs.TrackedSceneProcessor, ohs.SceneProcessor)
    for name in ("set_directions", "set_directions_from_sofa", "process", "process_xyz", "process_ptr", "last_launch", "rows", "reset", "sync"):
        assert callable(getattr(ohs.TrackedSceneProcessor, name)), name
    with pytest.raises(ValueError):
        ohs.TrackedSceneProcessor(2, OCTA_POS, np.array([[0, 1, 6]], np.uint32))
    with pytest.raises(ValueError):
        ohs.TrackedSceneProcessor(2, OCTA_POS, OCTA_TRI, grid=257)


# ---- 2. the kernel's resources and the build --------------------------------------------------------------------------------------
def test_kernel_resources_and_the_build():
    from open_headstage_amd import build
    res = build.resources()
    fields = ("vgprs", "agprs", "sgprs", "scratch_bytes_per_lane", "lds_bytes", "occupancy_waves_per_simd")
    # as built: one object per lane, and four where K is a multiple of 4 (twelve 128-bit loads in flight)
    assert {f: res["k_scene_rows_seal<1>"][f] for f in fields} == \
        {"vgprs": 26, "agprs": 0, "sgprs": 37, "scratch_bytes_per_lane": 0, "lds_bytes": 0, "occupancy_waves_per_simd": 8}
    assert {f: res["k_scene_rows_seal<4>"][f] for f in fields} == \
        {"vgprs": 50, "agprs": 0, "sgprs": 62, "scratch_bytes_per_lane": 0, "lds_bytes": 0, "occupancy_waves_per_simd": 8}
    for f in ("scene_rows_kernels.hip", "scene_rows_body.hpp", "scene_rows_internal.h", "api_tracked.hip"):
        assert "asm" not in open(os.path.join(PKG, "csrc", f)).read(), f
    assert build.is_current() and os.path.exists(build.TRACKED_LIB) and os.path.basename(build.TRACKED_LIB) == "libohs_tracked.so"
    assert [u for u, _ in build.TRACKED_UNITS] == ["scene_rows_kernels.hip", "api_tracked.hip"]
    assert not {u for u, _ in build.TRACKED_UNITS} & {u for u, _ in build.LOOKUP3P_UNITS + build.LOOKUP3_UNITS + build.LOOKUP_UNITS + build._units()}
    # the tracked units depend on their own headers, the pruned lookup's and the product's; no older unit depends on the new headers
    deps = {os.path.basename(d) for d in build._deps("api_tracked.hip")}
    assert {"scene_rows_body.hpp", "scene_rows_internal.h", "lookup3p_body.hpp", "lookup3p_internal.h", "lookup3_body.hpp", "lookup_body.hpp",
            "api_internal.h", "api_scene_bodies.inc", "ohs_tracked.h", "ohs_hip.h", "tracked_exports.map"} <= deps
    for unit in ("api_core.hip", "api_scene3.hip", "conv_objects_blend3_kernels.hip", "lookup3p_kernels.hip"):
        assert not {"scene_rows_body.hpp", "scene_rows_internal.h", "ohs_tracked.h"} & {os.path.basename(d) for d in build._deps(unit)}, unit
    # the three scene kernels are where they were (tests/test_cpu_scene*.py pin their figures; here: they are still recorded)
    for name in ("k_conv_p1_objects", "k_conv_p1_objects_blend", "k_conv_p1_objects_blend3"):
        assert res[name]["scratch_bytes_per_lane"] == 0, name


# ---- 3. the model's two restatements -------------------------------------------------------------------------------------------------
SHAPES = [(S, n_segs, K) for K in (1, 2, 5, 63, 64) for S, n_segs in ((2, 1), (3, 3))]


def _cases():
    """(rows, n_blocks, seg_blocks, fade, carry or None): every shape FRESH and CARRY, faded and not, whole and ragged last segments"""
    out = []
    for i, (S, n_segs, K) in enumerate(SHAPES):
        for j, (seg_blocks, ragged) in enumerate(((1, 0), (3, 0), (3, 2))):
            n_blocks = n_segs * seg_blocks - ragged
            if n_blocks <= (n_segs - 1) * seg_blocks:
                continue
            rows = tm.random_rows(S, n_segs, K, seed=100 * i + j)
            for fade in (True, False):
                out.append((rows, n_blocks, seg_blocks, fade, None))
                out.append((rows, n_blocks, seg_blocks, fade, tm.random_carry(S, K, seed=7 * i + j, like=rows)))
    return out


def _combination_cases():
    """one object (K = 1) and one pair (K = 2) over two segments, w1 and w2 before and after drawn from {+0.0, -0.0, 0.5} in every
    combination, d1 and d2 moving or not, everything else held: each pass kind and each "never read" clause by construction"""
    out = []
    wb = (0x00000000, 0x80000000, 0x3F000000)
    for ow1, ow2, cw1, cw2, m1, m2 in itertools.product(wb, wb, wb, wb, (0, 1), (0, 1)):
        rows = np.zeros((6, 1, 2, 2), np.uint32)
        rows[tm.G] = tm.ONE
        rows[tm.W1, 0, :, 0] = (ow1, cw1)
        rows[tm.W2, 0, :, 0] = (ow2, cw2)
        rows[tm.D1, 0, 1, 0] = m1
        rows[tm.D2, 0, 1, 0] = m2
        out.append((rows, 4, 2, True, None))
        out.append((np.ascontiguousarray(rows[:, :, :, :1]), 4, 2, True, None))
    return out


def test_the_two_restatements_agree_and_every_clause_occurs():
    seen = set()
    for rows, n_blocks, seg_blocks, fade, carry in _cases() + _combination_cases():
        m = tm.seal(rows, n_blocks, seg_blocks, fade, carry)
        prev = {} if carry is None else dict(prev_idx=carry[0], prev_idx1=carry[1], prev_idx2=carry[2], prev_weight=carry[3], prev_weight2=carry[4],
                                             prev_gain=carry[5])
        f, b, t, staged = tm.host_scan(n_blocks, seg_blocks, fade, rows[0], rows[1], rows[2], rows[3], rows[4], rows[5], **prev)
        assert (f, b, t) == (m["fading"], m["blended"], m["blended3"]), (rows.shape, n_blocks, seg_blocks, fade, carry is not None)
        if fade:
            assert np.array_equal(staged, m["front"])
        assert np.array_equal(m["carry"], rows[:, :, -1, :])
        # which clauses this case meets (objects of segments behind the first: their entry in front is the segment before)
        if fade and rows.shape[2] > 1:
            c, o = rows[:, :, 1:, :], rows[:, :, :-1, :]
            same = (c[tm.D0] == o[tm.D0]) & (c[tm.G] == o[tm.G]) & (c[tm.W1] == o[tm.W1]) & (c[tm.W2] == o[tm.W2])
            if (same & (c[tm.W2] == 0) & (c[tm.D2] != o[tm.D2]) & ((c[tm.W1] != 0) | (c[tm.D1] == o[tm.D1]))).any():
                seen.add("d2 moves beside w2 = +0.0 on both sides, nothing else does")
            if (same & (c[tm.W1] == 0) & (c[tm.D1] != o[tm.D1]) & ((c[tm.W2] != 0) | (c[tm.D2] == o[tm.D2]))).any():
                seen.add("d1 moves beside w1 = +0.0 on both sides, nothing else does")
            if ((c[tm.W2] == 0x80000000) | (c[tm.W1] == 0x80000000)).any():
                seen.add("a weight of -0.0")
        if m["fading"]:
            seen.add("fading")
        if m["blended"]:
            seen.add("four-row passes")
        if m["blended3"]:
            seen.add("six-row passes")
        if m["fading"] == 0 and m["blended"] == 0 and m["blended3"] == 0:
            seen.add("two-row passes only")
    assert len(seen) == 7, seen


# ---- 4. scene_rows_body.hpp on the host ----------------------------------------------------------------------------------------------
def _cxx():
    from open_headstage_amd import build
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc()))), "llvm", "bin", "clang++")
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx, "no host C++ compiler"
    return cxx


def _compile(exe, extra=(), include=None):
    return subprocess.run([_cxx(), "-O2", "-std=c++17", *extra, "-I", include or os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tests", "scene_rows_host_check.cpp"), "-o", exe], capture_output=True, text=True)


def _run(exe, cases, tmp_path, env=None):
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.uint32(len(cases)).tobytes())
        for rows, n_blocks, seg_blocks, fade, carry in cases:
            _, S, n_segs, K = rows.shape
            clamped, _ = tm.seg_lens(n_blocks, seg_blocks)
            f.write(np.array([S, n_segs, K, clamped, n_blocks, int(fade), int(carry is not None)], np.uint32).tobytes())
            f.write(np.ascontiguousarray(rows, np.uint32).tobytes())
            if carry is not None:
                f.write(np.ascontiguousarray(carry, np.uint32).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = np.fromfile(tmp_path / "out.bin", np.uint32)
    out, at = [], 0
    for rows, *_ in cases:
        _, S, n_segs, K = rows.shape
        n = 6 * S * K
        front, carry = got[at:at + n].reshape(6, S, K), got[at + n:at + 2 * n].reshape(6, S, K)
        counts = got[at + 2 * n:at + 2 * n + 6].view(np.uint64)
        at += 2 * n + 6
        out.append(dict(front=front, carry=carry, fading=int(counts[0]), blended=int(counts[1]), blended3=int(counts[2])))
    assert at == len(got)
    return out


def _differences(cases, got):
    """the cases in which the program's answer is not the model's, by what differs"""
    bad = []
    for i, (case, g) in enumerate(zip(cases, got)):
        m = tm.seal(*case)
        for key in ("front", "carry", "fading", "blended", "blended3"):
            if not np.array_equal(m[key], g[key]):
                bad.append((i, key))
    return bad


def test_scene_rows_body_on_the_host(tmp_path):
    exe = str(tmp_path / "scene_rows_host_check")
    r = _compile(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    cases = _cases() + _combination_cases()
    assert {c[0].shape[3] for c in cases} == {1, 2, 5, 63, 64} and {c[0].shape[2] for c in cases} == {1, 2, 3}
    got = _run(exe, cases, tmp_path)
    assert _differences(cases, got) == []
    # the counts are libohs_scene3.so's host scan's as well (the restatement of api_batch.hip)
    for (rows, n_blocks, seg_blocks, fade, carry), g in zip(cases, got):
        prev = {} if carry is None else dict(prev_idx=carry[0], prev_idx1=carry[1], prev_idx2=carry[2], prev_weight=carry[3], prev_weight2=carry[4],
                                             prev_gain=carry[5])
        f, b, t, _ = tm.host_scan(n_blocks, seg_blocks, fade, rows[0], rows[1], rows[2], rows[3], rows[4], rows[5], **prev)
        assert (f, b, t) == (g["fading"], g["blended"], g["blended3"])


MUTANTS = {
    "d2 compared beside w2 = +0.0": ("((cur.w2 | old.w2) != 0u && cur.d2 != old.d2)", "(cur.d2 != old.d2)", {"fading", "blended", "blended3"}),
    "a fading old pass not counted in blended3": ("p.old6 = ch && old_tri ? 1u : 0u;", "p.old6 = 0u;", {"blended3"}),
    "the carry taken from the first segment": ("return n_segs - 1; }", "return 0 * n_segs; }", {"carry"}),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_a_mutant_of_the_header_is_caught(tmp_path, name):
    old, new, where = MUTANTS[name]
    text = open(BODY).read()
    assert text.count(old) == 1, name
    (tmp_path / "inc").mkdir()
    (tmp_path / "inc" / "scene_rows_body.hpp").write_text(text.replace(old, new))
    exe = str(tmp_path / "scene_rows_host_check_mutant")
    r = _compile(exe, include=str(tmp_path / "inc"))
    assert r.returncode == 0, r.stderr[-2000:]
    cases = _cases() + _combination_cases()
    bad = _differences(cases, _run(exe, cases, tmp_path))
    assert bad and {key for _, key in bad} <= where, (name, bad[:8])


def test_the_host_program_under_the_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined.  A stand-alone program: nothing is preloaded and Python loads none of
    it.  Skips where the sanitizers' runtime is not installed."""
    exe = str(tmp_path / "scene_rows_host_check_san")
    r = _compile(exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))
    if r.returncode != 0:
        pytest.skip("the address / undefined-behaviour sanitizers' runtime is not installed: " + r.stderr.strip()[-200:])
    cases = _cases() + _combination_cases()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    assert _differences(cases, _run(exe, cases, tmp_path, env=env)) == []

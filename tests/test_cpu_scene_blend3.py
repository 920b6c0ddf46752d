"""Three-direction object scenes (libohs_scene3.so, include/ohs_scene3.h), the part that needs no GPU.

* the block-wise f64 model of tests/scene_blend3_model.py (it blends signals) agrees to 1e-13 with a direct time-domain evaluation that
  blends the responses, and carries prev_* and the tail over a cut;
* with w2 = +0.0 everywhere it is tests/scene_blend_model.py's model, with w1 = +0.0 as well tests/scene_model.py's, figure for figure;
* it agrees with the 3 K identity evaluated by the EXISTING tests/scene_model.py on 3 K objects, below the project's FFT bar (1e-6
  relative RMS);
* four wrong readings of the rule are each far above that bar on the GPU tests' own inputs;
* the header's names, libohs_scene3.so's dynamic symbols and SCENE3_PROTOTYPES are one list of fifteen, every entry refuses NULL, and
  the four older libraries export their 119 / 13 / 14 / 7 names;
* k_conv_p1_objects_blend3 was built without scratch and AGPRs at three waves per SIMD;
* triangle_directions on an octahedron and on a latitude-longitude grid, triangulate_directions on the octahedron."""
import os
import re

import numpy as np
import pytest

from tests import scene_blend3_model as tm
from tests import scene_blend_model as bm
from tests import scene_model as sm
from tests.test_cpu_layout import BAR, BLOCK, make_input, make_layout, rel_rms_per_stream
from tests.test_cpu_scene import _dynamic_symbols, rel_rms_per_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "open_headstage_amd")
GAIN = 0.7
N_DIRS = 7


# ---- 1. the two evaluations of the rule agree ----------------------------------------------------------------------------------
@pytest.mark.parametrize("K,seg_blocks,shared,fade", [(1, 1, False, True), (3, 2, False, True), (5, 3, True, True), (4, 2, False, False)])
def test_block_wise_model_is_the_direct_evaluation(K, seg_blocks, shared, fade):
    S, blocks = 2, 6
    dirs = make_layout(N_DIRS, 8)
    x = make_input(S, K, blocks, seed=9500 + K)
    sc = tm.make_blend3_scene(S, K, blocks, seg_blocks, N_DIRS, seed=K, shared=shared)
    a = tm.model_blend3_f64(x, dirs, *tm.args(sc), seg_blocks, crossfade=fade, gain=GAIN, **tm.kw(sc))
    b = tm.direct_blend3_f64(x, dirs, *tm.args(sc), seg_blocks, crossfade=fade, gain=GAIN, **tm.kw(sc))
    err = rel_rms_per_stream(a, b)
    print(f"K = {K}, seg_blocks {seg_blocks}: signals blended against responses blended, relative RMS per stream, worst {err.max():.3e}")
    assert (err <= 1e-13).all(), err


def test_two_renders_in_a_row_with_prev_and_the_tail_equal_one():
    S, K, blocks, seg = 2, 3, 8, 2
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S, K, blocks, seed=9700)
    sc = tm.make_blend3_scene(S, K, blocks, seg, N_DIRS, seed=3)
    whole, tw = tm.model_blend3_f64(x, dirs, *tm.args(sc), seg, gain=GAIN, with_tail=True, **tm.kw(sc))
    first = {k: sc[k][:, :2] for k in tm.ROWS}
    a, tail = tm.model_blend3_f64(x[:, :, :4 * BLOCK], dirs, *tm.args(first), seg, gain=GAIN, with_tail=True, **dict(tm.kw(sc), gains=first["gains"]))
    second = {k: sc[k][:, 2:] for k in tm.ROWS}
    prev = dict(gains=second["gains"], prev_idx=sc["idx"][:, 1], prev_idx1=sc["idx1"][:, 1], prev_idx2=sc["idx2"][:, 1], prev_w1=sc["w1"][:, 1],
                prev_w2=sc["w2"][:, 1], prev_gains=sc["gains"][:, 1])
    b, tb = tm.model_blend3_f64(x[:, :, 4 * BLOCK:], dirs, *tm.args(second), seg, gain=GAIN, tail_in=tail, with_tail=True, **prev)
    assert np.allclose(np.concatenate([a, b], axis=2), whole, rtol=0, atol=1e-14)
    assert np.allclose(tb, tw, rtol=0, atol=1e-14)


# ---- 2. the older models inside this one ----------------------------------------------------------------------------------------
def test_w2_zero_is_the_two_direction_model_and_w1_zero_too_the_one_direction_model():
    S, K, blocks, seg = 2, 3, 6, 2
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S, K, blocks, seed=9600)
    b = bm.make_blend_scene(S, K, blocks, seg, N_DIRS, seed=5)
    rng = np.random.default_rng(96)
    moving = rng.integers(0, N_DIRS, b["idx"].shape).astype(np.uint32)         # idx2 moves by itself, in front of the call too
    before = ((moving[:, 0] + 1) % N_DIRS).astype(np.uint32)
    assert (moving[:, 1:] != moving[:, :-1]).any(axis=(0, 2)).all()
    zero, pzero = np.zeros_like(b["weights"]), np.zeros_like(b["prev_weights"])
    rows = (b["idx"], b["idx1"], moving, b["weights"], zero)
    keys = dict(gains=b["gains"], prev_idx=b["prev_idx"], prev_idx1=b["prev_idx1"], prev_idx2=before, prev_w1=b["prev_weights"], prev_w2=pzero,
                prev_gains=b["prev_gains"])
    got = tm.model_blend3_f64(x, dirs, *rows, seg, gain=GAIN, **keys)
    want = bm.model_blend_f64(x, dirs, b["idx"], b["idx1"], b["weights"], seg, b["gains"], b["prev_idx"], b["prev_idx1"], b["prev_weights"],
                              b["prev_gains"], True, GAIN)
    assert np.allclose(got, want, rtol=0, atol=1e-14)
    plan = tm.blend3_plan(S, K, blocks, *rows, seg, keys["gains"], keys["prev_idx"], keys["prev_idx1"], before, keys["prev_w1"], pzero,
                          keys["prev_gains"], True)
    plan2 = bm.blend_plan(S, K, blocks, b["idx"], b["idx1"], b["weights"], seg, b["gains"], b["prev_idx"], b["prev_idx1"], b["prev_weights"],
                          b["prev_gains"], True)
    assert (tm.count_fading_passes(plan), tm.count_blended_passes(plan), tm.count_blended3_passes(plan)) == \
        (bm.count_fading_passes(plan2), bm.count_blended_passes(plan2, K), 0)
    assert bm.count_fading_passes(plan2) > 0 and bm.count_blended_passes(plan2, K) > 0
    # w1 = +0.0 as well, idx1 moving too: the one-direction scene on idx, fade for fade
    rows = (b["idx"], moving[:, ::-1].copy(), moving, zero, zero)
    keys = dict(keys, prev_idx1=before, prev_w1=pzero)
    got = tm.model_blend3_f64(x, dirs, *rows, seg, gain=GAIN, **keys)
    want = sm.model_scene_f64(x, dirs, b["idx"], seg, b["gains"], b["prev_idx"], b["prev_gains"], True, GAIN)
    assert np.allclose(got, want, rtol=0, atol=1e-14)
    plan = tm.blend3_plan(S, K, blocks, *rows, seg, keys["gains"], keys["prev_idx"], before, before, pzero, pzero, keys["prev_gains"], True)
    one = sm.scene_plan(S, K, blocks, b["idx"], seg, b["gains"], b["prev_idx"], b["prev_gains"], True)
    assert (tm.count_fading_passes(plan), tm.count_blended_passes(plan), tm.count_blended3_passes(plan)) == (sm.count_fading_passes(one), 0, 0)


def test_a_third_index_changes_an_object_only_beside_a_w2():
    """idx2 alone: a change where w2 is not +0.0 on both sides (-0.0 is not +0.0), none where it is; and the GPU tests' scenes hold both,
    beside changes in w2 alone"""
    from tests.test_gpu_scene_blend3 import BLEND3_CASES, blend3_case
    i0, g = np.zeros((1, 4, 1), np.uint32), np.ones((1, 4, 1), np.float32)
    i2 = np.array([1, 2, 3, 4], np.uint32).reshape(1, 4, 1)
    w1 = np.full((1, 4, 1), 0.25, np.float32)
    for w2, fades in [([0.0, 0.0, 0.0, 0.0], [0, 0, 0, 0]), ([0.5, 0.5, 0.5, 0.5], [1, 1, 1, 1]), ([0.0, 0.0, 0.5, 0.0], [0, 0, 1, 1]),
                      ([-0.0, -0.0, 0.0, 0.0], [1, 1, 1, 0])]:
        plan = tm.blend3_plan(1, 1, 4, i0, i0, i2, w1, np.array(w2, np.float32).reshape(1, 4, 1), 1, g, None, None, np.array([[0]], np.uint32), None,
                              None, None, True)
        assert [int(any(p[8] for p in passes)) for passes in plan[0]] == fades, (w2, fades)
    only_idx2 = zero_idx2 = only_w2 = 0
    for case in BLEND3_CASES:
        _, _, _, sc = blend3_case(*case)
        shape = (3,) + np.shape(sc["idx"])[-2:]
        r = {k: np.broadcast_to(np.asarray(sc[k]).reshape((-1,) + shape[1:]), shape) for k in tm.ROWS}
        same = (r["idx"][:, 1:] == r["idx"][:, :-1]) & (r["gains"][:, 1:] == r["gains"][:, :-1]) & (r["w1"][:, 1:] == r["w1"][:, :-1]) & \
            (r["idx1"][:, 1:] == r["idx1"][:, :-1])
        moved = r["idx2"][:, 1:] != r["idx2"][:, :-1]
        read = (r["w2"][:, 1:] != 0) | (r["w2"][:, :-1] != 0)
        only_idx2 += int((same & moved & read & (r["w2"][:, 1:] == r["w2"][:, :-1])).sum())
        zero_idx2 += int((moved & ~read).sum())
        only_w2 += int((same & ~moved & (r["w2"][:, 1:] != r["w2"][:, :-1])).sum())
    print(f"the GPU cases' scenes: {only_idx2} changes in idx2 alone beside a w2, {zero_idx2} beside +0.0, {only_w2} in w2 alone")
    assert only_idx2 > 0 and zero_idx2 > 0 and only_w2 > 0


# ---- 3. the 3 K identity through the existing model ----------------------------------------------------------------------------
def test_model_against_the_3k_identity_through_the_existing_scene_model():
    from tests.test_gpu_scene_blend3 import BLEND3_CASES, blend3_case
    worst = 0.0
    for case in BLEND3_CASES:
        x, dirs, seg, sc = blend3_case(*case)
        for fade in (True, False):
            ref = tm.model_blend3_f64(x, dirs, *tm.args(sc), seg, crossfade=fade, gain=GAIN, **tm.kw(sc))
            x3, idx3, gains3, pi3, pg3 = tm.as_3k_scene(x, *tm.args(sc), **tm.kw(sc))
            y = sm.model_scene_f64(x3, dirs, idx3, seg, gains3, pi3, pg3, fade, GAIN)
            e, eb = rel_rms_per_stream(y, ref), rel_rms_per_block(y, ref)
            print(f"{case}, crossfade {fade}: 3 K objects through scene_model against the model: per stream worst {e.max():.3e}, "
                  f"per block worst {eb.max():.3e}")
            assert (e <= BAR).all() and (eb <= BAR).all(), (case, fade, e, eb.max())
            worst = max(worst, float(eb.max()))
    assert worst > 0.0          # (f32 products: the two are not the same arithmetic)


# ---- 4. what a test at the bar sees, on the GPU tests' inputs ------------------------------------------------------------------
def test_mutants_against_the_bar_on_the_gpu_tests_inputs():
    from tests.test_gpu_scene_blend3 import BLEND3_CASES, blend3_case
    seen = {m: 0.0 for m in tm.MUTANTS}
    for case in BLEND3_CASES:
        x, dirs, seg, sc = blend3_case(*case)
        ref = tm.model_blend3_f64(x, dirs, *tm.args(sc), seg, gain=GAIN, **tm.kw(sc))
        for m in tm.MUTANTS:
            y = tm.model_blend3_f64(x, dirs, *tm.args(sc), seg, gain=GAIN, mutant=m, **tm.kw(sc))
            e, eb = rel_rms_per_stream(y, ref), rel_rms_per_block(y, ref)
            print(f"{case}: mutant {m}: per stream {e.min():.3e} .. {e.max():.3e}, worst block {eb.max():.3e}")
            seen[m] = max(seen[m], float(e.max()))
    for m in tm.MUTANTS:
        assert seen[m] > 1e3 * BAR, (m, seen[m])        # some case of the GPU file shows the mutant, far above the bar


def test_the_gpu_files_scenes_hold_what_they_name():
    """the mixed scene's four kinds of pair, the 65 536-row scene's corners, the fuzz sequence's entries and setters -- all without a GPU"""
    from tests import test_gpu_scene_blend3 as g
    K, sc = g.mixed_scene()
    w1, w2 = sc["w1"], sc["w2"]
    assert K == 7 and (w1[..., :2] == 0).all() and (w2[..., :4] == 0).all() and (w1[..., 2:] > 0).all() and (w2[..., 4:] > 0).all()
    assert ((w1 + w2).astype(np.float32) <= 1).all()
    big, small = g.full_scene3()
    for k in ("idx", "idx1", "idx2"):
        assert {0, 65535} <= set(np.concatenate([big[k].ravel(), big["prev_" + k].ravel()]).tolist()), k
        assert int(small[k].max()) <= 8
    assert (big["w2"][:, :, 1] == 0).all() and (big["w2"][:, :, [0, 2]] > 0).all() and ((big["w1"] + big["w2"]).astype(np.float32) <= 1).all()
    ops = g.draw_sequence()
    calls = [op[1] for op in ops if op[0] == "call"]
    assert {c["entry"] for c in calls} == {1, 2, 3} and {op[0] for op in ops} == {"call", "set_gain", "reset", "set_directions"}
    assert {c["fade"] for c in calls} == {True, False} and {c["sc"]["idx"].ndim for c in calls} == {2, 3}
    for name in ("gains", "prev_idx2", "prev_w2"):
        assert {c["sc"][name] is None for c in calls} == {True, False}, name


# ---- 5. the surface ------------------------------------------------------------------------------------------------------------
def test_header_library_and_prototypes_are_one_list_of_fifteen():
    from open_headstage_amd import _ffi, lookup, scene, scene2, scene3
    hdr = open(os.path.join(ROOT, "include", "ohs_scene3.h")).read()
    declared = sorted(set(re.findall(r"\b(ohs_scene3_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) == 15, declared
    assert declared == sorted(scene3.SCENE3_PROTOTYPES)
    assert declared == _dynamic_symbols(os.path.join(PKG, "libohs_scene3.so"))
    shared = sorted(n.replace("ohs_scene3_", "ohs_scene_", 1) for n in declared if n not in ("ohs_scene3_process_blended", "ohs_scene3_process_blended3"))
    assert shared == sorted(scene.SCENE_PROTOTYPES) and len(shared) == 13
    for n in shared:        # identical signatures, but the launch record's figures
        if n != "ohs_scene_last_launch":
            assert scene.SCENE_PROTOTYPES[n] == scene3.SCENE3_PROTOTYPES[n.replace("ohs_scene_", "ohs_scene3_", 1)], n
    assert len(scene3.SCENE3_PROTOTYPES["ohs_scene3_last_launch"][1]) == 6
    assert scene3.SCENE3_PROTOTYPES["ohs_scene3_process_blended"] == scene2.SCENE2_PROTOTYPES["ohs_scene2_process_blended"]
    assert len(scene3.SCENE3_PROTOTYPES["ohs_scene3_process_blended3"][1]) == len(scene2.SCENE2_PROTOTYPES["ohs_scene2_process_blended"][1]) + 4
    # the four older libraries are what they were
    assert len(_dynamic_symbols(os.path.join(PKG, "libohs_hip.so"))) == 119 and len(_ffi.PROTOTYPES) == 119
    assert _dynamic_symbols(os.path.join(PKG, "libohs_scene.so")) == sorted(scene.SCENE_PROTOTYPES) and len(scene.SCENE_PROTOTYPES) == 13
    assert _dynamic_symbols(os.path.join(PKG, "libohs_scene2.so")) == sorted(scene2.SCENE2_PROTOTYPES) and len(scene2.SCENE2_PROTOTYPES) == 14
    assert len(_dynamic_symbols(os.path.join(PKG, "libohs_lookup.so"))) == 7 and len(lookup.LOOKUP_PROTOTYPES) == 7
    emap = open(os.path.join(PKG, "csrc", "scene3_exports.map")).read()
    assert "global: ohs_scene3_*;" in emap and "local: *;" in emap
    for out_of_scope in ("four or more directions", "found on the device", "weight ramps other than the one-block fade", "one partition",
                         "in-place", "node twin"):
        assert out_of_scope in re.sub(r"\s*\n \*\s*", " ", hdr), out_of_scope
    for written_out in ("(u * A[dir] + w1 * A[dir1]) + w2 * A[dir2]", "u = (1.0f - w1) - w2", "The pass rule", "The change rule"):
        assert written_out in hdr, written_out
    doc = open(os.path.join(ROOT, "SCENES.md")).read()
    for name in declared:
        assert re.search(r"\bfn " + name + r"\(", doc), f"{name} is not listed in SCENES.md"
    assert "ohs_scene3_" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_every_entry_refuses_null():
    from open_headstage_amd import _ffi, scene3
    L = scene3.scene3_lib()
    INV = _ffi.OHS_ERR_INVALID_ARG
    assert L.ohs_scene3_create(0, 1, 10, None) == INV
    L.ohs_scene3_destroy(None)
    assert L.ohs_scene3_set_direction_irs(None, 0, None, 0) == INV
    assert L.ohs_scene3_process(None, None, None, 1, 1024, 512, 1024, 512, 1, 1, None, None, 0, None, None, 1, None) == INV
    assert b"NULL" in L.ohs_scene3_last_error()
    assert L.ohs_scene3_process_blended(None, None, None, 1, 1024, 512, 1024, 512, 1, 1, None, None, 0, None, None, 1, None,
                                        None, None, None, None) == INV
    assert b"NULL" in L.ohs_scene3_last_error()
    assert L.ohs_scene3_process_blended3(None, None, None, 1, 1024, 512, 1024, 512, 1, 1, None, None, 0, None, None, 1, None,
                                         None, None, None, None, None, None, None, None) == INV
    assert b"NULL" in L.ohs_scene3_last_error()
    assert L.ohs_scene3_set_gain(None, 1.0) == INV
    assert L.ohs_scene3_set_eq_band_coeffs(None, 0, None, 0) == INV
    assert L.ohs_scene3_set_eq_enabled(None, 0) == INV
    assert L.ohs_scene3_set_flush_denormals(None, 0) == INV
    assert L.ohs_scene3_reset(None) == INV
    assert L.ohs_scene3_sync(None, None) == INV
    assert L.ohs_scene3_last_launch(None, None, None, None, None, None) == INV
    assert L.ohs_scene3_status_string(INV) == _ffi.lib().ohs_status_string(INV)
    import open_headstage_amd as ohs
    assert issubclass(ohs.TriSceneProcessor, ohs.BlendSceneProcessor)
    assert ohs.TriSceneProcessor.last_launch is not ohs.BlendSceneProcessor.last_launch
    assert callable(ohs.triangle_directions) and callable(ohs.triangulate_directions)


# ---- 6. the kernel's resources -------------------------------------------------------------------------------------------------
def test_kernel_resources():
    from open_headstage_amd import build
    res = build.resources()
    fields = ("vgprs", "agprs", "sgprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd")
    k = res["k_conv_p1_objects_blend3"]
    # the condition: no scratch, no AGPRs, three waves per SIMD (at most 168 VGPRs)
    assert k["scratch_bytes_per_lane"] == 0 and k["agprs"] == 0 and k["occupancy_waves_per_simd"] == 3 and k["vgprs"] <= 168, k
    # ... and the figures as built, with the six-row pass's window at four rows
    assert {f: k[f] for f in fields} == {"vgprs": 168, "agprs": 0, "sgprs": 106, "scratch_bytes_per_lane": 0, "occupancy_waves_per_simd": 3}, k
    # the three object kernels' text is one header's; the units hold a stub each
    body = open(os.path.join(PKG, "csrc", "conv_objects_body.hpp")).read()
    assert re.search(r"#define OHS_P1_BLEND3_ROWS 4\b", body)
    assert "asm volatile(\"\" :" in body
    for name in ("conv_objects_body.hpp", "conv_objects_kernels.hip", "conv_objects_blend_kernels.hip", "conv_objects_blend3_kernels.hip"):
        src = open(os.path.join(PKG, "csrc", name)).read()
        assert "conv_objects_body.hpp" in src
        assert not re.search(r"asm\s+volatile\s*\(\s*\"[^\"]", src), name       # (register fences only)
    assert build.is_current() and os.path.exists(build.SCENE3_LIB)
    assert {os.path.basename(p) for p in (build.LIB, build.SCENE_LIB, build.SCENE2_LIB, build.SCENE3_LIB, build.LOOKUP_LIB)} == \
        {"libohs_hip.so", "libohs_scene.so", "libohs_scene2.so", "libohs_scene3.so", "libohs_lookup.so"}


# ---- 7. the host helpers -------------------------------------------------------------------------------------------------------
OCTA_POS = np.array([[0, 0, 1], [90, 0, 1], [180, 0, 1], [270, 0, 1], [0, 90, 1], [0, -90, 1]], np.float32)
OCTA_TRI = np.array([[r, (r + 1) % 4, p] for p in (4, 5) for r in range(4)], np.uint32)


def grid_mesh(n_az=12, els=(-60.0, -30.0, 0.0, 30.0, 60.0)):
    """a latitude-longitude grid without poles (an OPEN mesh), every cell split into two triangles by index arithmetic:
    -> (positions [M][3], triangles [T][3]); point (ring e, step a) is index e * n_az + a"""
    pos = np.array([[360.0 * a / n_az, el, 1.0] for el in els for a in range(n_az)], np.float32)
    tri = []
    for e in range(len(els) - 1):
        for a in range(n_az):
            p00, p01 = e * n_az + a, e * n_az + (a + 1) % n_az
            p10, p11 = p00 + n_az, p01 + n_az
            tri += [[p00, p01, p11], [p00, p11, p10]]
    return pos, np.array(tri, np.uint32)


def _cart(az, el):
    a, e = np.radians(np.asarray(az, np.float64)), np.radians(np.asarray(el, np.float64))
    return np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], -1)


def _sph(v):
    v = v / np.linalg.norm(v, axis=-1, keepdims=True)
    return np.degrees(np.arctan2(v[..., 1], v[..., 0])), np.degrees(np.arcsin(np.clip(v[..., 2], -1, 1)))


@pytest.mark.parametrize("mesh", ["octahedron", "grid"])
def test_triangle_directions(mesh):
    from open_headstage_amd.scene3 import triangle_directions
    pos, tri = (OCTA_POS, OCTA_TRI) if mesh == "octahedron" else grid_mesh()
    M = pos.shape[0]
    p = _cart(pos[:, 0], pos[:, 1])
    zero_bits = lambda a: (np.ascontiguousarray(a).view(np.uint32) == 0).all()      # noqa: E731  (+0.0, not -0.0)
    # a vertex: (v, ., ., +0.0, +0.0)
    i0, i1, i2, w1, w2 = triangle_directions(pos, tri, pos[:, 0], pos[:, 1])
    assert [a.dtype for a in (i0, i1, i2, w1, w2)] == [np.uint32] * 3 + [np.float32] * 2 and i0.shape == (M,)
    assert (i0 == np.arange(M)).all() and zero_bits(w1) and zero_bits(w2)
    tri_sets = {frozenset(int(v) for v in t) for t in tri}
    assert all(frozenset((int(a), int(b), int(c))) in tri_sets for a, b, c in zip(i0, i1, i2))
    # an edge's midpoint: its two ends at a half each, +0.0 for the third
    edges = sorted({tuple(sorted((int(t[a]), int(t[b])))) for t in tri for a, b in ((0, 1), (1, 2), (0, 2))})
    ea, eb = np.array(edges).T
    az, el = _sph(p[ea] + p[eb])
    i0, i1, i2, w1, w2 = triangle_directions(pos, tri, az.astype(np.float32), el.astype(np.float32))
    assert all({int(a), int(b)} == {int(c), int(d)} for a, b, c, d in zip(i0, i1, ea, eb))
    assert np.abs(w1 - 0.5).max() <= 1e-6 and zero_bits(w2), (np.abs(w1 - 0.5).max(), w2)
    # a triangle's centroid: thirds
    az, el = _sph(p[tri[:, 0]] + p[tri[:, 1]] + p[tri[:, 2]])
    i0, i1, i2, w1, w2 = triangle_directions(pos, tri, az.astype(np.float32), el.astype(np.float32))
    for t, a, b, c in zip(tri, i0, i1, i2):
        assert {int(a), int(b), int(c)} == {int(v) for v in t}
    print(f"{mesh}: centroids: w1 and w2 off a third by at most {np.abs(w1 - 1 / 3).max():.3e}, {np.abs(w2 - 1 / 3).max():.3e}")
    assert np.abs(w1 - 1 / 3).max() <= 1e-6 and np.abs(w2 - 1 / 3).max() <= 1e-6, (w1, w2)
    # random queries inside the mesh: weights in range, ordered, a triangle of the mesh, and sum w_i p_i parallel to the query
    rng = np.random.default_rng(79)
    az = rng.uniform(-360.0, 360.0, 200).astype(np.float32)
    el = rng.uniform(-89.0, 89.0, 200).astype(np.float32) if mesh == "octahedron" else rng.uniform(-59.0, 59.0, 200).astype(np.float32)
    i0, i1, i2, w1, w2 = triangle_directions(pos, tri, az.reshape(4, 50), el.reshape(4, 50))
    assert i0.shape == (4, 50) and w2.shape == (4, 50)
    i0, i1, i2, w1, w2 = (a.ravel() for a in (i0, i1, i2, w1, w2))
    u = 1.0 - w1.astype(np.float64) - w2
    assert (w2 >= 0).all() and (w1 >= w2).all() and (u >= w1 - 1e-7).all() and (w1 <= 0.5).all() and (w2 <= np.float32(1 / 3) + 1e-7).all()
    assert ((np.float32(w1) + np.float32(w2)).astype(np.float32) <= 1).all()
    assert all(frozenset((int(a), int(b), int(c))) in tri_sets for a, b, c in zip(i0, i1, i2))
    v = u[:, None] * p[i0] + w1[:, None].astype(np.float64) * p[i1] + w2[:, None].astype(np.float64) * p[i2]
    q = _cart(az.astype(np.float64), el.astype(np.float64))
    sin = np.linalg.norm(np.cross(v / np.linalg.norm(v, axis=1, keepdims=True), q), axis=1)
    print(f"{mesh}: sum w_i p_i against the query, the sine of the angle between them, worst {sin.max():.3e}")
    assert sin.max() <= 1e-6 and (np.einsum("ij,ij->i", v, q) > 0).all()
    # equal weights: ascending index
    if mesh == "octahedron":
        a, b, c, _, _ = triangle_directions(pos, tri, np.float32(45.0), np.float32(0.0))
        assert (int(a), int(b)) == (0, 1)
    # just outside an open mesh the rim's edge answers, with weights in range
    if mesh == "grid":
        a, b, c, x1, x2 = triangle_directions(pos, tri, np.float32(12.0), np.float32(62.0))
        assert {int(a), int(b)} == {48, 49} and 0 < float(x1) <= 0.5 and zero_bits(x2), (a, b, c, x1, x2)
    # a singular triangle is refused, and so is an index outside the positions
    with pytest.raises(ValueError, match="singular"):
        flat = [0, 2, 1] if mesh == "octahedron" else [0, 6, 12]      # (three directions in one plane through the origin)
        triangle_directions(pos, np.concatenate([tri, [flat]]).astype(np.uint32), 0.0, 0.0)
    with pytest.raises(ValueError):
        triangle_directions(pos, np.array([[0, 1, M]], np.uint32), 0.0, 0.0)


def test_the_residue_rule_from_both_sides_and_the_fallback():
    """step 5 of triangle_directions: a third gain of 2^-19 of the largest is kept, one of 2^-21 is written +0.0 (the line is 2^-20);
    and a query that faces away from the only triangle goes to the corner with the largest gain, whole"""
    from open_headstage_amd.scene3 import triangle_directions
    p = _cart(OCTA_POS[:, 0], OCTA_POS[:, 1])
    for power, kept in ((-19, True), (-21, False)):
        # a + b + eps c over the triangle (0, 1, 4): gains (1, 1, eps) / norm, eps the third gain's share of the largest
        eps = 2.0 ** power
        az, el = _sph(p[0] + p[1] + eps * p[4])
        i0, i1, i2, w1, w2 = triangle_directions(OCTA_POS, OCTA_TRI, np.float32(az), np.float32(el))
        assert {int(i0), int(i1)} == {0, 1} and int(i2) == 4 and abs(float(w1) - 0.5) <= 1e-6, (power, i0, i1, i2, w1)
        if kept:
            assert abs(float(w2) / (eps / (2 + eps)) - 1) <= 1e-3, (power, w2)
        else:
            assert w2.view(np.uint32) == 0, (power, w2)
    one = OCTA_TRI[:1]                                      # the triangle (0, 1, 4) alone: an open mesh
    az, el = _sph(-(p[0] + 2 * p[1] + 3 * p[4]))            # gains (-1, -2, -3) / norm: corner 0 has the largest
    i0, i1, i2, w1, w2 = triangle_directions(OCTA_POS, one, np.float32(az), np.float32(el))
    assert int(i0) == 0 and w1.view(np.uint32) == 0 and w2.view(np.uint32) == 0, (i0, i1, i2, w1, w2)


def test_the_fade_does_something_in_the_gpu_files_scenes():
    from tests.test_gpu_scene_blend3 import BLEND3_CASES, blend3_case
    x, dirs, seg, sc = blend3_case(*BLEND3_CASES[2])
    a, b = (tm.model_blend3_f64(x, dirs, *tm.args(sc), seg, crossfade=fade, gain=GAIN, **tm.kw(sc)) for fade in (False, True))
    assert (rel_rms_per_stream(a, b) > 1e-3).all()


def test_triangulate_directions_on_the_octahedron():
    pytest.importorskip("scipy")
    from open_headstage_amd.scene3 import triangle_directions, triangulate_directions
    tri = triangulate_directions(OCTA_POS)
    assert tri.dtype == np.uint32 and tri.shape == (8, 3)
    assert {frozenset(int(v) for v in t) for t in tri} == {frozenset(int(v) for v in t) for t in OCTA_TRI}
    i0, _, _, w1, w2 = triangle_directions(OCTA_POS, tri, OCTA_POS[:, 0], OCTA_POS[:, 1])
    assert (i0 == np.arange(6)).all() and (w1 == 0).all() and (w2 == 0).all()

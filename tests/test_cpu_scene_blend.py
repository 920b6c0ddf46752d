"""Blended object scenes (libohs_scene2.so, include/ohs_scene2.h), the part that needs no GPU.

* the block-wise f64 model of tests/scene_blend_model.py (it blends signals) agrees to 1e-13 with a direct time-domain evaluation that
  blends the responses, and carries prev_* and the tail over a cut;
* the model agrees with the 2 K identity -- conv(u h0 + w h1, x) = conv(h0, u x) + conv(h1, w x) -- evaluated by the EXISTING
  tests/scene_model.py on 2 K objects: the two differ in which pairs fade and in f32 products, and stay below the project's FFT bar
  (1e-6 relative RMS);
* five wrong readings of the rule are each above that bar on the GPU tests' own inputs; on the wide scenes of
  tests/test_gpu_scene_wide.py the three wide mutants of tests/scene_model.py are more than 1e3 times the bar away in some block of
  every scene, and the model still equals the direct evaluation at K = 64;
* the header's names, libohs_scene2.so's dynamic symbols and SCENE2_PROTOTYPES are one list of fourteen, every entry refuses NULL;
  libohs_scene.so still exports thirteen names and libohs_hip.so 119;
* k_conv_p1_objects_blend was built without scratch, and every kernel that existed has the figures it had;
* bracket_directions on a measured ring."""
import os
import re

import numpy as np
import pytest

from tests import scene_blend_model as bm
from tests import scene_model as sm
from tests.test_cpu_layout import BAR, BLOCK, make_input, make_layout, rel_rms_per_stream, ring_sofa  # noqa: F401
from tests.test_cpu_scene import _dynamic_symbols, rel_rms_per_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "open_headstage_amd")
GAIN = 0.7
N_DIRS = 7


def _args(sc):
    return (sc["idx"], sc["idx1"], sc["weights"])


def _kw(sc):
    return dict(gains=sc["gains"], prev_idx=sc["prev_idx"], prev_idx1=sc["prev_idx1"], prev_weights=sc["prev_weights"],
                prev_gains=sc["prev_gains"])


# ---- 1. the two evaluations of the rule agree ----------------------------------------------------------------------------------
@pytest.mark.parametrize("K,seg_blocks,shared,fade", [(1, 1, False, True), (3, 2, False, True), (5, 3, True, True), (4, 2, False, False)])
def test_block_wise_model_is_the_direct_evaluation(K, seg_blocks, shared, fade):
    S, blocks = 2, 6
    dirs = make_layout(N_DIRS, 8)
    x = make_input(S, K, blocks, seed=7500 + K)
    sc = bm.make_blend_scene(S, K, blocks, seg_blocks, N_DIRS, seed=K, shared=shared)
    a = bm.model_blend_f64(x, dirs, *_args(sc), seg_blocks, crossfade=fade, gain=GAIN, **_kw(sc))
    b = bm.direct_blend_f64(x, dirs, *_args(sc), seg_blocks, crossfade=fade, gain=GAIN, **_kw(sc))
    err = rel_rms_per_stream(a, b)
    print(f"K = {K}, seg_blocks {seg_blocks}: signals blended against responses blended, relative RMS per stream, worst {err.max():.3e}")
    assert (err <= 1e-13).all(), err


def test_weights_zero_and_one_are_the_one_direction_model():
    S, K, blocks, seg = 2, 3, 6, 2
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S, K, blocks, seed=7600)
    sc = bm.make_blend_scene(S, K, blocks, seg, N_DIRS, seed=5)
    zero, one = np.zeros_like(sc["weights"]), np.ones_like(sc["weights"])
    # w = 0 with idx1 moving by itself, in front of the call too: the one-direction scene on idx, fade for fade; w = 1: on idx1
    moving = np.random.default_rng(76).integers(0, N_DIRS, sc["idx1"].shape).astype(np.uint32)
    pj = (moving[:, 0] + 1) % N_DIRS
    assert (moving[:, 1:] != moving[:, :-1]).any(axis=(0, 2)).all()
    a = bm.model_blend_f64(x, dirs, sc["idx"], moving, zero, seg, sc["gains"], sc["prev_idx"], pj, None, sc["prev_gains"], True, GAIN)
    want = sm.model_scene_f64(x, dirs, sc["idx"], seg, sc["gains"], sc["prev_idx"], sc["prev_gains"], True, GAIN)
    assert np.allclose(a, want, rtol=0, atol=1e-14)
    plan = bm.blend_plan(S, K, blocks, sc["idx"], moving, zero, seg, sc["gains"], sc["prev_idx"], pj, None, sc["prev_gains"], True)
    one_dir = sm.scene_plan(S, K, blocks, sc["idx"], seg, sc["gains"], sc["prev_idx"], sc["prev_gains"], True)
    old_halves = sum(len({p[0] // 2 for p in passes if p[3] is sm.RAMP_G}) for row in one_dir for passes in row)
    assert bm.count_fading_passes(plan) == old_halves > 0 and bm.count_blended_passes(plan, K) == 0
    fixed0 = np.broadcast_to(sc["idx"][:, :1], sc["idx"].shape).copy()
    b = bm.model_blend_f64(x, dirs, fixed0, sc["idx1"], one, seg, sc["gains"], None, sc["prev_idx1"], None, sc["prev_gains"], True, GAIN)
    want = sm.model_scene_f64(x, dirs, sc["idx1"], seg, sc["gains"], sc["prev_idx1"], sc["prev_gains"], True, GAIN)
    assert np.allclose(b, want, rtol=0, atol=1e-14)


def test_a_second_index_changes_an_object_only_beside_a_weight():
    """idx1 alone: a change where the weight is not +0.0 on both sides (-0.0 is not +0.0), none where it is; and the GPU tests' scenes hold
    both, beside changes in w alone"""
    from tests.test_gpu_scene_blend import BLEND_CASES, blend_case
    i0, g = np.zeros((1, 4, 1), np.uint32), np.ones((1, 4, 1), np.float32)
    i1 = np.array([1, 2, 3, 4], np.uint32).reshape(1, 4, 1)
    for w, fades in [([0.0, 0.0, 0.0, 0.0], [0, 0, 0, 0]), ([0.5, 0.5, 0.5, 0.5], [1, 1, 1, 1]), ([0.0, 0.0, 0.5, 0.0], [0, 0, 1, 1]),
                     ([-0.0, -0.0, 0.0, 0.0], [1, 1, 1, 0])]:
        plan = bm.blend_plan(1, 1, 4, i0, i1, np.array(w, np.float32).reshape(1, 4, 1), 1, g, None, np.array([[0]], np.uint32), None, None, True)
        assert [int(any(p[6] for p in passes)) for passes in plan[0]] == fades, (w, fades)
    only_idx1 = zero_idx1 = only_w = 0
    for case in BLEND_CASES:
        _, _, _, sc = blend_case(*case)
        K = case[0]
        rows = [np.broadcast_to(np.asarray(sc[k]).reshape((-1,) + np.shape(sc[k])[-2:]), (3,) + np.shape(sc[k])[-2:]) for k in ("idx", "idx1", "weights", "gains")]
        i, j, w, gn = rows
        same = (i[:, 1:] == i[:, :-1]) & (gn[:, 1:] == gn[:, :-1])
        moved = j[:, 1:] != j[:, :-1]
        blended = (w[:, 1:] != 0) | (w[:, :-1] != 0)
        only_idx1 += int((same & moved & blended & (w[:, 1:] == w[:, :-1])).sum())
        zero_idx1 += int((same & moved & ~blended).sum())
        only_w += int((same & ~moved & (w[:, 1:] != w[:, :-1])).sum())
    print(f"the GPU cases' scenes: {only_idx1} changes in idx1 alone beside a weight, {zero_idx1} beside +0.0, {only_w} in w alone")
    assert only_idx1 > 0 and zero_idx1 > 0 and only_w > 0


def test_two_renders_in_a_row_with_prev_and_the_tail_equal_one():
    S, K, blocks, seg = 2, 3, 8, 2
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S, K, blocks, seed=7700)
    sc = bm.make_blend_scene(S, K, blocks, seg, N_DIRS, seed=3)
    whole, tw = bm.model_blend_f64(x, dirs, *_args(sc), seg, gain=GAIN, with_tail=True, **_kw(sc))
    a, tail = bm.model_blend_f64(x[:, :, :4 * BLOCK], dirs, *(v[:, :2] for v in _args(sc)), seg, gain=GAIN, with_tail=True,
                                 **dict(_kw(sc), gains=sc["gains"][:, :2]))
    b, tb = bm.model_blend_f64(x[:, :, 4 * BLOCK:], dirs, *(v[:, 2:] for v in _args(sc)), seg, sc["gains"][:, 2:], sc["idx"][:, 1],
                               sc["idx1"][:, 1], sc["weights"][:, 1], sc["gains"][:, 1], True, GAIN, tail_in=tail, with_tail=True)
    assert np.allclose(np.concatenate([a, b], axis=2), whole, rtol=0, atol=1e-14)
    assert np.allclose(tb, tw, rtol=0, atol=1e-14)


# ---- 2. the 2 K identity through the existing model ----------------------------------------------------------------------------
def test_model_against_the_2k_identity_through_the_existing_scene_model():
    from tests.test_gpu_scene_blend import BLEND_CASES, blend_case
    worst = 0.0
    for case in BLEND_CASES:
        x, dirs, seg, sc = blend_case(*case)
        for fade in (True, False):
            ref = bm.model_blend_f64(x, dirs, *_args(sc), seg, crossfade=fade, gain=GAIN, **_kw(sc))
            x2, idx2, gains2, pi2, pg2 = bm.as_2k_scene(x, *_args(sc), **_kw(sc))
            y = sm.model_scene_f64(x2, dirs, idx2, seg, gains2, pi2, pg2, fade, GAIN)
            e, eb = rel_rms_per_stream(y, ref), rel_rms_per_block(y, ref)
            print(f"{case}, crossfade {fade}: 2 K objects through scene_model against the blended model: per stream worst {e.max():.3e}, "
                  f"per block worst {eb.max():.3e}")
            assert (e <= BAR).all() and (eb <= BAR).all(), (case, fade, e, eb.max())
            worst = max(worst, float(eb.max()))
    assert worst > 0.0          # (f32 products: the two are not the same arithmetic)


# ---- 3. what a test at the bar sees, on the GPU tests' inputs ------------------------------------------------------------------
def test_mutants_against_the_bar_on_the_gpu_tests_inputs():
    from tests.test_gpu_scene_blend import BLEND_CASES, blend_case
    seen = {m: 0.0 for m in bm.MUTANTS}
    for case in BLEND_CASES:
        x, dirs, seg, sc = blend_case(*case)
        ref = bm.model_blend_f64(x, dirs, *_args(sc), seg, gain=GAIN, **_kw(sc))
        for m in bm.MUTANTS:
            y = bm.model_blend_f64(x, dirs, *_args(sc), seg, gain=GAIN, mutant=m, **_kw(sc))
            e, eb = rel_rms_per_stream(y, ref), rel_rms_per_block(y, ref)
            print(f"{case}: mutant {m}: per stream {e.min():.3e} .. {e.max():.3e}, worst block {eb.max():.3e}")
            seen[m] = max(seen[m], float(e.max()))
    for m in bm.MUTANTS:
        assert seen[m] > 1e3 * BAR, (m, seen[m])        # some case of the GPU file shows the mutant, far above the bar


def test_wide_mutants_are_far_from_every_wide_scene():
    """every scene of tests/test_gpu_scene_wide.py, few loud and all loud, against each wide mutant that exists at its K: more than
    1e3 BAR away in at least one 512-frame block"""
    from tests.test_cpu_scene import wide_mutant_applies
    from tests.test_gpu_scene_wide import WIDE_CASES, kinds_of_change, wide_case
    for K, half in WIDE_CASES:
        for all_loud in (False, True):
            x, dirs, seg, sc = wide_case(K, half, all_loud, True)
            print(f"K = {K}, patterns {3 * half} .. {3 * half + 2}: changes in w alone, in idx1 alone: {kinds_of_change(sc)}")
            ref = bm.model_blend_f64(x, dirs, *_args(sc), seg, gain=GAIN, **_kw(sc))
            for m in bm.WIDE_MUTANTS:
                y = bm.model_blend_f64(x, dirs, *_args(sc), seg, gain=GAIN, mutant=m, **_kw(sc))
                eb = rel_rms_per_block(y, ref)
                print(f"K = {K}, patterns {3 * half} .. {3 * half + 2}, {'all' if all_loud else 'few'} loud: mutant {m}: worst block {eb.max():.3e}")
                if wide_mutant_applies(m, K):
                    assert eb.max() > 1e3 * BAR, (K, half, all_loud, m, eb.max())
                else:
                    assert eb.max() == 0.0, (K, half, all_loud, m, eb.max())


def test_block_wise_model_is_the_direct_evaluation_at_64_objects():
    S, K, blocks, seg = 1, 64, 6, 2
    dirs = make_layout(N_DIRS, 8)
    x = make_input(S, K, blocks, seed=7800)
    sc = bm.make_wide_blend_scene(S, K, blocks, seg, sm.wide_patterns(K)[3:6], None, N_DIRS, seed=64)
    a = bm.model_blend_f64(x, dirs, *_args(sc), seg, gain=GAIN, **_kw(sc))
    b = bm.direct_blend_f64(x, dirs, *_args(sc), seg, gain=GAIN, **_kw(sc))
    err = rel_rms_per_stream(a, b)
    print(f"K = 64: signals blended against responses blended, relative RMS per stream, worst {err.max():.3e}")
    assert (err <= 1e-13).all(), err


def test_the_fuzz_sequences_cover_what_they_name():
    """over the four seeds: both entries, both switch modes, both row forms, gains and every prev_* given and None, every K, every
    seg_blocks, every setter, 64 objects in a blended CROSSFADE call (tests/test_gpu_scene_fuzz.py's generator alone)"""
    from tests.test_gpu_scene_fuzz import KS, SEEDS, SEGS, draw_sequence
    calls = [op[1] for seed in SEEDS for op in draw_sequence(seed) if op[0] == "call"]
    setters = {op[0] for seed in SEEDS for op in draw_sequence(seed) if op[0] != "call"}
    assert setters == {"set_gain", "reset", "set_directions"}, setters
    assert {c["K"] for c in calls} == set(KS) and {c["seg"] for c in calls} == set(SEGS)
    for flag in ("blended", "fade", "shared"):
        assert {c[flag] for c in calls} == {True, False}, flag
    for name in ("gains", "prev_idx", "prev_gains"):
        assert {c[name] is None for c in calls} == {True, False}, name
    for name in ("prev_idx1", "prev_weights"):
        assert {c[name] is None for c in calls if c["blended"]} == {True, False}, name
    assert any(c["K"] == 64 and c["blended"] and c["fade"] for c in calls)
    assert any(c["gains"] is None and c["prev_gains"] is not None and c["shared"] for c in calls)


# ---- 4. the surface ------------------------------------------------------------------------------------------------------------
def test_header_library_and_prototypes_are_one_list_of_fourteen():
    from open_headstage_amd import _ffi, scene, scene2
    hdr = open(os.path.join(ROOT, "include", "ohs_scene2.h")).read()
    declared = sorted(set(re.findall(r"\b(ohs_scene2_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) == 14, declared
    assert declared == sorted(scene2.SCENE2_PROTOTYPES)
    assert declared == _dynamic_symbols(os.path.join(PKG, "libohs_scene2.so"))
    shared = sorted(n.replace("ohs_scene2_", "ohs_scene_", 1) for n in declared if n != "ohs_scene2_process_blended")
    assert shared == sorted(scene.SCENE_PROTOTYPES) and len(shared) == 13
    for n in shared:        # identical signatures, but the launch record's fourth figure
        if n != "ohs_scene_last_launch":
            assert scene.SCENE_PROTOTYPES[n] == scene2.SCENE2_PROTOTYPES[n.replace("ohs_scene_", "ohs_scene2_", 1)], n
    assert len(scene2.SCENE2_PROTOTYPES["ohs_scene2_last_launch"][1]) == 5
    assert len(scene2.SCENE2_PROTOTYPES["ohs_scene2_process_blended"][1]) == len(scene.SCENE_PROTOTYPES["ohs_scene_process"][1]) + 4
    # the two older libraries are what they were
    assert len(_dynamic_symbols(os.path.join(PKG, "libohs_scene.so"))) == 13
    assert _dynamic_symbols(os.path.join(PKG, "libohs_scene.so")) == sorted(scene.SCENE_PROTOTYPES)
    assert len(_dynamic_symbols(os.path.join(PKG, "libohs_hip.so"))) == 119 and len(_ffi.PROTOTYPES) == 119
    emap = open(os.path.join(PKG, "csrc", "scene2_exports.map")).read()
    assert "global: ohs_scene2_*;" in emap and "local: *;" in emap
    for out_of_scope in ("three or more directions", "per-sample weight ramps", "session-renderer", "one partition", "in-place", "node twin",
                         "fades other than one block"):
        assert out_of_scope in hdr, out_of_scope
    doc = open(os.path.join(ROOT, "SCENES.md")).read()
    for name in declared:
        assert re.search(r"\bfn " + name + r"\(", doc), f"{name} is not listed in SCENES.md"
    assert "ohs_scene2_" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_every_entry_refuses_null():
    from open_headstage_amd import _ffi, scene2
    L = scene2.scene2_lib()
    INV = _ffi.OHS_ERR_INVALID_ARG
    assert L.ohs_scene2_create(0, 1, 10, None) == INV
    L.ohs_scene2_destroy(None)
    assert L.ohs_scene2_set_direction_irs(None, 0, None, 0) == INV
    assert L.ohs_scene2_process(None, None, None, 1, 1024, 512, 1024, 512, 1, 1, None, None, 0, None, None, 1, None) == INV
    assert b"NULL" in L.ohs_scene2_last_error()
    assert L.ohs_scene2_process_blended(None, None, None, 1, 1024, 512, 1024, 512, 1, 1, None, None, 0, None, None, 1, None,
                                        None, None, None, None) == INV
    assert b"NULL" in L.ohs_scene2_last_error()
    assert L.ohs_scene2_set_gain(None, 1.0) == INV
    assert L.ohs_scene2_set_eq_band_coeffs(None, 0, None, 0) == INV
    assert L.ohs_scene2_set_eq_enabled(None, 0) == INV
    assert L.ohs_scene2_set_flush_denormals(None, 0) == INV
    assert L.ohs_scene2_reset(None) == INV
    assert L.ohs_scene2_sync(None, None) == INV
    assert L.ohs_scene2_last_launch(None, None, None, None, None) == INV
    assert L.ohs_scene2_status_string(INV) == _ffi.lib().ohs_status_string(INV)
    import open_headstage_amd as ohs
    assert issubclass(ohs.BlendSceneProcessor, ohs.SceneProcessor)
    assert ohs.BlendSceneProcessor.last_launch is not ohs.SceneProcessor.last_launch
    assert callable(ohs.bracket_directions)


# ---- 5. the kernels' resources -------------------------------------------------------------------------------------------------
def test_kernel_resources():
    from open_headstage_amd import build
    res = build.resources()
    fields = ("vgprs", "sgprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd")
    # the new kernel, as built: three waves per SIMD without scratch
    k = res["k_conv_p1_objects_blend"]
    assert k["scratch_bytes_per_lane"] == 0, k
    assert {f: k[f] for f in fields} == {"vgprs": 168, "sgprs": 102, "scratch_bytes_per_lane": 0, "occupancy_waves_per_simd": 3}, k
    assert k["agprs"] == 0, k
    # every kernel that existed is the code it was
    assert {f: res["k_conv_p1_objects"][f] for f in fields} == \
        {"vgprs": 165, "sgprs": 86, "scratch_bytes_per_lane": 0, "occupancy_waves_per_simd": 3}
    assert {f: res["k_conv_p1_layout"][f] for f in fields} == \
        {"vgprs": 157, "sgprs": 54, "scratch_bytes_per_lane": 0, "occupancy_waves_per_simd": 3}
    assert {f: res["k_conv_p1_layout_irs"][f] for f in fields} == \
        {"vgprs": 162, "sgprs": 64, "scratch_bytes_per_lane": 0, "occupancy_waves_per_simd": 3}
    assert build.is_current() and os.path.exists(build.SCENE_LIB) and os.path.exists(build.SCENE2_LIB)


# ---- 6. the host helper --------------------------------------------------------------------------------------------------------
def test_bracket_directions_on_a_ring(ring_sofa):  # noqa: F811
    from open_headstage_amd import scene, scene2
    pos = np.stack([ring_sofa.position(m) for m in range(ring_sofa.num_measurements)]).astype(np.float32)
    M = pos.shape[0]
    # a query on a measurement: that measurement, w = 0
    i0, i1, w = scene2.bracket_directions(pos, pos[:, 0], pos[:, 1], float(pos[0, 2]))
    assert i0.dtype == np.uint32 and i1.dtype == np.uint32 and w.dtype == np.float32
    assert (i0 == np.arange(M)).all() and (w == 0).all()
    # midway between two ring neighbours: those two, w = 0.5
    ring = np.flatnonzero(pos[:, 1] == pos[0, 1])
    order = ring[np.argsort(pos[ring, 0])]
    a, b = order[:-1], order[1:]
    assert (np.diff(pos[order, 0]) > 0).all() and len(order) >= 3
    mid = ((pos[a, 0].astype(np.float64) + pos[b, 0]) / 2).astype(np.float32)
    el = pos[a, 1]
    i0, i1, w = scene2.bracket_directions(pos, mid, el, float(pos[0, 2]))
    for j in range(len(a)):
        assert {int(i0[j]), int(i1[j])} == {int(a[j]), int(b[j])}, (j, i0[j], i1[j], a[j], b[j])
    assert np.abs(w - 0.5).max() < 1e-4, w
    # idx0 is nearest_directions, anywhere; shapes broadcast; w in [0, 1]
    rng = np.random.default_rng(78)
    az = rng.uniform(-360.0, 360.0, 120).astype(np.float32)
    elq = rng.uniform(-60.0, 60.0, 120).astype(np.float32)
    i0, i1, w = scene2.bracket_directions(pos, az.reshape(4, 30), elq.reshape(4, 30))
    assert i0.shape == (4, 30) and (i0 == scene.nearest_directions(pos, az.reshape(4, 30), elq.reshape(4, 30))).all()
    assert (i1 != i0).all() and (w >= 0).all() and (w <= 1).all()
    # a quarter of the way along a ring: w = the chord's fraction of a point a quarter along the arc (below 0.25 + a little)
    q = (pos[a[0], 0] + 0.25 * (pos[b[0], 0] - pos[a[0], 0])).astype(np.float32)
    j0, j1, wq = scene2.bracket_directions(pos, q, el[0], float(pos[0, 2]))
    assert int(j0) == int(a[0]) and int(j1) == int(b[0]) and 0.2 < float(wq) < 0.3, (j0, j1, wq)
    # a table of one direction
    k0, k1, wk = scene2.bracket_directions(pos[:1], az[:5], elq[:5])
    assert (k0 == 0).all() and (k1 == 0).all() and (wk == 0).all()

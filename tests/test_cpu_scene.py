"""Object scenes (libohs_scene.so, include/ohs_scene.h), the part that needs no GPU.

* the block-wise f64 model of tests/scene_model.py agrees with the direct time-domain evaluation of the same rules, and carries prev_*
  and the tail over a cut;
* on the GPU tests' inputs three wrong readings of the rules -- a gain change that does not fade, the pair's partner taken from the
  wrong object, `old` taken from two segments back -- are far above the project's FFT bar (1e-6 relative RMS per stream, DESIGN
  section 2), per stream and in the worst 512-frame block; fading EVERY pair when one changes is the same mathematics and stays below
  it, which is why that case is compared in bits only where the header promises them;
* on the wide scenes of tests/test_gpu_scene_wide.py (K = 33, 63, 64) three more -- a change set cut to 32 bits, an old half that
  stops in front of pair 31, an odd K's missing partner rendered instead of silent -- are more than 1e3 times the bar away in some
  block of every scene, and the model still equals the direct evaluation at K = 64;
* the header's names, the library's dynamic symbols and SCENE_PROTOTYPES are one list, every entry refuses NULL, and libohs_hip.so
  still exports exactly ohs_hip.h's 119;
* k_conv_p1_objects was built without scratch at three waves per SIMD, the layout kernels have the figures they had;
* nearest_directions is MySofa.nearest, rotate_sources with pitch = roll = 0 the yaw rule of layout_yaw_irs;
* without a device ohs_scene_create answers NO_DEVICE."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import scene_model as sm
from tests.test_cpu_layout import BAR, BLOCK, make_input, make_layout, rel_rms_per_stream, ring_sofa  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "open_headstage_amd")
GAIN = 0.7
N_DIRS = 7


def rel_rms_per_block(test, ref):
    """[S][n_blocks]: the relative RMS of every 512-frame block (both ears), against that block's reference"""
    t, r = np.asarray(test, np.float64), np.asarray(ref, np.float64)
    S, _, frames = r.shape
    t, r = t.reshape(S, 2, frames // BLOCK, BLOCK), r.reshape(S, 2, frames // BLOCK, BLOCK)
    return np.sqrt(np.mean((t - r) ** 2, axis=(1, 3))) / np.sqrt(np.mean(r ** 2, axis=(1, 3)))


# ---- 1. the two evaluations of the rules agree ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K,seg_blocks,shared,fade", [(1, 1, False, True), (3, 2, False, True), (5, 3, True, True), (2, 2, False, False)])
def test_block_wise_model_is_the_direct_evaluation(K, seg_blocks, shared, fade):
    S, blocks = 2, 6
    dirs = make_layout(N_DIRS, 8)
    x = make_input(S, K, blocks, seed=7000 + K)
    idx, gains, pi, pg = sm.make_scene(S, K, blocks, seg_blocks, N_DIRS, seed=K, shared=shared)
    a = sm.model_scene_f64(x, dirs, idx, seg_blocks, gains, pi, pg, fade, GAIN)
    b = sm.direct_scene_f64(x, dirs, idx, seg_blocks, gains, pi, pg, fade, GAIN)
    err = rel_rms_per_stream(a, b)
    print(f"K = {K}, seg_blocks {seg_blocks}: block-wise against direct, relative RMS per stream, worst {err.max():.3e}")
    assert (err <= 1e-13).all(), err


def test_static_scene_with_unit_gains_is_the_layout_model(oracle):
    from tests.test_cpu_layout import model_layout_f64
    S, K, blocks = 2, 3, 4
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S, K, blocks, seed=7100)
    row = np.array([4, 0, 6], np.uint32)
    y = sm.model_scene_f64(x, dirs, np.repeat(row[None], 2, axis=0), 2, None, None, None, True, GAIN)
    want = model_layout_f64(oracle, x, dirs[row], GAIN)
    err = rel_rms_per_stream(y, want)
    assert (err <= 1e-13).all(), err


def test_two_renders_in_a_row_with_prev_and_the_tail_equal_one():
    S, K, blocks, seg = 2, 3, 8, 2
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S, K, blocks, seed=7200)
    idx, gains, pi, pg = sm.make_scene(S, K, blocks, seg, N_DIRS, seed=3)
    whole, tw = sm.model_scene_f64(x, dirs, idx, seg, gains, pi, pg, True, GAIN, with_tail=True)
    a, tail = sm.model_scene_f64(x[:, :, :4 * BLOCK], dirs, idx[:, :2], seg, gains[:, :2], pi, pg, True, GAIN, with_tail=True)
    b, tb = sm.model_scene_f64(x[:, :, 4 * BLOCK:], dirs, idx[:, 2:], seg, gains[:, 2:], idx[:, 1], gains[:, 1], True, GAIN,
                               tail_in=tail, with_tail=True)
    assert np.allclose(np.concatenate([a, b], axis=2), whole, rtol=0, atol=1e-14)
    assert np.allclose(tb, tw, rtol=0, atol=1e-14)


# ---- 2. what a test at the bar sees, on the GPU tests' inputs ---------------------------------------------------------------------
def test_mutants_against_the_bar_on_the_gpu_tests_inputs():
    from tests.test_gpu_scene import TRAJECTORY_CASES, trajectory_case
    seen = {m: 0.0 for m in sm.MUTANTS}
    for case in TRAJECTORY_CASES:
        x, dirs, idx, seg, gains, pi, pg = trajectory_case(*case)
        ref = sm.model_scene_f64(x, dirs, idx, seg, gains, pi, pg, True, GAIN)
        for m in sm.MUTANTS:
            y = sm.model_scene_f64(x, dirs, idx, seg, gains, pi, pg, True, GAIN, mutant=m)
            e, eb = rel_rms_per_stream(y, ref), rel_rms_per_block(y, ref)
            print(f"{case}: mutant {m}: per stream {e.min():.3e} .. {e.max():.3e}, worst block {eb.max():.3e}")
            if m == "fade_all":
                assert (e <= BAR).all() and (eb <= BAR).all(), (case, m, e, eb.max())
            seen[m] = max(seen[m], float(e.max()))
    for m in ("gain_no_fade", "wrong_partner", "old_two_back"):
        assert seen[m] > 1e3 * BAR, (m, seen[m])       # some case of the GPU file shows the mutant, far above the bar
    assert 0.0 < seen["fade_all"] <= BAR, seen


def wide_mutant_applies(m, K):
    """mask32 needs an object past 31 (every wide K), pair31_dropped a pair 31 (K >= 63), odd_partner_row0 an odd K"""
    return {"mask32": K > 32, "pair31_dropped": K >= 63, "odd_partner_row0": K % 2 == 1}[m]


def test_wide_mutants_are_far_from_every_wide_scene():
    """every scene of tests/test_gpu_scene_wide.py, few loud and all loud, against each wide mutant that exists at its K: more than
    1e3 BAR away in at least one 512-frame block"""
    from tests.test_gpu_scene_wide import WIDE_CASES, wide_case
    for K, half in WIDE_CASES:
        assert [m for m in sm.WIDE_MUTANTS if wide_mutant_applies(m, K)], K
        for all_loud in (False, True):
            x, dirs, seg, (idx, gains, pi, pg) = wide_case(K, half, all_loud, False)
            ref = sm.model_scene_f64(x, dirs, idx, seg, gains, pi, pg, True, GAIN)
            for m in sm.WIDE_MUTANTS:
                y = sm.model_scene_f64(x, dirs, idx, seg, gains, pi, pg, True, GAIN, mutant=m)
                eb = rel_rms_per_block(y, ref)
                print(f"K = {K}, patterns {3 * half} .. {3 * half + 2}, {'all' if all_loud else 'few'} loud: mutant {m}: worst block {eb.max():.3e}")
                if wide_mutant_applies(m, K):
                    assert eb.max() > 1e3 * BAR, (K, half, all_loud, m, eb.max())
                else:
                    assert eb.max() == 0.0, (K, half, all_loud, m, eb.max())


def test_block_wise_model_is_the_direct_evaluation_at_64_objects():
    S, K, blocks, seg = 1, 64, 6, 2
    dirs = make_layout(N_DIRS, 8)
    x = make_input(S, K, blocks, seed=7300)
    idx, gains, pi, pg = sm.make_wide_scene(S, K, blocks, seg, sm.wide_patterns(K)[3:6], None, N_DIRS, seed=64)
    a = sm.model_scene_f64(x, dirs, idx, seg, gains, pi, pg, True, GAIN)
    b = sm.direct_scene_f64(x, dirs, idx, seg, gains, pi, pg, True, GAIN)
    err = rel_rms_per_stream(a, b)
    print(f"K = 64: block-wise against direct, relative RMS per stream, worst {err.max():.3e}")
    assert (err <= 1e-13).all(), err


# ---- 3. the surface -------------------------------------------------------------------------------------------------------------
def _dynamic_symbols(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    return sorted(l.split()[-1].split("@")[0] for l in out.splitlines() if l.split() and l.split()[-2] in "TtWwBbDdRr")


def test_header_library_and_prototypes_are_one_list():
    from open_headstage_amd import _ffi, scene
    hdr = open(os.path.join(ROOT, "include", "ohs_scene.h")).read()
    declared = sorted(set(re.findall(r"\b(ohs_scene_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) == 13, declared
    assert declared == sorted(scene.SCENE_PROTOTYPES)
    assert declared == _dynamic_symbols(os.path.join(PKG, "libohs_scene.so"))
    assert not set(declared) & set(_ffi.PROTOTYPES) and len(_ffi.PROTOTYPES) == 119
    main_hdr = open(os.path.join(ROOT, "include", "ohs_hip.h")).read()
    main = sorted(set(re.findall(r"\b(ohs_[a-z0-9_]+)\s*\(", main_hdr)))
    assert len(main) == 119 and main == _dynamic_symbols(os.path.join(PKG, "libohs_hip.so"))
    emap = open(os.path.join(PKG, "csrc", "scene_exports.map")).read()
    assert "global: ohs_scene_*;" in emap and "local: *;" in emap
    for out_of_scope in ("session-renderer", "interpolation", "one partition", "in-place", "node twin", "fades other than one block"):
        assert out_of_scope in hdr, out_of_scope
    doc = open(os.path.join(ROOT, "SCENES.md")).read()
    for name in declared:
        assert re.search(r"\bfn " + name + r"\(", doc), f"{name} is not listed in SCENES.md"
    assert "ohs_scene_" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_every_entry_refuses_null():
    from open_headstage_amd import _ffi, scene
    L = scene.scene_lib()
    INV = _ffi.OHS_ERR_INVALID_ARG
    assert L.ohs_scene_create(0, 1, 10, None) == INV
    L.ohs_scene_destroy(None)
    assert L.ohs_scene_set_direction_irs(None, 0, None, 0) == INV
    assert L.ohs_scene_process(None, None, None, 1, 1024, 512, 1024, 512, 1, 1, None, None, 0, None, None, 1, None) == INV
    assert b"NULL" in L.ohs_scene_last_error()
    assert L.ohs_scene_set_gain(None, 1.0) == INV
    assert L.ohs_scene_set_eq_band_coeffs(None, 0, None, 0) == INV
    assert L.ohs_scene_set_eq_enabled(None, 0) == INV
    assert L.ohs_scene_set_flush_denormals(None, 0) == INV
    assert L.ohs_scene_reset(None) == INV
    assert L.ohs_scene_sync(None, None) == INV
    assert L.ohs_scene_last_launch(None, None, None, None) == INV
    assert L.ohs_scene_status_string(INV) == _ffi.lib().ohs_status_string(INV)
    import open_headstage_amd as ohs
    for m in ("set_directions", "set_directions_from_sofa", "process", "process_ptr", "set_gain", "set_band_coeffs", "set_eq_enabled",
              "set_flush_denormals", "reset", "last_launch"):
        assert hasattr(ohs.SceneProcessor, m), m


def test_without_a_device_create_answers_no_device():
    from open_headstage_amd import _ffi, scene
    n = C.c_int(0)
    have = _ffi.lib().ohs_device_count(C.byref(n)) == _ffi.OHS_OK and n.value > 0
    h = C.c_void_p(1)
    rc = scene.scene_lib().ohs_scene_create(0, 2, 10, C.byref(h))
    if have:                    # (a machine with a GPU: the handle comes and goes)
        assert rc == _ffi.OHS_OK and h.value
        scene.scene_lib().ohs_scene_destroy(h)
        return
    assert rc == _ffi.OHS_ERR_NO_DEVICE and not h.value
    with pytest.raises(scene.SceneError) as ei:
        scene.SceneProcessor(2)
    assert ei.value.status == _ffi.OHS_ERR_NO_DEVICE


# ---- 4. the kernel's resources ----------------------------------------------------------------------------------------------------
def test_kernel_resources():
    from open_headstage_amd import build
    res = build.resources()
    k = res["k_conv_p1_objects"]
    assert k["scratch_bytes_per_lane"] == 0, k
    assert k["occupancy_waves_per_simd"] == 3 and k["occupancy_waves_per_simd"] >= 2, k       # what the shipped build gives
    assert k["vgprs"] <= 168 and k["agprs"] == 0, k
    # the layout kernels are the code they were before this kernel existed
    assert {f: res["k_conv_p1_layout"][f] for f in ("vgprs", "sgprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd")} == \
        {"vgprs": 157, "sgprs": 54, "scratch_bytes_per_lane": 0, "occupancy_waves_per_simd": 3}
    assert {f: res["k_conv_p1_layout_irs"][f] for f in ("vgprs", "sgprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd")} == \
        {"vgprs": 162, "sgprs": 64, "scratch_bytes_per_lane": 0, "occupancy_waves_per_simd": 3}
    assert build.is_current() and os.path.exists(build.SCENE_LIB)


# ---- 5. the host helpers ------------------------------------------------------------------------------------------------------------
def test_nearest_directions_is_mysofa_nearest(ring_sofa):  # noqa: F811
    from open_headstage_amd import scene
    pos = np.stack([ring_sofa.position(m) for m in range(ring_sofa.num_measurements)])
    rng = np.random.default_rng(77)
    az = rng.uniform(-360.0, 360.0, 300).astype(np.float32)
    el = rng.uniform(-60.0, 60.0, 300).astype(np.float32)
    got = scene.nearest_directions(pos, az, el)
    want = np.array([ring_sofa.nearest(float(a), float(e)) for a, e in zip(az, el)], np.uint32)
    assert got.dtype == np.uint32 and (got == want).all(), np.flatnonzero(got != want)
    assert scene.nearest_directions(pos, az.reshape(3, 100), el.reshape(3, 100)).shape == (3, 100)


def test_rotate_sources_with_yaw_only_is_the_yaw_rule_of_layout_yaw_irs(ring_sofa):  # noqa: F811
    from open_headstage_amd import scene, sofa, synth
    az = np.array([-30.0, 30.0, 0.0, 110.0, -110.0, 179.0], np.float32)
    el = np.zeros(6, np.float32)
    yaws = np.array([0.0, 10.0, -25.0, 170.0, 200.0, -179.5, 360.0], np.float32)
    a2, e2 = scene.rotate_sources(az[None, :], el[None, :], yaws[:, None])
    assert a2.shape == (7, 6) and a2.dtype == np.float32 and (e2 == 0).all()
    assert (a2 >= -180.0).all() and (a2 < 180.0).all()
    table = sofa.layout_yaw_irs(ring_sofa, az, el, yaws, 1.0, synth.FS)
    for j in range(len(yaws)):
        assert sofa.layout_irs(ring_sofa, a2[j], e2[j], 1.0, synth.FS, table.shape[3]).tobytes() == table[j].tobytes(), j
    # a full rotation matrix: yaw alone gives the same angles, and pitch moves a frontal source down by the pitch
    a3, e3 = scene.rotate_sources(az[None, :], el[None, :], yaws[:, None], 1e-30, 0.0)
    d = (a3.astype(np.float64) - a2 + 180.0) % 360.0 - 180.0
    assert np.abs(d).max() < 1e-3 and np.abs(e3).max() < 1e-3
    a4, e4 = scene.rotate_sources(0.0, 0.0, 0.0, 20.0, 0.0)
    assert abs(float(a4)) < 1e-4 and abs(float(e4) + 20.0) < 1e-4

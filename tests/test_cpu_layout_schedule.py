"""A schedule of speaker layouts (ohs_batch_process_layout_scheduled), the part that needs no GPU: the yardsticks of
tests/test_gpu_layout_schedule.py are checked against each other here, and the GPU file imports them from this one.

The f64 model is the definition of the call.  fade_plan (tests/test_cpu_ir_crossfade.py) names, per stream and block, the set `cur`
of the block's segment and the set `old` in front of it; every set j of the table then sees the input x_j -- x where cur == old == j,
x f where cur == j and x g where old == j in a fading block (f[n] = n / 512, g[n] = (512 - n) / 512, one f32 multiplication per
sample and channel), zero elsewhere -- and

    y = sum_j model_layout_f64(x_j, table[j])            (tests/test_cpu_layout.py: direct convolution in f64)

* constant rows are model_layout_f64 exactly;
* with two channels the model is model_ir_crossfade on the sets [Lsl, Lsr, Rsl, Rsr] = table[j][0][0], [0][1], [1][0], [1][1];
* on the GPU tests' inputs RING_OUT and CROSSFADE, and two different tables, are far more than the 1e-6 bar apart;
* two renders in a row, the second given prev and the first one's tail, equal one render;
* the four entries are in the header, the ctypes prototypes, the library and INTEGRATION.md, and refuse NULL;
* ohs_sofa_layout_yaw_irs is ohs_sofa_layout_irs at the rotated angles, set for set;
* k_conv_p1_layout_irs was built without scratch at three waves per SIMD, and k_conv_p1_layout still is."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_cpu_ir_crossfade import RAMP_F, RAMP_G, fade_plan, model_ir_crossfade
from tests.test_cpu_ir_schedule import make_rows
from tests.test_cpu_layout import BAR, BLOCK, make_input, make_layout, model_layout_f64, rel_rms_per_stream, ring_sofa  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ohs_batch_set_layout_schedule_irs", "ohs_batch_process_layout_scheduled", "ohs_batch_last_layout_scheduled",
         "ohs_sofa_layout_yaw_irs"]
RING_OUT, CROSSFADE = 0, 1


# ---- inputs shared with the GPU tests -----------------------------------------------------------------------------------------
def make_table(n_sets, K, taps=512, seed=0):
    """[n_sets][K][2][taps] float32: make_layout(K, taps, seed + j) per set -- unrelated responses from set to set"""
    return np.stack([make_layout(K, taps, seed=seed + j) for j in range(n_sets)])


# ---- the f64 model ------------------------------------------------------------------------------------------------------------
def split_by_set(x, n_sets, cur, old):
    """x [S][>= K][n * 512] float32 -> {j: x_j float32}, only the sets that see any input"""
    x = np.asarray(x, np.float32)
    out = {}
    for s in range(x.shape[0]):
        for t in range(cur.shape[1]):
            sl = slice(t * BLOCK, (t + 1) * BLOCK)
            c, o = int(cur[s, t]), int(old[s, t])
            parts = [(c, x[s, :, sl])] if c == o else [(o, x[s, :, sl] * RAMP_G), (c, x[s, :, sl] * RAMP_F)]
            for j, v in parts:
                assert 0 <= j < n_sets
                out.setdefault(j, np.zeros_like(x))[s, :, sl] = v
    return out


def model_layout_schedule_f64(oracle, x, table, idx, seg_blocks, prev=None, crossfade=True, gain=1.0, tail_in=None, with_tail=False):
    """x [S][>= K][n * 512] float32, table [n_sets][K][2][len], idx a row [n_segs] for all streams or rows [S][n_segs]; prev: the set
    in front of the call's first block (a scalar or [S]; None: no boundary there; ignored unless crossfade); tail_in [S][2][512] f64:
    what an earlier render left (already times gain) -> gain * y [S][2][n * 512] f64 (with_tail: and the tail it leaves)"""
    x = np.asarray(x, np.float32)
    table = np.asarray(table, np.float32)
    S, n = x.shape[0], x.shape[2] // BLOCK
    cur, old = fade_plan(S, n, idx, seg_blocks, prev if crossfade else None)
    if not crossfade:
        old = cur
    y = np.zeros((S, 2, (n + 1) * BLOCK), np.float64)
    pad = np.zeros((S, x.shape[1], BLOCK), np.float32)
    for j, xj in sorted(split_by_set(x, table.shape[0], cur, old).items()):
        y += model_layout_f64(oracle, np.concatenate([xj, pad], axis=2), table[j], gain)
    if tail_in is not None:
        y[:, :, :BLOCK] += tail_in
    return (y[:, :, :n * BLOCK], y[:, :, n * BLOCK:]) if with_tail else y[:, :, :n * BLOCK]


# ---- 1. constant rows are the layout model, exactly ---------------------------------------------------------------------------
def test_constant_rows_are_exactly_the_layout_model(oracle):
    K = 3
    table = make_table(4, K)
    x = make_input(3, K, 7, seed=2000)
    rows = np.array([[2] * 4, [0] * 4, [3] * 4], np.uint32)
    for idx, prev in [(rows, None), (rows, rows[:, 0]), (rows[0], None), (rows[0], 2)]:
        for fade in (True, False):
            y = model_layout_schedule_f64(oracle, x, table, idx, 2, prev, fade, 0.7)
            r = np.broadcast_to(idx, (3, 4))
            for s in range(3):
                want = model_layout_f64(oracle, x[s:s + 1], table[int(r[s, 0])], 0.7)
                assert np.abs(y[s:s + 1] - want).max() == 0.0, (s, fade)


# ---- 2. two channels: the crossfade model of the stereo call ------------------------------------------------------------------
@pytest.mark.parametrize("seg_blocks", [1, 2, 3])
def test_two_channels_are_the_ir_crossfade_model(oracle, seg_blocks):
    S, blocks = 3, 9
    table = make_table(5, 2)
    sets = table.reshape(5, 4, -1)          # [Lsl, Lsr, Rsl, Rsr] = [0][0], [0][1], [1][0], [1][1]
    x = make_input(S, 2, blocks, seed=2100)
    idx = make_rows(S, -(-blocks // seg_blocks), 5)
    prev = np.array([4, 3, 2])
    y = model_layout_schedule_f64(oracle, x, table, idx, seg_blocks, prev)
    ref, _ = model_ir_crossfade(oracle, x, sets, idx, seg_blocks, prev)
    err = rel_rms_per_stream(y, ref)
    print(f"K = 2, seg_blocks {seg_blocks}: against model_ir_crossfade, relative RMS per stream, worst {err.max():.3e}")
    assert (err <= 1e-12).all(), err


# ---- 3. a test at the bar tells the modes, and two tables, apart ----------------------------------------------------------------
def test_modes_and_tables_differ_by_far_more_than_the_bar_on_the_gpu_tests_inputs(oracle):
    S, blocks, K, n_sets = 5, 13, 6, 5
    table, other = make_table(n_sets, K), make_table(n_sets, K, seed=50)
    x = make_input(S, K, blocks, seed=3100)
    for seg in (1, 2, 5):
        idx = make_rows(S, -(-blocks // seg), n_sets)
        prev = (idx[:, 0] + 1) % n_sets
        xf = model_layout_schedule_f64(oracle, x, table, idx, seg, prev, True, 0.7)
        ro = model_layout_schedule_f64(oracle, x, table, idx, seg, prev, False, 0.7)
        ot = model_layout_schedule_f64(oracle, x, other, idx, seg, prev, True, 0.7)
        da, db = rel_rms_per_stream(xf, ro), rel_rms_per_stream(xf, ot)
        print(f"seg_blocks {seg}: CROSSFADE against RING_OUT {da.min():.3f} .. {da.max():.3f}, against another table "
              f"{db.min():.3f} .. {db.max():.3f}")
        assert (da > 1e-3).all() and (db > 1e-3).all(), (seg, da, db)


# ---- 4. prev and the tail carry over a call boundary --------------------------------------------------------------------------
def test_two_renders_in_a_row_with_prev_and_the_tail_equal_one(oracle):
    S, K, n_sets = 2, 3, 4
    table = make_table(n_sets, K)
    x = make_input(S, K, 8, seed=2200)
    idx = make_rows(S, 4, n_sets)
    whole, tw = model_layout_schedule_f64(oracle, x, table, idx, 2, None, True, 0.7, with_tail=True)
    a, tail = model_layout_schedule_f64(oracle, x[:, :, :4 * BLOCK], table, idx[:, :2], 2, None, True, 0.7, with_tail=True)
    b, tb = model_layout_schedule_f64(oracle, x[:, :, 4 * BLOCK:], table, idx[:, 2:], 2, idx[:, 1], True, 0.7, tail_in=tail, with_tail=True)
    assert np.allclose(np.concatenate([a, b], axis=2), whole, rtol=0, atol=1e-15)
    assert np.allclose(tb, tw, rtol=0, atol=1e-15)
    # ... and without prev the second render's first block does not fade: far off
    c = model_layout_schedule_f64(oracle, x[:, :, 4 * BLOCK:], table, idx[:, 2:], 2, None, True, 0.7, tail_in=tail)
    d = rel_rms_per_stream(c, whole[:, :, 4 * BLOCK:])
    print("second render without prev: relative RMS", d)
    assert (d > 1e-3).all(), d


# ---- 5. the entries exist -----------------------------------------------------------------------------------------------------
def test_entries_are_declared_listed_exported_and_refuse_null():
    from open_headstage_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "ohs_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    emap = open(os.path.join(ROOT, "open_headstage_amd", "csrc", "exports.map")).read()
    declared = set(re.findall(r"\b(ohs_[a-z0-9_]+)\s*\(", hdr))
    L = _ffi.lib()
    assert "ohs_*" in emap
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/ohs_hip.h"
        assert re.search(r"\bfn " + name + r"\(", doc), f"{name} is not listed in INTEGRATION.md"
        assert name in _ffi.PROTOTYPES, f"{name} has no ctypes prototype"
        assert hasattr(L, name), f"{name} is not exported"
    assert re.search(r"OHS_LAYOUT_SWITCH_RING_OUT = 0, OHS_LAYOUT_SWITCH_CROSSFADE = 1", hdr)
    INV = _ffi.OHS_ERR_INVALID_ARG
    assert L.ohs_batch_set_layout_schedule_irs(None, 0, 0, None, 0) == INV
    assert L.ohs_batch_process_layout_scheduled(None, None, None, 1, 3072, 512, 1024, 512, 1, None, 0, None, 1, None) == INV
    assert L.ohs_batch_last_layout_scheduled(None, None) == INV
    assert L.ohs_sofa_layout_yaw_irs(None, 2, None, None, 1.0, 0.0, 1, None, None, 0, None) == INV
    import open_headstage_amd as ohs
    from open_headstage_amd import sofa
    for m in ("set_layout_table", "set_layout_table_yaws", "process_layout_scheduled", "process_layout_scheduled_ptr",
              "last_layout_scheduled"):
        assert hasattr(ohs.BatchProcessor, m), m
    assert hasattr(sofa, "layout_yaw_irs")
    for text in (open(os.path.join(ROOT, "README.md")).read(), open(os.path.join(ROOT, "DESIGN.md")).read()):
        assert "119 entr" in text and not re.search(r"\b11[0-8] entr", text)
    assert len(declared) == 119, len(declared)


# ---- 6. ohs_sofa_layout_yaw_irs is ohs_sofa_layout_irs at the rotated angles ---------------------------------------------------
def _wrap(a):
    return (np.asarray(a, np.float64) + 180.0) % 360.0 - 180.0


def test_sofa_layout_yaw_irs_is_layout_irs_at_the_rotated_angles(ring_sofa):  # noqa: F811
    import open_headstage_amd as ohs
    from open_headstage_amd import sofa, synth
    az, el = [r[1] for r in ohs.LAYOUT_5_1], [r[2] for r in ohs.LAYOUT_5_1]
    yaws = [0.0, 30.0, -100.0]
    tab = sofa.layout_yaw_irs(ring_sofa, az, el, yaws, 1.0, synth.FS)
    assert tab.shape == (3, 6, 2, 160)
    for j, yaw in enumerate(yaws):
        rot = _wrap(np.array(az) - yaw)
        assert (np.abs(rot) <= 180.0).all()
        want = sofa.layout_irs(ring_sofa, rot, el, 1.0, synth.FS)
        assert tab[j].tobytes() == want.tobytes(), yaw
    assert any(abs(a - (-100.0)) > 180.0 for a in az)            # (Rs at 110 - (-100) = 210: across the wrap)
    assert tab[0].tobytes() == sofa.layout_irs(ring_sofa, az, el, 1.0, synth.FS).tobytes()
    assert tab[0].tobytes() != tab[1].tobytes() and tab[1].tobytes() != tab[2].tobytes()
    # yaw to the right by 30: the left speaker at -30 is heard where a speaker at -60 stands
    assert tab[1, 0].tobytes() == sofa.layout_irs(ring_sofa, [-60.0], [0.0], 1.0, synth.FS)[0].tobytes()


def test_sofa_layout_yaw_irs_query_short_len_and_refusals(ring_sofa):  # noqa: F811
    from open_headstage_amd import _ffi, synth
    L = _ffi.lib()
    az = np.array([-30.0, 30.0, 0.0], np.float32)
    el = np.zeros(3, np.float32)
    yaw = np.array([0.0, 45.0], np.float32)
    n = C.c_size_t(0)
    azp, elp, yp = az.ctypes.data_as(_ffi.fp), el.ctypes.data_as(_ffi.fp), yaw.ctypes.data_as(_ffi.fp)
    f = L.ohs_sofa_layout_yaw_irs
    assert f(ring_sofa._h, 3, azp, elp, 1.0, synth.FS, 2, yp, None, 0, C.byref(n)) == _ffi.OHS_OK
    assert n.value == 160
    out = np.full((2, 3, 2, 200), 7.0, np.float32)
    n.value = 0
    assert f(ring_sofa._h, 3, azp, elp, 1.0, synth.FS, 2, yp, out.ctypes.data_as(_ffi.fp), 159, C.byref(n)) == _ffi.OHS_ERR_INVALID_ARG
    assert (out == 7.0).all() and n.value == 160        # nothing written, the length still reported
    assert f(ring_sofa._h, 3, azp, elp, 1.0, synth.FS, 2, yp, out.ctypes.data_as(_ffi.fp), 200, C.byref(n)) == _ffi.OHS_OK
    assert out[:, :, :, :160].any() and not out[:, :, :, 160:].any()
    INV = _ffi.OHS_ERR_INVALID_ARG
    assert f(ring_sofa._h, 3, azp, elp, 1.0, synth.FS, 0, yp, None, 0, C.byref(n)) == INV
    assert f(ring_sofa._h, 0, azp, elp, 1.0, synth.FS, 2, yp, None, 0, C.byref(n)) == INV
    assert f(ring_sofa._h, 17, azp, elp, 1.0, synth.FS, 2, yp, None, 0, C.byref(n)) == INV
    assert f(ring_sofa._h, 3, azp, elp, 1.0, synth.FS, 2, None, None, 0, C.byref(n)) == INV
    assert f(ring_sofa._h, 3, azp, elp, 1.0, synth.FS, 2, yp, None, 0, None) == INV


# ---- 7. the kernels' resources -------------------------------------------------------------------------------------------------
def test_scheduled_layout_kernel_has_no_scratch_at_three_waves_per_simd():
    """Figures hipcc reported when the library was built"""
    from open_headstage_amd import _ffi, build
    _ffi.lib()
    res = build.resources()
    for name in ("k_conv_p1_layout_irs", "k_conv_p1_layout"):
        assert name in res, sorted(res)
        k = res[name]
        print(name, k)
        assert k["scratch_bytes_per_lane"] == 0, (name, k)
        assert k["occupancy_waves_per_simd"] >= 3, (name, k)

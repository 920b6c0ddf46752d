"""Crossfaded IR-scheduled batch calls (ohs_batch_process_ir_crossfaded), the part that needs no GPU: the f64 model the GPU tests
of tests/test_gpu_ir_crossfade.py measure against, and its properties.

The model is built from render_f64 of tests/test_cpu_ir_schedule.py (direct convolution in f64, a set per block, per-path
tails).  Block t of stream s has the set of its segment, cur, and a set it fades from, old (the previous segment's in the first
block of a segment, `prev` in the first block of the call, cur everywhere else).  Where old != cur the block's input is split
in float32 by the exact ramps f[n] = n / 512 and g[n] = (512 - n) / 512, and

    y = render_f64(x_new, the rows) + render_f64(x_old, the rows moved one segment on)

with x_new = x f and x_old = x g in the fading blocks, x and 0 in all others: every tail rings out, nothing is cut.

* constant rows are exactly the RING_OUT model;
* on the GPU tests' inputs the model is far from both existing modes, so a test at the 1e-6 bar tells the three apart;
* equal sets under different indices give the plain render (the ramps sum to one);
* `prev` and the per-path tails carry a render over a call boundary;
* a sine through two sets 6 dB apart keeps the input's smoothness, where RING_OUT puts a step at every boundary;
* the entry is in the header, the ctypes prototypes, the library and INTEGRATION.md; the kernel's register figures."""
import os
import re

import numpy as np

from tests.test_cpu_ir_schedule import (BLOCK, CUT, RING_OUT, make_rows, make_sets, model_ir_schedule, rel_rms_per_stream,
                                        render_f64)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ohs_batch_process_ir_crossfaded"
RAMP_F = (np.arange(BLOCK, dtype=np.float32) / np.float32(BLOCK)).astype(np.float32)
RAMP_G = ((np.float32(BLOCK) - np.arange(BLOCK, dtype=np.float32)) / np.float32(BLOCK)).astype(np.float32)


# ---- the f64 model ------------------------------------------------------------------------------------------------------------
def fade_plan(S, n_blocks, idx, seg_blocks, prev=None):
    """-> (cur [S][n_blocks], old [S][n_blocks]) set indices per stream and block"""
    idx = np.asarray(idx)
    rows = np.broadcast_to(idx, (S, idx.shape[-1]))
    pv = None if prev is None else np.broadcast_to(np.asarray(prev).reshape(-1), (S,))
    cur = np.zeros((S, n_blocks), np.int64)
    old = np.zeros((S, n_blocks), np.int64)
    for s in range(S):
        for t in range(n_blocks):
            k = t // seg_blocks
            cur[s, t] = rows[s, k]
            if t % seg_blocks:
                old[s, t] = cur[s, t]
            elif k > 0:
                old[s, t] = rows[s, k - 1]
            else:
                old[s, t] = cur[s, t] if pv is None else pv[s]
    return cur, old


def split_input(x, cur, old):
    """x [S][2][n * 512] float32 -> (x_new, x_old) float32: x f and x g in the fading blocks (one f32 multiplication per sample
    and channel), x and 0 elsewhere"""
    x = np.asarray(x, np.float32)
    x_new, x_old = x.copy(), np.zeros_like(x)
    for s in range(x.shape[0]):
        for t in np.flatnonzero(cur[s] != old[s]):
            sl = slice(t * BLOCK, (t + 1) * BLOCK)
            x_new[s, :, sl] = x[s, :, sl] * RAMP_F
            x_old[s, :, sl] = x[s, :, sl] * RAMP_G
    return x_new, x_old


def model_ir_crossfade(oracle, x, sets, idx, seg_blocks, prev=None, tail_in=None):
    """the crossfaded call on x: idx a row [n_segs] for all streams or rows [S][n_segs]; prev: the set in front of the call's
    first block (a scalar or [S]; None: the call's start is no boundary); tail_in: the per-path tails an earlier render left
    -> (y f64, per-path tails at rest)"""
    x = np.asarray(x, np.float32)
    S, n = x.shape[0], x.shape[2] // BLOCK
    cur, old = fade_plan(S, n, idx, seg_blocks, prev)
    x_new, x_old = split_input(x, cur, old)
    y_new, t_new = render_f64(oracle, x_new, lambda s, t: sets[int(cur[s, t])], None, tail_in)
    y_old, t_old = render_f64(oracle, x_old, lambda s, t: sets[int(old[s, t])])
    return y_new + y_old, t_new + t_old


# ---- 1. constant rows are exactly RING_OUT ------------------------------------------------------------------------------------
def test_ramps_are_exact_and_sum_to_one():
    n = np.arange(BLOCK, dtype=np.float64)
    assert (RAMP_F.astype(np.float64) == n / BLOCK).all() and (RAMP_G.astype(np.float64) == (BLOCK - n) / BLOCK).all()
    assert (RAMP_F.astype(np.float64) + RAMP_G.astype(np.float64) == 1.0).all()


def test_constant_rows_are_exactly_the_ring_out_model(oracle):
    from open_headstage_amd import synth
    sets = make_sets(4)
    x = synth.white_noise(range(700, 703), 7 * BLOCK)
    rows = np.array([[2] * 4, [0] * 4, [3] * 4], np.uint32)
    for idx, prev in [(rows, None), (rows, rows[:, 0]), (rows[0], None), (rows[0], 2)]:
        a, ta = model_ir_crossfade(oracle, x, sets, idx, 2, prev)
        b, tb = model_ir_schedule(oracle, x, sets, idx, 2, RING_OUT)
        assert np.abs(a - b).max() == 0.0 and np.abs(ta - tb).max() == 0.0


# ---- 2. a test at the 1e-6 bar tells the three apart --------------------------------------------------------------------------
def test_model_differs_from_both_switch_modes_by_far_more_than_the_bar_on_the_gpu_tests_inputs(oracle):
    from open_headstage_amd import synth
    sets = make_sets(6)
    for S, blocks, seg in [(5, 13, 1), (5, 13, 2), (5, 13, 3), (5, 23, 7)]:
        x = synth.white_noise(range(500, 500 + S), blocks * BLOCK)
        idx = make_rows(S, -(-blocks // seg), 6)
        y, _ = model_ir_crossfade(oracle, x, sets, idx, seg)
        a, _ = model_ir_schedule(oracle, x, sets, idx, seg, RING_OUT)
        b, _ = model_ir_schedule(oracle, x, sets, idx, seg, CUT)
        da, db = rel_rms_per_stream(y, a), rel_rms_per_stream(y, b)
        print(f"seg_blocks {seg}: against RING_OUT {da.min():.3f} .. {da.max():.3f}, against CUT {db.min():.3f} .. {db.max():.3f}")
        assert (da > 1e-3).all() and (db > 1e-3).all(), (seg, da, db)


# ---- 3. the ramps sum to one --------------------------------------------------------------------------------------------------
def test_equal_sets_under_different_indices_give_the_plain_render(oracle):
    from open_headstage_amd import synth
    one = make_sets(1)[0]
    sets = np.stack([one] * 5)
    x = synth.white_noise(range(730, 733), 9 * BLOCK)
    idx = make_rows(3, 9, 5)
    y, _ = model_ir_crossfade(oracle, x, sets, idx, 1, prev=np.array([4, 3, 2]))
    ref, _ = render_f64(oracle, x, lambda s, t: one)
    err = rel_rms_per_stream(y, ref)
    print("equal sets, a fade in every block: relative RMS", err)
    assert (err > 0).any()                  # (x f and x g are rounded to f32: the split is not the identity)
    assert (err <= 1e-7).all(), err


# ---- 4. prev and the per-path tails carry over a call boundary ----------------------------------------------------------------
def test_two_renders_in_a_row_with_prev_and_tails_equal_one(oracle):
    from open_headstage_amd import synth
    sets = make_sets(4)
    x = synth.white_noise(range(720, 722), 8 * BLOCK)
    idx = make_rows(2, 8, 4)
    whole, tw = model_ir_crossfade(oracle, x, sets, idx, 1)
    a, tails = model_ir_crossfade(oracle, x[:, :, :3 * BLOCK], sets, idx[:, :3], 1)
    b, tb = model_ir_crossfade(oracle, x[:, :, 3 * BLOCK:], sets, idx[:, 3:], 1, prev=idx[:, 2], tail_in=tails)
    assert np.allclose(np.concatenate([a, b], axis=2), whole, rtol=0, atol=1e-15)
    assert np.allclose(tb, tw, rtol=0, atol=1e-15)
    # ... and without prev the second render's first block does not fade: far off
    c, _ = model_ir_crossfade(oracle, x[:, :, 3 * BLOCK:], sets, idx[:, 3:], 1, tail_in=tails)
    d = rel_rms_per_stream(c, whole[:, :, 3 * BLOCK:])
    print("second render without prev: relative RMS", d)
    assert (d > 1e-3).all(), d


# ---- 5. what the feature is for: no step at a boundary ------------------------------------------------------------------------
def test_a_sine_keeps_its_smoothness_across_boundaries_where_ring_out_steps(oracle):
    """100 Hz left, 130 Hz right, amplitude 1, through two sets 6 dB apart that alternate every two blocks.  The sets are a
    direct tap per path, L1-normalised per ear as the project's sets are, so a stationary output moves by no more than the
    input does from one sample to the next.  In a fading block the output is x (g + f / 2) delayed: it moves by the input's
    step plus at most |x| / 1024.  RING_OUT changes the gain by a factor of two between two samples."""
    fs, blocks, seg = 48000.0, 16, 2
    n = np.arange(blocks * BLOCK, dtype=np.float64)
    x = np.stack([np.sin(2 * np.pi * 100.0 * n / fs), np.sin(2 * np.pi * 130.0 * n / fs)])[None].astype(np.float32)
    a = np.zeros((4, BLOCK), np.float32)
    for p, (d, g) in enumerate([(30, 1.0), (45, 0.4), (45, 0.4), (30, 1.0)]):
        a[p, d] = g / 1.4
    sets = np.stack([a, 0.5 * a])
    idx = np.array([k % 2 for k in range(blocks // seg)], np.uint32)
    own = np.abs(np.diff(x.astype(np.float64), axis=2)).max()
    y, _ = model_ir_crossfade(oracle, x, sets, idx, seg)
    r, _ = model_ir_schedule(oracle, x, sets, idx, seg, RING_OUT)
    step_xf, step_ro = np.abs(np.diff(y, axis=2)).max(), np.abs(np.diff(r, axis=2)).max()
    print(f"largest sample step: input {own:.4f}, crossfaded {step_xf:.4f}, RING_OUT {step_ro:.4f}")
    assert step_xf <= 1.5 * own, (step_xf, own)
    assert step_ro > 10 * own, (step_ro, own)


# ---- 6. the entry exists ------------------------------------------------------------------------------------------------------
def test_entry_is_declared_listed_exported_and_refuses_null():
    from open_headstage_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "ohs_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    declared = set(re.findall(r"\b(ohs_[a-z0-9_]+)\s*\(", hdr))
    L = _ffi.lib()
    assert NAME in declared, f"{NAME} is not declared in include/ohs_hip.h"
    assert re.search(r"\bfn " + NAME + r"\(", doc), f"{NAME} is not listed in INTEGRATION.md"
    assert NAME in _ffi.PROTOTYPES, f"{NAME} has no ctypes prototype"
    assert hasattr(L, NAME), f"{NAME} is not exported"
    assert L.ohs_batch_process_ir_crossfaded(None, None, None, 1, 1024, 512, 1, None, 0, None, None) == _ffi.OHS_ERR_INVALID_ARG
    from open_headstage_amd.batch import BatchProcessor
    for m in ("process_ir_crossfaded", "process_ir_crossfaded_ptr", "last_conv_ir_crossfaded"):
        assert hasattr(BatchProcessor, m), m


def test_crossfading_kernel_register_budget():
    """Figures hipcc reported when the library was built.  Firm: k_conv_p1_irs_xf has no scratch and runs four waves per SIMD
    (a 16-wave workgroup: at most 128 registers per lane).  The target 4 x alloc(k_conv_p1_irs_xf) + alloc(k_eq_ring) <= 512 at
    the granule of 8 -- an EQ wave beside four convolution waves on a SIMD -- is MISSED: the kernel holds 127 registers, 128
    allocated, 4 x 128 + 32 = 544 (DESIGN 4.5d says what was tried); the test pins that figure, so that a change that costs
    a spill or a wave shows, and k_conv_p1_irs, which the target is met by, stays what it is."""
    from open_headstage_amd import _ffi, build
    _ffi.lib()
    res = build.resources()
    assert "k_conv_p1_irs_xf" in res and "k_conv_p1_state_irs_xf" in res, sorted(res)

    def alloc(k):
        return -(-(res[k]["vgprs"] + res[k]["agprs"]) // 8) * 8

    k = res["k_conv_p1_irs_xf"]
    assert k["scratch_bytes_per_lane"] == 0 and k["occupancy_waves_per_simd"] >= 4, k
    assert alloc("k_conv_p1_irs_xf") <= 128, k
    assert res["k_conv_p1_state_irs_xf"]["scratch_bytes_per_lane"] == 0, res["k_conv_p1_state_irs_xf"]
    assert 4 * alloc("k_conv_p1_irs") + alloc("k_eq_ring") <= 512, (res["k_conv_p1_irs"], res["k_eq_ring"])

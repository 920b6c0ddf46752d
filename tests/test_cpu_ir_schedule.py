"""IR-scheduled batch calls (ohs_batch_process_ir_scheduled), the part that needs no GPU: the yardsticks of
tests/test_gpu_ir_schedule.py are checked against each other here, and the GPU file imports them from this one.

The f64 model is the definition of the call.  Block t of stream s (512 frames) goes through the four responses of ITS set
by direct convolution in f64 (the oracle's ohs_or_direct_conv_f64), each path by itself; the 1023 frames that come out are
placed at frame 512 t of the stream's output:

    RING_OUT   y_s = sum_t place(conv(x_{s,t}, h[idx_s(t)]), 512 t)      every block's tail is added to the next block
    CUT        the part of a block's tail that crosses a boundary is dropped -- a boundary lies in front of the first block
               of every run of equal indices, and in front of the first block of a call

`render_f64` is the general form (a set per block, tails dropped per path in front of chosen blocks), so that mixed
sequences -- plain calls, a set_ir of ONE path between calls -- have a model too.

* a constant index is the plain convolution: the model equals oracle.binaural_f64;
* the CUT model agrees with the oracle's ConvolutionEngine driven the reference's way (set_ir x 4 in front of every run) to the
  project's FFT bar, 1e-6 relative RMS per stream;
* on the inputs the GPU tests use the two modes differ by far more than that bar, so a test at the bar tells them apart;
* the three entries are in the header, the ctypes prototypes, the library and INTEGRATION.md."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ohs_batch_set_schedule_irs", "ohs_batch_process_ir_scheduled", "ohs_batch_last_conv_ir_scheduled"]
BLOCK = 512
RING_OUT, CUT = 0, 1


# ---- inputs shared with the GPU tests -----------------------------------------------------------------------------------------
def make_sets(n_sets, taps=512, seed=3):
    """n_sets sets of four responses [n_sets][4][taps] float32, all different, with energy in their second half (a slow decay:
    tau = taps / 2), a direct tap per path as synth.hrir_set has it, L1-normalised per ear"""
    rng = np.random.default_rng(seed)
    k = np.arange(taps, dtype=np.float64)
    out = np.zeros((n_sets, 4, taps), np.float32)
    for i in range(n_sets):
        hs = []
        for p, (d, g) in enumerate([(30, 1.0), (45, 0.4), (45, 0.4), (30, 1.0)]):
            h = 0.5 * rng.standard_normal(taps) * np.exp(-k / (taps / 2.0))
            dd = (d + 3 * i + p) % taps
            h[dd] += 1.0
            hs.append(g * h)
        nl = np.abs(hs[0]).sum() + np.abs(hs[2]).sum()
        nr = np.abs(hs[1]).sum() + np.abs(hs[3]).sum()
        for p, n in enumerate([nl, nr, nl, nr]):
            out[i, p] = (hs[p] / n).astype(np.float32)
    assert len({out[i].tobytes() for i in range(n_sets)}) == n_sets
    return out


def make_rows(streams, n_segs, n_sets, call=0):
    """[streams][n_segs] uint32: every stream its own row, the index changes in EVERY segment of every stream (never two equal
    neighbours), and the rows differ from each other"""
    assert n_sets >= 3
    idx = np.zeros((streams, n_segs), np.uint32)
    for s in range(streams):
        step = 1 + s % (n_sets - 1)
        for k in range(n_segs):
            idx[s, k] = (s + 2 * call + k * step) % n_sets
    assert all(idx[s, k] != idx[s, k - 1] for s in range(streams) for k in range(1, n_segs))
    return idx


def runs_of(row):
    """[(first segment, one past the last, index)] of the runs of equal indices of one row"""
    out, k0 = [], 0
    for k in range(1, len(row) + 1):
        if k == len(row) or row[k] != row[k0]:
            out.append((k0, k, int(row[k0])))
            k0 = k
    return out


# ---- the f64 model ------------------------------------------------------------------------------------------------------------
def render_f64(oracle, x, block_set, drop=None, tail_in=None):
    """x [S][2][n * 512] float32.  block_set(s, t) -> the four responses [lsl, lsr, rsl, rsr] block t of stream s is convolved
    with.  drop(s, t) -> the paths (0 .. 3) whose tail arriving from block t - 1 is dropped in front of block t (None: nothing
    is dropped anywhere).  tail_in: per-path tails [S][4][512] f64 entering block 0 (what an earlier render left), or None.
    -> (y [S][2][n * 512] f64, tails [S][4][512] f64 the last block leaves, per path)"""
    x = np.asarray(x, np.float32)
    S, _, frames = x.shape
    n = frames // BLOCK
    y = np.zeros((S, 2, frames), np.float64)
    tails = np.zeros((S, 4, BLOCK), np.float64) if tail_in is None else np.array(tail_in, np.float64)
    ear = [0, 1, 0, 1]      # lsl -> left ear, lsr -> right, rsl -> left, rsr -> right
    src = [0, 0, 1, 1]      # the L speaker's signal feeds lsl, lsr; the R speaker's rsl, rsr
    pad = np.zeros(2 * BLOCK, np.float32)
    for s in range(S):
        for t in range(n):
            for p in (drop(s, t) if drop else ()):
                tails[s, p] = 0.0
            hs = block_set(s, t)
            sl = slice(t * BLOCK, (t + 1) * BLOCK)
            for p in range(4):
                pad[:BLOCK] = x[s, src[p], sl]
                full = oracle.direct_conv_f64(pad, hs[p])       # 1024 frames: the block's own 512 and its tail
                y[s, ear[p], sl] += full[:BLOCK] + tails[s, p]
                tails[s, p] = full[BLOCK:]
    return y, tails


def model_ir_schedule(oracle, x, sets, idx, seg_blocks, mode, tail_in=None):
    """the IR-scheduled call on x: idx a row [n_segs] for all streams or rows [S][n_segs]; -> (y, per-path tails at rest)"""
    S = x.shape[0]
    idx = np.asarray(idx)
    rows = np.broadcast_to(idx, (S, idx.shape[-1]))

    def block_set(s, t):
        return sets[int(rows[s, t // seg_blocks])]

    def drop(s, t):
        if mode != CUT or t % seg_blocks:
            return ()
        k = t // seg_blocks
        return range(4) if (k == 0 or rows[s, k] != rows[s, k - 1]) else ()

    return render_f64(oracle, x, block_set, drop, tail_in)


def rel_rms_per_stream(test, ref):
    test, ref = np.asarray(test, np.float64), np.asarray(ref, np.float64)
    e = np.sqrt(np.mean((test - ref) ** 2, axis=(1, 2)))
    r = np.sqrt(np.mean(ref ** 2, axis=(1, 2)))
    return e / r


def engine_cut_reference(oracle, x, sets, idx, seg_blocks):
    """the reference's way: per stream an oracle ConvolutionEngine, set_ir for all four paths in front of every run of equal
    indices, process_block per run -> y [S][2][frames] float32"""
    x = np.asarray(x, np.float32)
    S, _, frames = x.shape
    idx = np.asarray(idx)
    rows = np.broadcast_to(idx, (S, idx.shape[-1]))
    y = np.zeros_like(x)
    for s in range(S):
        eng = oracle.ConvolutionEngine()
        for k0, k1, i in runs_of(rows[s]):
            for p in range(4):
                eng.set_ir(p, sets[i][p])
            sl = slice(k0 * seg_blocks * BLOCK, min(k1 * seg_blocks * BLOCK, frames))
            if sl.start >= frames:
                break
            y[s, 0, sl], y[s, 1, sl] = eng.process_block(np.ascontiguousarray(x[s, 0, sl]), np.ascontiguousarray(x[s, 1, sl]))
    return y


# ---- 1. a constant index is the plain convolution -----------------------------------------------------------------------------
def test_constant_index_is_binaural_f64(oracle):
    from open_headstage_amd import synth
    sets = make_sets(3)
    x = synth.white_noise(range(700, 702), 7 * BLOCK)
    for mode in (RING_OUT, CUT):
        y, _ = model_ir_schedule(oracle, x, sets, np.full(4, 2, np.uint32), 2, mode)
        for s in range(2):
            l, r = oracle.binaural_f64(x[s, 0], x[s, 1], list(sets[2]))
            ref = np.stack([l, r])
            err = np.sqrt(np.mean((y[s] - ref) ** 2)) / np.sqrt(np.mean(ref ** 2))
            assert err <= 1e-13, (mode, s, err)


# ---- 2. the CUT model is the reference engine's set_ir behaviour --------------------------------------------------------------
def test_cut_model_agrees_with_the_oracle_engine_driven_with_set_ir(oracle):
    from open_headstage_amd import synth
    sets = make_sets(5)
    S, seg = 3, 2
    x = synth.white_noise(range(710, 710 + S), 11 * BLOCK)
    idx = make_rows(S, 6, 5)
    idx[0, 2] = idx[0, 1]           # a run of two segments: no boundary inside it
    y, _ = model_ir_schedule(oracle, x, sets, idx, seg, CUT)
    ref = engine_cut_reference(oracle, x, sets, idx, seg)
    err = rel_rms_per_stream(ref, y)
    assert (err <= 1e-6).all(), err
    # ... and the RING_OUT model is NOT what the engine does
    y2, _ = model_ir_schedule(oracle, x, sets, idx, seg, RING_OUT)
    assert (rel_rms_per_stream(ref, y2) > 1e-3).all()


# ---- 3. a test at the 1e-6 bar tells the modes apart --------------------------------------------------------------------------
def test_modes_differ_by_far_more_than_the_bar_on_the_gpu_tests_inputs(oracle):
    from open_headstage_amd import synth
    sets = make_sets(6)
    # the second half of the responses carries energy (a tail worth cutting)
    assert all((sets[i, p, 256:].astype(np.float64) ** 2).sum() > 0.05 * (sets[i, p].astype(np.float64) ** 2).sum()
               for i in range(6) for p in range(4))
    for S, blocks, seg in [(5, 13, 1), (5, 13, 2), (5, 13, 3), (5, 23, 7)]:
        x = synth.white_noise(range(500, 500 + S), blocks * BLOCK)
        idx = make_rows(S, -(-blocks // seg), 6)
        a, _ = model_ir_schedule(oracle, x, sets, idx, seg, RING_OUT)
        b, _ = model_ir_schedule(oracle, x, sets, idx, seg, CUT)
        d = rel_rms_per_stream(a, b)
        assert (d > 1e-3).all(), (seg, d)


def test_per_path_tails_of_the_model_add_up_to_its_output(oracle):
    """render_f64's per-path tails are what the next render starts from: two renders in a row equal one"""
    from open_headstage_amd import synth
    sets = make_sets(4)
    x = synth.white_noise(range(720, 722), 8 * BLOCK)
    idx = make_rows(2, 8, 4)
    whole, _ = model_ir_schedule(oracle, x, sets, idx, 1, RING_OUT)
    a, tails = model_ir_schedule(oracle, x[:, :, :3 * BLOCK], sets, idx[:, :3], 1, RING_OUT)
    b, _ = model_ir_schedule(oracle, x[:, :, 3 * BLOCK:], sets, idx[:, 3:], 1, RING_OUT, tail_in=tails)
    assert np.allclose(np.concatenate([a, b], axis=2), whole, rtol=0, atol=1e-15)


# ---- 4. the entries exist -----------------------------------------------------------------------------------------------------
def test_entries_are_declared_listed_exported_and_refuse_null():
    from open_headstage_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "ohs_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    declared = set(re.findall(r"\b(ohs_[a-z0-9_]+)\s*\(", hdr))
    L = _ffi.lib()
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/ohs_hip.h"
        assert re.search(r"\bfn " + name + r"\(", doc), f"{name} is not listed in INTEGRATION.md"
        assert name in _ffi.PROTOTYPES, f"{name} has no ctypes prototype"
        assert hasattr(L, name), f"{name} is not exported"
    assert re.search(r"OHS_IR_SWITCH_RING_OUT\s*=\s*0\s*,\s*OHS_IR_SWITCH_CUT\s*=\s*1", hdr)
    assert L.ohs_batch_set_schedule_irs(None, 0, None, 0) == _ffi.OHS_ERR_INVALID_ARG
    assert L.ohs_batch_process_ir_scheduled(None, None, None, 1, 1024, 512, 1, None, 0, 0, None) == _ffi.OHS_ERR_INVALID_ARG
    assert L.ohs_batch_last_conv_ir_scheduled(None, None) == _ffi.OHS_ERR_INVALID_ARG
    from open_headstage_amd.batch import BatchProcessor
    for m in ("set_schedule_irs", "set_schedule_speakers", "process_ir_scheduled", "process_ir_scheduled_ptr", "last_conv_ir_scheduled"):
        assert hasattr(BatchProcessor, m), m


def test_ir_scheduled_kernel_register_budget():
    """Figures hipcc reported when the library was built: k_conv_p1_irs has no scratch, runs four waves per SIMD, and leaves room
    for an EQ wave beside them, as k_conv_p1 does (4 x alloc(k_conv_p1_irs) + alloc(k_eq_ring) <= 512 registers per lane at the
    granule of 8) -- the overlapped batch step hides the convolution under the EQ on the same CUs."""
    from open_headstage_amd import _ffi, build
    _ffi.lib()
    res = build.resources()
    assert "k_conv_p1_irs" in res, sorted(res)

    def alloc(k):
        return -(-(res[k]["vgprs"] + res[k]["agprs"]) // 8) * 8

    k = res["k_conv_p1_irs"]
    assert k["scratch_bytes_per_lane"] == 0 and k["occupancy_waves_per_simd"] >= 4, k
    assert 4 * alloc("k_conv_p1_irs") + alloc("k_eq_ring") <= 512, (k, res["k_eq_ring"])

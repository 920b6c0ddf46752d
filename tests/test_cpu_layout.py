"""Speaker layouts (ohs_batch_process_layout), the part that needs no GPU: the yardsticks of tests/test_gpu_layout.py are
checked against each other here, and the GPU file imports them from this one.

The f64 model is the definition of the call: every channel c of a stream through its two responses h[c][0] (left ear) and
h[c][1] (right ear) by direct convolution in f64 (the oracle's ohs_or_direct_conv_f64), summed over the channels per ear:

    y[s][e][n] = sum_c sum_k h[c][e][k] x[s][c][n - k]

* the second yardstick -- one oracle ConvolutionEngine per PAIR of channels (Lsl = h[2p][0], Lsr = h[2p][1], Rsl = h[2p+1][0],
  Rsr = h[2p+1][1]; an odd last channel with a zero partner), the pairs' outputs summed in f32 -- agrees with the model to the
  project's FFT bar, 1e-6 relative RMS per stream, with room to spare;
* moving one channel's response to another channel changes the model by far more than the bar, so a test at the bar sees a
  routing error;
* the four entries are in the header, the ctypes prototypes, the library and INTEGRATION.md, and refuse NULL;
* ohs_sofa_layout_irs is ohs_sofa_speaker_irs per speaker;
* k_conv_p1_layout was built without scratch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.util import write_minimal_sofa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ohs_batch_set_layout_irs", "ohs_batch_process_layout", "ohs_batch_last_layout_launch", "ohs_sofa_layout_irs"]
BLOCK = 512
BAR = 1e-6


# ---- inputs shared with the GPU tests -----------------------------------------------------------------------------------------
def make_layout(K, taps=512, seed=11):
    """[K][2][taps] float32: decaying noise with a direct tap per channel and ear, all different, L1-normalised per ear (the
    sum over the channels of an ear's |h| is 1, so no ear can clip)"""
    rng = np.random.default_rng(seed + 100 * K + taps)
    k = np.arange(taps, dtype=np.float64)
    h = 0.5 * rng.standard_normal((K, 2, taps)) * np.exp(-k / max(taps / 2.0, 1.0))
    for c in range(K):
        for e in range(2):
            h[c, e, (7 * c + 13 * e + 3) % taps] += 1.0 if (c + e) % 2 == 0 else 0.4
    h /= np.abs(h).sum(axis=(0, 2), keepdims=True)
    out = h.astype(np.float32)
    assert len({out[c, e].tobytes() for c in range(K) for e in range(2)}) == 2 * K
    return out


def make_input(S, K, blocks, seed=800):
    """[S][K][blocks * 512] float32 white noise, every channel of every stream its own sequence"""
    from open_headstage_amd import synth
    x = synth.white_noise(range(seed, seed + S * K), blocks * BLOCK)      # [S * K][2][frames]
    return np.ascontiguousarray(x[:, 0, :].reshape(S, K, blocks * BLOCK))


# ---- the f64 model ------------------------------------------------------------------------------------------------------------
def model_layout_f64(oracle, x, irs, gain=1.0):
    """x [S][>= K][frames] float32, irs [K][2][len] -> gain * y [S][2][frames] f64 (from rest: zero history)"""
    x = np.asarray(x, np.float32)
    irs = np.asarray(irs, np.float32)
    S, _, frames = x.shape
    y = np.zeros((S, 2, frames), np.float64)
    for s in range(S):
        for c in range(irs.shape[0]):
            xc = np.ascontiguousarray(x[s, c])
            for e in range(2):
                y[s, e] += oracle.direct_conv_f64(xc, np.ascontiguousarray(irs[c, e]))[:frames]
    return gain * y


def engines_layout(oracle, x, irs, gain=1.0, engines=None):
    """one oracle ConvolutionEngine per pair of channels and stream, the pairs' outputs summed in f32, times gain (f32);
    engines: those of an earlier call (state carried) -> (y [S][2][frames] float32, engines)"""
    x = np.asarray(x, np.float32)
    irs = np.asarray(irs, np.float32)
    S, _, frames = x.shape
    K = irs.shape[0]
    P = (K + 1) // 2
    zero_h, zero_x = np.zeros(irs.shape[2], np.float32), np.zeros(frames, np.float32)
    if engines is None:
        engines = []
        for s in range(S):
            row = []
            for p in range(P):
                eng = oracle.ConvolutionEngine()
                odd = 2 * p + 1 >= K
                for path, h in enumerate([irs[2 * p, 0], irs[2 * p, 1], zero_h if odd else irs[2 * p + 1, 0],
                                          zero_h if odd else irs[2 * p + 1, 1]]):
                    eng.set_ir(path, np.ascontiguousarray(h))
                row.append(eng)
            engines.append(row)
    y = np.zeros((S, 2, frames), np.float32)
    for s in range(S):
        for p in range(P):
            a = np.ascontiguousarray(x[s, 2 * p])
            b = zero_x if 2 * p + 1 >= K else np.ascontiguousarray(x[s, 2 * p + 1])
            l, r = engines[s][p].process_block(a, b)
            y[s, 0] += np.asarray(l, np.float32)
            y[s, 1] += np.asarray(r, np.float32)
    return (y * np.float32(gain)).astype(np.float32), engines


def rel_rms_per_stream(test, ref):
    test, ref = np.asarray(test, np.float64), np.asarray(ref, np.float64)
    e = np.sqrt(np.mean((test - ref) ** 2, axis=(1, 2)))
    r = np.sqrt(np.mean(ref ** 2, axis=(1, 2)))
    return e / r


# ---- 1. the two yardsticks agree ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 6, 8, 16])
def test_summed_oracle_engines_agree_with_the_f64_model(oracle, K):
    S, blocks = 5, 13
    irs = make_layout(K)
    x = make_input(S, K, blocks)
    ref = model_layout_f64(oracle, x, irs)
    y, _ = engines_layout(oracle, x, irs)
    err = rel_rms_per_stream(y, ref)
    print(f"K = {K}: summed engines vs f64 model, relative RMS per stream, worst {err.max():.3e}")
    assert (err <= BAR).all(), (K, err)


# ---- 2. a test at the bar sees a routing error --------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 6, 8])
def test_moving_a_response_to_another_channel_is_far_above_the_bar(oracle, K):
    irs = make_layout(K)
    x = make_input(2, K, 5, seed=840)
    ref = model_layout_f64(oracle, x, irs)
    for a, b in [(0, 1), (K - 1, 0), (K - 2, K - 1)]:
        moved = irs.copy()
        moved[[a, b]] = moved[[b, a]]
        assert (rel_rms_per_stream(model_layout_f64(oracle, x, moved), ref) > 1e-3).all(), (K, a, b)
    ears = irs[:, ::-1].copy()          # ... and so are swapped ears
    assert (rel_rms_per_stream(model_layout_f64(oracle, x, ears), ref) > 1e-3).all()


# ---- 3. the entries exist -----------------------------------------------------------------------------------------------------
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
    INV = _ffi.OHS_ERR_INVALID_ARG
    assert L.ohs_batch_set_layout_irs(None, 0, None, 0) == INV
    assert L.ohs_batch_process_layout(None, None, None, 1, 3072, 512, 1024, 512, None) == INV
    assert L.ohs_batch_last_layout_launch(None, None, None) == INV
    assert L.ohs_sofa_layout_irs(None, 2, None, None, 1.0, 0.0, None, 0, None) == INV
    import open_headstage_amd as ohs
    for m in ("set_layout_irs", "set_layout_speakers", "process_layout", "process_layout_ptr", "last_layout_launch"):
        assert hasattr(ohs.BatchProcessor, m), m
    assert [(n, az) for n, az, _ in ohs.LAYOUT_5_1] == [("L", -30.0), ("R", 30.0), ("C", 0.0), ("LFE", 0.0), ("Ls", -110.0), ("Rs", 110.0)]
    assert [(n, az) for n, az, _ in ohs.LAYOUT_7_1] == [("L", -30.0), ("R", 30.0), ("C", 0.0), ("LFE", 0.0), ("Lb", -135.0), ("Rb", 135.0),
                                                        ("Ls", -90.0), ("Rs", 90.0)]


# ---- 4. ohs_sofa_layout_irs is ohs_sofa_speaker_irs per speaker ----------------------------------------------------------------
@pytest.fixture(scope="module")
def ring_sofa(tmp_path_factory):
    from open_headstage_amd import sofa, synth
    rng = np.random.default_rng(5)
    az = np.arange(0.0, 360.0, 10.0)
    pos = np.stack([az, np.zeros_like(az), np.ones_like(az)], 1)
    ir = 0.05 * rng.standard_normal((len(pos), 2, 160)) * np.exp(-np.arange(160) / 40.0)
    path = write_minimal_sofa(str(tmp_path_factory.mktemp("layout") / "ring.sofa"), ir, pos, synth.FS)
    return sofa.MySofa(path)


def test_sofa_layout_irs_of_two_speakers_is_speaker_irs(ring_sofa):
    from open_headstage_amd import sofa, synth
    four = sofa.speaker_irs_plugin_angles(ring_sofa, -30.0, 0.0, 30.0, 0.0, 1.0, synth.FS)
    lay = sofa.layout_irs(ring_sofa, [-30.0, 30.0], [0.0, 0.0], 1.0, synth.FS)
    assert lay.shape == (2, 2, max(len(h) for h in four))
    for p, h in enumerate(four):
        got = lay[p // 2, p % 2]
        assert got[:len(h)].tobytes() == h.tobytes() and not got[len(h):].any(), p
    assert lay[0, 0].tobytes() != lay[1, 0].tobytes()


def test_sofa_layout_irs_of_5_1_is_speaker_irs_per_speaker(ring_sofa):
    import open_headstage_amd as ohs
    from open_headstage_amd import sofa, synth
    az, el = [r[1] for r in ohs.LAYOUT_5_1], [r[2] for r in ohs.LAYOUT_5_1]
    lay = sofa.layout_irs(ring_sofa, az, el, 1.0, synth.FS)
    assert lay.shape[:2] == (6, 2)
    for c in range(6):
        l, r, _, _ = sofa.speaker_irs_plugin_angles(ring_sofa, az[c], el[c], az[c], el[c], 1.0, synth.FS)
        assert lay[c, 0, :len(l)].tobytes() == l.tobytes() and not lay[c, 0, len(l):].any(), c
        assert lay[c, 1, :len(r)].tobytes() == r.tobytes() and not lay[c, 1, len(r):].any(), c
    assert lay[2].tobytes() == lay[3].tobytes()         # C and LFE share their direction
    assert lay[4].tobytes() != lay[5].tobytes() and lay[0].tobytes() != lay[4].tobytes()
    # the other sampling rate: the same per-speaker equality through the resampler
    lay2 = sofa.layout_irs(ring_sofa, az, el, 1.0, 44100.0)
    l, r, _, _ = sofa.speaker_irs_plugin_angles(ring_sofa, az[4], el[4], az[4], el[4], 1.0, 44100.0)
    assert lay2[4, 0, :len(l)].tobytes() == l.tobytes() and lay2[4, 1, :len(r)].tobytes() == r.tobytes()


def test_sofa_layout_irs_query_and_short_len(ring_sofa):
    from open_headstage_amd import _ffi, synth
    L = _ffi.lib()
    az = np.array([-30.0, 30.0, 0.0], np.float32)
    el = np.zeros(3, np.float32)
    n = C.c_size_t(0)
    azp, elp = az.ctypes.data_as(_ffi.fp), el.ctypes.data_as(_ffi.fp)
    assert L.ohs_sofa_layout_irs(ring_sofa._h, 3, azp, elp, 1.0, synth.FS, None, 0, C.byref(n)) == _ffi.OHS_OK
    assert n.value == 160
    out = np.full((3, 2, 200), 7.0, np.float32)
    assert L.ohs_sofa_layout_irs(ring_sofa._h, 3, azp, elp, 1.0, synth.FS, out.ctypes.data_as(_ffi.fp), 159, C.byref(n)) == _ffi.OHS_ERR_INVALID_ARG
    assert (out == 7.0).all() and n.value == 160        # nothing written, the length still reported
    assert L.ohs_sofa_layout_irs(ring_sofa._h, 3, azp, elp, 1.0, synth.FS, out.ctypes.data_as(_ffi.fp), 200, C.byref(n)) == _ffi.OHS_OK
    assert out[:, :, :160].any() and not out[:, :, 160:].any()
    assert L.ohs_sofa_layout_irs(ring_sofa._h, 0, azp, elp, 1.0, synth.FS, None, 0, C.byref(n)) == _ffi.OHS_ERR_INVALID_ARG
    assert L.ohs_sofa_layout_irs(ring_sofa._h, 17, azp, elp, 1.0, synth.FS, None, 0, C.byref(n)) == _ffi.OHS_ERR_INVALID_ARG


# ---- 5. the kernel's resources -------------------------------------------------------------------------------------------------
def test_layout_kernel_has_no_scratch():
    """Figures hipcc reported when the library was built: no scratch, and at least the three waves per SIMD its workgroup shape
    (twelve waves per CU) asks for"""
    from open_headstage_amd import _ffi, build
    _ffi.lib()
    res = build.resources()
    assert "k_conv_p1_layout" in res, sorted(res)
    k = res["k_conv_p1_layout"]
    assert k["scratch_bytes_per_lane"] == 0, k
    assert k["occupancy_waves_per_simd"] >= 3, k

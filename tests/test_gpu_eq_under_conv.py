"""The quad ring with the convolution underneath it: an overlapped batch call -- six EQ launches, chunk i's
convolution on a second stream under the EQ launch of chunk i + 1 -- whose big chunks still take the wave ring.  64 blocks: the
first three chunks are exactly 8 192 samples (the shortest launch the rule gives to the wave ring); 128 blocks: 16 384.  The
EQ's own bits are pinned by tests/test_gpu_eq_quad_ring.py; the experiments build's second loop, with a fill instruction in the
slots that carry nothing, by tests/test_cpu_eq_quad_fill.py.

Here: the whole chain against oracle.chain_process driven with the same whole-call input, to the suite's 1e-6 (RMS error,
absolute and relative, as smoke()); a 128-block call against a 64 + 64 split, bit for bit (the EQ state and the convolution's
overlap cross a call edge where the single call has a launch edge); which form serves a launch of a chunk's length; and, with the
experiments library, the loop with the fill against the loop with v_nop, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS = 48000.0
S_MAX, BLOCKS_MAX, GAIN = 9, 128, 0.75


def _bands():
    from open_headstage_amd import synth
    bands = list(synth.eq_table())
    assert len(bands) == 10
    return bands


def _batch(S, library=None):
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    bp = ohs.BatchProcessor(S, num_bands=10, library=library) if library is not None else ohs.BatchProcessor(S, num_bands=10)
    irs = synth.hrir_set(512)
    for p in range(4):
        bp.set_ir(p, irs[p])
    coeffs = _coeffs()
    for i, b in enumerate(_bands()):
        bp.set_band_coeffs(i, coeffs[i], bool(b.enabled) and i != 4)        # ten bands, one of them switched off
    bp.set_eq_enabled(True)
    bp.set_gain(GAIN)
    return bp


def _coeffs():
    import open_headstage_amd as ohs
    return [ohs.biquad_coefficients(b.filter_type, FS, b.center_freq, b.q, b.gain_db) for b in _bands()]


@pytest.fixture(scope="module")
def signal():
    from open_headstage_amd import synth
    return synth.white_noise(range(300, 300 + S_MAX), BLOCKS_MAX * 512)


@pytest.fixture(scope="module")
def reference(oracle, signal):
    """oracle.chain_process over the whole 128-block input of every stream, computed once (float64 copy, read only): a
    shorter call's reference is its prefix"""
    from open_headstage_amd import synth
    irs = synth.hrir_set(512)
    coeffs = _coeffs()
    out = np.empty(signal.shape, np.float64)
    for s in range(S_MAX):
        eng = oracle.ConvolutionEngine()
        for p in range(4):
            eng.set_ir(p, irs[p])
        eq = oracle.StereoParametricEQ(10, FS)
        for i, b in enumerate(_bands()):
            eq.set_band_coeffs(i, coeffs[i], bool(b.enabled) and i != 4)
        l, r = signal[s, 0].copy(), signal[s, 1].copy()
        oracle.chain_process(eng, eq, l, r, eq_enable=True, gain=GAIN)
        out[s, 0], out[s, 1] = l, r
    out.setflags(write=False)
    return out


def _call(bp, x):
    import torch
    y = bp.process(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("blocks", [64, 128])
@pytest.mark.parametrize("S", [3, 9])
def test_overlapped_call_against_the_oracle(signal, reference, S, blocks):
    n = blocks * 512
    bp = _batch(S)
    y = _call(bp, signal[:S, :, :n])
    worst = 0.0
    for s in range(S):
        ref = reference[s, :, :n]
        err = float(np.sqrt(np.mean((y[s] - ref) ** 2)))
        rel = err / float(np.sqrt(np.mean(ref ** 2)))
        print(f"streams {S} blocks {blocks} stream {s}: RMS error {err:.3e}, relative {rel:.3e}")
        worst = max(worst, err, rel)
    assert worst <= 1e-6, worst
    # the call's last EQ launch is its 2 % chunk (2 or 3 blocks: the row form); a launch of the first chunks' length --
    # 16 or 32 blocks, below the 64 from which a call overlaps -- takes the wave ring
    _call(bp, signal[:S, :, :n // 4])
    assert bp.last_eq_form() == ("wave_ring", False), bp.last_eq_form()


@pytest.mark.parametrize("S", [3, 9])
def test_one_call_equals_two_halves(signal, S):
    """128 blocks in one call == 64 + 64: the chunk plan differs (16 384-sample launches against 8 192), the bits do not"""
    n = BLOCKS_MAX * 512
    x = signal[:S]
    whole = _call(_batch(S), x)
    bp = _batch(S)
    halves = np.concatenate([_call(bp, x[:, :, :n // 2]), _call(bp, x[:, :, n // 2:])], axis=2)
    assert np.array_equal(whole.view(np.uint32), halves.view(np.uint32))


@pytest.mark.parametrize("S", [3, 9])
def test_fill_and_nop_loops_give_the_same_bits(exp_tuning, signal, S):
    """experiments library: Tuning::eq_quad_fill = 1 is the loop with the fill instruction in the slots that carry nothing"""
    exp_tuning.DEFAULTS.setdefault("eq_quad_fill", "0")
    n = 64 * 512
    outs = []
    for fill in (0, 1):
        exp_tuning("eq_quad_fill", fill)
        bp = _batch(S, exp_tuning.lib)
        outs.append(_call(bp, signal[:S, :, :n]))
        _call(bp, signal[:S, :, :n // 4])
        assert bp.last_eq_form() == ("wave_ring", False)
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    # and the product library's bits
    assert np.array_equal(outs[0].view(np.uint32), _call(_batch(S), signal[:S, :, :n]).view(np.uint32))

"""The conditions that make tests/test_gpu_flush_modes.py legitimate, and proof that its checkers can fail -- all on the CPU.

* Oracle: the reference arithmetic itself, under oracle.flush_denormals(m), has the three properties of tests/flush_modes.py at the
  tap counts and call lists of the GPU test's families: A (the mode changes no bit of a loud signal), B (silence out, silence kept)
  and C (no subnormal sample leaves, while the IEEE run of the same input holds thousands).
* Mutants: a clean result damaged in the ways the checkers exist to catch is caught, and the message names stream, channel, frame,
  block and value; a twin that shows nothing trips the vacuity conditions."""
import numpy as np
import pytest

from tests import flush_modes as fm

BLOCK = fm.BLOCK
GAIN = 0.75
N_STREAMS = 2
# taps, call lengths in blocks, {call: [(path, taps of the response it is re-loaded with)]}: tests/test_gpu_special_values.family()'s
SHAPES = {"taps_512": (512, (3, 17), {}), "taps_200": (200, (19, 5), {}), "taps_1300_reload": (1300, (7, 3, 18), {1: [(1, 900)]}),
          "taps_1300": (1300, (7, 16, 9), {}), "taps_8192": (8192, (129, 135), {}), "taps_16384": (16384, (129, 135), {})}


def _engine(oracle, taps):
    from open_headstage_amd import synth
    eng = oracle.ConvolutionEngine()
    for p, h in enumerate(synth.hrir_set(taps)):
        eng.set_ir(p, h)
    return eng


def _reload(eng, events, k):
    from open_headstage_amd import synth
    for p, t in events.get(k, ()):
        eng.set_ir(p, synth.hrir_set(t)[p])


def _run(oracle, eng, x1, mode, starts=None, events=None):
    """x1 [2][frames] through eng (four paths -> gain) block by block under the mode; events applied where their call starts"""
    eq = oracle.StereoParametricEQ(1, 48000.0)
    l, r = x1[0].copy(), x1[1].copy()
    with oracle.flush_denormals(mode):
        for t in range(l.size // BLOCK):
            if starts and t in starts:
                _reload(eng, events, starts[t])
            oracle.chain_process(eng, eq, l[t * BLOCK:(t + 1) * BLOCK], r[t * BLOCK:(t + 1) * BLOCK], eq_enable=False, gain=GAIN)
    return np.stack([l, r])


def oracle_case(oracle, shape, x, mode):
    """x [S][2][frames] -> (y [S][2][frames], the engines)"""
    taps, calls, events = SHAPES[shape]
    starts = {sum(calls[:k]): k for k in range(1, len(calls))}
    engs = [_engine(oracle, taps) for _ in range(x.shape[0])]
    return np.stack([_run(oracle, e, x[s], mode, starts, events) for s, e in enumerate(engs)]), engs


@pytest.fixture(scope="module")
def noise():
    from open_headstage_amd import synth
    return synth.white_noise(range(720, 720 + N_STREAMS), (264 + 129) * BLOCK)


def _frames(shape):
    return sum(SHAPES[shape][1]) * BLOCK


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------------
def test_input_builders(noise):
    u = noise[:, :, :40 * BLOCK]
    xs = fm.silent_input(u)
    assert xs.dtype == np.float32 and float(np.abs(xs).max()) * 16384 < float(fm.TINY) and np.count_nonzero(xs) > xs.size * 0.99
    assert np.array_equal(np.ldexp(xs.astype(np.float64), 149), np.round(u.astype(np.float64) * 256))
    xd = fm.subnormal_input(u)
    assert fm.subnormal_mask(xd).sum() == np.count_nonzero(xd) > xd.size * 0.99
    c = 6
    xc = fm.falling_input(u, c)
    # stream s at frame c 512: u 2^(-124 - s); one block later half of it
    for s in range(N_STREAMS):
        n = c * BLOCK
        assert xc[s, 0, n] == np.float32(np.ldexp(np.float64(u[s, 0, n]), -124 - s))
        assert xc[s, 0, n + BLOCK] == np.float32(np.ldexp(np.float64(u[s, 0, n + BLOCK]), -125 - s))
    assert fm.subnormal_mask(xc).sum() > 1000 and not xc[:, :, (c + 27) * BLOCK:].any()
    loud = fm.falling_input(noise[:, :, :200 * BLOCK], 130)
    assert np.array_equal(loud[0, :, :6 * BLOCK], noise[0, :, :6 * BLOCK])      # min(0, .): amplitude 1 at most
    m = fm.subnormal_mask(np.asarray([0.0, -0.0, 2.0 ** -126, -2.0 ** -127, 2.0 ** -149, np.nan, np.inf], np.float32))
    assert m.tolist() == [False, False, False, True, True, False, False]


# ---- the oracle has the three properties -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_oracle_a_normal_range(oracle, noise, shape, mode):
    x = noise[:, :, :_frames(shape)]
    twin, _ = oracle_case(oracle, shape, x, 0)
    assert float(np.abs(twin).max()) > 0.01
    fm.check_same_bits(oracle_case(oracle, shape, x, mode)[0], twin, f"oracle A, {shape}, mode {mode}")


@pytest.mark.parametrize("which,mode", [("silent", 1), ("silent", 2), ("subnormal", 2)])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_oracle_b_below_the_range(oracle, noise, shape, which, mode):
    n = _frames(shape)
    x = {"silent": fm.silent_input, "subnormal": fm.subnormal_input}[which](noise[:, :, :n])
    twin, _ = oracle_case(oracle, shape, x[:1], 0)       # (IEEE arithmetic on subnormals is slow on a CPU: one stream shows that the case is alive)
    y, engs = oracle_case(oracle, shape, x, mode)
    fm.check_silent(y, f"oracle B, {shape}, {which} input, mode {mode}", twin=twin)
    taps, calls, events = SHAPES[shape]
    more = noise[:, :, n:n + calls[0] * BLOCK]
    for s, e in enumerate(engs):
        fresh = _engine(oracle, taps)
        for k in sorted(events):
            _reload(fresh, events, k)
        got, want = _run(oracle, e, more[s], mode), _run(oracle, fresh, more[s], mode)
        assert np.isfinite(want).all() and float(np.abs(want).max()) > 0.01 and np.array_equal(got, want), (shape, s)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_oracle_c_through_the_range(oracle, noise, shape, mode):
    x = fm.falling_input(noise[:, :, :_frames(shape)], SHAPES[shape][1][0] + 1)
    twin, _ = oracle_case(oracle, shape, x, 0)
    counts = fm.check_no_subnormal(oracle_case(oracle, shape, x, mode)[0], f"oracle C, {shape}, mode {mode}", twin=twin)
    print(f"flush-modes oracle C, {shape}: subnormal samples per stream of the IEEE run: {counts}")


# ---- the object scenes' case C is not vacuous ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["plain", "blend"])
def test_scene_case_c_leaves_every_stream_subnormal_samples(kernel):
    """tests/test_gpu_scene_modes.py's falling input on its scene and call list: the f64 model of the two calls, rounded to f32, holds
    at least NEED subnormal samples in every stream, and every stream's input passes 2^-126 inside the first call"""
    from tests import test_gpu_scene_modes as gm
    x = fm.falling_input(gm.modes_noise(), gm.CROSSING)
    assert x.shape == (gm.S, gm.K, gm.TOTAL * BLOCK)
    for s in range(gm.S):
        peak = np.abs(x[s]).reshape(gm.K, gm.TOTAL, BLOCK).max(axis=(0, 2))
        below = np.flatnonzero(peak < fm.TINY)
        assert peak[0] >= fm.TINY and below.size and 0 < below[0] < gm.CALLS[0], (s, below)
    ref = gm.model_calls(kernel, x, gm.C_GAIN_POW).astype(np.float32)
    counts = fm.subnormal_mask(ref).sum(axis=(1, 2))
    print(f"scene case C, {kernel} kernel: subnormal samples per stream of the f64 model rounded to f32: {counts.tolist()}")
    assert (counts >= fm.NEED).all(), counts
    normal = (np.abs(ref) >= fm.TINY).sum(axis=(1, 2))
    print(f"scene case C, {kernel} kernel: samples per stream in the normal range: {normal.tolist()}")
    assert (normal >= fm.NEED).all(), normal            # (the output starts in the normal range and falls through it)


# ---- the checkers can fail -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean(oracle, noise):
    """taps 512: (loud output, the IEEE run of the falling input, its FTZ run)"""
    loud, _ = oracle_case(oracle, "taps_512", noise[:, :, :_frames("taps_512")], 0)
    x = fm.falling_input(noise[:, :, :_frames("taps_512")], 4)
    return loud, oracle_case(oracle, "taps_512", x, 0)[0], oracle_case(oracle, "taps_512", x, 1)[0]


def test_mutant_one_subnormal_sample(clean):
    _, ieee, ftz = clean
    fm.check_no_subnormal(ftz, twin=ieee)
    m = ftz.copy()
    m[1, 0, 9 * BLOCK + 5] = np.float32(-3e-39)
    with pytest.raises(AssertionError, match=r"case: 1 subnormal .* in streams \[1\], first at stream 1, channel 0, frame 4613, block 9: .*-3e-39.*bits 0x80"):
        fm.check_no_subnormal(m, "case", twin=ieee)
    with pytest.raises(AssertionError, match=r"block 12: "):        # a call's output names the block within the case
        fm.check_no_subnormal(m, "case", first_block=3)
    m = ftz.copy()
    m[0, 1, 3] = np.nan
    with pytest.raises(AssertionError, match=r"stream 0, channel 1, frame 3, block 0: .*nan"):
        fm.check_no_subnormal(m)


def test_mutant_twin_without_subnormals_is_vacuous(clean):
    loud, ieee, ftz = clean
    with pytest.raises(AssertionError, match=r"vacuous: the mode-0 twin's stream 0 holds 0 subnormal samples, the case needs 100"):
        fm.check_no_subnormal(ftz, twin=ftz)
    few = ftz.copy()
    few[1, 0, :99] = np.float32(1e-40)
    few[0] = ieee[0]
    with pytest.raises(AssertionError, match=r"vacuous: the mode-0 twin's stream 1 holds 99 subnormal"):
        fm.check_no_subnormal(ftz, twin=few)
    few[1, 0, 99] = np.float32(1e-40)
    assert fm.check_no_subnormal(ftz, twin=few)[1] == 100


def test_mutant_one_non_zero_sample_in_silence(clean):
    loud, _, _ = clean
    z = np.zeros_like(loud)
    z[0, 0, ::3] = -0.0
    fm.check_silent(z, twin=loud)
    m = z.copy()
    m[1, 1, 17 * BLOCK + 1] = np.float32(2.0 ** -149)
    with pytest.raises(AssertionError, match=r"1 samples of streams \[1\] are not zero, first at stream 1, channel 1, frame 8705, block 17: .*1e-45.*bits 0x00000001"):
        fm.check_silent(m, twin=loud)
    half = loud.copy()
    half[1, :, ::2] = 0.0
    with pytest.raises(AssertionError, match=r"vacuous: the mode-0 twin's stream 1 is non-zero in"):
        fm.check_silent(z, twin=half)


def test_mutant_one_bit_flipped_in_one_stream(clean):
    loud, ieee, _ = clean
    fm.check_same_bits(loud.copy(), loud)
    m = loud.copy()
    m.view(np.uint32)[1, 1, 2 * BLOCK + 9] ^= 1
    with pytest.raises(AssertionError, match=r"1 samples of streams \[1\] differ from the mode-0 twin, first at stream 1, channel 1, frame 1033, block 2: "):
        fm.check_same_bits(m, loud)
    m = loud.copy()
    m[0, 0, 5] = -m[0, 0, 5]
    with pytest.raises(AssertionError, match=r"streams \[0\].*frame 5, block 0"):
        fm.check_same_bits(m, loud)
    with pytest.raises(AssertionError, match=r"the mode-0 twin holds \d+ subnormal samples.*not a case of the normal range"):
        fm.check_same_bits(ieee, ieee)

"""The conditions that make tests/test_gpu_special_values.py legitimate, and proof that its checkers can fail -- all on the CPU.

* Oracle scaling: the oracle alone is bit-homogeneous under 2^k at every scale and response shape the GPU test uses, EQ on and
  off (no case needed a smaller |k|: every one holds at the full +-80).
* Oracle windows: a NaN / +Inf / -Inf sample in block b makes exactly the blocks reference_window(b, Pmax) non-finite, every
  other block bit-identical to the clean run.
* Mutants: a clean result damaged in the ways the checkers exist to catch is caught, and the message names the right stream and
  block."""
import numpy as np
import pytest

from tests import special_values as sv

GAIN = 0.75
N_BLOCKS = 24
UNEQUAL = sv.UNEQUAL
SHAPES = {"taps_200": (200,) * 4, "taps_512": (512,) * 4, "taps_1300": (1300,) * 4, "taps_8192": (8192,) * 4, "unequal": UNEQUAL}
irs_for, parts_of, pmax_of = sv.irs_for, sv.parts_of, sv.pmax_of


def oracle_run(oracle, x1, irs, eq_on, gain=GAIN):
    """one stream x1 [2][frames] through the oracle's chain (EQ -> four paths -> gain), block by block -> [2][frames] f32"""
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    bands = synth.eq_table()
    eng = oracle.ConvolutionEngine()
    for p in range(4):
        eng.set_ir(p, irs[p])
    eq = oracle.StereoParametricEQ(len(bands), synth.FS)
    for i, b in enumerate(bands):
        eq.set_band_coeffs(i, ohs.biquad_coefficients(b.filter_type, synth.FS, b.center_freq, b.q, b.gain_db), b.enabled)
    l, r = x1[0].copy(), x1[1].copy()
    for o in range(0, l.size, sv.BLOCK):
        oracle.chain_process(eng, eq, l[o:o + sv.BLOCK], r[o:o + sv.BLOCK], eq_enable=eq_on, gain=gain)
    return np.stack([l, r])


@pytest.fixture(scope="module")
def noise():
    from open_headstage_amd import synth
    return synth.white_noise(range(700, 705), N_BLOCKS * sv.BLOCK)


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def test_scaled_and_unscaled_are_exact_inverses(noise):
    ks = sv.scales_for(5)
    xs = sv.scaled(noise, ks)
    assert xs.dtype == np.float32 and np.isfinite(xs).all()
    assert np.array_equal(sv.unscaled(xs, ks).view(np.uint32), noise.view(np.uint32))
    nz = noise[3] != 0
    assert np.array_equal(xs[3][nz].view(np.uint32) - noise[3][nz].view(np.uint32), np.full(int(nz.sum()), 80 << 23, np.uint32))


def test_windows():
    assert sv.reference_window(5, 1) == (5, 6) and sv.reference_window(5, 4) == (5, 9)
    assert sv.allowed_window(9, 3, 2, 4) == (7, 16)
    assert sv.allowed_window(9, 3, 4, 0, call_first=7) == (7, 12)
    assert sv.allowed_window(9, 3, 1, 0, call_first=7) == (8, 12)
    m = sv.window_mask(8 * sv.BLOCK, (2, 3), from_frame=2 * sv.BLOCK + 17, channels=(1,))
    assert not m[0].any() and np.flatnonzero(m[1])[[0, -1]].tolist() == [2 * sv.BLOCK + 17, 4 * sv.BLOCK - 1]


def test_poison_copies(noise):
    y = sv.poison(noise, 1, 0, 17, np.inf)
    assert np.isinf(y[1, 0, 17]) and np.isfinite(noise).all() and int((~np.isfinite(y)).sum()) == 1
    with pytest.raises(AssertionError):
        sv.poison(noise, 1, 0, 17, 1.0)


# ---- the oracle is bit-homogeneous at the GPU test's scales and shapes -----------------------------------------------------------------
@pytest.mark.parametrize("eq_on", [False, True], ids=["eq_off", "eq_on"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_oracle_scaling(oracle, noise, shape, eq_on):
    """every scale of the GPU test, (0, +40, -40, +80, -80), one stream each; held at the full |k| = 80 for every shape"""
    irs = irs_for(SHAPES[shape])
    ks = sv.scales_for(5)
    xs = sv.scaled(noise, ks)
    twin = np.stack([oracle_run(oracle, noise[s], irs, eq_on) for s in range(5)])
    got = np.stack([oracle_run(oracle, xs[s], irs, eq_on) for s in range(5)])
    assert np.isfinite(got).all() and float(np.abs(twin).max()) > 0.01
    sv.check_scaling(got, twin, ks, f"oracle, {shape}")


# ---- the oracle's window is [b, b + Pmax], exactly ------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", [0, 17, 511])
@pytest.mark.parametrize("channel", [0, 1], ids=["L", "R"])
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "pinf", "ninf"])
@pytest.mark.parametrize("shape", ["taps_512", "taps_1300", "unequal"])
def test_oracle_windows(oracle, noise, shape, value, channel, frame):
    taps = SHAPES[shape]
    irs = irs_for(taps)
    b = 5
    x = sv.poison(noise[:1], 0, channel, b * sv.BLOCK + frame, value)
    clean = oracle_run(oracle, noise[0], irs, False)
    got = oracle_run(oracle, x[0], irs, False)
    # the paths the poisoned channel feeds: L -> (Lsl, Lsr), R -> (Rsl, Rsr); the longest of them sets the window
    reach = max(parts_of(taps[2 * channel + e]) for e in range(2))
    lo, hi = sv.reference_window(b, reach)
    assert sv.nonfinite_blocks(got) == list(range(lo, hi + 1)), (sv.nonfinite_blocks(got), (lo, hi))
    if reach == pmax_of(taps):
        assert (lo, hi) == sv.reference_window(b, pmax_of(taps))
    outside = np.ones(N_BLOCKS * sv.BLOCK, bool)
    outside[lo * sv.BLOCK:(hi + 1) * sv.BLOCK] = False
    assert np.array_equal(got[:, outside].view(np.uint32), clean[:, outside].view(np.uint32))
    # per ear: path 2 * channel + ear (the muted path of `unequal` is Rsl: R into the left ear, blocks [b, b + 1])
    for ear in range(2):
        want = list(range(b, b + parts_of(taps[2 * channel + ear]) + 1))
        assert sv.nonfinite_blocks(np.stack([got[ear], got[ear]])) == want, (ear, want)
    # and the checker accepts the oracle against itself under the reference's own window
    sv.check_containment(np.stack([got, clean]), np.stack([clean, clean]), 0, (lo, hi), b * sv.BLOCK + frame, ~np.isfinite(got))


# ---- the checkers can fail -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clean(oracle, noise):
    """(twin [5][2][frames], the scaled run's output, ks): the oracle on taps 512, EQ off"""
    irs = irs_for(SHAPES["taps_512"])
    ks = sv.scales_for(5)
    twin = np.stack([oracle_run(oracle, noise[s], irs, False) for s in range(5)])
    ys = sv.scaled(twin, ks)
    sv.check_scaling(ys, twin, ks)
    return twin, ys, ks


def test_scaling_mutant_one_ulp_in_another_stream(clean):
    twin, ys, ks = clean
    m = ys.copy()
    m[3, 1, 7 * sv.BLOCK + 5] = np.nextafter(m[3, 1, 7 * sv.BLOCK + 5], np.float32(np.inf))
    with pytest.raises(AssertionError, match=r"stream 3 \(scale 2\^80\).* in 1 samples.*channel 1, frame 3589, block 7.*largest difference 1 ulp"):
        sv.check_scaling(m, twin, ks)


@pytest.mark.parametrize("s", [0, 2])
def test_scaling_mutant_leak_from_the_next_stream(clean, s):
    """y[s] += 2^-30 y[s + 1] in the scaled run: a relative leak of 1e-9 between streams of equal level, far below the RMS bar and
    below half an ulp; beside a neighbour 2^40 (s = 0) or 2^120 (s = 2) louder it is anything but"""
    twin, ys, ks = clean
    m = ys.copy()
    m[s] = (m[s].astype(np.float64) + 2.0 ** -30 * m[s + 1].astype(np.float64)).astype(np.float32)
    with pytest.raises(AssertionError, match=rf"stream {s} \(scale 2\^{int(ks[s])}\)"):
        sv.check_scaling(m, twin, ks)
    same = twin.copy()
    same[s] = (same[s].astype(np.float64) + 2.0 ** -30 * same[s + 1].astype(np.float64)).astype(np.float32)
    assert float(np.sqrt(np.mean((same[s].astype(np.float64) - twin[s]) ** 2))) < 1e-8      # what assert_parity would have seen


def test_scaling_mutant_added_constant(clean):
    twin, ys, ks = clean
    m = ys.copy()
    m[2] = m[2] + np.float32(1e-12)         # stream 2 runs at 2^-40 = 9e-13
    with pytest.raises(AssertionError, match=r"stream 2 \(scale 2\^-40\)"):
        sv.check_scaling(m, twin, ks)
    k0 = twin.copy()
    k0[2] = k0[2] + np.float32(1e-12)
    assert int(sv._bits_differ(k0[2], twin[2]).sum()) < twin[2].size // 100     # at amplitude 1 it rounds away almost everywhere


def _contained(clean, b=9, pmax=1):
    """a poisoned run that respects the window: stream 1 non-finite in [b, b + pmax] from frame 17 on"""
    twin = clean[0]
    y = twin.copy()
    ref = sv.window_mask(twin.shape[2], sv.reference_window(b, pmax), from_frame=b * sv.BLOCK + 17)
    y[1][ref] = np.nan
    return twin, y, ref, b * sv.BLOCK + 17


def test_containment_accepts_the_allowed_window(clean):
    twin, y, ref, at = _contained(clean)
    sv.check_containment(y, twin, 1, sv.allowed_window(9, 1, 0, 0), at, ref)
    y[1, :, 8 * sv.BLOCK:13 * sv.BLOCK] = np.inf
    sv.check_containment(y, twin, 1, sv.allowed_window(9, 1, 1, 2), at, ref)


def test_containment_mutant_nan_lingers_one_block_behind(clean):
    twin, y, ref, at = _contained(clean)
    y[1, 0, 13 * sv.BLOCK + 3] = np.nan
    with pytest.raises(AssertionError, match=r"stream 1 \(outside the allowed window of blocks \[8, 12\]: behind it\).*blocks \[13\].*block 13, frame 6659"):
        sv.check_containment(y, twin, 1, sv.allowed_window(9, 1, 1, 2), at, ref)


def test_containment_mutant_nan_one_block_in_front(clean):
    twin, y, ref, at = _contained(clean)
    y[1, 1, 8 * sv.BLOCK - 1] = np.nan
    with pytest.raises(AssertionError, match=r"stream 1 \(outside the allowed window of blocks \[8, 12\]: in front of it\).*blocks \[7\].*block 7, frame 4095"):
        sv.check_containment(y, twin, 1, sv.allowed_window(9, 1, 1, 2), at, ref)


def test_containment_mutant_nan_in_a_neighbour(clean):
    twin, y, ref, at = _contained(clean)
    y[2, 0, 10 * sv.BLOCK] = np.nan
    with pytest.raises(AssertionError, match=r"stream 2 \(a neighbour of the poisoned stream 1\).*block 10, frame 5120"):
        sv.check_containment(y, twin, 1, sv.allowed_window(9, 1, 1, 2), at, ref)


def test_containment_mutant_one_ulp_in_a_neighbour_and_behind_the_window(clean):
    twin, y, ref, at = _contained(clean)
    m = y.copy()
    m[0, 0, 3] = np.nextafter(m[0, 0, 3], np.float32(2))
    with pytest.raises(AssertionError, match=r"stream 0 .*block 0, frame 3\).*finite but different"):
        sv.check_containment(m, twin, 1, sv.allowed_window(9, 1, 1, 2), at, ref)
    m = y.copy()
    m[1, 0, 20 * sv.BLOCK] = np.nextafter(m[1, 0, 20 * sv.BLOCK], np.float32(2))
    with pytest.raises(AssertionError, match=r"stream 1 .*behind it.*block 20"):
        sv.check_containment(m, twin, 1, sv.allowed_window(9, 1, 1, 2), at, ref)


def test_containment_mutant_masked_arithmetically(clean):
    """a device that answers finite values where the reference is non-finite"""
    twin, y, ref, at = _contained(clean)
    y[1, 1, 10 * sv.BLOCK + 100] = 0.0
    with pytest.raises(AssertionError, match=r"stream 1: 1 samples that the reference makes non-finite are finite.*channel 1, block 10, frame 5220"):
        sv.check_containment(y, twin, 1, sv.allowed_window(9, 1, 1, 2), at, ref)

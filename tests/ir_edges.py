"""Response lengths on partition edges, with the energy where an indexing error would hit it.

Every convolution family rounds a response's length up to partitions somewhere: ceil(len / 512) for block 512, groups of four
512-tap partitions padded to a multiple of four for block 2048, (Pmax + 15) / 16 for block 8192, exactly one partition for the table
families.  An off-by-one in any of them shows only at a length that sits on the edge -- a last partition of one tap, a partition
that is exactly full, the last tap of a window wrapping round, a handover between plans when set_ir crosses an edge -- and only if
the taps next to the edge carry energy, which a decaying response's do not.

* edge_loaded_irs / edge_loaded_table: FLAT Gaussian noise (sigma 0.02) plus taps of magnitude about 1 at index 0, at taps - 1 and
  at b - 1, b, b + 1 for b in (512, 2048, 8192) wherever those exist, alternating in sign, amplitudes differing from path to path,
  each ear L1-normalised as synth.hrir_set does.  At 16384 taps one edge tap is about a quarter of a path's L2 amplitude: a
  dropped, doubled or misplaced tap is an error of order 0.1 of the output, not 1e-4.
* reference_f64: f64 FFT convolution in numpy, with the reference's set_ir semantics for responses that change in mid-stream (a
  path's new response sees nothing of the frames in front of it, the tail of the old one is dropped).  Independent of the oracle's
  f32 engine.
* check: relative RMS per stream and per block of 512 frames (tests/stream_placement.py's metric) against RMS_TOL = 1e-6; a failure
  names stream, block, family and length.
* the impulse probe: one unit impulse per stream at a frame that is not on a block boundary; the output must be the response tap for
  tap and nothing behind tap taps - 1.  Its figure is max |error| over the whole output / max |h|.  The bar cannot be derived from
  the formats alone, so it is MEASURED ON THE ORACLE (the f32 restatement of the reference, on the CPU), never on the library under
  test: over LENGTHS["probe"] the oracle's worst figure is 1.36e-7 (taps 2049; tests/test_cpu_ir_edges.py::test_the_oracle_sets_the_impulse_bar
  asserts that ORACLE_PROBE_FIGURE bounds it); the large-transform plans are recorded at up to about twice the oracle's RMS distance
  from f64 and a maximum is noisier than an RMS, so the device is allowed IMPULSE_BAR = 4 x ORACLE_PROBE_FIGURE =
  5.6e-7.

numpy only; nothing here touches the GPU."""
import numpy as np

from tests.stream_placement import assert_sample_within_bar
from tests.util import RMS_TOL

BLOCK = 512
EDGES = (512, 2048, 8192)
SIGMA = 0.02

ORACLE_PROBE_FIGURE = 1.4e-7            # the oracle's worst impulse-probe figure over LENGTHS["probe"] (measured: 1.36e-7), rounded up
IMPULSE_BAR = 4 * ORACLE_PROBE_FIGURE

LONG = (513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 6144, 6145, 8191, 8192, 8193, 16383, 16384, 16385)
LENGTHS = {
    "block512_p1": (1, 2, 511, 512),
    "hop1536_p1": (1, 2, 511, 512),
    "sequential": LONG,
    "block512_tp": LONG,
    "block2048": LONG,
    "block8192": (513, 2049, 8191, 8192, 8193, 16383, 16384),
    "engine": (511, 512, 513, 1025, 8193, 16385),
    "tables": (1, 2, 511, 512),
    "probe": (512, 513, 2048, 2049, 8192, 8193, 16384),
}
MIXED = ((512, 513, 1, 2049), (8192, 8193, 0, 2048), (16384, 16385, 511, 513))
TRANSITIONS = ((512, 513), (2048, 2049), (8192, 8193), (16384, 16385))


def all_lengths():
    return sorted({t for v in LENGTHS.values() for t in v})


def partitions(taps, block=BLOCK):
    """partitions of `block` taps a response of `taps` taps occupies; an empty response is one partition of zeros"""
    return max(1, -(-int(taps) // block))


def edge_indices(taps):
    idx = {0, taps - 1} | {b + d for b in EDGES for d in (-1, 0, 1)}
    return sorted(i for i in idx if 0 <= i < taps)


def _edge_loaded_rows(n_rows, taps, seed):
    """[n_rows][taps] f64, not normalised: the flat background and the edge taps; row r's j-th edge tap is (-1)^(j + r) (0.7 + 0.1
    ((r + 2 j) mod 4))"""
    rng = np.random.default_rng([int(seed), int(taps), int(n_rows)])
    h = SIGMA * rng.standard_normal((n_rows, taps))
    for r in range(n_rows):
        for j, i in enumerate(edge_indices(taps)):
            h[r, i] += (-1.0) ** (j + r) * (0.7 + 0.1 * ((r + 2 * j) % 4))
    return h


def edge_loaded_irs(taps, seed=0):
    """[lsl, lsr, rsl, rsr], float32 [taps] each (taps == 0: four empty responses); out_l = lsl + rsl, out_r = lsr + rsr are
    L1-normalised per ear"""
    if taps == 0:
        return [np.zeros(0, np.float32) for _ in range(4)]
    h = _edge_loaded_rows(4, taps, seed)
    nl = np.abs(h[0]).sum() + np.abs(h[2]).sum()
    nr = np.abs(h[1]).sum() + np.abs(h[3]).sum()
    return [(h[0] / nl).astype(np.float32), (h[1] / nr).astype(np.float32), (h[2] / nl).astype(np.float32), (h[3] / nr).astype(np.float32)]


def edge_loaded_table(K, taps, seed=0):
    """[K][2][taps] float32 for layouts and direction tables: entry k's (left, right) responses, built the same way; each ear's K
    responses are L1-normalised together"""
    h = _edge_loaded_rows(2 * K, taps, seed).reshape(K, 2, taps)
    return (h / np.abs(h).sum(axis=(0, 2), keepdims=True)).astype(np.float32)


def mixed_irs(lengths, seed=0):
    """four paths of four different lengths: path p is path p of edge_loaded_irs(lengths[p]) (an ear's L1 sum is at most 1)"""
    return [edge_loaded_irs(t, seed + p)[p] for p, t in enumerate(lengths)]


# ---- the f64 reference ------------------------------------------------------------------------------------------------------------
def conv_f64(x, h):
    """the first len(x) samples of the linear convolution of x with h, in f64 by one real FFT"""
    x, h = np.asarray(x, np.float64), np.asarray(h, np.float64)
    if h.size == 0 or x.size == 0:
        return np.zeros(x.size)
    n = 1 << int(np.ceil(np.log2(x.size + h.size)))
    return np.fft.irfft(np.fft.rfft(x, n) * np.fft.rfft(h, n), n)[:x.size]


def timeline_of(irs):
    """irs: four responses, or per path a list of (first frame, response) -> the latter"""
    return [list(v) if isinstance(v, list) else [(0, v)] for v in irs]


def binaural(x, irs, conv1=conv_f64):
    """x [2][n] through the four paths -> [2][n] f64.  A path whose response changes sees, from the new response's first frame on,
    nothing of the frames in front of it, and the old response's tail is dropped (the reference's set_ir).  conv1(x, h): the
    convolver of one path (the mutants of tests/test_cpu_ir_edges.py replace it)."""
    x = np.asarray(x)
    n = x.shape[1]
    y = np.zeros((2, n))
    for p, tl in enumerate(timeline_of(irs)):
        for i, (t0, h) in enumerate(tl):
            t1 = tl[i + 1][0] if i + 1 < len(tl) else n
            if len(h) and t1 > t0:
                y[p & 1, t0:t1] += conv1(x[p >> 1, t0:t1], h)
    return y


def reference_f64(x, irs, gain=1.0):
    """x [S][2][n] -> [S][2][n] f64"""
    return gain * np.stack([binaural(xs, irs) for xs in np.asarray(x)])


# ---- the checker ------------------------------------------------------------------------------------------------------------------
def check(got, ref, streams, family, taps, against, bar=RMS_TOL):
    """got, ref [len(streams)][2][k * 512]: relative RMS per stream and block of 512 at most `bar` (every reference block must carry
    signal: the helper asserts it); a failure names stream, block, family and length -> the worst figure"""
    return assert_sample_within_bar(got, ref, list(streams), bar, f"{family}, taps {taps}, against {against}")


# ---- the impulse probe ------------------------------------------------------------------------------------------------------------
PROBE_FRAMES = (517, 1023, 1541)        # stream s: channel s mod 2, frame PROBE_FRAMES[s mod 3]: none on a block boundary


def _streams(streams):
    return list(range(streams)) if isinstance(streams, (int, np.integer)) else [int(s) for s in streams]


def probe_input(S, frames):
    x = np.zeros((S, 2, frames), np.float32)
    for s in range(S):
        x[s, s % 2, PROBE_FRAMES[s % 3]] = 1.0
    return x


def probe_expected(streams, frames, irs):
    """what the probe must return for the streams `streams` (a count: 0 .. count - 1), exactly: the two responses of the impulse's
    channel, tap for tap from the impulse's frame on, zeros in front and behind"""
    streams = _streams(streams)
    want = np.zeros((len(streams), 2, frames))
    for i, s in enumerate(streams):
        c, f = s % 2, PROBE_FRAMES[s % 3]
        for ear in range(2):
            h = np.asarray(irs[2 * c + ear], np.float64)
            assert f + h.size <= frames, "the probe must see the whole response and what lies behind it"
            want[i, ear, f:f + h.size] = h
    return want


def probe_figure(got, irs, streams=None, want=None):
    """got [len(streams)][2][frames] -> (max |error| over the whole output / max |h|, (stream, ear, tap index relative to the
    impulse) of it).  want: the expectation where it is not probe_expected's (responses that change behind the impulse)"""
    got = np.asarray(got, np.float64)
    streams = _streams(got.shape[0] if streams is None else streams)
    err = np.abs(got - (probe_expected(streams, got.shape[2], irs) if want is None else want))
    i, ear, f = np.unravel_index(int(np.argmax(err)), err.shape)
    hmax = max(float(np.abs(np.asarray(h)).max()) for h in irs if len(h))
    return float(err.max()) / hmax, (streams[i], int(ear), int(f) - PROBE_FRAMES[streams[i] % 3])


def assert_probe(got, irs, family, taps, streams=None, want=None, bar=IMPULSE_BAR):
    assert np.isfinite(np.asarray(got)).all(), f"{family}, taps {taps}: non-finite samples in the impulse probe"
    fig, (s, ear, tap) = probe_figure(got, irs, streams, want)
    assert fig <= bar, (f"impulse probe, {family}, taps {taps}: |error| / max|h| = {fig:.3e} in stream {s}, ear {ear}, tap {tap} "
                        f"(block {(tap + PROBE_FRAMES[s % 3]) // BLOCK}; the response ends at tap {taps - 1}); bar {bar:.1e}")
    return fig

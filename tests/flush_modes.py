"""The convolution under the handle's flush-denormals mode: the inputs and checkers of tests/test_cpu_flush_modes.py and
tests/test_gpu_flush_modes.py.

set_flush_denormals(1) flushes subnormal RESULTS to zero (FTZ), (2) also reads subnormal INPUTS as zero (FTZ | DAZ).  Three
observable promises follow for every kernel a handle launches, each held against a twin handle in mode 0:

A. normal range: on input of amplitude 1 no operand and no result is subnormal, so the mode changes no bit (same_bits) -- a wrong
   register field (rounding instead of denormals), a mode-dependent kernel variant or an uninitialised mode field does;
B. below the range: `silent_input` (every partial sum of 16 384 samples still subnormal: modes 1 and 2) and `subnormal_input`
   (every sample subnormal: mode 2) come out as zeros, and the state they leave is silence (check_silent; the twin must be alive);
C. through the range: on `falling_input`, which crosses 2^-126 one octave per block, no subnormal sample ever leaves
   (check_no_subnormal; the twin must hold at least NEED of them per stream, or the case shows nothing).

Pure numpy.  Audio is [streams][channels][frames] float32; a block is 512 frames; a subnormal sample is 0 < |v| < 2^-126."""
import numpy as np

BLOCK = 512
TINY = np.float32(2.0 ** -126)
NEED = 100              # subnormal samples per stream of the mode-0 twin over a case of property C: a condition, not a tolerance


# ---- the inputs, each from the same noise u [S][C][frames] of amplitude 1 ----------------------------------------------------------------
def silent_input(u):
    """round(u 256) 2^-149: |x| <= 2^-141, on the grid of the smallest subnormal; a sum over 16 384 of them stays below 2^-126"""
    u = np.asarray(u, np.float64)
    x = np.ldexp(np.round(u * 256.0), -149).astype(np.float32)
    assert float(np.abs(x).max()) <= 2.0 ** -141
    return x


def subnormal_input(u):
    """u 2^-126: every sample subnormal or zero (|u| < 1)"""
    u = np.asarray(u, np.float64)
    assert float(np.abs(u).max()) < 1.0
    x = np.ldexp(u, -126).astype(np.float32)
    assert not (np.abs(x) >= TINY).any()
    return x


def falling_input(u, c):
    """stream s, frame n: u 2^min(0, -124 - s + (c 512 - n) / 512) as f32: one octave down per block, through 2^-124 at block c"""
    u = np.asarray(u, np.float64)
    S, _, frames = u.shape
    e = -124.0 - np.arange(S)[:, None, None] + (c * BLOCK - np.arange(frames)[None, None, :]) / BLOCK
    return (u * np.exp2(np.minimum(0.0, e))).astype(np.float32)


def subnormal_mask(y):
    a = np.abs(np.asarray(y, np.float32))
    return (a > 0) & (a < TINY)


# ---- the checkers --------------------------------------------------------------------------------------------------------------------------
def _bits(v):
    return f"{int(np.float32(v).view(np.uint32)):#010x}"


def _where(y, idx, first_block):
    s, c, f = (int(v) for v in idx)
    return f"stream {s}, channel {c}, frame {f}, block {first_block + f // BLOCK}: {y[s, c, f]!r} (bits {_bits(y[s, c, f])})"


def _first(mask):
    idx = np.argwhere(mask)
    return idx[np.lexsort((idx[:, 1], idx[:, 0], idx[:, 2]))[0]]       # the earliest frame


def _audio(y):
    y = np.ascontiguousarray(y, np.float32)
    assert y.ndim == 3, y.shape
    return y


def check_same_bits(y, y_twin, what="", first_block=0):
    """A: every sample of every stream has the twin's bits; the twin (mode 0) holds no subnormal sample"""
    y, y_twin = _audio(y), _audio(y_twin)
    assert y.shape == y_twin.shape, (y.shape, y_twin.shape)
    pre = what + ": " if what else ""
    sub = subnormal_mask(y_twin)
    assert not sub.any(), f"{pre}the mode-0 twin holds {int(sub.sum())} subnormal samples, first at {_where(y_twin, _first(sub), first_block)}: not a case of the normal range"
    d = y.view(np.uint32) != y_twin.view(np.uint32)
    if d.any():
        i = _first(d)
        raise AssertionError(f"{pre}{int(d.sum())} samples of streams {sorted({int(s) for s in np.argwhere(d)[:, 0]})} differ from the mode-0 twin, "
                             f"first at {_where(y, i, first_block)} against {y_twin[tuple(i)]!r} (bits {_bits(y_twin[tuple(i)])})")


def check_silent(y, what="", first_block=0, twin=None):
    """B: every sample is a zero of either sign; twin (the mode-0 run of the same input, when given) is non-zero in more than half
    the samples of every stream -- else the case is vacuous"""
    y = _audio(y)
    pre = what + ": " if what else ""
    nz = y != 0             # (NaN != 0 as well)
    if nz.any():
        raise AssertionError(f"{pre}{int(nz.sum())} samples of streams {sorted({int(s) for s in np.argwhere(nz)[:, 0]})} are not zero, first at "
                             f"{_where(y, _first(nz), first_block)}")
    if twin is not None:
        twin = _audio(twin)
        for s in range(twin.shape[0]):
            n = int(np.count_nonzero(twin[s]))
            assert 2 * n > twin[s].size, f"{pre}vacuous: the mode-0 twin's stream {s} is non-zero in {n} of {twin[s].size} samples only"


def check_no_subnormal(y, what="", first_block=0, twin=None, need=NEED):
    """C: no sample is subnormal (and all are finite); twin (the mode-0 run of the same input, when given) holds at least `need`
    subnormal samples in every stream -- else the case is vacuous"""
    y = _audio(y)
    pre = what + ": " if what else ""
    bad = subnormal_mask(y) | ~np.isfinite(y)
    if bad.any():
        raise AssertionError(f"{pre}{int(bad.sum())} subnormal (or non-finite) samples left in streams {sorted({int(s) for s in np.argwhere(bad)[:, 0]})}, "
                             f"first at {_where(y, _first(bad), first_block)}")
    if twin is not None:
        counts = subnormal_mask(_audio(twin)).sum(axis=(1, 2))
        for s, n in enumerate(counts):
            assert int(n) >= need, f"{pre}vacuous: the mode-0 twin's stream {s} holds {int(n)} subnormal samples, the case needs {need}"
        return [int(n) for n in counts]

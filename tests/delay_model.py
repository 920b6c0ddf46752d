"""The object-distance stage (libohs_delay.so, include/ohs_delay.h) restated in elementwise numpy: THE ARITHMETIC of the header, f64 and
f32, every operation rounded by itself, with the history and the carry.  The device (tests/test_gpu_delay.py) and the host build of
csrc/delay_body.hpp (tests/test_cpu_delay.py) are held to this model's bits; the cases both run are built here.

Host-only: numpy and nothing else.
"""
import numpy as np

BLOCK = 512
TILE = 256              # ohs::DELAY_TILE
LDS_WINDOW = 2048       # ohs::DELAY_LDS_WINDOW
SIXTH = np.float32(1.0 / 6.0)
assert SIXTH == np.float32(float.fromhex("0x1.555556p-3"))

MUTANTS = ("taps_reversed", "ramp_at_j_over_L", "history_one_short", "carry_from_last_d")


def n_segments(n_blocks, seg_blocks):
    return -(-int(n_blocks) // int(seg_blocks))


def weights(f):
    """f: f32 array -> (c_-1, c_0, c_1, c_2), f32"""
    assert f.dtype == np.float32
    one, two, half = np.float32(1.0), np.float32(2.0), np.float32(0.5)
    fm1, fm2, fp1 = f - one, f - two, f + one
    return (((f * fm1) * fm2) * -SIXTH, ((fp1 * fm1) * fm2) * half, ((fp1 * f) * fm2) * -half, ((fp1 * f) * fm1) * SIXTH)


def core(ext, H, front_d, front_g, row_d, row_g, seg_frames, max_delay, mutant=None):
    """One call.  ext [S][K][H + N] f32: the H = max_delay + 2 frames in front of the call, then the call's N; front_* [S][K]; row_*
    [S][segs][K].  -> (y [S][K][N] f32, d at the call's last frame [S][K], (tiles staged in LDS, tiles gathered))"""
    S, K, total = ext.shape
    N = total - H
    assert ext.dtype == np.float32 and N % BLOCK == 0 and H == int(max_delay) + 2
    y = np.empty((S, K, N), np.float32)
    lds = gather = 0
    last_d = None
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(row_d.shape[1]):
            n0 = k * seg_frames
            L = min(seg_frames, N - n0)
            Dp = (front_d if k == 0 else row_d[:, k - 1])[..., None].astype(np.float64)
            Gp = (front_g if k == 0 else row_g[:, k - 1])[..., None].astype(np.float64)
            D, G = row_d[:, k][..., None].astype(np.float64), row_g[:, k][..., None].astype(np.float64)
            j = np.arange(L, dtype=np.float64)
            a = (j if mutant == "ramp_at_j_over_L" else j + 1.0) / np.float64(L)
            d = Dp + (D - Dp) * a
            d = np.minimum(np.maximum(d, 1.0), np.float64(max_delay))
            i = np.floor(d)
            f = (d - i).astype(np.float32)
            g = (Gp + (G - Gp) * a).astype(np.float32)
            c = weights(f)
            if mutant == "taps_reversed":
                c = c[::-1]
            m = (np.arange(n0, n0 + L, dtype=np.int64) + H) - i.astype(np.int64) + 1         # the newest tap's place in ext
            x = [np.take_along_axis(ext, m - t, axis=2) for t in range(4)]
            y[:, :, n0:n0 + L] = g * (((c[0] * x[0] + c[1] * x[1]) + c[2] * x[2]) + c[3] * x[3])
            last_d = d[..., -1]
            # the tiles' forms: the window follows from the delays at a tile's two ends (csrc/delay_body.hpp, delay_window)
            ia, ib = i[..., 0:L:TILE], i[..., TILE - 1:L:TILE]
            wide = (TILE + 3 + np.abs(ia - ib)) > LDS_WINDOW
            gather += int(wide.sum())
            lds += int(wide.size - wide.sum())
    return y, last_d, (lds, gather)


class DelayModel:
    """ohs_delay_create .. ohs_delay_process on the host.  mutant: one of MUTANTS, a deliberately wrong model."""

    def __init__(self, n_streams, max_objects, max_delay, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.S, self.Kmax, self.max_delay, self.mutant = int(n_streams), int(max_objects), int(max_delay), mutant
        self.H = self.max_delay + 2
        self.trace = None           # a list: every call's inputs to core() and its results are appended
        self.reset()

    def reset(self):
        self.hist = np.zeros((self.S, self.Kmax, self.H), np.float32)
        self.carried = None         # (D [S][K] f64, G [S][K] f32)
        self.last_launch = (0, 0)

    def rows(self, a, n_segs, K, dtype):
        a = np.asarray(a, dtype)
        if a.ndim == 2:
            a = np.broadcast_to(a[None], (self.S,) + a.shape)
        assert a.shape[0] == self.S and a.shape[1] >= n_segs and a.shape[2] == K, a.shape
        return np.ascontiguousarray(a[:, :n_segs])

    def process(self, x, delay, seg_blocks, gains=None, carry=None):
        """x [S][K][N] f32; delay [segs][K] or [S][segs][K] f64; gains likewise f32 or None; carry None: True when carried"""
        x = np.asarray(x, np.float32)
        S, K, N = x.shape
        assert S == self.S and 1 <= K <= self.Kmax and N % BLOCK == 0 and N
        n_segs = n_segments(N // BLOCK, seg_blocks)
        seg_frames = min(int(seg_blocks) * BLOCK, N)
        row_d = self.rows(delay, n_segs, K, np.float64)
        row_g = np.ones((S, n_segs, K), np.float32) if gains is None else self.rows(gains, n_segs, K, np.float32)
        assert np.isfinite(row_d).all() and (row_d >= 1).all() and (row_d <= self.max_delay).all() and np.isfinite(row_g).all()
        carry = self.carried is not None if carry is None else bool(carry)
        if carry:
            assert self.carried is not None and self.carried[0].shape[1] == K
            front_d, front_g = self.carried
            hist = self.hist[:, :K]
        else:
            front_d, front_g = row_d[:, 0], row_g[:, 0]
            hist = np.zeros((S, K, self.H), np.float32)
        if self.mutant == "history_one_short":
            hist = hist.copy()
            hist[:, :, 0] = 0.0
        ext = np.concatenate([hist, x], axis=2)
        y, last_d, self.last_launch = core(ext, self.H, front_d, front_g, row_d, row_g, seg_frames, self.max_delay, self.mutant)
        if self.trace is not None:
            self.trace.append(dict(ext=ext, front_d=np.ascontiguousarray(front_d, np.float64), front_g=np.ascontiguousarray(front_g, np.float32),
                                   row_d=row_d, row_g=row_g, seg_frames=seg_frames, y=y, forms=self.last_launch))
        self.hist[:, :K] = ext[:, :, -self.H:]
        self.carried = ((last_d if self.mutant == "carry_from_last_d" else row_d[:, -1]).copy(), row_g[:, -1].copy())
        return y


# ---- the checker -----------------------------------------------------------------------------------------------------------------------
def mismatches(got, want):
    """indices at which got and want differ: bit for bit, a NaN matching any NaN at the same position"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    both_nan = np.isnan(got) & np.isnan(want)
    return np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~both_nan)


def check_bits(got, want, what=""):
    bad = mismatches(got, want)
    assert not len(bad), (f"{what}: {len(bad)} of {np.asarray(got).size} samples differ from the model's bits; first at {bad[0].tolist()}: "
                          f"{np.asarray(got)[tuple(bad[0])]!r} against {np.asarray(want)[tuple(bad[0])]!r}")


# ---- the cases (tests/test_gpu_delay.py runs them on the device, tests/test_cpu_delay.py on the host build and on the mutants) ----------
def noise(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def carry_probe():
    """(D0, D1): a ramp from D0 to D1 whose d at the last frame, D0 + (D1 - D0) as rounded, is not D1.  D1's fraction lies 2^-50 above
    the midpoint of two f32 and rounds up; D0's grid is too coarse for the 2^-50, so that d is the midpoint itself and rounds down, to
    the even neighbour.  Behind the ramp, a segment that holds D1 has the upper f throughout if the carry is D1 as given, and the
    lower one in its first half if the carry is that d."""
    k = (1 << 23) + 2 * 12345                                   # even: the tie (2k + 1) 2^-25 rounds down, to k 2^-24
    tie = np.float64(2 * k + 1) * 2.0 ** -25
    D0, D1 = np.float64(300.7), np.float64(5.0) + tie + 2.0 ** -50     # D1 is just above the tie: f = (k + 1) 2^-24
    end = D0 + (D1 - D0) * np.float64(1.0)                      # D0's grid is 2^-44: the 2^-50 is lost, the tie itself comes back
    assert end != D1 and end == np.float64(5.0) + tie
    assert np.float32(D1 - 5.0) == np.float32((k + 1) * 2.0 ** -24) and np.float32(end - 5.0) == np.float32(k * 2.0 ** -24)
    return float(D0), float(D1)


def base_rows(S=3, K=3, n_segs=4, max_delay=600):
    """per (stream, object) one kind of row, all kinds present: exactly 1 at gain 1; a constant fraction; ramps up and down;
    i + 1 - 2^-40 (f rounds to 1); gains ramping through 0"""
    rng = np.random.default_rng(5)
    d = np.empty((S, n_segs, K), np.float64)
    g = np.ones((S, n_segs, K), np.float32)
    kinds = ["one", "fraction", "up", "down", "edge", "gain0", "up", "down", "fraction"]
    for s in range(S):
        for c in range(K):
            kind = kinds[(s * K + c) % len(kinds)]
            if kind == "one":
                d[s, :, c] = 1.0
            elif kind == "fraction":
                d[s, :, c] = 37.0 + rng.uniform(0.05, 0.95)
                g[s, :, c] = 0.7
            elif kind == "up":
                d[s, :, c] = np.cumsum(rng.uniform(5.0, 120.0, n_segs)) + 1.5
            elif kind == "down":
                d[s, :, c] = (max_delay - np.cumsum(rng.uniform(5.0, 120.0, n_segs)))
                g[s, :, c] = rng.uniform(0.1, 2.0, n_segs)
            elif kind == "edge":
                d[s, :, c] = np.float64(17 + s) + 1.0 - 2.0 ** -40
            elif kind == "gain0":
                d[s, :, c] = 9.25
                g[s, :, c] = np.where(np.arange(n_segs) % 2 == 0, 0.8, -0.6)
    d = np.minimum(np.maximum(d, 1.0), float(max_delay))
    assert (d[0, :, 0] == 1.0).all() and (g[0, :, 0] == 1.0).all()
    edge = d[1, 0, 1]
    assert np.float32(edge - np.floor(edge)) == np.float32(1.0)
    return d, g


def base_case(seg_blocks, S=3, K=3, n_blocks=4, max_delay=600):
    n_segs = n_segments(n_blocks, seg_blocks)
    d, g = base_rows(S, K, 4, max_delay)
    return dict(S=S, Kmax=K, max_delay=max_delay, seg_blocks=seg_blocks,
                calls=[dict(x=noise((S, K, n_blocks * BLOCK), 11), delay=d[:, :n_segs], gains=g[:, :n_segs], carry=False)])


def both_forms_case():
    """one stream, one object, max_delay 65 536: a steady segment, a jump across the whole range inside one segment, steady, and back"""
    d = np.array([[[1.0]], [[65536.0]], [[65535.5]], [[2.25]]]).reshape(1, 4, 1)
    return dict(S=1, Kmax=1, max_delay=65536, seg_blocks=1,
                calls=[dict(x=noise((1, 1, 4 * BLOCK), 12), delay=d, gains=None, carry=False),
                       dict(x=noise((1, 1, 4 * BLOCK), 13), delay=d[:, ::-1].copy(), gains=None, carry=True)])


def chained_case(max_delay, cuts=(1, 2, 1), S=2, K=3, seg_blocks=1):
    """a signal of sum(cuts) blocks as one call and cut into calls under carry; the carry probe is object 0 of stream 0: its second
    row is D1, reached from D0, and the third row holds D1"""
    n_blocks = sum(cuts)
    rng = np.random.default_rng(max_delay)
    n_segs = n_segments(n_blocks, seg_blocks)
    d = rng.uniform(1.0, float(max_delay), (S, n_segs, K))
    g = rng.uniform(-1.5, 1.5, (S, n_segs, K)).astype(np.float32)
    D0, D1 = carry_probe()
    assert n_segs >= 4 and max_delay >= 400
    d[0, 0, 0], d[0, 1, 0], d[0, 2, 0] = D0, D0, D1
    d[0, 3, 0] = D1
    d[1, :, 1] = float(max_delay)           # the oldest tap of the longest delay: the first frame of the history
    x = noise((S, K, n_blocks * BLOCK), 14 + max_delay)
    whole = dict(S=S, Kmax=K, max_delay=max_delay, seg_blocks=seg_blocks, calls=[dict(x=x, delay=d, gains=g, carry=False)])
    calls, at = [], 0
    for n in cuts:
        k0, k1 = at // seg_blocks, n_segments(at + n, seg_blocks)
        assert at % seg_blocks == 0
        calls.append(dict(x=np.ascontiguousarray(x[:, :, at * BLOCK:(at + n) * BLOCK]), delay=np.ascontiguousarray(d[:, k0:k1]),
                          gains=np.ascontiguousarray(g[:, k0:k1]), carry=at > 0))
        at += n
    return whole, dict(whole, calls=calls)


def special_case():
    """max_delay 300, two calls under carry.  Stream 0 object 0 holds the longest delay and an infinity sits max_delay + 2 frames in
    front of the second call: its oldest tap, weight 0, reads it -- 0 * inf is a NaN.  Object 1: a NaN and an infinity in the middle of
    the calls; object 2: subnormal input under a gain of 0.5"""
    max_delay, S, K = 300, 1, 3
    H = max_delay + 2
    d = np.empty((S, 2, K))
    d[0, :, 0], d[0, :, 1], d[0, :, 2] = max_delay, [17.3, 44.9], 5.5
    g = np.array([1.0, 1.0, 0.5], np.float32) * np.ones((S, 2, 1), np.float32)
    x1, x2 = noise((S, K, 2 * BLOCK), 15), noise((S, K, BLOCK), 16)
    x1[0, 0, 2 * BLOCK - H] = np.inf
    x1[0, 1, 300], x1[0, 1, 700], x2[0, 1, 100] = np.nan, np.inf, -np.inf
    x1[0, 2], x2[0, 2] = x1[0, 2] * np.float32(1e-41), x2[0, 2] * np.float32(1e-41)
    assert (np.abs(x1[0, 2]) < np.finfo(np.float32).tiny).all() and (x1[0, 2] != 0).any()
    return dict(S=S, Kmax=K, max_delay=max_delay, seg_blocks=1,
                calls=[dict(x=x1, delay=d, gains=g, carry=False), dict(x=x2, delay=d[:, :1], gains=g[:, :1], carry=True)])


def all_cases():
    """name -> case: everything tests/test_gpu_delay.py compares bit for bit"""
    out = {f"base, seg_blocks {sb}": base_case(sb) for sb in (1, 2, 8)}
    out["both forms"] = both_forms_case()
    for max_delay in (600, 4096):
        out[f"one call, max_delay {max_delay}"], out[f"chained, max_delay {max_delay}"] = chained_case(max_delay)
    out["special values"] = special_case()
    return out


def run_model(case, mutant=None, trace=None):
    m = DelayModel(case["S"], case["Kmax"], case["max_delay"], mutant)
    m.trace = trace
    return [m.process(c["x"], c["delay"], case["seg_blocks"], c["gains"], c["carry"]) for c in case["calls"]]

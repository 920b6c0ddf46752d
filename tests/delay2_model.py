"""The filtered object-distance stage (libohs_delay2.so, include/ohs_delay2.h) restated in elementwise numpy: THE ARITHMETIC of the header,
f64 and f32, every operation rounded by itself, with the pass chosen per segment row, the longer history and the carry of
(D, G, H[5]).  The device (tests/test_gpu_delay2.py) and the host build of csrc/delay2_body.hpp (tests/test_cpu_delay2.py) are held to
this model's bits; the cases both run are built here.  The plain pass is tests/delay_model.py's arithmetic.

Host-only: numpy and tests/delay_model.py.
"""
import numpy as np

from tests import delay_model as dm

BLOCK, TILE, LDS_WINDOW = dm.BLOCK, dm.TILE, dm.LDS_WINDOW
R = 4                   # OHS_DELAY2_FIR_RADIUS
TAPS = R + 1
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 0.0], np.float32)
MIN_FILTERED = 1.0 + R  # the filtered pass's lower clamp, and the smallest delay a filtered call takes

MUTANTS = ("taps_asymmetric", "h_at_j_over_L", "ring_one_short", "clamp_at_1")


def is_identity(h):
    """h [...][5] f32 -> [...] bool: (1.0f, +0, +0, +0, +0) by its bits"""
    h = np.ascontiguousarray(h, np.float32)
    return (h.view(np.uint32) == IDENTITY.view(np.uint32)).all(-1)


def _plain(ext, H, n0, L, Dp, D, Gp, G, a, max_delay):
    """delay_model.core's segment: -> (y [S][K][L], whole delays i [S][K][L])"""
    d = Dp + (D - Dp) * a
    d = np.minimum(np.maximum(d, 1.0), np.float64(max_delay))
    i = np.floor(d)
    f = (d - i).astype(np.float32)
    g = (Gp + (G - Gp) * a).astype(np.float32)
    c = dm.weights(f)
    m = (np.arange(n0, n0 + L, dtype=np.int64) + H) - i.astype(np.int64) + 1
    x = [np.take_along_axis(ext, m - t, axis=2) for t in range(4)]
    return g * (((c[0] * x[0] + c[1] * x[1]) + c[2] * x[2]) + c[3] * x[3]), i


def _filtered(ext, H, n0, L, Dp, D, Gp, G, Hp, Hh, a, max_delay, mutant):
    """the FILTERED pass of one segment.  Hp, Hh [S][K][5] f32 -> (y [S][K][L], i)"""
    d = Dp + (D - Dp) * a
    d = np.minimum(np.maximum(d, 1.0 if mutant == "clamp_at_1" else MIN_FILTERED), np.float64(max_delay))
    i = np.floor(d)
    f = (d - i).astype(np.float32)
    g = (Gp + (G - Gp) * a).astype(np.float32)
    c = dm.weights(f)
    ah = (np.arange(L, dtype=np.float64) / np.float64(L)) if mutant == "h_at_j_over_L" else a
    h = [(Hp[..., r, None].astype(np.float64) + (Hh[..., r, None].astype(np.float64) - Hp[..., r, None].astype(np.float64)) * ah).astype(np.float32)
         for r in range(TAPS)]
    m = (np.arange(n0, n0 + L, dtype=np.int64) + H) - i.astype(np.int64) + 1             # frame m's place in ext
    if mutant == "clamp_at_1":                                                             # (a whole delay below 5 reads behind the call's end)
        ext = np.concatenate([ext, np.zeros(ext.shape[:2] + (R,), np.float32)], axis=2)
    assert (m - 7).min() >= 0 and (m + R).max() < ext.shape[2]
    x = [np.take_along_axis(ext, m - 7 + q, axis=2) for q in range(4 + 2 * R)]            # x[q] is frame m - 7 + q
    v = []
    for e in range(4):                                                                     # the nodes m, m - 1, m - 2, m - 3
        t = 7 - e
        acc = h[0] * x[t]
        for r in range(1, TAPS):
            acc = acc + h[r] * ((x[t - r] + x[t - r]) if mutant == "taps_asymmetric" else (x[t - r] + x[t + r]))
        v.append(acc)
    return g * (((c[0] * v[0] + c[1] * v[1]) + c[2] * v[2]) + c[3] * v[3]), i


def core(ext, H, front_d, front_g, front_h, row_d, row_g, row_h, seg_frames, max_delay, mutant=None):
    """One call.  ext [S][K][H + N] f32: the H = max_delay + 2 + R frames in front of the call, then the call's N; front_* [S][K]
    (front_h [S][K][5]); row_* [S][segs][K] (row_h [S][segs][K][5]); front_h and row_h None: the unfiltered call.
    -> (y [S][K][N] f32, (tiles staged in LDS, tiles gathered, tiles that took the filtered pass))"""
    S, K, total = ext.shape
    N = total - H
    assert ext.dtype == np.float32 and N % BLOCK == 0 and H == int(max_delay) + 2 + R
    y = np.empty((S, K, N), np.float32)
    lds = gather = filtered = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(row_d.shape[1]):
            n0 = k * seg_frames
            L = min(seg_frames, N - n0)
            Dp = (front_d if k == 0 else row_d[:, k - 1])[..., None].astype(np.float64)
            Gp = (front_g if k == 0 else row_g[:, k - 1])[..., None].astype(np.float64)
            D, G = row_d[:, k][..., None].astype(np.float64), row_g[:, k][..., None].astype(np.float64)
            a = (np.arange(L, dtype=np.float64) + 1.0) / np.float64(L)
            yk, i = _plain(ext, H, n0, L, Dp, D, Gp, G, a, max_delay)
            width = TILE + 3 + np.abs(i[..., 0:L:TILE] - i[..., TILE - 1:L:TILE])
            if row_h is not None:
                Hp, Hh = (front_h if k == 0 else row_h[:, k - 1]), row_h[:, k]
                choose = ~(is_identity(Hp) & is_identity(Hh))                                   # [S][K]: the pass is the row's
                if choose.any():
                    yf, i_f = _filtered(ext, H, n0, L, Dp, D, Gp, G, Hp, Hh, a, max_delay, mutant)
                    yk = np.where(choose[..., None], yf, yk)
                    width = np.where(choose[..., None], TILE + 3 + 2 * R + np.abs(i_f[..., 0:L:TILE] - i_f[..., TILE - 1:L:TILE]), width)
                    filtered += int(choose.sum()) * (L // TILE)
            y[:, :, n0:n0 + L] = yk
            gather += int((width > LDS_WINDOW).sum())
            lds += int((width <= LDS_WINDOW).sum())
    return y, (lds, gather, filtered)


class Delay2Model:
    """ohs_delay2_create .. ohs_delay2_process_filtered on the host.  mutant: one of MUTANTS, a deliberately wrong model."""

    def __init__(self, n_streams, max_objects, max_delay, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.S, self.Kmax, self.max_delay, self.mutant = int(n_streams), int(max_objects), int(max_delay), mutant
        self.H = self.max_delay + 2 + R
        self.trace = None           # a list: every call's inputs to core() and its results are appended
        self.reset()

    def reset(self):
        self.hist = np.zeros((self.S, self.Kmax, self.H), np.float32)
        self.carried = None         # (D [S][K] f64, G [S][K] f32, H [S][K][5] f32)
        self.last_launch = (0, 0, 0)

    def rows(self, a, n_segs, K, dtype, inner=()):
        a = np.asarray(a, dtype)
        if a.ndim == 2 + len(inner):
            a = np.broadcast_to(a[None], (self.S,) + a.shape)
        assert a.shape[0] == self.S and a.shape[1] >= n_segs and a.shape[2:] == (K,) + inner, a.shape
        return np.ascontiguousarray(a[:, :n_segs])

    def process(self, x, delay, seg_blocks, gains=None, fir=None, carry=None):
        """x [S][K][N] f32; delay [segs][K] or [S][segs][K] f64; gains likewise f32 or None; fir [segs][K][5] or [S][segs][K][5] f32
        or None: the unfiltered call; carry None: True when carried"""
        x = np.asarray(x, np.float32)
        S, K, N = x.shape
        assert S == self.S and 1 <= K <= self.Kmax and N % BLOCK == 0 and N
        n_segs = dm.n_segments(N // BLOCK, seg_blocks)
        seg_frames = min(int(seg_blocks) * BLOCK, N)
        row_d = self.rows(delay, n_segs, K, np.float64)
        row_g = np.ones((S, n_segs, K), np.float32) if gains is None else self.rows(gains, n_segs, K, np.float32)
        row_h = None if fir is None else self.rows(fir, n_segs, K, np.float32, (TAPS,))
        assert np.isfinite(row_d).all() and (row_d >= 1).all() and (row_d <= self.max_delay).all() and np.isfinite(row_g).all()
        carry = self.carried is not None if carry is None else bool(carry)
        if carry:
            assert self.carried is not None and self.carried[0].shape[1] == K
            front_d, front_g, front_h = self.carried
            hist = self.hist[:, :K]
        else:
            front_d, front_g, front_h = row_d[:, 0], row_g[:, 0], None if row_h is None else row_h[:, 0]
            hist = np.zeros((S, K, self.H), np.float32)
        if row_h is not None:       # what the filtered call refuses
            assert np.isfinite(row_h).all() and (row_d >= MIN_FILTERED).all() and (front_d >= MIN_FILTERED).all()
        if self.mutant == "ring_one_short":
            hist = hist.copy()
            hist[:, :, 0] = 0.0
        ext = np.concatenate([hist, x], axis=2)
        y, self.last_launch = core(ext, self.H, front_d, front_g, front_h if row_h is not None else None, row_d, row_g, row_h, seg_frames,
                                   self.max_delay, self.mutant)
        if self.trace is not None:
            self.trace.append(dict(ext=ext, front_d=np.ascontiguousarray(front_d, np.float64), front_g=np.ascontiguousarray(front_g, np.float32),
                                   front_h=None if row_h is None else np.ascontiguousarray(front_h, np.float32), row_d=row_d, row_g=row_g,
                                   row_h=row_h, seg_frames=seg_frames, max_delay=self.max_delay, y=y, forms=self.last_launch))
        self.hist[:, :K] = ext[:, :, -self.H:]
        last_h = np.ascontiguousarray(np.broadcast_to(IDENTITY, (S, K, TAPS))) if row_h is None else row_h[:, -1].copy()
        self.carried = (row_d[:, -1].copy(), row_g[:, -1].copy(), last_h)
        return y


check_bits, mismatches, noise = dm.check_bits, dm.mismatches, dm.noise


def response(h, w):
    """|H(w)| of the symmetric filter with centre h[0] and sides h[1 .. 4], in f64 from the taps as they are"""
    h = np.asarray(h, np.float64)
    return abs(h[0] + 2.0 * sum(h[r] * np.cos(r * w) for r in range(1, TAPS)))


# ---- the cases (tests/test_gpu_delay2.py runs them on the device, tests/test_cpu_delay2.py on the host build and on the mutants) --------
def random_taps(shape, seed):
    """[shape][5] f32: a centre of 0.3 .. 1 and four signed sides, no two rows alike"""
    rng = np.random.default_rng(seed)
    h = rng.uniform(-0.2, 0.2, tuple(shape) + (TAPS,))
    h[..., 0] = rng.uniform(0.3, 1.0, shape)
    return h.astype(np.float32)


def base_case(seg_blocks, S=3, K=3, n_blocks=4, max_delay=600):
    """delay_model's base rows (fractions, ramps up and down, f rounding to 1, gains through 0) floored at 5 frames, and taps that
    differ in every segment, so that they ramp between them"""
    n_segs = dm.n_segments(n_blocks, seg_blocks)
    d, g = dm.base_rows(S, K, 4, max_delay)
    d = np.maximum(d, MIN_FILTERED)
    assert (d[0, :, 0] == MIN_FILTERED).all()
    h = random_taps((S, 4, K), 31)
    return dict(S=S, Kmax=K, max_delay=max_delay, seg_blocks=seg_blocks,
                calls=[dict(x=noise((S, K, n_blocks * BLOCK), 41), delay=d[:, :n_segs], gains=g[:, :n_segs], fir=h[:, :n_segs], carry=False)])


def mixed_pass_case():
    """four segments of one block.  Object 0: identity, identity, taps, identity -- segment 2's own taps are not the identity while
    the row in front is, segment 3 the reverse; object 1: taps, identity, identity, taps; object 2: the identity throughout.  The
    second call, under carry, starts with the identity everywhere: object 1 is filtered in its first segment by what is carried."""
    S, K, max_delay = 2, 3, 600
    rng = np.random.default_rng(32)
    d = rng.uniform(MIN_FILTERED, 300.0, (S, 4, K))
    g = rng.uniform(0.2, 1.5, (S, 4, K)).astype(np.float32)
    h = random_taps((S, 4, K), 33)
    for k, c in ((0, 0), (1, 0), (3, 0), (1, 1), (2, 1), (0, 2), (1, 2), (2, 2), (3, 2)):
        h[:, k, c] = IDENTITY
    h2 = np.ascontiguousarray(np.broadcast_to(IDENTITY, (S, 2, K, TAPS)))
    return dict(S=S, Kmax=K, max_delay=max_delay, seg_blocks=1,
                calls=[dict(x=noise((S, K, 4 * BLOCK), 42), delay=d, gains=g, fir=h, carry=False),
                       dict(x=noise((S, K, 2 * BLOCK), 43), delay=d[:, :2], gains=g[:, :2], fir=h2, carry=True)])


def edge_case():
    """max_delay 7: a ring of 13 frames.  Object 0 holds a delay of exactly 5.0 -- its newest input is x[n] itself --, object 1 one of
    exactly max_delay: its oldest input, x[n - 13], is the ring's far end.  In the second call, under carry, an infinity stands there
    for frame 0, under the weight c_2 h_4 = 0 h_4: a NaN in that frame.  Object 2 ramps between the two."""
    S, K, max_delay = 1, 3, 7
    d = np.array([[[5.0, 7.0, 5.0]], [[5.0, 7.0, 7.0]]]).reshape(1, 2, 3)
    h = random_taps((S, 2, K), 34)
    x1, x2 = noise((S, K, BLOCK), 44), noise((S, K, BLOCK), 45)
    x1[0, 1, BLOCK - (max_delay + 2 + R)] = np.inf
    return dict(S=S, Kmax=K, max_delay=max_delay, seg_blocks=1,
                calls=[dict(x=x1, delay=d[:, :1], gains=None, fir=h[:, :1], carry=False),
                       dict(x=x2, delay=d[:, 1:], gains=None, fir=h[:, 1:], carry=True)])


def chained_case(max_delay, cuts=(1, 2, 1), S=2, K=3, seg_blocks=1):
    """a signal of sum(cuts) blocks as one call and cut into calls under carry.  Object 1 of stream 1 holds max_delay at a fraction:
    the oldest input of the longest delay, one frame short of the ring's far end, under a weight that is not 0"""
    n_blocks = sum(cuts)
    rng = np.random.default_rng(max_delay)
    n_segs = dm.n_segments(n_blocks, seg_blocks)
    d = rng.uniform(MIN_FILTERED, float(max_delay), (S, n_segs, K))
    g = rng.uniform(-1.5, 1.5, (S, n_segs, K)).astype(np.float32)
    h = random_taps((S, n_segs, K), 35 + max_delay)
    d[1, :, 1] = float(max_delay) - 0.5
    d[0, :, 2] = float(max_delay)
    x = noise((S, K, n_blocks * BLOCK), 46 + max_delay)
    whole = dict(S=S, Kmax=K, max_delay=max_delay, seg_blocks=seg_blocks, calls=[dict(x=x, delay=d, gains=g, fir=h, carry=False)])
    calls, at = [], 0
    for n in cuts:
        k0, k1 = at // seg_blocks, dm.n_segments(at + n, seg_blocks)
        calls.append(dict(x=np.ascontiguousarray(x[:, :, at * BLOCK:(at + n) * BLOCK]), delay=np.ascontiguousarray(d[:, k0:k1]),
                          gains=np.ascontiguousarray(g[:, k0:k1]), fir=np.ascontiguousarray(h[:, k0:k1]), carry=at > 0))
        at += n
    return whole, dict(whole, calls=calls)


def tile_spread(Dp, D, L=BLOCK, max_delay=4090):
    """the largest i_hi - i_lo among the tiles of a filtered segment of L frames that ramps from Dp to D"""
    a = (np.arange(L, dtype=np.float64) + 1.0) / np.float64(L)
    i = np.floor(np.minimum(np.maximum(Dp + (D - Dp) * a, MIN_FILTERED), np.float64(max_delay)))
    return int(np.abs(i[0:L:TILE] - i[TILE - 1:L:TILE]).max())


def window_edge_case():
    """a delay jump inside one segment of 512 frames: object 0's widest filtered window is exactly LDS_WINDOW frames, T + 3 + 2 R +
    (i_hi - i_lo) with a spread of 1 781, and is staged; object 1's is one frame wider and is gathered.  Segment 0 holds 5.0."""
    max_delay, want = 4090, LDS_WINDOW - (TILE + 3 + 2 * R)
    found = {}
    for step in range(4000):
        D = 3570.0 + 0.125 * step
        found.setdefault(tile_spread(5.0, D), D)
    assert want in found and want + 1 in found, sorted(found)[:5]
    d = np.array([[[5.0, 5.0], [found[want], found[want + 1]]]])
    h = random_taps((1, 2, 2), 36)
    return dict(S=1, Kmax=2, max_delay=max_delay, seg_blocks=1, calls=[dict(x=noise((1, 2, 2 * BLOCK), 47), delay=d, gains=None, fir=h, carry=False)])


def all_cases():
    """name -> case: what tests/test_gpu_delay2.py compares bit for bit from this list"""
    out = {f"base, seg_blocks {sb}": base_case(sb) for sb in (1, 2, 8)}
    out["mixed passes"] = mixed_pass_case()
    out["ring of 13"] = edge_case()
    for max_delay in (600, 4090):
        out[f"one call, max_delay {max_delay}"], out[f"chained, max_delay {max_delay}"] = chained_case(max_delay)
    out["window edge"] = window_edge_case()
    return out


def clamp_probe():
    """core()'s inputs for what no call reaches: a filtered row whose front delay, 2.5, lies below 1 + R -- the call refuses it, so the
    clamp of the filtered pass at 5 is held where it can be, at core() and at the host build of delay2_body.hpp.  The first 160 frames
    of the ramp to 21 lie below 5 and are clamped there."""
    S, K, max_delay = 1, 2, 40
    H = max_delay + 2 + R
    ext = noise((S, K, H + BLOCK), 48)
    front_d, row_d = np.array([[2.5, 5.0]]), np.array([[[21.0, 9.5]]])
    ones = np.ones((S, K), np.float32)
    h = random_taps((S, 2, K), 37)
    return dict(ext=ext, front_d=front_d, front_g=ones, front_h=h[:, 0], row_d=row_d, row_g=ones[:, None], row_h=h[:, 1:], seg_frames=BLOCK,
                max_delay=max_delay)


def run_core(t, mutant=None):
    return core(t["ext"], int(t["max_delay"]) + 2 + R, t["front_d"], t["front_g"], t["front_h"], t["row_d"], t["row_g"], t["row_h"], t["seg_frames"],
                t["max_delay"], mutant)


def run_model(case, mutant=None, trace=None, carried=None):
    m = Delay2Model(case["S"], case["Kmax"], case["max_delay"], mutant)
    m.trace = trace
    out = []
    for c in case["calls"]:
        out.append(m.process(c["x"], c["delay"], case["seg_blocks"], c["gains"], c["fir"], c["carry"]))
        if carried is not None:
            carried.append(m.carried)
    return out

"""The f64 model of the object scenes (ohs_scene_process, include/ohs_scene.h) and the scenes the tests run on.  Pure numpy; checked by
tests/test_cpu_scene.py, used by tests/test_gpu_scene.py.

The rules (the header's): object c of stream s has a direction index and a gain per segment.  `old` is the previous segment's entry,
prev_* in front of the call's first block, the block's own without them.  Under CROSSFADE an object CHANGES in the first block of a
segment when its index or its gain's bits differ from old; the PAIR (2 p, 2 p + 1) fades when either of its objects changes.  A fading
pair's frames go (x gain_old) g[n] through the old directions and (x gain_cur) f[n] through the current ones, every other pair's
x gain_cur through the current ones (the products in f32, as the kernel forms them; everything behind them in f64).

model_scene_f64 is block-wise: per block and direction the weighted input, convolved with the direction's two responses and
overlap-added, the tail carried in and out.  direct_scene_f64 evaluates the same rule object by object over the whole signal."""
import numpy as np

BLOCK = 512
RAMP_F = (np.arange(BLOCK, dtype=np.float32) / np.float32(BLOCK)).astype(np.float32)
RAMP_G = ((np.float32(BLOCK) - np.arange(BLOCK, dtype=np.float32)) / np.float32(BLOCK)).astype(np.float32)
MUTANTS = ("gain_no_fade", "wrong_partner", "old_two_back", "fade_all")
# wrong readings that only a WIDE scene shows (tests/test_gpu_scene_wide.py): the change set cut to 32 bits; the old half ending in
# front of pair 31; an odd K's missing partner rendered -- the channel that lies behind the last one, through row 0 at gain 1 --
# instead of being silence (a row alone would not show: the kernel also feeds that partner zeros)
WIDE_MUTANTS = ("mask32", "pair31_dropped", "odd_partner_row0")


def _rows(a, S, n_segs, K, dtype, fill=None):
    if a is None:
        return np.full((S, n_segs, K), fill, dtype)
    a = np.asarray(a, dtype)
    if a.ndim == 2:
        a = np.broadcast_to(a[None], (S,) + a.shape)
    assert a.shape[0] == S and a.shape[1] >= n_segs and a.shape[2] == K, a.shape
    return a[:, :n_segs]


def _prev(p, S, K, dtype):
    if p is None:
        return None
    p = np.asarray(p, dtype)
    return np.broadcast_to(p.reshape(-1, K), (S, K)) if p.size == K else p.reshape(S, K)


def scene_plan(S, K, n_blocks, idx, seg_blocks, gains, prev_idx, prev_gains, crossfade, mutant=None):
    """-> per stream and block a list of passes (object, direction, gain f32, ramp or None): what every object's frames are weighted
    with and which direction they go through.  mutant: one of MUTANTS, a deliberately wrong reading of the rules."""
    seg_blocks = min(int(seg_blocks), n_blocks)
    n_segs = -(-n_blocks // seg_blocks)
    idx = _rows(idx, S, n_segs, K, np.uint32)
    gains = _rows(gains, S, n_segs, K, np.float32, 1.0)
    prev_idx, prev_gains = _prev(prev_idx, S, K, np.uint32), _prev(prev_gains, S, K, np.float32)
    plan = []
    for s in range(S):
        row = []
        for t in range(n_blocks):
            k = t // seg_blocks
            ci, cg = idx[s, k], gains[s, k]
            back = 2 if mutant == "old_two_back" else 1
            if k - back >= 0:
                oi, og = idx[s, k - back], gains[s, k - back]
            else:
                oi = ci if prev_idx is None else prev_idx[s]
                og = cg if prev_gains is None else prev_gains[s]
            first = crossfade and t % seg_blocks == 0
            ch = np.zeros(K, bool)
            if first:
                ch = ci != oi
                if mutant != "gain_no_fade":
                    ch = ch | (cg.view(np.uint32) != np.ascontiguousarray(og).view(np.uint32))
                if mutant == "mask32":
                    ch[32:] = False
            passes = []
            for c in range(K):
                partner = c ^ 1
                fading = bool(ch[c]) or (partner < K and bool(ch[partner]))
                if mutant == "fade_all":
                    fading = bool(ch.any())
                e = c       # the entry object c's direction and gain are read from
                if mutant == "wrong_partner" and c % 2 == 1:        # the pair's second object reads its neighbour's entry
                    e = c + 1 if c + 1 < K else c - 1
                if fading:
                    if not (mutant == "pair31_dropped" and c // 2 == 31):
                        passes.append((c, int(oi[e]), np.float32(og[e]), RAMP_G))
                    passes.append((c, int(ci[e]), np.float32(cg[e]), RAMP_F))
                else:
                    passes.append((c, int(ci[e]), np.float32(cg[e]), None))
            if mutant == "odd_partner_row0" and K % 2 == 1:     # "object" K: see chan()
                passes += [(K, 0, np.float32(1), RAMP_G), (K, 0, np.float32(1), RAMP_F)] if ch[K - 1] else [(K, 0, np.float32(1), None)]
            row.append(passes)
        plan.append(row)
    return plan


def count_fading_passes(plan):
    """the passes through old directions: per stream and block, one per pair with an old half"""
    return sum(len({c // 2 for c, _, _, ramp in passes if ramp is RAMP_G}) for row in plan for passes in row)


def chan(x, s, c):
    """channel c of stream s; behind the last channel, what a contiguous [S][C][frames] holds there: the next stream's first"""
    S, C = x.shape[:2]
    return x[(s + c // C) % S, c % C]


def _weighted(xb, g, ramp):
    v = (xb * g).astype(np.float32)         # the kernel's products, each rounded to f32
    return v if ramp is None else (v * ramp).astype(np.float32)


def model_scene_f64(x, dirs, idx, seg_blocks, gains=None, prev_idx=None, prev_gains=None, crossfade=True, gain=1.0, tail_in=None,
                    with_tail=False, mutant=None):
    """x [S][>= K][n * 512] float32, dirs [n_dirs][2][len], idx / gains [n_segs][K] or [S][n_segs][K] -> gain * y [S][2][n * 512] f64;
    tail_in [S][2][512] f64: what an earlier render left (already times gain); with_tail: also the tail this one leaves"""
    x = np.asarray(x, np.float32)
    h = np.asarray(dirs, np.float32).astype(np.float64)
    S, n = x.shape[0], x.shape[2] // BLOCK
    K = int(np.shape(idx)[-1])
    plan = scene_plan(S, K, n, idx, seg_blocks, gains, prev_idx, prev_gains, crossfade, mutant)
    L = h.shape[2]
    y = np.zeros((S, 2, (n + 1) * BLOCK), np.float64)
    for s in range(S):
        for t in range(n):
            sl = slice(t * BLOCK, (t + 1) * BLOCK)
            u = {}
            for c, d, g, ramp in plan[s][t]:
                u[d] = u.get(d, 0.0) + _weighted(chan(x, s, c)[sl], g, ramp).astype(np.float64)
            for d, ud in u.items():
                for e in range(2):
                    y[s, e, t * BLOCK:t * BLOCK + BLOCK + L - 1] += np.convolve(ud, h[d, e])
    y *= gain
    if tail_in is not None:
        y[:, :, :BLOCK] += tail_in
    return (y[:, :, :n * BLOCK], y[:, :, n * BLOCK:]) if with_tail else y[:, :, :n * BLOCK]


def direct_scene_f64(x, dirs, idx, seg_blocks, gains=None, prev_idx=None, prev_gains=None, crossfade=True, gain=1.0):
    """the same rule, object by object over the whole signal: every object's frames, weighted by ramp and gain, through each
    direction's full response in one time-domain convolution, summed"""
    x = np.asarray(x, np.float32)
    h = np.asarray(dirs, np.float32).astype(np.float64)
    S, frames = x.shape[0], x.shape[2]
    n, K = frames // BLOCK, int(np.shape(idx)[-1])
    plan = scene_plan(S, K, n, idx, seg_blocks, gains, prev_idx, prev_gains, crossfade)
    y = np.zeros((S, 2, frames), np.float64)
    for s in range(S):
        for c in range(K):
            sig = {}
            for t in range(n):
                sl = slice(t * BLOCK, (t + 1) * BLOCK)
                for cc, d, g, ramp in plan[s][t]:
                    if cc == c:
                        sig.setdefault(d, np.zeros(frames, np.float64))[sl] += _weighted(x[s, c, sl], g, ramp)
            for d, u in sig.items():
                for e in range(2):
                    y[s, e] += np.convolve(u, h[d, e])[:frames]
    return gain * y


# ---- the scenes the tests run on ------------------------------------------------------------------------------------------------
def make_scene(S, K, n_blocks, seg_blocks, n_dirs=7, seed=0, shared=False):
    """Independent trajectories: -> (idx [S][n_segs][K] uint32, gains [S][n_segs][K] float32, prev_idx [S][K], prev_gains [S][K]);
    shared: one row for all streams ([n_segs][K], [K]).  Object c moves only in segments k with (k + c) % 3 == 0 -- objects change in
    different segments, pairs with one changing object exist --, object 1 (if any) never moves but changes its gain in every second
    segment, object K - 1 of stream 0 is silent (gain 0) throughout; the other gains are 0.5 .. 1.25, constant per object."""
    rng = np.random.default_rng(9000 + seed)
    n_segs = -(-n_blocks // min(seg_blocks, n_blocks))
    R = 1 if shared else S
    idx = np.zeros((R, n_segs, K), np.uint32)
    gains = np.zeros((R, n_segs, K), np.float32)
    prev_idx = rng.integers(0, n_dirs, (R, K)).astype(np.uint32)
    base = rng.choice(np.array([0.5, 0.75, 1.0, 1.25], np.float32), (R, K))
    for r in range(R):
        cur = prev_idx[r].copy()
        for k in range(n_segs):
            for c in range(K):
                if (k + c) % 3 == 0 and c != 1:
                    cur[c] = (cur[c] + 1 + rng.integers(0, n_dirs - 1)) % n_dirs      # always another direction
            idx[r, k] = cur
            gains[r, k] = base[r]
            if K > 1:
                gains[r, k, 1] = base[r, 1] * np.float32(0.5 if (k // 2) % 2 else 1.0)
        if r == 0 and K > 2:
            gains[r, :, K - 1] = 0.0
    prev_gains = gains[:, 0].copy()
    if K > 1:
        prev_gains[:, 1] = gains[:, 0, 1] * np.float32(0.5)     # a gain change at the call's start
    if K > 2:
        prev_gains[0, K - 1] = 0.0
    if shared:
        return idx[0], gains[0], prev_idx[0], prev_gains[0]
    return idx, gains, prev_idx, prev_gains


def make_switching_rows(S, K, n_segs, n_dirs=7, seed=0):
    """EVERY object's direction differs between consecutive segments (and from prev): -> (idx [S][n_segs][K], prev_idx [S][K])"""
    rng = np.random.default_rng(9500 + seed)
    idx = np.zeros((S, n_segs + 1, K), np.uint32)
    idx[:, 0] = rng.integers(0, n_dirs, (S, K))
    for k in range(1, n_segs + 1):
        idx[:, k] = (idx[:, k - 1] + 1 + rng.integers(0, n_dirs - 1, (S, K))) % n_dirs
    return idx[:, 1:].copy(), idx[:, 0].copy()


# ---- wide scenes: up to 64 objects, an explicit list of the objects that change --------------------------------------------------
def wide_patterns(K):
    """The change patterns of a K-object scene, K in (33, 63, 64): tuples of objects, one pattern per segment.  K = 64: bit 63 alone;
    62 alone (pair 31 through its even object, n_p == 32 behind it); 32 and 33 (the first pair past bit 31); 0 and 63 (the skip from
    pair 0 to pair 31 inside one old half); 31 and 32 (neighbours in different pairs across the 32-bit line); all.  K = 63 and 33: the
    same with the odd last object, whose partner is the zero row, in the place of 63 -- alone first."""
    top = K - 1
    if K == 64:
        pats = [(63,), (62,), (32, 33), (0, 63), (31, 32), tuple(range(K))]
    elif K == 63:
        pats = [(62,), (32, 33), (0, 62), (31, 32), tuple(range(K)), (61,)]
    else:
        assert K == 33, K
        pats = [(32,), (31, 32), (0, 32), tuple(range(K)), (31,), (1, 32)]
    assert all(max(p) <= top for p in pats)
    return pats


def wide_loud(K):
    """the few loud objects of a wide scene: 30 .. 35 (those that exist) and the last six"""
    return tuple(sorted({c for c in range(30, 36) if c < K} | set(range(K - 6, K))))


def _wide_rows(S, K, n_segs, changed, loud, n_dirs, seed, blend):
    """-> dict of [S][n_segs + 1][K] rows (entry 0 stands in front of the call): idx, gains, and with blend idx1, weights.  In segment
    k exactly the objects of changed[k] differ from the entry in front, everything else is HELD.  How an object changes rotates
    from one changing object to the next and from stream to stream: its direction; its gain (halved or doubled back; a silent object moves instead: its gain stays 0.0); with
    blend also its weight alone and its second direction alone (beside a weight that is not +0.0; an object with w = +0.0 on both
    sides moves its weight instead).  Weights by c % 4: random in (0, 1); +0.0; j / 8; 0.0 or 1.0.  The second direction of a held
    object with w = +0.0 moves in EVERY segment: never read, no change."""
    assert len(changed) == n_segs and all(0 <= c < K for seg in changed for c in seg)
    rng = np.random.default_rng(9900 + seed)
    loud = set(range(K) if loud is None else loud)
    idx = np.zeros((S, n_segs + 1, K), np.uint32)
    idx1 = np.zeros_like(idx)
    gains = np.zeros((S, n_segs + 1, K), np.float32)
    w = np.zeros((S, n_segs + 1, K), np.float32)
    base = rng.choice(np.array([0.5, 0.75, 1.0, 1.25], np.float32), (S, K))
    idx[:, 0] = rng.integers(0, n_dirs, (S, K))
    off = rng.integers(1, n_dirs, (S, K))           # idx1 = idx + off mod n_dirs: never idx itself
    for c in range(K):
        gains[:, 0, c] = base[:, c] if c in loud else 0.0
        w[:, 0, c] = (rng.uniform(0.05, 0.95, S), 0.0, (1 + c % 7) / 8.0, float(c % 8 == 3))[c % 4]
    idx1[:, 0] = (idx[:, 0] + off) % n_dirs

    def move(a):
        return (int(a) + 1 + int(rng.integers(0, n_dirs - 1))) % n_dirs      # always another direction

    for k in range(1, n_segs + 1):
        for a in (idx, gains, w):
            a[:, k] = a[:, k - 1]
        for s in range(S):
            turn = k
            for c in range(K):
                if c not in changed[k - 1]:
                    continue
                how = (turn + s) % (4 if blend else 2)
                turn += 1
                if how == 1 and c not in loud:
                    how = 0
                if how == 3 and w[s, k - 1, c] == 0:
                    how = 2
                if how == 2 and c % 4 == 1:
                    how = 0
                if how == 0:
                    idx[s, k, c] = move(idx[s, k - 1, c])
                elif how == 1:
                    gains[s, k, c] = gains[s, k - 1, c] * np.float32(0.5 if gains[s, k - 1, c] == base[s, c] else 2.0)
                elif how == 2:
                    w[s, k, c] = (np.float32(rng.uniform(0.05, 0.95)), 0.0, np.float32(1 + (k + c) % 7) / np.float32(8),
                                  np.float32(1.0) - w[s, k - 1, c])[c % 4]
                    if w[s, k, c] == w[s, k - 1, c]:
                        w[s, k, c] = np.float32(0.5) * w[s, k - 1, c]
                else:
                    off[s, c] = 1 + off[s, c] % (n_dirs - 1)
        held_zero = np.array([[c not in changed[k - 1] and w[s, k, c] == 0 and w[s, k - 1, c] == 0 for c in range(K)] for s in range(S)])
        off = np.where(held_zero, 1 + off % (n_dirs - 1), off)
        idx1[:, k] = (idx[:, k] + off) % n_dirs
    out = dict(idx=idx, gains=gains)
    if blend:
        out.update(idx1=idx1, weights=w)
        assert (idx1 != idx).all() and (w >= 0).all() and (w <= 1).all()
    return out


def make_wide_scene(S, K, n_blocks, seg_blocks, changed, loud=None, n_dirs=7, seed=0):
    """A scene of up to 64 objects in which segment k changes exactly the objects changed[k] (segment 0 against prev_*) and holds all
    others: -> (idx [S][n_segs][K] uint32, gains, prev_idx [S][K], prev_gains).  loud: the objects with a gain other than 0.0 (None:
    all).  A changed object moves or, if it is loud, in turn changes its gain."""
    n_segs = -(-n_blocks // min(seg_blocks, n_blocks))
    r = _wide_rows(S, K, n_segs, changed, loud, n_dirs, seed, False)
    return tuple(np.ascontiguousarray(v) for v in (r["idx"][:, 1:], r["gains"][:, 1:], r["idx"][:, 0], r["gains"][:, 0]))

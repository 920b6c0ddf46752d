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
                    passes.append((c, int(oi[e]), np.float32(og[e]), RAMP_G))
                    passes.append((c, int(ci[e]), np.float32(cg[e]), RAMP_F))
                else:
                    passes.append((c, int(ci[e]), np.float32(cg[e]), None))
            row.append(passes)
        plan.append(row)
    return plan


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
                u[d] = u.get(d, 0.0) + _weighted(x[s, c, sl], g, ramp).astype(np.float64)
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

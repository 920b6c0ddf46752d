"""The f64 model of the blended object scenes (ohs_scene2_process_blended, include/ohs_scene2.h) and the scenes its tests run on.  Pure
numpy; checked by tests/test_cpu_scene_blend.py, used by tests/test_gpu_scene_blend.py.

The rule (the header's): object c of stream s has per segment a direction d0, a second direction d1, a weight w in [0, 1] and a gain,
and is rendered through (1 - w) h[d0] + w h[d1].  `old` is the previous segment's entry, prev_* in front of the call's first block, the
block's own without them.  Under CROSSFADE an object CHANGES in the first block of a segment when d0, the weight's bits or the gain's
bits differ from old, or d1 does beside a weight that is not +0.0 on both sides (d1 beside +0.0 before and after is never read: no
change); the PAIR (2 p, 2 p + 1) fades when either of its objects changes.  A fading pair's frames go
(x gain_old) g[n] through the OLD (d0, d1, w) and (x gain_cur) f[n] through the current ones, every other pair's x gain_cur through the
current ones.  The products on the signal and u = 1 - w are formed in f32, as the kernel forms them; everything behind them in f64.

model_blend_f64 is block-wise and blends SIGNALS: per block and direction the weighted input times its share, convolved with the
direction's two responses and overlap-added.  direct_blend_f64 blends RESPONSES: pass by pass the explicit (1 - w) h[d0] + w h[d1],
one time-domain convolution each.  as_2k_scene is the identity conv(u h0 + w h1, x) = conv(h0, u x) + conv(h1, w x) as rows for the
one-direction model and library: 2 K objects on duplicated channels."""
import numpy as np

from tests.scene_model import BLOCK, RAMP_F, RAMP_G, WIDE_MUTANTS, _prev, _rows, _weighted, chan  # noqa: F401

MUTANTS = ("swap_w", "partner_weight", "weight_no_fade", "old_half_cur_weight", "prev_weight_ignored")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def blend_plan(S, K, n_blocks, idx, idx1, weights, seg_blocks, gains, prev_idx, prev_idx1, prev_weights, prev_gains, crossfade,
               mutant=None):
    """-> per stream and block a list of passes (object, d0, d1, w f32, gain f32, ramp or None, old half?)"""
    seg_blocks = min(int(seg_blocks), n_blocks)
    n_segs = -(-n_blocks // seg_blocks)
    idx, idx1 = _rows(idx, S, n_segs, K, np.uint32), _rows(idx1, S, n_segs, K, np.uint32)
    weights = _rows(weights, S, n_segs, K, np.float32)
    gains = _rows(gains, S, n_segs, K, np.float32, 1.0)
    prev_idx, prev_idx1 = _prev(prev_idx, S, K, np.uint32), _prev(prev_idx1, S, K, np.uint32)
    prev_weights, prev_gains = _prev(prev_weights, S, K, np.float32), _prev(prev_gains, S, K, np.float32)
    if mutant == "prev_weight_ignored":
        prev_weights = None
    plan = []
    for s in range(S):
        row = []
        for t in range(n_blocks):
            k = t // seg_blocks
            ci, cj, cw, cg = idx[s, k], idx1[s, k], weights[s, k], gains[s, k]
            if k > 0:
                oi, oj, ow, og = idx[s, k - 1], idx1[s, k - 1], weights[s, k - 1], gains[s, k - 1]
            else:
                oi = ci if prev_idx is None else prev_idx[s]
                oj = cj if prev_idx1 is None else prev_idx1[s]
                ow = cw if prev_weights is None else prev_weights[s]
                og = cg if prev_gains is None else prev_gains[s]
            ch = np.zeros(K, bool)
            if crossfade and t % seg_blocks == 0:
                ch = (ci != oi) | ((cj != oj) & ((_bits(cw) | _bits(ow)) != 0)) | (_bits(cg) != _bits(og))
                if mutant != "weight_no_fade":
                    ch = ch | (_bits(cw) != _bits(ow))
                if mutant == "mask32":
                    ch[32:] = False
            passes = []
            for c in range(K):
                partner = c ^ 1
                fading = bool(ch[c]) or (partner < K and bool(ch[partner]))
                e = partner if mutant == "partner_weight" and partner < K else c     # the entry the WEIGHT is read from
                if fading:
                    w_old = cw[e] if mutant == "old_half_cur_weight" else ow[e]
                    if not (mutant == "pair31_dropped" and c // 2 == 31):
                        passes.append((c, int(oi[c]), int(oj[c]), np.float32(w_old), np.float32(og[c]), RAMP_G, True))
                    passes.append((c, int(ci[c]), int(cj[c]), np.float32(cw[e]), np.float32(cg[c]), RAMP_F, False))
                else:
                    passes.append((c, int(ci[c]), int(cj[c]), np.float32(cw[e]), np.float32(cg[c]), None, False))
            if mutant == "odd_partner_row0" and K % 2 == 1:     # "object" K (scene_model.chan) through row 0, w = +0.0, gain 1
                z, one = np.float32(0), np.float32(1)
                passes += [(K, 0, 0, z, one, RAMP_G, True), (K, 0, 0, z, one, RAMP_F, False)] if ch[K - 1] else [(K, 0, 0, z, one, None, False)]
            row.append(passes)
        plan.append(row)
    return plan


def _shares(w, mutant=None):
    """(share of d0, share of d1): u = 1 - w in f32, as the kernel forms it"""
    w = np.float32(w)
    u = np.float32(np.float32(1.0) - w)
    return (float(w), float(u)) if mutant == "swap_w" else (float(u), float(w))


def count_blended_passes(plan, K):
    """the passes that load four table rows: per stream, block, half and pair, one if a weight of the pair is not +0.0"""
    n = 0
    for row in plan:
        for passes in row:
            seen = set()
            for c, _, _, w, _, _, old in passes:
                if int(_bits(np.float32(w)).ravel()[0]) != 0:
                    seen.add((c // 2, old))
            n += len(seen)
    return n


def count_fading_passes(plan):
    """the passes through old directions: per stream and block, one per pair with an old half"""
    return sum(len({c // 2 for c, _, _, _, _, _, old in passes if old}) for row in plan for passes in row)


def model_blend_f64(x, dirs, idx, idx1, weights, seg_blocks, gains=None, prev_idx=None, prev_idx1=None, prev_weights=None,
                    prev_gains=None, crossfade=True, gain=1.0, tail_in=None, with_tail=False, mutant=None):
    """x [S][>= K][n * 512] float32, dirs [n_dirs][2][len], rows [n_segs][K] or [S][n_segs][K] -> gain * y [S][2][n * 512] f64;
    tail_in [S][2][512] f64: what an earlier render left (already times gain); with_tail: also the tail this one leaves"""
    x = np.asarray(x, np.float32)
    h = np.asarray(dirs, np.float32).astype(np.float64)
    S, n = x.shape[0], x.shape[2] // BLOCK
    K = int(np.shape(idx)[-1])
    plan = blend_plan(S, K, n, idx, idx1, weights, seg_blocks, gains, prev_idx, prev_idx1, prev_weights, prev_gains, crossfade, mutant)
    L = h.shape[2]
    y = np.zeros((S, 2, (n + 1) * BLOCK), np.float64)
    for s in range(S):
        for t in range(n):
            sl = slice(t * BLOCK, (t + 1) * BLOCK)
            u = {}
            for c, d0, d1, w, g, ramp, _ in plan[s][t]:
                v = _weighted(chan(x, s, c)[sl], g, ramp).astype(np.float64)
                s0, s1 = _shares(w, mutant)
                u[d0] = u.get(d0, 0.0) + s0 * v
                u[d1] = u.get(d1, 0.0) + s1 * v
            for d, ud in u.items():
                for e in range(2):
                    y[s, e, t * BLOCK:t * BLOCK + BLOCK + L - 1] += np.convolve(ud, h[d, e])
    y *= gain
    if tail_in is not None:
        y[:, :, :BLOCK] += tail_in
    return (y[:, :, :n * BLOCK], y[:, :, n * BLOCK:]) if with_tail else y[:, :, :n * BLOCK]


def direct_blend_f64(x, dirs, idx, idx1, weights, seg_blocks, gains=None, prev_idx=None, prev_idx1=None, prev_weights=None,
                     prev_gains=None, crossfade=True, gain=1.0):
    """the same rule with the RESPONSES blended: pass by pass the explicit response u h[d0] + w h[d1], convolved in the time domain
    with the pass's weighted frames placed in an otherwise silent signal of the whole length"""
    x = np.asarray(x, np.float32)
    h = np.asarray(dirs, np.float32).astype(np.float64)
    S, frames = x.shape[0], x.shape[2]
    n, K = frames // BLOCK, int(np.shape(idx)[-1])
    plan = blend_plan(S, K, n, idx, idx1, weights, seg_blocks, gains, prev_idx, prev_idx1, prev_weights, prev_gains, crossfade)
    y = np.zeros((S, 2, frames), np.float64)
    for s in range(S):
        for t in range(n):
            for c, d0, d1, w, g, ramp, _ in plan[s][t]:
                sig = np.zeros(frames, np.float64)
                sig[t * BLOCK:(t + 1) * BLOCK] = _weighted(x[s, c, t * BLOCK:(t + 1) * BLOCK], g, ramp)
                s0, s1 = _shares(w)
                for e in range(2):
                    y[s, e] += np.convolve(sig, s0 * h[d0, e] + s1 * h[d1, e])[:frames]
    return gain * y


def as_2k_scene(x, idx, idx1, weights, gains=None, prev_idx=None, prev_idx1=None, prev_weights=None, prev_gains=None):
    """The blended scene of K objects as a one-direction scene of 2 K: channel 2 c is x[c] on d0 with gain (1 - w) g, channel 2 c + 1
    is x[c] again on d1 with gain w g (f32 products).  -> (x2, idx2, gains2, prev_idx2, prev_gains2) in the shapes given; prev_*2 are
    None where BOTH their sources are None."""
    x = np.asarray(x, np.float32)
    K = int(np.shape(idx)[-1])
    x2 = np.ascontiguousarray(np.repeat(x[:, :K], 2, axis=1))

    def inter(a, b, dtype):
        a, b = np.asarray(a, dtype), np.asarray(b, dtype)
        return np.ascontiguousarray(np.stack([a, b], axis=-1).reshape(a.shape[:-1] + (2 * K,)))

    def split(w, g):
        w = np.asarray(w, np.float32)
        g = np.ones_like(w) if g is None else np.asarray(g, np.float32)
        u = (np.float32(1.0) - w).astype(np.float32)
        return inter((u * g).astype(np.float32), (w * g).astype(np.float32), np.float32)
    idx2, gains2 = inter(idx, idx1, np.uint32), split(weights, gains)
    first = (lambda a: np.asarray(a)[..., 0, :])
    pi2 = pg2 = None
    if prev_idx is not None or prev_idx1 is not None:
        pi2 = inter(first(idx) if prev_idx is None else prev_idx, first(idx1) if prev_idx1 is None else prev_idx1, np.uint32)
    if prev_weights is not None or prev_gains is not None:
        g0 = None if gains is None else first(gains)
        pg2 = split(first(weights) if prev_weights is None else prev_weights, g0 if prev_gains is None else prev_gains)
    return x2, idx2, gains2, pi2, pg2


# ---- the scenes the tests run on ------------------------------------------------------------------------------------------------
def make_blend_scene(S, K, n_blocks, seg_blocks, n_dirs=7, seed=0, shared=False):
    """tests.scene_model.make_scene's trajectories (idx, gains, prev_idx, prev_gains) with a second direction and a weight per object:
    -> dict(idx, idx1, weights, gains, prev_idx, prev_idx1, prev_weights, prev_gains).  By object c % 4:
      0  weights random f32 in (0, 1), a new one whenever (k + c) % 2 == 0 -- between them the object changes ONLY in w, or not at all;
      1  weight +0.0 throughout (a plain object beside a blended one in its pair); idx1 moves whenever k % 3 == 1, which is NO change;
      2  weights j / 8, j stepping through 1 .. 7 every second segment; idx1 moves at every odd k: there a change ONLY in idx1;
      3  weights 0 or 1: 1.0 in segments with k % 4 >= 2.
    idx1 never equals idx.  prev_weights differs from the first segment's weights for the objects 0 and 2 mod 4 (a change only in w at
    the call's start); prev_idx1 is the first segment's idx1 except for the objects 1 mod 4 (+0.0 on both sides: no change)."""
    from tests.scene_model import make_scene
    idx, gains, prev_idx, prev_gains = make_scene(S, K, n_blocks, seg_blocks, n_dirs, seed, shared)
    rng = np.random.default_rng(9700 + seed)
    three = idx.ndim == 3
    I = idx if three else idx[None]
    R, n_segs, _ = I.shape
    idx1 = np.zeros_like(I)
    w = np.zeros(I.shape, np.float32)
    for r in range(R):
        off = rng.integers(1, n_dirs, K)              # idx1 = idx + off mod n_dirs: never idx itself
        cur_w = rng.uniform(0.05, 0.95, K).astype(np.float32)
        for k in range(n_segs):
            for c in range(K):
                kind = c % 4
                if kind == 0:
                    if (k + c) % 2 == 0:
                        cur_w[c] = np.float32(rng.uniform(0.05, 0.95))
                    w[r, k, c] = cur_w[c]
                elif kind == 1:
                    if k % 3 == 1:
                        off[c] = 1 + (off[c] % (n_dirs - 1))
                elif kind == 2:
                    if k % 2 == 1:
                        off[c] = 1 + (off[c] % (n_dirs - 1))
                    w[r, k, c] = np.float32(1 + ((k // 2) + c) % 7) / np.float32(8)
                else:
                    w[r, k, c] = np.float32(1.0 if k % 4 >= 2 else 0.0)
                idx1[r, k, c] = (int(I[r, k, c]) + int(off[c])) % n_dirs
    prev_idx1 = idx1[:, 0].copy()
    prev_w = w[:, 0].copy()
    for c in range(K):
        if c % 4 == 1:
            prev_idx1[:, c] = (prev_idx1[:, c] + 1) % n_dirs
        if c % 4 in (0, 2):
            prev_w[:, c] = np.float32(1.0) - prev_w[:, c] * np.float32(0.5)
    assert (idx1 != I).all() and (w >= 0).all() and (w <= 1).all() and (prev_w >= 0).all() and (prev_w <= 1).all()
    if not three:
        idx1, w, prev_idx1, prev_w = idx1[0], w[0], prev_idx1[0], prev_w[0]
    return dict(idx=idx, idx1=idx1, weights=w, gains=gains, prev_idx=prev_idx, prev_idx1=prev_idx1, prev_weights=prev_w,
                prev_gains=prev_gains)


def make_wide_blend_scene(S, K, n_blocks, seg_blocks, changed, loud=None, n_dirs=7, seed=0):
    """tests.scene_model.make_wide_scene with a second direction and a weight per object: segment k changes exactly the objects
    changed[k] and holds all others -> dict(idx, idx1, weights, gains, prev_idx, prev_idx1, prev_weights, prev_gains), rows per stream.
    A changed object in turn moves, changes its gain, changes ONLY its weight, changes ONLY its second direction (_wide_rows)."""
    from tests.scene_model import _wide_rows
    n_segs = -(-n_blocks // min(seg_blocks, n_blocks))
    r = _wide_rows(S, K, n_segs, changed, loud, n_dirs, seed, True)
    out = {}
    for k, v in r.items():
        out[k], out["prev_" + k] = np.ascontiguousarray(v[:, 1:]), np.ascontiguousarray(v[:, 0])
    return out

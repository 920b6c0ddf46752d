"""The f64 model of the three-direction object scenes (ohs_scene3_process_blended3, include/ohs_scene3.h) and the scenes its tests run
on.  Pure numpy; checked by tests/test_cpu_scene_blend3.py, used by tests/test_gpu_scene_blend3.py.  It follows
tests/scene_blend_model.py.

The rule (the header's): object c of stream s has per segment three directions d0, d1, d2, two weights w1, w2 (each >= 0, w1 + w2 <= 1)
and a gain, and is rendered through u h[d0] + w1 h[d1] + w2 h[d2], u = (1 - w1) - w2.  `old` is the previous segment's entry, prev_* in
front of the call's first block, the block's own without them.  Under CROSSFADE an object CHANGES in the first block of a segment when
d0, the bits of w1, of w2 or of the gain differ from old, or d1 does beside a w1 that is not +0.0 on both sides, or d2 beside a w2 that
is not +0.0 on both sides; the PAIR (2 p, 2 p + 1) fades when either of its objects changes.  A fading pair's frames go
(x gain_old) g[n] through the OLD (d0, d1, d2, w1, w2) and (x gain_cur) f[n] through the current ones, every other pair's x gain_cur
through the current ones.  The products on the signal and u are formed in f32, as the kernel forms them; everything behind them in f64.

model_blend3_f64 is block-wise and blends SIGNALS; direct_blend3_f64 blends RESPONSES, one time-domain convolution per pass.
as_3k_scene is the identity conv(u h0 + w1 h1 + w2 h2, x) = conv(h0, u x) + conv(h1, w1 x) + conv(h2, w2 x) as rows for the
one-direction model and library: 3 K objects on triplicated channels.  count_* are the launch figures."""
import numpy as np

from tests.scene_model import BLOCK, RAMP_F, RAMP_G, _prev, _rows, _weighted, chan  # noqa: F401

# u formed as 1 - w1; an object whose w2 is +0.0 reads its d2 with the partner's w2 (d2 read beside w2 = +0.0); the old half of a fade
# with the new w2; a change of idx2 ignored beside a nonzero w2
MUTANTS = ("u_without_w2", "d2_beside_zero", "old_half_cur_w2", "idx2_change_ignored")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def blend3_plan(S, K, n_blocks, idx, idx1, idx2, w1, w2, seg_blocks, gains, prev_idx, prev_idx1, prev_idx2, prev_w1, prev_w2, prev_gains,
                crossfade, mutant=None):
    """-> per stream and block a list of passes (object, d0, d1, d2, w1 f32, w2 f32, gain f32, ramp or None, old half?)"""
    seg_blocks = min(int(seg_blocks), n_blocks)
    n_segs = -(-n_blocks // seg_blocks)
    idx, idx1, idx2 = (_rows(a, S, n_segs, K, np.uint32) for a in (idx, idx1, idx2))
    w1, w2 = _rows(w1, S, n_segs, K, np.float32), _rows(w2, S, n_segs, K, np.float32)
    gains = _rows(gains, S, n_segs, K, np.float32, 1.0)
    prev_idx, prev_idx1, prev_idx2 = (_prev(a, S, K, np.uint32) for a in (prev_idx, prev_idx1, prev_idx2))
    prev_w1, prev_w2, prev_gains = (_prev(a, S, K, np.float32) for a in (prev_w1, prev_w2, prev_gains))
    plan = []
    for s in range(S):
        row = []
        for t in range(n_blocks):
            k = t // seg_blocks
            ci, cj, ck, cw, cv, cg = idx[s, k], idx1[s, k], idx2[s, k], w1[s, k], w2[s, k], gains[s, k]
            if k > 0:
                oi, oj, ok, ow, ov, og = idx[s, k - 1], idx1[s, k - 1], idx2[s, k - 1], w1[s, k - 1], w2[s, k - 1], gains[s, k - 1]
            else:
                oi = ci if prev_idx is None else prev_idx[s]
                oj = cj if prev_idx1 is None else prev_idx1[s]
                ok = ck if prev_idx2 is None else prev_idx2[s]
                ow = cw if prev_w1 is None else prev_w1[s]
                ov = cv if prev_w2 is None else prev_w2[s]
                og = cg if prev_gains is None else prev_gains[s]
            ch = np.zeros(K, bool)
            if crossfade and t % seg_blocks == 0:
                ch = (ci != oi) | (_bits(cw) != _bits(ow)) | (_bits(cv) != _bits(ov)) | (_bits(cg) != _bits(og))
                ch = ch | ((cj != oj) & ((_bits(cw) | _bits(ow)) != 0))
                if mutant != "idx2_change_ignored":
                    ch = ch | ((ck != ok) & ((_bits(cv) | _bits(ov)) != 0))
            passes = []
            for c in range(K):
                partner = c ^ 1
                fading = bool(ch[c]) or (partner < K and bool(ch[partner]))

                def third(v, c=c, partner=partner):     # the w2 this object's d2 is read with
                    if mutant == "d2_beside_zero" and partner < K and int(_bits(v[c]).ravel()[0]) == 0:
                        return np.float32(v[partner])
                    return np.float32(v[c])
                if fading:
                    v_old = third(cv) if mutant == "old_half_cur_w2" else third(ov)
                    passes.append((c, int(oi[c]), int(oj[c]), int(ok[c]), np.float32(ow[c]), v_old, np.float32(og[c]), RAMP_G, True))
                    passes.append((c, int(ci[c]), int(cj[c]), int(ck[c]), np.float32(cw[c]), third(cv), np.float32(cg[c]), RAMP_F, False))
                else:
                    passes.append((c, int(ci[c]), int(cj[c]), int(ck[c]), np.float32(cw[c]), third(cv), np.float32(cg[c]), None, False))
            row.append(passes)
        plan.append(row)
    return plan


def _shares(w1, w2, mutant=None):
    """(share of d0, of d1, of d2): u = (1 - w1) - w2 in f32, as the kernel forms it"""
    w1, w2 = np.float32(w1), np.float32(w2)
    u = np.float32(np.float32(1.0) - w1)
    if mutant != "u_without_w2":
        u = np.float32(u - w2)
    return float(u), float(w1), float(w2)


def _pass_kinds(passes):
    """{(pair, old half?): 2 if a w2 of the pair is not +0.0, else 1 if a w1 is not, else 0}"""
    kinds = {}
    for c, _, _, _, w1, w2, _, _, old in passes:
        k = 2 if int(_bits(np.float32(w2)).ravel()[0]) != 0 else 1 if int(_bits(np.float32(w1)).ravel()[0]) != 0 else 0
        kinds[(c // 2, old)] = max(kinds.get((c // 2, old), 0), k)
    return kinds


def count_blended_passes(plan):
    """the passes that load four table rows: per stream, block, half and pair, one if a w1 of the pair is not +0.0 and both w2 are"""
    return sum(sum(1 for v in _pass_kinds(passes).values() if v == 1) for row in plan for passes in row)


def count_blended3_passes(plan):
    """the passes that load six table rows: per stream, block, half and pair, one if a w2 of the pair is not +0.0"""
    return sum(sum(1 for v in _pass_kinds(passes).values() if v == 2) for row in plan for passes in row)


def count_fading_passes(plan):
    """the passes through old directions: per stream and block, one per pair with an old half"""
    return sum(len({p[0] // 2 for p in passes if p[8]}) for row in plan for passes in row)


def _plan_of(x, idx, idx1, idx2, w1, w2, seg_blocks, gains, prev_idx, prev_idx1, prev_idx2, prev_w1, prev_w2, prev_gains, crossfade, mutant=None):
    S, n = x.shape[0], x.shape[2] // BLOCK
    K = int(np.shape(idx)[-1])
    return blend3_plan(S, K, n, idx, idx1, idx2, w1, w2, seg_blocks, gains, prev_idx, prev_idx1, prev_idx2, prev_w1, prev_w2, prev_gains,
                       crossfade, mutant)


def model_blend3_f64(x, dirs, idx, idx1, idx2, w1, w2, seg_blocks, gains=None, prev_idx=None, prev_idx1=None, prev_idx2=None, prev_w1=None,
                     prev_w2=None, prev_gains=None, crossfade=True, gain=1.0, tail_in=None, with_tail=False, mutant=None):
    """x [S][>= K][n * 512] float32, dirs [n_dirs][2][len], rows [n_segs][K] or [S][n_segs][K] -> gain * y [S][2][n * 512] f64;
    tail_in [S][2][512] f64: what an earlier render left (already times gain); with_tail: also the tail this one leaves"""
    x = np.asarray(x, np.float32)
    h = np.asarray(dirs, np.float32).astype(np.float64)
    S, n = x.shape[0], x.shape[2] // BLOCK
    plan = _plan_of(x, idx, idx1, idx2, w1, w2, seg_blocks, gains, prev_idx, prev_idx1, prev_idx2, prev_w1, prev_w2, prev_gains, crossfade, mutant)
    L = h.shape[2]
    y = np.zeros((S, 2, (n + 1) * BLOCK), np.float64)
    for s in range(S):
        for t in range(n):
            sl = slice(t * BLOCK, (t + 1) * BLOCK)
            u = {}
            for c, d0, d1, d2, a1, a2, g, ramp, _ in plan[s][t]:
                v = _weighted(chan(x, s, c)[sl], g, ramp).astype(np.float64)
                for d, share in zip((d0, d1, d2), _shares(a1, a2, mutant)):
                    u[d] = u.get(d, 0.0) + share * v
            for d, ud in u.items():
                for e in range(2):
                    y[s, e, t * BLOCK:t * BLOCK + BLOCK + L - 1] += np.convolve(ud, h[d, e])
    y *= gain
    if tail_in is not None:
        y[:, :, :BLOCK] += tail_in
    return (y[:, :, :n * BLOCK], y[:, :, n * BLOCK:]) if with_tail else y[:, :, :n * BLOCK]


def direct_blend3_f64(x, dirs, idx, idx1, idx2, w1, w2, seg_blocks, gains=None, prev_idx=None, prev_idx1=None, prev_idx2=None, prev_w1=None,
                      prev_w2=None, prev_gains=None, crossfade=True, gain=1.0):
    """the same rule with the RESPONSES blended: pass by pass the explicit response u h[d0] + w1 h[d1] + w2 h[d2], convolved in the
    time domain with the pass's weighted frames placed in an otherwise silent signal of the whole length"""
    x = np.asarray(x, np.float32)
    h = np.asarray(dirs, np.float32).astype(np.float64)
    S, frames = x.shape[0], x.shape[2]
    plan = _plan_of(x, idx, idx1, idx2, w1, w2, seg_blocks, gains, prev_idx, prev_idx1, prev_idx2, prev_w1, prev_w2, prev_gains, crossfade)
    y = np.zeros((S, 2, frames), np.float64)
    for s in range(S):
        for t in range(frames // BLOCK):
            for c, d0, d1, d2, a1, a2, g, ramp, _ in plan[s][t]:
                sig = np.zeros(frames, np.float64)
                sig[t * BLOCK:(t + 1) * BLOCK] = _weighted(x[s, c, t * BLOCK:(t + 1) * BLOCK], g, ramp)
                s0, s1, s2 = _shares(a1, a2)
                for e in range(2):
                    y[s, e] += np.convolve(sig, s0 * h[d0, e] + s1 * h[d1, e] + s2 * h[d2, e])[:frames]
    return gain * y


def as_3k_scene(x, idx, idx1, idx2, w1, w2, gains=None, prev_idx=None, prev_idx1=None, prev_idx2=None, prev_w1=None, prev_w2=None,
                prev_gains=None):
    """The scene of K objects as a one-direction scene of 3 K: channels 3 c, 3 c + 1, 3 c + 2 are x[c] on d0, d1, d2 with the gains
    u g, w1 g, w2 g (f32 products).  -> (x3, idx3, gains3, prev_idx3, prev_gains3) in the shapes given; prev_*3 are None where ALL
    their sources are None."""
    x = np.asarray(x, np.float32)
    K = int(np.shape(idx)[-1])
    x3 = np.ascontiguousarray(np.repeat(x[:, :K], 3, axis=1))

    def inter(a, b, c, dtype):
        a, b, c = (np.asarray(v, dtype) for v in (a, b, c))
        return np.ascontiguousarray(np.stack([a, b, c], axis=-1).reshape(a.shape[:-1] + (3 * K,)))

    def split(a1, a2, g):
        a1, a2 = np.asarray(a1, np.float32), np.asarray(a2, np.float32)
        g = np.ones_like(a1) if g is None else np.asarray(g, np.float32)
        u = ((np.float32(1.0) - a1).astype(np.float32) - a2).astype(np.float32)
        return inter((u * g).astype(np.float32), (a1 * g).astype(np.float32), (a2 * g).astype(np.float32), np.float32)
    first = (lambda a: np.asarray(a)[..., 0, :])

    def or_first(p, rows):
        return first(rows) if p is None else p
    idx3, gains3 = inter(idx, idx1, idx2, np.uint32), split(w1, w2, gains)
    pi3 = pg3 = None
    if prev_idx is not None or prev_idx1 is not None or prev_idx2 is not None:
        pi3 = inter(or_first(prev_idx, idx), or_first(prev_idx1, idx1), or_first(prev_idx2, idx2), np.uint32)
    if prev_w1 is not None or prev_w2 is not None or prev_gains is not None:
        g0 = None if gains is None else first(gains)
        pg3 = split(or_first(prev_w1, w1), or_first(prev_w2, w2), g0 if prev_gains is None else prev_gains)
    return x3, idx3, gains3, pi3, pg3


# ---- the scenes the tests run on ------------------------------------------------------------------------------------------------
ROWS = ("idx", "idx1", "idx2", "w1", "w2", "gains")


def make_blend3_scene(S, K, n_blocks, seg_blocks, n_dirs=7, seed=0, shared=False):
    """tests.scene_blend_model.make_blend_scene's trajectories with a third direction and a second weight per object:
    -> dict(idx, idx1, idx2, w1, w2, gains, prev_idx, prev_idx1, prev_idx2, prev_w1, prev_w2, prev_gains).  By object c % 3:
      0  w1 is that scene's weight times 0.6, w2 random f32 in (0.02, 0.39), a new one whenever (k + c) % 2 == 1 -- between them the
         object changes ONLY in w2, or not at all;
      1  w2 +0.0 throughout, w1 that scene's weight (a two-direction or, where that is +0.0 too, a plain object -- beside a
         three-direction one in its pair where it has a partner 0 mod 3); idx2 moves at every odd k, which is NO change;
      2  w1 that scene's FIRST weight times 0.5, held; w2 = (1 + c % 7) / 16, held; idx2 moves in every segment behind the first: a
         change ONLY in idx2 wherever nothing else of the object moves.
    idx2 never equals idx.  prev_w2 differs from the first segment's w2 for the objects 0 mod 3 (a change only in w2 at the call's
    start); prev_idx2 is the first segment's idx2 except for the objects 1 mod 3 (+0.0 on both sides: no change)."""
    from tests.scene_blend_model import make_blend_scene
    sc = make_blend_scene(S, K, n_blocks, seg_blocks, n_dirs, seed, shared)
    rng = np.random.default_rng(9900 + seed)
    three = sc["idx"].ndim == 3
    I = sc["idx"] if three else sc["idx"][None]
    W = (sc["weights"] if three else sc["weights"][None]).astype(np.float32)
    PW = (sc["prev_weights"] if three else sc["prev_weights"][None]).astype(np.float32)
    R, n_segs, _ = I.shape
    idx2 = np.zeros_like(I)
    w1, w2, pw1 = W.copy(), np.zeros(I.shape, np.float32), PW.copy()
    for r in range(R):
        off = rng.integers(1, n_dirs, K)
        cur = rng.uniform(0.02, 0.39, K).astype(np.float32)
        for k in range(n_segs):
            for c in range(K):
                kind = c % 3
                if kind == 0:
                    if (k + c) % 2 == 1:
                        cur[c] = np.float32(rng.uniform(0.02, 0.39))
                    w1[r, k, c] = W[r, k, c] * np.float32(0.6)
                    w2[r, k, c] = cur[c]
                elif kind == 1:
                    if k % 2 == 1:
                        off[c] = 1 + (off[c] % (n_dirs - 1))
                else:
                    if k >= 1:
                        off[c] = 1 + (off[c] % (n_dirs - 1))
                    w1[r, k, c] = W[r, 0, c] * np.float32(0.5)
                    w2[r, k, c] = np.float32(1 + c % 7) / np.float32(16)
                idx2[r, k, c] = (int(I[r, k, c]) + int(off[c])) % n_dirs
    prev_idx2, prev_w2 = idx2[:, 0].copy(), w2[:, 0].copy()
    for c in range(K):
        if c % 3 == 0:
            pw1[:, c] = PW[:, c] * np.float32(0.6)
            prev_w2[:, c] = np.float32(0.4) - prev_w2[:, c] * np.float32(0.5)
        elif c % 3 == 1:
            prev_idx2[:, c] = (prev_idx2[:, c] + 1) % n_dirs
        else:
            pw1[:, c] = PW[:, c] * np.float32(0.5)
    for a, b in ((w1, w2), (pw1, prev_w2)):
        assert (a >= 0).all() and (b >= 0).all() and ((a + b).astype(np.float32) <= 1).all()
    assert (idx2 != I).all()
    if not three:
        idx2, w1, w2, prev_idx2, pw1, prev_w2 = idx2[0], w1[0], w2[0], prev_idx2[0], pw1[0], prev_w2[0]
    return dict(idx=sc["idx"], idx1=sc["idx1"], idx2=idx2, w1=w1, w2=w2, gains=sc["gains"], prev_idx=sc["prev_idx"],
                prev_idx1=sc["prev_idx1"], prev_idx2=prev_idx2, prev_w1=pw1, prev_w2=prev_w2, prev_gains=sc["prev_gains"])


def args(sc):
    """the scene dict as model_blend3_f64's positional rows"""
    return (sc["idx"], sc["idx1"], sc["idx2"], sc["w1"], sc["w2"])


def kw(sc):
    """... and its keyword rows"""
    return {k: sc[k] for k in ("gains", "prev_idx", "prev_idx1", "prev_idx2", "prev_w1", "prev_w2", "prev_gains")}

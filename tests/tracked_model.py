"""What k_scene_rows_seal (csrc/scene_rows_kernels.hip, csrc/scene_rows_body.hpp) does to the rows of a tracked scene call, in numpy:
the planes in front of the call, the carry, and the launch record's three counts.  Two restatements that are held to each other:

  seal        elementwise numpy over whole planes -- the definition the kernel and the host program are held to;
  host_scan   the scan of batch_process_objects_any (api_batch.hip) for three directions and rows per stream, loop for loop, with
              its prev_* arguments -- what libohs_scene3.so counts for the composed path.

Planes are uint32 [6][S][n_segs][K]: idx0, idx1, idx2, the bits of w1, of w2 and of the gain.
"""
import numpy as np

ONE = np.uint32(0x3F800000)
PLANES = 6
D0, D1, D2, W1, W2, G = range(6)


def seg_lens(n_blocks, seg_blocks):
    """-> (seg_blocks clamped to the call, the blocks of every segment)"""
    seg_blocks = min(int(seg_blocks), max(int(n_blocks), 1))
    n_segs = -(-int(n_blocks) // seg_blocks)
    return seg_blocks, np.array([min(seg_blocks, n_blocks - k * seg_blocks) for k in range(n_segs)], np.uint64)


def seal(rows, n_blocks, seg_blocks, fade, carry=None):
    """rows [6][S][n_segs][K]; carry [6][S][K] (CARRY) or None (FRESH) -> dict(front, carry, fading, blended, blended3).
    front: the planes in front of the call; carry: what the handle holds for the next call."""
    rows = np.asarray(rows, np.uint32)
    assert rows.ndim == 4 and rows.shape[0] == PLANES
    _, S, n_segs, K = rows.shape
    _, lens = seg_lens(n_blocks, seg_blocks)
    assert len(lens) == n_segs
    front = rows[:, :, 0, :].copy() if carry is None else np.asarray(carry, np.uint32).reshape(PLANES, S, K).copy()
    old = np.concatenate([front[:, :, None, :], rows[:, :, :-1, :]], axis=2)
    cur = rows
    cur_w1, cur_w2 = cur[W1] != 0, cur[W2] != 0
    old_w1, old_w2 = old[W1] != 0, old[W2] != 0
    ch = (cur[D0] != old[D0]) | (cur[G] != old[G]) | (cur[W1] != old[W1]) | (cur[W2] != old[W2])
    ch |= ((cur[W1] | old[W1]) != 0) & (cur[D1] != old[D1])
    ch |= ((cur[W2] | old[W2]) != 0) & (cur[D2] != old[D2])
    if not fade:
        ch[:] = False
        old_w1[:] = False
        old_w2[:] = False

    def pairs(a):       # [S][n_segs][K] -> [S][n_segs][ceil(K / 2)]: either object of the pair (the absent partner has none)
        pad = np.zeros(a.shape[:-1] + (K % 2,), bool)
        return np.concatenate([a, pad], -1).reshape(a.shape[:-1] + (-1, 2)).any(-1)
    ch, cur_w1, cur_w2, old_w1, old_w2 = (pairs(a) for a in (ch, cur_w1, cur_w2, old_w1, old_w2))
    L = lens[None, :, None]
    fading = int(ch.sum())
    blended = int(((cur_w1 & ~cur_w2) * L).sum() + (ch & old_w1 & ~old_w2).sum())
    blended3 = int((cur_w2 * L).sum() + (ch & old_w2).sum())
    return dict(front=front, carry=rows[:, :, n_segs - 1, :].copy(), fading=fading, blended=blended, blended3=blended3)


def host_scan(n_blocks, seg_blocks, fade, dir_idx, dir_idx1, dir_idx2, weight, weight2, obj_gain=None, prev_idx=None, prev_idx1=None,
              prev_idx2=None, prev_weight=None, prev_weight2=None, prev_gain=None):
    """batch_process_objects_any's scan for a three-direction call with rows per stream: arrays [S][n_segs][K] (bits, uint32), prev_*
    [S][K] or None -> (fading, blended, blended3, prev planes [6][S][K] as the host stages them under CROSSFADE, else None)"""
    ci_, cj_, ck_, cw_, cv_ = (np.asarray(a, np.uint32) for a in (dir_idx, dir_idx1, dir_idx2, weight, weight2))
    S, n_segs, K = ci_.shape
    seg_blocks, lens = seg_lens(n_blocks, seg_blocks)
    cg_ = None if obj_gain is None else np.asarray(obj_gain, np.uint32)
    if obj_gain is None and prev_gain is not None:      # (a gain in front of the call beside no gain rows: the rows read as 1.0)
        cg_ = np.full((S, n_segs, K), ONE, np.uint32)
    if not fade:
        prev_idx = prev_idx1 = prev_idx2 = prev_weight = prev_weight2 = prev_gain = None
    fading = blended = blended3 = 0
    prev = np.zeros((PLANES, S, K), np.uint32) if fade else None
    for r in range(S):
        row, row1, row2, wrow, w2row = ci_[r], cj_[r], ck_[r], cw_[r], cv_[r]
        grow = None if cg_ is None else cg_[r]
        oi = None if prev_idx is None else np.asarray(prev_idx, np.uint32)[r]
        oj = None if prev_idx1 is None else np.asarray(prev_idx1, np.uint32)[r]
        ok = None if prev_idx2 is None else np.asarray(prev_idx2, np.uint32)[r]
        ow = None if prev_weight is None else np.asarray(prev_weight, np.uint32)[r]
        ov = None if prev_weight2 is None else np.asarray(prev_weight2, np.uint32)[r]
        og = None if prev_gain is None else np.asarray(prev_gain, np.uint32)[r]
        if fade:
            oi = row[0] if oi is None else oi
            oj = row1[0] if oj is None else oj
            ow = wrow[0] if ow is None else ow
            og = (None if grow is None else grow[0]) if og is None else og
            ok = row2[0] if ok is None else ok
            ov = w2row[0] if ov is None else ov
            for pl, a in enumerate((oi, oj, ok, ow, ov, og)):
                prev[pl, r] = ONE if a is None else a
        for k in range(n_segs):
            ci, cj, ck, cw, cv = row[k], row1[k], row2[k], wrow[k], w2row[k]
            cg = None if grow is None else grow[k]
            seg_len = int(lens[k])
            for p in range((K + 1) // 2):
                ch = cur_blend = old_blend = cur_tri = old_tri = False
                for o in range(2 * p, min(2 * p + 2, K)):
                    cur_blend = cur_blend or cw[o] != 0
                    cur_tri = cur_tri or cv[o] != 0
                    if not fade:
                        continue
                    old_blend = old_blend or ow[o] != 0
                    old_tri = old_tri or ov[o] != 0
                    ch = ch or (cv[o] != ov[o] or ((cv[o] | ov[o]) != 0 and ck[o] != ok[o]))
                    ch = ch or ci[o] != oi[o] or (ONE if cg is None else cg[o]) != (ONE if og is None else og[o])
                    ch = ch or (cw[o] != ow[o] or ((cw[o] | ow[o]) != 0 and cj[o] != oj[o]))
                fading += 1 if ch else 0
                blended += (seg_len if cur_blend and not cur_tri else 0) + (1 if ch and old_blend and not old_tri else 0)
                blended3 += (seg_len if cur_tri else 0) + (1 if ch and old_tri else 0)
            oi, oj, ow, og, ok, ov = ci, cj, cw, cg, ck, cv
    return fading, blended, blended3, prev


# ---- rows that meet every clause ---------------------------------------------------------------------------------------------------
WEIGHT_BITS = np.array([0x00000000, 0x00000000, 0x80000000, 0x3E800000, 0x3F000000], np.uint32)     # +0.0 (twice as likely), -0.0, 0.25, 0.5
GAIN_BITS = np.array([0x3F800000, 0x3F800000, 0x3F000000], np.uint32)


def random_rows(S, n_segs, K, seed, n_dirs=3, hold=0.5):
    """[6][S][n_segs][K]: few directions and few weights, and every word held from the segment in front with probability `hold`, so
    that each clause of the change rule meets both of its outcomes -- a d1 / d2 that moves beside weights of +0.0 on both sides, one
    that moves beside a weight on one side only, objects that do not change at all"""
    rng = np.random.default_rng(seed)
    rows = np.empty((PLANES, S, n_segs, K), np.uint32)
    for pl in range(PLANES):
        draw = (rng.integers(0, n_dirs, (S, n_segs, K)).astype(np.uint32) if pl < 3 else
                WEIGHT_BITS[rng.integers(0, len(WEIGHT_BITS), (S, n_segs, K))] if pl < 5 else GAIN_BITS[rng.integers(0, len(GAIN_BITS), (S, n_segs, K))])
        for k in range(1, n_segs):
            keep = rng.random((S, K)) < hold
            draw[:, k, :] = np.where(keep, draw[:, k - 1, :], draw[:, k, :])
        rows[pl] = draw
    return rows


def random_carry(S, K, seed, like=None, n_dirs=3):
    """[6][S][K] in front of a call: random_rows' alphabet, half of the words those of `like`'s first segment"""
    c = random_rows(S, 1, K, seed, n_dirs)[:, :, 0, :]
    if like is not None:
        keep = np.random.default_rng(seed + 1).random(c.shape) < 0.5
        c = np.where(keep, like[:, :, 0, :], c)
    return np.ascontiguousarray(c, np.uint32)

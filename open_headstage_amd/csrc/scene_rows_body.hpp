// scene_rows_body.hpp -- the per-object and per-pair step of k_scene_rows_seal (scene_rows_kernels.hip), host and device alike: the
// device form of the scan over the rows in batch_process_objects_any (api_batch.hip), three directions per object.  An entry is an
// object's six words in a segment -- idx0, idx1, idx2, the bits of w1, w2 and of the gain --, `cur` the segment's own and `old` the
// ones in front of it (the segment before; in front of the call's first segment the carried rows, or that segment's own entries).
// tests/scene_rows_host_check.cpp compiles this file for the host and holds it to tests/tracked_model.py.
#pragma once

#ifndef OHS_ROWS_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define OHS_ROWS_HD __host__ __device__
#else
#define OHS_ROWS_HD
#endif
#endif

namespace ohs {

struct SceneRowsEntry {
    unsigned d0, d1, d2, w1, w2, g;
};

// an object's part in its pair's passes
enum : unsigned {
    SCENE_ROWS_CHANGE = 1u,     // the object changes against the entry in front (under CROSSFADE only)
    SCENE_ROWS_CUR_W1 = 2u,     // its w1 is not +0.0 ...
    SCENE_ROWS_CUR_W2 = 4u,     // ... its w2
    SCENE_ROWS_OLD_W1 = 8u,     // the entry in front: its w1 is not +0.0 (under CROSSFADE only) ...
    SCENE_ROWS_OLD_W2 = 16u,    // ... its w2
};

// The object's flags.  It changes when idx0 differs from the entry in front, or the bits of w1, of w2 or of the gain do, or idx1
// beside a w1 that is not +0.0 on both sides, or idx2 beside such a w2 (a second / third index beside a weight of +0.0 before and after
// is never read).  Without a fade nothing in front is looked at.
OHS_ROWS_HD inline unsigned scene_rows_object(const SceneRowsEntry &cur, const SceneRowsEntry &old, bool fade)
{
    unsigned f = (cur.w1 != 0u ? SCENE_ROWS_CUR_W1 : 0u) | (cur.w2 != 0u ? SCENE_ROWS_CUR_W2 : 0u);
    if (!fade) return f;
    f |= (old.w1 != 0u ? SCENE_ROWS_OLD_W1 : 0u) | (old.w2 != 0u ? SCENE_ROWS_OLD_W2 : 0u);
    bool ch = cur.w2 != old.w2 || ((cur.w2 | old.w2) != 0u && cur.d2 != old.d2);
    ch = ch || cur.d0 != old.d0 || cur.g != old.g;
    ch = ch || cur.w1 != old.w1 || ((cur.w1 | old.w1) != 0u && cur.d1 != old.d1);
    return f | (ch ? SCENE_ROWS_CHANGE : 0u);
}

// what a pair of objects adds to the launch record over a segment of seg_len blocks; `flags`: its two objects' flags, or-ed (the absent
// partner of an odd last object has none)
struct SceneRowsPair {
    unsigned fading;            // 1: the pair goes through its old entries in the segment's first block
    unsigned cur4, cur6;        // the current pass loads four rows / six rows, in every block of the segment
    unsigned old4, old6;        // the fading old pass loads four rows / six
};

OHS_ROWS_HD inline SceneRowsPair scene_rows_pair(unsigned flags)
{
    const bool ch = (flags & SCENE_ROWS_CHANGE) != 0u;
    const bool cur_blend = (flags & SCENE_ROWS_CUR_W1) != 0u, cur_tri = (flags & SCENE_ROWS_CUR_W2) != 0u;
    const bool old_blend = (flags & SCENE_ROWS_OLD_W1) != 0u, old_tri = (flags & SCENE_ROWS_OLD_W2) != 0u;
    SceneRowsPair p;
    p.fading = ch ? 1u : 0u;
    // (a pass with a nonzero w2 loads six rows; one without it and with a nonzero w1 loads four)
    p.cur4 = cur_blend && !cur_tri ? 1u : 0u;
    p.cur6 = cur_tri ? 1u : 0u;
    p.old4 = ch && old_blend && !old_tri ? 1u : 0u;
    p.old6 = ch && old_tri ? 1u : 0u;
    return p;
}

// the blocks of segment k of a call of n_blocks cut every seg_blocks (the last segment may be ragged)
OHS_ROWS_HD inline unsigned long long scene_rows_seg_len(unsigned long long k, unsigned long long seg_blocks, unsigned long long n_blocks)
{
    const unsigned long long left = n_blocks - k * seg_blocks;
    return left < seg_blocks ? left : seg_blocks;
}

// the segment whose entries stand in front of the NEXT call (the carry): this call's last
OHS_ROWS_HD inline unsigned long long scene_rows_carry_segment(unsigned long long n_segs) { return n_segs - 1; }

}  // namespace ohs

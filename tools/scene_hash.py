#!/usr/bin/env python3
"""SHA-256 of the object scenes' output on fixed seeded scenes, through all six processing entries: ohs_scene_process (libohs_scene.so),
ohs_scene2_process and ohs_scene2_process_blended (libohs_scene2.so), ohs_scene3_process, ohs_scene3_process_blended and
ohs_scene3_process_blended3 (libohs_scene3.so).  Two builds whose arithmetic is meant to be identical must print the same lines;
tests/golden/scene_output_sha256.txt holds the lines of the build in front of the one that folded the three kernels' text into
csrc/conv_objects_body.hpp, and tests/test_gpu_scene_bits.py holds every later build to them.
    python tools/scene_hash.py [> tests/golden/scene_output_sha256.txt]

Every case: 5 streams, 7 blocks of 512 frames in segments of 2 (four segments, the last one a single block; more than one block range
per stream), 64 directions of 512 taps, gain 0.7, the call made twice on one handle (the second call starts on the first one's
overlap).  The last stream is scaled by 2^-130, so that the flush mode has denormals to decide about.
Pair p of a scene is of kind p % 3 -- 0: both weights +0.0 (two table rows per pass); 1: w1 > 0, w2 +0.0 (four rows); 2: w2 > 0 as
well (six rows) -- and every object's first index moves in every segment and in front of the call, so that under CROSSFADE every pair
of every kind fades in every segment's first block: `expected_launch` is the launch record that follows from that."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

S, BLOCKS, SEG, N_DIRS, TAPS, BLOCK, GAIN = 5, 7, 2, 64, 512, 512, 0.7
N_SEGS = (BLOCKS + SEG - 1) // SEG
# (name, K, crossfade, gains given, one row for all streams, flush mode)
CASES = [("k5", 5, True, True, False, 0), ("k64", 64, True, False, True, 1), ("ringout", 5, False, True, False, 0)]
ENTRIES = ["scene_process", "scene2_process", "scene2_process_blended", "scene3_process", "scene3_process_blended",
           "scene3_process_blended3"]


def directions(seed=4100):
    rng = np.random.default_rng(seed)
    decay = np.exp(-np.arange(TAPS) / 90.0).astype(np.float32)
    return (rng.standard_normal((N_DIRS, 2, TAPS)).astype(np.float32) * decay * np.float32(0.2)).astype(np.float32)


def scene(K, gains, shared, seed):
    """-> (x [S][K][frames], dict of rows); rows [S][N_SEGS][K] (shared: [N_SEGS][K]) and prev_* [S][K] ([K])"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((S, K, BLOCKS * BLOCK)) * 0.25).astype(np.float32)
    x[S - 1] = np.ldexp(x[S - 1], -130)
    R = 1 if shared else S
    step = rng.integers(1, N_DIRS, (R, N_SEGS + 1, K))                      # a step of 1 .. 63 modulo 64: the index moves every time
    idx = (rng.integers(0, N_DIRS, (R, 1, K)) + np.cumsum(step, axis=1)) % N_DIRS
    kind = (np.arange(K) // 2) % 3

    def other():
        return rng.integers(0, N_DIRS, (R, N_SEGS + 1, K))

    def weight(lo, hi, on):
        return np.where(on, rng.uniform(lo, hi, (R, N_SEGS + 1, K)), 0.0).astype(np.float32)
    rows = dict(idx=idx, idx1=other(), idx2=other(), w1=weight(0.05, 0.5, kind >= 1), w2=weight(0.05, 0.4, kind == 2),
                gains=rng.uniform(0.5, 1.5, (R, N_SEGS + 1, K)).astype(np.float32))
    sc = {}
    for name, a in rows.items():
        a = a.astype(np.float32 if a.dtype.kind == "f" else np.uint32)
        cur, prev = np.ascontiguousarray(a[:, 1:]), np.ascontiguousarray(a[:, 0])
        sc[name], sc["prev_" + name] = (cur[0], prev[0]) if shared else (cur, prev)
    if not gains:
        sc["gains"] = sc["prev_gains"] = None
    return x, sc


def expected_launch(K, crossfade, entry):
    """the launch record of `entry` on a scene of K objects: (pairs, fading, four-row, six-row passes), the last two as far as the
    entry's record has them -- the block ranges per stream depend on the device and are not part of it"""
    P = (K + 1) // 2
    n = [len(range(k, P, 3)) for k in range(3)]                             # pairs of kind 0, 1, 2
    per_pair = BLOCKS + (N_SEGS if crossfade else 0)                        # passes of one pair in one stream
    fading = S * N_SEGS * P if crossfade else 0
    if entry in ("scene_process", "scene2_process", "scene3_process"):
        four, six = 0, 0
    elif entry in ("scene2_process_blended", "scene3_process_blended"):     # (w2 is not given: kinds 1 and 2 load four rows)
        four, six = S * (n[1] + n[2]) * per_pair, 0
    else:
        four, six = S * n[1] * per_pair, S * n[2] * per_pair
    width = {"scene_process": 0, "scene2_process": 1, "scene2_process_blended": 1}.get(entry, 2)
    return (P, fading) + (four, six)[:width]


def run_entry(entry, K, crossfade, flush, dirs, x, sc):
    """-> (sha256 of the two calls' outputs, (pairs, ranges, fading[, four-row[, six-row]]) of the second launch)"""
    import torch

    import open_headstage_amd as ohs
    cls = {"scene_": ohs.SceneProcessor, "scene2": ohs.BlendSceneProcessor, "scene3": ohs.TriSceneProcessor}[entry[:6]]
    h = cls(S, num_bands=10)
    h.set_gain(GAIN)
    h.set_flush_denormals(flush)
    h.set_directions(dirs)
    args = [sc["idx"], SEG, sc["gains"], sc["prev_idx"], sc["prev_gains"], crossfade]
    if "blended" in entry:
        args += [sc["idx1"], sc["w1"], sc["prev_idx1"], sc["prev_w1"]]
    if entry.endswith("blended3"):
        args += [sc["idx2"], sc["w2"], sc["prev_idx2"], sc["prev_w2"]]
    d = torch.from_numpy(x).cuda()
    digest = hashlib.sha256()
    for _ in range(2):
        y = h.process(d, *args)
        torch.cuda.synchronize()
        digest.update(y.cpu().numpy().tobytes())
    return digest.hexdigest(), h.last_launch()


def hashes():
    """yields (case name, entry, sha256, launch record, expected_launch's record) for every case and entry"""
    dirs = directions()
    for n, (name, K, crossfade, gains, shared, flush) in enumerate(CASES):
        x, sc = scene(K, gains, shared, seed=4200 + n)
        for entry in ENTRIES:
            digest, launch = run_entry(entry, K, crossfade, flush, dirs, x, sc)
            yield name, entry, digest, launch, expected_launch(K, crossfade, entry)


if __name__ == "__main__":
    for name, entry, digest, launch, want in hashes():
        assert launch[1] > 1 and launch[:1] + launch[2:] == want, (name, entry, launch, want)
        print(name, entry, digest, flush=True)

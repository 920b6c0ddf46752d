#!/usr/bin/env python3
"""Prices the three-direction object-scene call (ohs_scene3_process_blended3, libohs_scene3.so) against what libohs_scene.so offers for
the same scene, against two directions, and against not blending.

Shape (tools/bench_objects_blend.py's): 256 streams x 256 blocks (131 072 frames), K = 6, 8, 16 objects, seg_blocks 2, 512 taps, a
table of 1 024 directions, EQ off, gain 1; every object of every stream takes a new (d0, d1, d2, w1, w2) in every segment, under
CROSSFADE.  Four legs, alternated round by round in one process:

  blended3  one ohs_scene3_process_blended3 call: ceil(K / 2) forward transforms per block (twice that in a fading block), six table
            rows per pass, ONE inverse
  composed  the same scene through SceneProcessor (libohs_scene.so) as 3 K objects:
            conv(u h0 + w1 h1 + w2 h2, x) = conv(h0, u x) + conv(h1, w1 x) + conv(h2, w2 x), every input channel three times
            (triplicated once, outside the timed region), gains u, w1, w2: 1.5 K forward transforms per block, every input read three
            times.  `--composed-lib PATH` loads that library from PATH -- the one built from the parent commit, for the record that
            is committed; without it, the tree's own (the same kernel source)
  blended2  the two-direction call of the same handle class on (d0, d1, w1): what the third direction costs
  plain     the three-direction entry with every weight +0.0 on the same d0: what blending costs over not blending

Call time per round as HIP events on a stream of the tool's own see it -- the events bracket process_ptr, so a figure holds the host's
row scan, the rows' conversion and the staging copy (the GPU idle meanwhile) as well as the kernel; tools/bench_objects_blend.py's
method.  `--warmup` untimed rounds first; median and min - max of `--rounds`.  blended3 and composed are compared once (relative RMS;
they differ by f32 rounding).  No ratio is a condition: the record says whether blended3's median is below composed's at each K, and
the exit status is 0 either way.

    python tools/bench_objects_blend3.py [--rounds 5] [--warmup 5] [--composed-lib PATH] [--out profiles/objects_blend3_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench_one(a, K):
    import numpy as np
    import torch
    import open_headstage_amd as ohs
    from open_headstage_amd import synth

    dev = torch.device("cuda:0")
    S, nb, seg, n_dirs = a.streams, a.blocks, a.seg_blocks, a.dirs
    frames = nb * 512
    n_segs = -(-nb // seg)
    base = synth.hrir_set(a.taps)
    dirs = np.zeros((n_dirs, 2, a.taps), np.float32)
    for d in range(n_dirs):
        for e in range(2):
            dirs[d, e] = np.roll(base[(2 * d + e) % 4], (5 * d + e) % 97) * np.float32((1.0 - 0.0005 * d) / K)
    # every object of every stream a new (d0, d1, d2, w1, w2) in every segment (bench_objects_blend.py's d0 and d1)
    s_, k_, c_ = np.meshgrid(np.arange(S), np.arange(n_segs), np.arange(K), indexing="ij")
    idx = ((131 * s_ + 17 * c_ + k_ * (1 + (s_ + c_) % 7)) % n_dirs).astype(np.uint32)
    idx1 = ((idx + 1 + (3 * k_ + c_) % 5) % n_dirs).astype(np.uint32)
    idx2 = ((idx + 7 + (2 * k_ + 3 * c_) % 11) % n_dirs).astype(np.uint32)
    w1 = ((1 + (5 * k_ + 3 * c_ + s_) % 61) / np.float32(128)).astype(np.float32)       # 1/128 .. 61/128, never 0
    w2 = ((1 + (7 * k_ + 5 * c_ + 3 * s_) % 43) / np.float32(128)).astype(np.float32)   # 1/128 .. 43/128, never 0
    assert (idx[:, 1:] != idx[:, :-1]).all() and (idx1 != idx).all() and (idx2 != idx).all() and (idx2 != idx1).all()
    assert (w1 > 0).all() and (w2 > 0).all() and (w1 + w2 < 1).all() and (w1[:, 1:] != w1[:, :-1]).all() and (w2[:, 1:] != w2[:, :-1]).all()
    zero = np.zeros_like(w1)
    # the 3 K composition's rows: channels 3 c, 3 c + 1, 3 c + 2 on d0, d1, d2 with gains u, w1, w2
    u = ((np.float32(1.0) - w1).astype(np.float32) - w2).astype(np.float32)
    idx3 = np.ascontiguousarray(np.stack([idx, idx1, idx2], -1).reshape(S, n_segs, 3 * K))
    gains3 = np.ascontiguousarray(np.stack([u, w1, w2], -1).reshape(S, n_segs, 3 * K))

    tri, two, plain = (ohs.TriSceneProcessor(S, num_bands=10) for _ in range(3))
    composed = ohs.SceneProcessor(S, num_bands=10)
    for h in (tri, two, plain, composed):
        h.set_directions(dirs)

    x = torch.empty((S, K, frames), dtype=torch.float32, device=dev)
    for c in range(K):
        x[:, c] = synth.white_noise_torch(1000 * c, S, frames, dev)[:, 0]
    x3 = x.repeat_interleave(3, dim=1).contiguous()        # (once, outside the timed region)
    y = {n: torch.empty((S, 2, frames), dtype=torch.float32, device=dev) for n in ("blended3", "composed", "blended2", "plain")}
    stream = torch.cuda.Stream(dev)
    hs = stream.cuda_stream

    def run_blended3():
        tri.process_ptr(x.data_ptr(), y["blended3"].data_ptr(), nb, K * frames, frames, 2 * frames, frames, K, seg, idx, None, None, None,
                        True, hs, idx1, w1, None, None, idx2, w2, None, None)

    def run_composed():
        composed.process_ptr(x3.data_ptr(), y["composed"].data_ptr(), nb, 3 * K * frames, frames, 2 * frames, frames, 3 * K, seg, idx3,
                             gains3, None, None, True, hs)

    def run_blended2():
        two.process_ptr(x.data_ptr(), y["blended2"].data_ptr(), nb, K * frames, frames, 2 * frames, frames, K, seg, idx, None, None, None,
                        True, hs, idx1, w1, None, None)

    def run_plain():
        plain.process_ptr(x.data_ptr(), y["plain"].data_ptr(), nb, K * frames, frames, 2 * frames, frames, K, seg, idx, None, None, None,
                          True, hs, idx1, zero, None, None, idx2, zero, None, None)

    legs = [("blended3", run_blended3), ("composed", run_composed), ("blended2", run_blended2), ("plain", run_plain)]
    ms = {n: [] for n, _ in legs}
    torch.cuda.synchronize(dev)     # (the inputs were filled on torch's own stream; `stream` does not wait for it by itself)
    with torch.cuda.stream(stream):
        for _ in range(a.warmup):
            for h in (tri, composed, two, plain):
                h.reset()
            for _, fn in legs:
                fn()
        stream.synchronize()
        d = y["blended3"].double() - y["composed"].double()
        rel = float(torch.sqrt((d * d).mean()) / torch.sqrt((y["composed"].double() ** 2).mean()))
        for _ in range(a.rounds):
            for n, fn in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                stream.synchronize()
                ms[n].append(e0.elapsed_time(e1))
    rec = {"objects": K, "pairs": (K + 1) // 2, "streams": S, "blocks": nb, "seg_blocks": seg, "taps": a.taps, "directions": n_dirs,
           "eq": 0, "rounds": a.rounds, "warmup": a.warmup, "blended3_launch": list(tri.last_launch()),
           "composed_launch": list(composed.last_launch()), "blended2_launch": list(two.last_launch()),
           "plain_launch": list(plain.last_launch()), "blended3_against_composed_relative_rms": rel}
    for n in ms:
        v = ms[n]
        rec[n] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                  "all_ms": [round(t, 4) for t in v]}
    rec["blended3_median_below_composed_median"] = rec["blended3"]["median_ms"] < rec["composed"]["median_ms"]
    for other in ("composed", "blended2", "plain"):
        rec[f"blended3_median_over_{other}_median"] = round(rec["blended3"]["median_ms"] / rec[other]["median_ms"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--seg-blocks", type=int, default=2)
    ap.add_argument("--taps", type=int, default=512)
    ap.add_argument("--dirs", type=int, default=1024)
    ap.add_argument("--objects", type=int, nargs="+", default=[6, 8, 16])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--composed-lib", default=None, help="libohs_scene.so of another build for the composed leg (the parent commit's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objects_blend3_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_objects_blend3.py needs a GPU")
    from open_headstage_amd import build, scene
    if a.composed_lib:
        if not os.path.exists(a.composed_lib):
            sys.exit(f"{a.composed_lib} not found")
        scene.SCENE_LIB_PATH = os.path.abspath(a.composed_lib)      # (read when the library is first loaded)
    res = build.resources()
    out = {"tool": "tools/bench_objects_blend3.py", "device": torch.cuda.get_device_name(0),
           "composed_library": "libohs_scene.so built from the parent commit" if a.composed_lib else "libohs_scene.so of this tree",
           "kernel_resources": {k: res.get(k, {}) for k in ("k_conv_p1_objects_blend3", "k_conv_p1_objects_blend", "k_conv_p1_objects")},
           "cases": []}
    for K in a.objects:
        rec = bench_one(a, K)
        out["cases"].append(rec)
        print(json.dumps(rec))
    out["blended3_median_below_composed_median_everywhere"] = all(c["blended3_median_below_composed_median"] for c in out["cases"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

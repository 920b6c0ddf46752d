#!/usr/bin/env python3
"""Prices the blended object-scene call (ohs_scene2_process_blended, libohs_scene2.so) against what libohs_scene.so offered for the
same scene, and against not blending.

Shape (tools/bench_objects.py's): 256 streams x 256 blocks (131 072 frames), K = 6, 8, 16 objects, seg_blocks 2, 512 taps, a table of
1 024 directions, EQ off, gain 1; every object of every stream takes a new (d0, d1, w) in every segment, under CROSSFADE.  Three legs,
alternated round by round in one process:

  blended   one ohs_scene2_process_blended call: ceil(K / 2) forward transforms per block (twice that in a fading block), four table
            rows per pass, ONE inverse
  composed  the same scene through the UNCHANGED SceneProcessor as 2 K objects: conv(u h0 + w h1, x) = conv(h0, u x) + conv(h1, w x),
            every input channel twice (duplicated once, outside the timed region), gains (1 - w) and w: K forward transforms per block,
            every input read twice, the same table rows
  plain     the blended entry at K with every weight +0.0 on the same d0: what blending costs over not blending

Call time per round as HIP events on a stream of the tool's own see it -- the events bracket process_ptr, so a figure holds the host's
row scan, the rows' conversion and the staging copy (the GPU idle meanwhile) as well as the kernel; tools/bench_objects.py's method.
blended and composed scan the same number of entries (4 K against 2 x 2 K per segment), so the comparison is a fair one; it is not
kernel time.  `--warmup` untimed rounds first (the first rounds of a leg run 15 - 40 % slow: clocks); median and min - max of `--rounds`.
blended and composed are compared once (relative RMS; they differ by f32 rounding).  The one condition: blended's median is no larger
than composed's, at every K (exit status 1 otherwise) -- no margin: blended does half of composed's forward transforms and reads half
the input.

    python tools/bench_objects_blend.py [--rounds 5] [--warmup 5] [--out profiles/objects_blend_bench.json]
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
    # every object of every stream a new (d0, d1, w) in every segment
    s_, k_, c_ = np.meshgrid(np.arange(S), np.arange(n_segs), np.arange(K), indexing="ij")
    idx = ((131 * s_ + 17 * c_ + k_ * (1 + (s_ + c_) % 7)) % n_dirs).astype(np.uint32)
    idx1 = ((idx + 1 + (3 * k_ + c_) % 5) % n_dirs).astype(np.uint32)
    w = ((1 + (5 * k_ + 3 * c_ + s_) % 61) / np.float32(64)).astype(np.float32)      # 1/64 .. 61/64, never 0
    assert (idx[:, 1:] != idx[:, :-1]).all() and (idx1 != idx).all() and (w > 0).all() and (w < 1).all()
    assert (w[:, 1:] != w[:, :-1]).all()
    zero = np.zeros_like(w)
    # the 2 K composition's rows: channel 2 c on d0 with gain 1 - w, channel 2 c + 1 on d1 with gain w
    idx2 = np.ascontiguousarray(np.stack([idx, idx1], -1).reshape(S, n_segs, 2 * K))
    gains2 = np.ascontiguousarray(np.stack([(np.float32(1.0) - w).astype(np.float32), w], -1).reshape(S, n_segs, 2 * K))

    blend = ohs.BlendSceneProcessor(S, num_bands=10)
    blend.set_directions(dirs)
    plain = ohs.BlendSceneProcessor(S, num_bands=10)
    plain.set_directions(dirs)
    composed = ohs.SceneProcessor(S, num_bands=10)
    composed.set_directions(dirs)

    x = torch.empty((S, K, frames), dtype=torch.float32, device=dev)
    for c in range(K):
        x[:, c] = synth.white_noise_torch(1000 * c, S, frames, dev)[:, 0]
    x2 = x.repeat_interleave(2, dim=1).contiguous()        # (once, outside the timed region)
    y = {n: torch.empty((S, 2, frames), dtype=torch.float32, device=dev) for n in ("blended", "composed", "plain")}
    stream = torch.cuda.Stream(dev)
    hs = stream.cuda_stream

    def run_blended():
        blend.process_ptr(x.data_ptr(), y["blended"].data_ptr(), nb, K * frames, frames, 2 * frames, frames, K, seg, idx, None, None, None,
                          True, hs, idx1, w, None, None)

    def run_composed():
        composed.process_ptr(x2.data_ptr(), y["composed"].data_ptr(), nb, 2 * K * frames, frames, 2 * frames, frames, 2 * K, seg, idx2,
                             gains2, None, None, True, hs)

    def run_plain():
        plain.process_ptr(x.data_ptr(), y["plain"].data_ptr(), nb, K * frames, frames, 2 * frames, frames, K, seg, idx, None, None, None,
                          True, hs, idx1, zero, None, None)

    legs = [("blended", run_blended), ("composed", run_composed), ("plain", run_plain)]
    ms = {n: [] for n, _ in legs}
    torch.cuda.synchronize(dev)     # (the inputs were filled on torch's own stream; `stream` does not wait for it by itself)
    with torch.cuda.stream(stream):
        for _ in range(a.warmup):
            for h in (blend, composed, plain):
                h.reset()
            for _, fn in legs:
                fn()
        stream.synchronize()
        d = y["blended"].double() - y["composed"].double()
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
           "eq": 0, "rounds": a.rounds, "warmup": a.warmup, "blended_launch": list(blend.last_launch()),
           "composed_launch": list(composed.last_launch()), "plain_launch": list(plain.last_launch()),
           "blended_against_composed_relative_rms": rel}
    for n in ms:
        v = ms[n]
        rec[n] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                  "all_ms": [round(t, 4) for t in v]}
    rec["blended_median_not_above_composed_median"] = rec["blended"]["median_ms"] <= rec["composed"]["median_ms"]
    rec["blended_median_over_composed_median"] = round(rec["blended"]["median_ms"] / rec["composed"]["median_ms"], 4)
    rec["blended_median_over_plain_median"] = round(rec["blended"]["median_ms"] / rec["plain"]["median_ms"], 4)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objects_blend_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_objects_blend.py needs a GPU")
    from open_headstage_amd import build
    res = build.resources()
    out = {"tool": "tools/bench_objects_blend.py", "device": torch.cuda.get_device_name(0),
           "kernel_resources": {k: res.get(k, {}) for k in ("k_conv_p1_objects_blend", "k_conv_p1_objects")}, "cases": []}
    for K in a.objects:
        rec = bench_one(a, K)
        out["cases"].append(rec)
        print(json.dumps(rec))
    out["blended_median_not_above_composed_median_everywhere"] = all(c["blended_median_not_above_composed_median"] for c in out["cases"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    sys.exit(0 if out["blended_median_not_above_composed_median_everywhere"] else 1)


if __name__ == "__main__":
    main()

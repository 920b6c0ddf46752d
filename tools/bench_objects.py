#!/usr/bin/env python3
"""Prices the object-scene call (ohs_scene_process, libohs_scene.so) against what the product library offered for the same mixdown.

Shape: 256 streams x 256 blocks (131 072 frames), K = 6, 8, 16 objects, seg_blocks 2, 512 taps, a table of 1 024 directions, EQ off,
gain 1; every object of every stream takes a new direction in every segment, under CROSSFADE.  Three legs, alternated round by round
in one process:

  scene     one ohs_scene_process call: ceil(K / 2) forward transforms per block (twice that in a fading block), ONE inverse
  composed  the same mixdown from existing calls: K handles with the directions as a K = 1 table of 1 024 sets, one
            ohs_batch_process_layout_scheduled per object on its channel of the same input tensor, each into its own
            [S][2][frames] slice of a scratch tensor, then K - 1 torch.add
  table     ohs_batch_process_layout_scheduled on a K-channel table of 64 sets that changes set in every segment: NOT the same
            mixdown (all channels switch together) but the same pass count -- it prices the on-the-fly combine of two direction
            rows against one precomputed (C, D) row

Device time per round by HIP events on a stream of the tool's own, after `--warmup` rounds; median and min - max of `--rounds`.
scene and composed are compared once (relative RMS; they differ by f32 rounding).  The one condition: scene's slowest round is
faster than composed's fastest, at every K (exit status 1 otherwise); the ratio to `table` is reported.

    python tools/bench_objects.py [--rounds 5] [--warmup 2] [--out profiles/objects_bench.json]
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
    S, nb, seg, n_dirs, n_sets = a.streams, a.blocks, a.seg_blocks, a.dirs, 64
    frames = nb * 512
    n_segs = -(-nb // seg)
    base = synth.hrir_set(a.taps)
    dirs = np.zeros((n_dirs, 2, a.taps), np.float32)
    for d in range(n_dirs):
        for e in range(2):
            dirs[d, e] = np.roll(base[(2 * d + e) % 4], (5 * d + e) % 97) * np.float32((1.0 - 0.0005 * d) / K)
    # every object of every stream a new direction in every segment
    s_, k_, c_ = np.meshgrid(np.arange(S), np.arange(n_segs), np.arange(K), indexing="ij")
    idx = ((131 * s_ + 17 * c_ + k_ * (1 + (s_ + c_) % 7)) % n_dirs).astype(np.uint32)
    assert (idx[:, 1:] != idx[:, :-1]).all()

    scene = ohs.SceneProcessor(S, num_bands=10)
    scene.set_directions(dirs)
    singles = []
    for c in range(K):
        h = ohs.BatchProcessor(S, num_bands=10)
        h.set_layout_table(dirs[:, None])           # [n_dirs][1][2][taps]
        singles.append(h)
    table = ohs.BatchProcessor(S, num_bands=10)
    table.set_layout_table(np.stack([dirs[(37 * j + 11 * np.arange(K)) % n_dirs] for j in range(n_sets)]))
    set_idx = ((7 * np.arange(S)[:, None] + np.arange(n_segs)[None, :] * (1 + np.arange(S)[:, None] % 5)) % n_sets).astype(np.uint32)
    assert (set_idx[:, 1:] != set_idx[:, :-1]).all()
    rows = [np.ascontiguousarray(idx[:, :, c]) for c in range(K)]

    x = torch.empty((S, K, frames), dtype=torch.float32, device=dev)
    for c in range(K):
        x[:, c] = synth.white_noise_torch(1000 * c, S, frames, dev)[:, 0]
    y = {n: torch.empty((S, 2, frames), dtype=torch.float32, device=dev) for n in ("scene", "composed", "table")}
    scratch = torch.empty((K, S, 2, frames), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(dev)
    hs = stream.cuda_stream

    def run_scene():
        scene.process_ptr(x.data_ptr(), y["scene"].data_ptr(), nb, K * frames, frames, 2 * frames, frames, K, seg, idx, None, None, None,
                          True, hs)

    def run_composed():
        for c, h in enumerate(singles):
            h.process_layout_scheduled_ptr(x.data_ptr() + 4 * c * frames, scratch[c].data_ptr(), nb, K * frames, frames, 2 * frames,
                                           frames, seg, rows[c], None, True, hs)
        torch.add(scratch[0], scratch[1], out=y["composed"])
        for c in range(2, K):
            y["composed"].add_(scratch[c])

    def run_table():
        table.process_layout_scheduled_ptr(x.data_ptr(), y["table"].data_ptr(), nb, K * frames, frames, 2 * frames, frames, seg, set_idx,
                                           None, True, hs)

    legs = [("scene", run_scene), ("composed", run_composed), ("table", run_table)]
    ms = {n: [] for n, _ in legs}
    torch.cuda.synchronize(dev)     # (the inputs were filled on torch's own stream; `stream` does not wait for it by itself)
    with torch.cuda.stream(stream):
        for _ in range(a.warmup):
            for h in [scene, table] + singles:
                h.reset()
            for _, fn in legs:
                fn()
        stream.synchronize()
        d = y["scene"].double() - y["composed"].double()
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
           "table_sets": n_sets, "eq": 0, "rounds": a.rounds, "warmup": a.warmup, "scene_launch": list(scene.last_launch()),
           "table_launch": list(table.last_layout_launch()), "scene_against_composed_relative_rms": rel}
    for n in ms:
        v = ms[n]
        rec[n] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                  "all_ms": [round(t, 4) for t in v]}
    rec["scene_slowest_below_composed_fastest"] = rec["scene"]["max_ms"] < rec["composed"]["min_ms"]
    rec["composed_median_over_scene_median"] = round(rec["composed"]["median_ms"] / rec["scene"]["median_ms"], 4)
    rec["scene_median_over_table_median"] = round(rec["scene"]["median_ms"] / rec["table"]["median_ms"], 4)
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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objects_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_objects.py needs a GPU")
    from open_headstage_amd import build
    res = build.resources().get("k_conv_p1_objects", {})
    out = {"tool": "tools/bench_objects.py", "device": torch.cuda.get_device_name(0), "kernel_resources": res, "cases": []}
    for K in a.objects:
        rec = bench_one(a, K)
        out["cases"].append(rec)
        print(json.dumps(rec))
    out["scene_slowest_below_composed_fastest_everywhere"] = all(c["scene_slowest_below_composed_fastest"] for c in out["cases"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    sys.exit(0 if out["scene_slowest_below_composed_fastest_everywhere"] else 1)


if __name__ == "__main__":
    main()

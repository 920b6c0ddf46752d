#!/usr/bin/env python3
"""Prices the object-distance stage (libohs_delay.so, ohs_delay_process) against two references measured in the same session:

  copy      a device-to-device copy of the same tensor on the same stream -- the floor: the stage moves the same bytes
  tracked   ohs_tracked_process on the stage's output, the call the stage feeds (it does not change it)

Shape: the tracked benchmark's -- 256 streams x 256 blocks, seg_blocks 2 -> 128 segments, K = 6, 8, 16 objects, every object moving in
every segment: each object's distance walks by up to 0.7 m per segment (33 m/s) between 1 and 55 m, rows per stream and segment
(`--shared-rows`: one row for all streams).  The three legs alternate inside every round; `--warmup` untimed rounds first, then the
median and min - max of `--rounds`, on the host's clock around call + sync; `held` is how long the caller's thread was held by the
call itself.  Every round carries the round before it.  No ratio is a condition: the tool reports.

    python tools/bench_delay.py [--rounds 20] [--warmup 3] [--out profiles/delay_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def bench_one(a, K):
    import numpy as np
    import torch
    import open_headstage_amd as ohs
    from open_headstage_amd import lookup, lookup3, synth

    dev = torch.device("cuda:0")
    S, nb, seg = a.streams, a.blocks, a.seg_blocks
    n_segs, frames = -(-nb // seg), nb * 512
    rng = np.random.default_rng(2000 + K)
    row_S = 1 if a.shared_rows else S
    # distances: a bounded walk, every object somewhere else at the end of every segment
    r = rng.uniform(1.0, 55.0, (row_S, 1, K)) + np.cumsum(rng.uniform(-0.7, 0.7, (row_S, n_segs, K)), 1)
    r = 1.0 + np.abs(np.abs(r - 1.0) % 108.0 - 54.0)                      # folded into 1 .. 55 m
    pos, tri = lookup3.octahedron_mesh(a.level)
    T = lookup.table_xyz(pos).astype(np.float64)
    direction = T[rng.integers(len(T), size=(n_segs, K))] + 0.05 * rng.standard_normal((n_segs, K, 3))
    direction /= np.linalg.norm(direction, axis=-1, keepdims=True)
    src = direction[None] * r[..., None] if not a.shared_rows else direction * r[0][..., None]
    delay, gain = ohs.distance_rows(src)
    assert delay.max() <= a.max_delay and delay.min() >= 1.0
    delay, gain = np.ascontiguousarray(delay.reshape(row_S, n_segs, K)), np.ascontiguousarray(gain.reshape(row_S, n_segs, K))
    yaw = np.cumsum(rng.uniform(-4, 4, (S, n_segs)), 1).astype(np.float32)
    R = np.ascontiguousarray(lookup.pose_matrices(yaw, rng.uniform(-20, 20, (S, n_segs)).astype(np.float32),
                                                  rng.uniform(-10, 10, (S, n_segs)).astype(np.float32)))
    dirs = (rng.standard_normal((len(pos), 2, a.taps)) * (0.05 / K)).astype(np.float32)

    dl = ohs.ObjectDelay(S, K, a.max_delay)
    tr = ohs.TrackedSceneProcessor(S, pos, tri, num_bands=10)
    tr.set_directions(dirs)
    x = torch.empty((S, K, frames), dtype=torch.float32, device=dev)
    for c in range(K):
        x[:, c] = synth.white_noise_torch(1000 * c, S, frames, dev)[:, 0]
    between, copied = torch.empty_like(x), torch.empty_like(x)
    y = torch.empty((S, 2, frames), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    geometry = (nb, K * frames, frames)
    v = np.ascontiguousarray(direction)                                     # the tracked call: sources shared by the streams

    def stage():
        t0 = time.perf_counter()
        dl.process_ptr(x.data_ptr(), between.data_ptr(), *geometry, K * frames, frames, K, seg, delay, gain, 0 if a.shared_rows else n_segs,
                       None, stream.cuda_stream)
        t1 = time.perf_counter()
        dl.sync(stream.cuda_stream)
        return t1 - t0, time.perf_counter() - t0

    def copy():
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            copied.copy_(x, non_blocking=True)
        t1 = time.perf_counter()
        stream.synchronize()
        return t1 - t0, time.perf_counter() - t0

    def tracked():
        t0 = time.perf_counter()
        tr.process_ptr(between.data_ptr(), y.data_ptr(), *geometry, 2 * frames, frames, K, seg, v, 0, 1, R, n_segs, None, True, None,
                       stream.cuda_stream)
        t1 = time.perf_counter()
        tr.sync(stream.cuda_stream)
        return t1 - t0, time.perf_counter() - t0

    legs = {"stage": stage, "copy": copy, "tracked": tracked}
    total, held = {name: [] for name in legs}, {name: [] for name in legs}
    for i in range(a.warmup + a.rounds):
        for name, fn in legs.items():
            h, t = fn()
            if i >= a.warmup:
                held[name].append(1e3 * h)
                total[name].append(1e3 * t)
    torch.cuda.synchronize(dev)
    tile, window, lds, gather = dl.last_launch()
    moved = 2 * x.numel() * 4
    rec = {"objects": K, "streams": S, "blocks": nb, "segments": n_segs, "max_delay": a.max_delay, "rows_per_stream": not a.shared_rows,
           "delay_frames": {"min": round(float(delay.min()), 1), "max": round(float(delay.max()), 1),
                            "largest_step_per_segment": round(float(np.abs(np.diff(delay, axis=1)).max()), 1)},
           "rounds": a.rounds, "warmup": a.warmup, "bytes_in_plus_out": moved,
           **{name: dict(_stats(total[name]), held=_stats(held[name])) for name in legs},
           "tiles": {"frames": tile, "lds_window": window, "lds": lds, "gather": gather, "lds_share": round(lds / max(1, lds + gather), 6)},
           "finite": bool(torch.isfinite(between).all()) and bool(torch.isfinite(y).all())}
    rec["stage_over_copy"] = round(rec["stage"]["median_ms"] / rec["copy"]["median_ms"], 4)
    rec["stage_over_tracked"] = round(rec["stage"]["median_ms"] / rec["tracked"]["median_ms"], 4)
    rec["stage_TB_per_s"] = round(moved / (rec["stage"]["median_ms"] * 1e-3) / 1e12, 3)
    rec["copy_TB_per_s"] = round(moved / (rec["copy"]["median_ms"] * 1e-3) / 1e12, 3)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--seg-blocks", type=int, default=2)
    ap.add_argument("--taps", type=int, default=512)
    ap.add_argument("--level", type=int, default=4, help="subdivisions of the octahedron mesh the tracked call looks up (4: 2 048 triangles)")
    ap.add_argument("--max-delay", type=int, default=8192)
    ap.add_argument("--objects", type=int, nargs="+", default=[6, 8, 16])
    ap.add_argument("--shared-rows", action="store_true", help="one row of delays and gains for all streams")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delay_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_delay.py needs a GPU")
    from open_headstage_amd import build
    res = build.resources()
    out = {"tool": "tools/bench_delay.py", "device": torch.cuda.get_device_name(0),
           "kernel_resources": {k: res.get(k, {}) for k in ("k_object_delay", "k_delay_history")}, "cases": []}
    for K in a.objects:
        rec = bench_one(a, K)
        out["cases"].append(rec)
        print(json.dumps(rec), flush=True)
    fmt = lambda s: f"{s['median_ms']:.2f} ({s['min_ms']:.2f} - {s['max_ms']:.2f})"       # noqa: E731
    print("| K | stage, call + sync, ms | copy, ms | tracked call, ms | stage / copy | stage / tracked | thread held: stage, ms | tiles staged in LDS |")
    print("|---|---|---|---|---|---|---|---|")
    for r in out["cases"]:
        print(f"| {r['objects']} | {fmt(r['stage'])} | {fmt(r['copy'])} | {fmt(r['tracked'])} | {r['stage_over_copy']:.2f} | "
              f"{r['stage_over_tracked']:.2f} | {fmt(r['stage']['held'])} | {100.0 * r['tiles']['lds_share']:.2f} % |", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

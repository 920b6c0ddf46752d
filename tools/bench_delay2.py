#!/usr/bin/env python3
"""Prices the filtered object-distance stage (libohs_delay2.so) against what it replaces and against its floor, all measured in the same
session on the same tensors:

  old        ObjectDelay.process_ptr: libohs_delay.so, the stage without a filter
  plain      FilteredObjectDelay.process_ptr with no taps: ohs_delay2_process, the same work through the new library
  filtered   the same call with taps: ohs_delay2_process_filtered, every row filtered
  copy       a device-to-device copy of the same tensor on the same stream

Shape: tools/bench_delay.py's -- 256 streams x 256 blocks, seg_blocks 2 -> 128 segments, K = 6, 8, 16 objects, every object moving in
every segment: each object's distance walks by up to 0.7 m per segment between 1 and 55 m, rows per stream and segment; the taps are
air_absorption_taps of those distances, so every row takes the filtered pass.  The four legs alternate inside every round;
`--warmup` untimed rounds first, then the median and min - max of `--rounds`, on the host's clock around call + sync; `held` is how long
the caller's thread was held by the call itself.  Every round carries the round before it.

Two bars, both relative to this session's own figures and recorded, not enforced:
  plain within the old stage's run-to-run spread of the old stage:     |plain - old| <= max(old) - min(old)
  filtered below the old stage plus one copy -- an unfused filter pass would have to move the tensor once more, so that sum is the
  least it could cost:                                                 filtered < old + copy

    python tools/bench_delay2.py [--rounds 20] [--warmup 3] [--out profiles/delay2_bench.json]
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
    from open_headstage_amd import synth

    dev = torch.device("cuda:0")
    S, nb, seg = a.streams, a.blocks, a.seg_blocks
    n_segs, frames = -(-nb // seg), nb * 512
    rng = np.random.default_rng(2000 + K)
    # distances: a bounded walk, every object somewhere else at the end of every segment (tools/bench_delay.py's)
    r = rng.uniform(1.0, 55.0, (S, 1, K)) + np.cumsum(rng.uniform(-0.7, 0.7, (S, n_segs, K)), 1)
    r = 1.0 + np.abs(np.abs(r - 1.0) % 108.0 - 54.0)                      # folded into 1 .. 55 m
    delay = np.ascontiguousarray(np.maximum(1.0, r * (48000.0 / 343.0)))
    gain = np.ascontiguousarray((1.0 / r).astype(np.float32))
    taps = ohs.air_absorption_taps(r)
    assert delay.max() <= a.max_delay and delay.min() >= 5.0 and taps.shape == (S, n_segs, K, 5)
    identity_rows = int((taps.reshape(-1, 5) == np.array([1, 0, 0, 0, 0], np.float32)).all(1).sum())

    old = ohs.ObjectDelay(S, K, a.max_delay)
    plain = ohs.FilteredObjectDelay(S, K, a.max_delay)
    filt = ohs.FilteredObjectDelay(S, K, a.max_delay)
    x = torch.empty((S, K, frames), dtype=torch.float32, device=dev)
    for c in range(K):
        x[:, c] = synth.white_noise_torch(1000 * c, S, frames, dev)[:, 0]
    out, copied = torch.empty_like(x), torch.empty_like(x)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    geometry = (nb, K * frames, frames, K * frames, frames, K, seg)

    def stage(handle, fir):
        def run():
            t0 = time.perf_counter()
            if fir is None:
                handle.process_ptr(x.data_ptr(), out.data_ptr(), *geometry, delay, gain, n_segs, None, stream.cuda_stream)
            else:
                handle.process_ptr(x.data_ptr(), out.data_ptr(), *geometry, delay, gain, n_segs, None, stream.cuda_stream, fir=fir)
            t1 = time.perf_counter()
            handle.sync(stream.cuda_stream)
            return t1 - t0, time.perf_counter() - t0
        return run

    def copy():
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            copied.copy_(x, non_blocking=True)
        t1 = time.perf_counter()
        stream.synchronize()
        return t1 - t0, time.perf_counter() - t0

    legs = {"old": stage(old, None), "plain": stage(plain, None), "filtered": stage(filt, taps), "copy": copy}
    total, held = {name: [] for name in legs}, {name: [] for name in legs}
    for i in range(a.warmup + a.rounds):
        for name, fn in legs.items():
            h, t = fn()
            if i >= a.warmup:
                held[name].append(1e3 * h)
                total[name].append(1e3 * t)
    torch.cuda.synchronize(dev)
    finite = bool(torch.isfinite(out).all())
    tile, window, lds, gather, filtered_tiles = filt.last_launch()
    p_tile, p_window, p_lds, p_gather, p_filtered = plain.last_launch()
    moved = 2 * x.numel() * 4
    rec = {"objects": K, "streams": S, "blocks": nb, "segments": n_segs, "max_delay": a.max_delay, "rows_per_stream": True,
           "distance_m": {"min": round(float(r.min()), 2), "max": round(float(r.max()), 2)}, "identity_rows": identity_rows,
           "rounds": a.rounds, "warmup": a.warmup, "bytes_in_plus_out": moved,
           **{name: dict(_stats(total[name]), held=_stats(held[name])) for name in legs},
           "tiles": {"frames": tile, "lds_window": window, "lds": lds, "gather": gather, "filtered": filtered_tiles,
                     "plain_call": {"lds": p_lds, "gather": p_gather, "filtered": p_filtered}},
           "finite": finite}
    med = {name: rec[name]["median_ms"] for name in legs}
    spread = rec["old"]["max_ms"] - rec["old"]["min_ms"]
    rec["plain_over_old"] = round(med["plain"] / med["old"], 4)
    rec["filtered_over_old"] = round(med["filtered"] / med["old"], 4)
    rec["filtered_over_old_plus_copy"] = round(med["filtered"] / (med["old"] + med["copy"]), 4)
    rec["old_over_copy"] = round(med["old"] / med["copy"], 4)
    rec["filtered_over_copy"] = round(med["filtered"] / med["copy"], 4)
    rec["old_spread_ms"] = round(spread, 4)
    rec["bars"] = {"plain_within_old_spread": bool(abs(med["plain"] - med["old"]) <= spread),
                   "filtered_below_old_plus_copy": bool(med["filtered"] < med["old"] + med["copy"])}
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--seg-blocks", type=int, default=2)
    ap.add_argument("--max-delay", type=int, default=8192)
    ap.add_argument("--objects", type=int, nargs="+", default=[6, 8, 16])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delay2_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_delay2.py needs a GPU")
    from open_headstage_amd import build
    res = build.resources()
    out = {"tool": "tools/bench_delay2.py", "device": torch.cuda.get_device_name(0),
           "kernel_resources": {k: res.get(k, {}) for k in ("k_object_delay", "k_object_delay2", "k_delay2_history")}, "cases": []}
    for K in a.objects:
        rec = bench_one(a, K)
        out["cases"].append(rec)
        print(json.dumps(rec), flush=True)
    fmt = lambda s: f"{s['median_ms']:.2f} ({s['min_ms']:.2f} - {s['max_ms']:.2f})"       # noqa: E731
    print("| K | old stage, ms | plain, ms | filtered, ms | copy, ms | plain / old | filtered / old | filtered / (old + copy) | thread held: old / filtered, ms |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in out["cases"]:
        print(f"| {r['objects']} | {fmt(r['old'])} | {fmt(r['plain'])} | {fmt(r['filtered'])} | {fmt(r['copy'])} | {r['plain_over_old']:.3f} | "
              f"{r['filtered_over_old']:.3f} | {r['filtered_over_old_plus_copy']:.3f} | {r['old']['held']['median_ms']:.2f} / "
              f"{r['filtered']['held']['median_ms']:.2f} |", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Prices SessionRenderer.render against a serial loop over the same chunks, host memory to host memory.

Shape: the one of profiles/layout_sched_bench.json -- 256 streams, 5.1 (6 channels), 72 sets of 512 taps, every stream a row of
its own with a new set every two blocks, 938 blocks (480 256 frames), crossfade on, EQ off -- cut into chunks of 64 blocks.  If the
pinned staging buffers cannot be had for 256 streams, the stream count is halved until they can, and recorded.

Two forms, alternating run by run in one process, `--runs` (5) timed runs each after one untimed run of both:

  serial     the same chunks through existing entry points, each step waiting for the one before: host copy into a pinned buffer,
             copy in, BatchProcessor.process_layout_scheduled_ptr, copy out, host copy into the result
  pipelined  SessionRenderer.render on the numpy array

Both write every frame of a preallocated result; the two results are compared bit for bit once.  Wall time by perf_counter around
the blocking call.  Criterion: the pipelined form's SLOWEST run is faster than the serial form's FASTEST.

Also recorded, without a threshold: Msamples/s (stream-frames per second, as bench.py counts them), bytes over the link per second
each way, the ratio of their sum to twice `pcie_inclusive`'s GB/s each way in the latest BENCH_*.json, and the device-only time of
the one-shot call on device-resident audio (HIP events, as tools/bench_layout.py --scheduled measures it; that tool's figure from
profiles/layout_sched_bench.json beside it).

    python tools/bench_session.py [--out profiles/session_bench.json]
"""
import argparse
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _find(o, key):
    """the first value under `key` anywhere in a decoded JSON document"""
    if isinstance(o, dict):
        if key in o:
            return o[key]
        o = list(o.values())
    if isinstance(o, list):
        for v in o:
            r = _find(v, key)
            if r is not None:
                return r
    return None


def _pcie_inclusive():
    """(file, GB/s each way) of the BENCH_*.json record with the highest run number `n` whose result line has the figure"""
    best = (None, None, -1)
    for f in glob.glob(os.path.join(ROOT, "BENCH_*.json")):
        try:
            rec = json.load(open(f))
            lines = [l for l in rec["run"]["stdout_tail"].splitlines() if l.startswith("{")]
            fig = _find(json.loads(lines[-1]), "pcie_inclusive")
            if isinstance(fig, dict) and "GBps_each_way" in fig and int(rec["n"]) > best[2]:
                best = (os.path.basename(f), float(fig["GBps_each_way"]), int(rec["n"]))
        except (OSError, KeyError, IndexError, TypeError, ValueError):
            continue
    return best[0], best[1]


def _sched_bench_figure():
    try:
        d = json.load(open(os.path.join(ROOT, "profiles", "layout_sched_bench.json")))
        return next(r["sched_xf"]["median_ms"] for r in d["results"] if r["name"] == "5.1")
    except (OSError, KeyError, StopIteration, ValueError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=938)
    ap.add_argument("--taps", type=int, default=512)
    ap.add_argument("--sets", type=int, default=72)
    ap.add_argument("--seg-blocks", type=int, default=2)
    ap.add_argument("--chunk-blocks", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    from open_headstage_amd.session import call_rows, plan_calls

    K, nb, seg, n_sets, chunk = 6, a.blocks, a.seg_blocks, a.sets, a.chunk_blocks
    assert nb % seg == 0, "the session is one render() call that is not final"
    frames = nb * 512
    n_segs = nb // seg
    base = synth.hrir_set(a.taps)
    table = np.zeros((n_sets, K, 2, a.taps), np.float32)
    for j in range(n_sets):
        for c in range(K):
            for e in range(2):
                table[j, c, e] = np.roll(base[(2 * c + e + j) % 4], (5 * c + e + 3 * j) % 23) * np.float32(1.0 - 0.02 * c)
        table[j] /= np.abs(table[j]).sum(axis=(0, 2), keepdims=True)
    grid = np.arange(n_sets) * (360.0 / n_sets) - 180.0

    S, r, requested = a.streams, None, a.streams
    while r is None:
        try:
            r = ohs.SessionRenderer.layout(S, table, grid, seg_blocks=seg, chunk_blocks=chunk)
            h_in = torch.empty(S * K * chunk * 512, dtype=torch.float32, pin_memory=True)
            h_out = torch.empty(S * 2 * chunk * 512, dtype=torch.float32, pin_memory=True)
        except RuntimeError as e:
            print(f"{S} streams: {e}; halving", file=sys.stderr)
            r = None
            S //= 2
            assert S >= 1
    idx = np.zeros((S, n_segs), np.uint32)
    for s in range(S):
        idx[s] = (7 * s + np.arange(n_segs) * (1 + s % 5)) % n_sets
    assert (idx[:, 1:] != idx[:, :-1]).all()

    rng = np.random.default_rng(1)
    x = rng.random((S, K, frames), dtype=np.float32)
    x -= np.float32(0.5)
    xt = torch.from_numpy(x)
    y_serial = np.zeros((S, 2, frames), np.float32)
    y_pipe = np.zeros((S, 2, frames), np.float32)
    yt = torch.from_numpy(y_serial)

    dev = torch.device("cuda:0")
    ref = ohs.BatchProcessor(S, num_bands=10)
    ref.set_layout_table(table)
    d_in = torch.empty(S * K * chunk * 512, dtype=torch.float32, device=dev)
    d_out = torch.empty(S * 2 * chunk * 512, dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(dev)
    calls = list(plan_calls(0, nb, seg, chunk))

    def serial():
        ref.reset()
        with torch.cuda.stream(stream):
            for start, n, g, _ in calls:
                nf, f0 = n * 512, start * 512
                hi, ho = h_in[:S * K * nf].view(S, K, nf), h_out[:S * 2 * nf].view(S, 2, nf)
                di, do = d_in[:S * K * nf].view(S, K, nf), d_out[:S * 2 * nf].view(S, 2, nf)
                hi.copy_(xt[:, :, f0:f0 + nf])
                di.copy_(hi, non_blocking=True)
                stream.synchronize()
                ref.process_layout_scheduled_ptr(di.data_ptr(), do.data_ptr(), n, K * nf, nf, 2 * nf, nf, g,
                                                 call_rows(idx, 0, start, n, g, seg),
                                                 None if start == 0 else np.ascontiguousarray(idx[:, (start - 1) // seg]), True,
                                                 stream.cuda_stream)
                stream.synchronize()
                ho.copy_(do, non_blocking=True)
                stream.synchronize()
                yt[:, :, f0:f0 + nf].copy_(ho)

    def pipelined():
        r.reset()
        r.render(x, rows=idx, out=y_pipe)

    forms = [("serial", serial), ("pipelined", pipelined)]
    for _, fn in forms:
        fn()
    same_bits = bool((y_serial.view(np.uint32) == y_pipe.view(np.uint32)).all()) and float(np.abs(y_pipe).max()) > 0.01
    sec = {n: [] for n, _ in forms}
    for _ in range(a.runs):
        for n, fn in forms:
            t0 = time.perf_counter()
            fn()
            sec[n].append(time.perf_counter() - t0)

    # the one-shot call on device-resident audio: device time by HIP events
    one_shot = None
    try:
        dx = torch.empty((S, K, frames), dtype=torch.float32, device=dev)
        for s0 in range(0, S, 32):
            dx[s0:s0 + 32].copy_(xt[s0:s0 + 32])
        dy = torch.empty((S, 2, frames), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        ms = []
        with torch.cuda.stream(stream):
            for rep in range(6):
                ref.reset()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                ref.process_layout_scheduled_ptr(dx.data_ptr(), dy.data_ptr(), nb, K * frames, frames, 2 * frames, frames, seg, idx, None,
                                                 True, stream.cuda_stream)
                e1.record(stream)
                stream.synchronize()
                if rep >= 2:
                    ms.append(e0.elapsed_time(e1))
        one_shot = {"median_ms": round(statistics.median(ms), 4), "all_ms": [round(t, 4) for t in ms],
                    "same_bits_as_the_session": bool((dy.cpu().numpy().view(np.uint32) == y_pipe.view(np.uint32)).all())}
    except RuntimeError as e:
        one_shot = {"error": str(e)}

    bench_file, gbps = _pcie_inclusive()
    rec = {"shape": {"streams": S, "streams_requested": requested, "channels": K, "sets": n_sets, "taps": a.taps, "seg_blocks": seg,
                     "blocks": nb, "frames": frames, "chunk_blocks": chunk, "calls": len(calls), "crossfade": 1, "eq": 0},
           "pinned_bytes_of_the_renderer": 2 * 4 * (S * K + S * 2) * chunk * 512,
           "device_bytes_of_the_renderer": 2 * 4 * (S * K + S * 2) * chunk * 512,
           "torch_threads": torch.get_num_threads(), "runs": a.runs, "serial_and_pipelined_same_bits": same_bits}
    for n in sec:
        v = sec[n]
        rec[n] = {"median_s": round(statistics.median(v), 4), "min_s": round(min(v), 4), "max_s": round(max(v), 4),
                  "all_s": [round(t, 4) for t in v]}
    rec["pipelined_max_below_serial_min"] = rec["pipelined"]["max_s"] < rec["serial"]["min_s"]
    rec["pipelined_median_over_serial_median"] = round(rec["pipelined"]["median_s"] / rec["serial"]["median_s"], 4)
    t = statistics.median(sec["pipelined"])
    rec["Msamples_s"] = round(S * frames / t / 1e6, 1)
    rec["link_GBps_in"] = round(4 * S * K * frames / t / 1e9, 3)
    rec["link_GBps_out"] = round(4 * S * 2 * frames / t / 1e9, 3)
    rec["pcie_inclusive"] = {"file": bench_file, "GBps_each_way": gbps,
                             "both_ways_over_twice_that": None if not gbps else
                             round((rec["link_GBps_in"] + rec["link_GBps_out"]) / (2 * gbps), 4),
                             "in_over_that": None if not gbps else round(rec["link_GBps_in"] / gbps, 4)}
    rec["one_shot_device_only"] = one_shot
    rec["one_shot_device_only_ms_in_layout_sched_bench"] = _sched_bench_figure()
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    return 0 if rec["pipelined_max_below_serial_min"] and same_bits else 1


if __name__ == "__main__":
    sys.exit(main())

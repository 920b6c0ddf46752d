#!/usr/bin/env python3
"""Prices ohs_batch_process_layout against the route the stereo entry points offer for the same mixdown.

Shape: 256 streams x 938 blocks (480 256 frames), 512 taps, EQ off, gain 1; the layouts 5.1 (6 channels, 3 pairs) and 7.1
(8 channels, 4 pairs).  Two routes, alternated repetition by repetition in one process:

  layout    one ohs_batch_process_layout call: [S][K][frames] -> [S][2][frames]
  composed  ceil(K / 2) handles, each loaded with one pair's four responses (Lsl, Lsr = channel 2 p to both ears, Rsl, Rsr =
            channel 2 p + 1); one ohs_batch_process per handle at the library's own plan choice, out of place, reading its pair
            of channels out of the same input tensor and writing a [S][2][frames] slice of a scratch tensor; then a torch sum of
            the slices

Device time per repetition by HIP events on a stream of the tool's own, after `--warmup` repetitions of both routes; median and
min - max of `--reps` repetitions.  The two routes' outputs are compared once (relative RMS; they differ by f32 rounding).

    python tools/bench_layout.py [--reps 12] [--warmup 3] [--out profiles/layout_bench.json]

--scheduled prices ohs_batch_process_layout_scheduled instead (head-tracked layouts: 72 sets, seg_blocks 2, every stream a row of
its own with a new set in every segment), four routes alternating in one process:

  sched_xf   one ohs_batch_process_layout_scheduled call, OHS_LAYOUT_SWITCH_CROSSFADE
  composed   what the library offered before: ceil(K / 2) handles, each holding one pair's four responses of every set as its
             set table, one ohs_batch_process_ir_crossfaded per handle at the same rows, then a torch sum
  sched_ro   the same call under OHS_LAYOUT_SWITCH_RING_OUT
  plain      ohs_batch_process_layout on set 0 (no schedule): what the walk through the table and the fades cost on top

    python tools/bench_layout.py --scheduled [--out profiles/layout_sched_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench_one(a, name, K):
    import numpy as np
    import torch
    import open_headstage_amd as ohs
    from open_headstage_amd import synth

    dev = torch.device("cuda:0")
    S, nb = a.streams, a.blocks
    frames = nb * 512
    P = (K + 1) // 2
    # K x 2 responses: synth's set, moved and scaled per channel -- all different, L1-normalised per ear over the layout
    base = synth.hrir_set(a.taps)
    irs = np.zeros((K, 2, a.taps), np.float32)
    for c in range(K):
        for e in range(2):
            irs[c, e] = np.roll(base[(2 * c + e) % 4], (5 * c + e) % 23) * np.float32(1.0 - 0.02 * c)
    irs /= np.abs(irs).sum(axis=(0, 2), keepdims=True)

    lay = ohs.BatchProcessor(S, num_bands=10)
    lay.set_layout_irs(irs)
    pairs = []
    for p in range(P):
        h = ohs.BatchProcessor(S, num_bands=10)
        zero = np.zeros(a.taps, np.float32)
        odd = 2 * p + 1 >= K
        for path, r in enumerate([irs[2 * p, 0], irs[2 * p, 1], zero if odd else irs[2 * p + 1, 0], zero if odd else irs[2 * p + 1, 1]]):
            h.set_ir(path, r)
        pairs.append(h)

    Kp = 2 * P
    x = torch.empty((S, Kp, frames), dtype=torch.float32, device=dev)
    for c in range(Kp):
        x[:, c] = synth.white_noise_torch(1000 * c, S, frames, dev)[:, 0] if c < K else 0.0
    y_lay = torch.empty((S, 2, frames), dtype=torch.float32, device=dev)
    scratch = torch.empty((S, Kp, frames), dtype=torch.float32, device=dev)
    y_cmp = torch.empty((S, 2, frames), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(dev)
    hs = stream.cuda_stream

    def layout():
        lay.process_layout_ptr(x.data_ptr(), y_lay.data_ptr(), nb, Kp * frames, frames, 2 * frames, frames, hs)

    def composed():
        for p, h in enumerate(pairs):
            off = 4 * 2 * p * frames
            h.process_ptr(x.data_ptr() + off, scratch.data_ptr() + off, nb, Kp * frames, frames, hs)
        torch.add(scratch[:, 0:2], scratch[:, 2:4], out=y_cmp)
        for p in range(2, P):
            y_cmp.add_(scratch[:, 2 * p:2 * p + 2])

    routes = [("layout", layout), ("composed", composed)]
    ms = {n: [] for n, _ in routes}
    torch.cuda.synchronize(dev)     # (the inputs were filled on torch's own stream; `stream` does not wait for it by itself)
    with torch.cuda.stream(stream):
        for _ in range(a.warmup):
            for _, fn in routes:
                fn()
        stream.synchronize()
        d = (y_lay.double() - y_cmp.double())
        rel = float(torch.sqrt((d * d).mean()) / torch.sqrt((y_cmp.double() ** 2).mean()))
        for _ in range(a.reps):
            for n, fn in routes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                stream.synchronize()
                ms[n].append(e0.elapsed_time(e1))
    rec = {"name": name, "channels": K, "pairs": P, "streams": S, "blocks": nb, "taps": a.taps, "eq": 0, "reps": a.reps,
           "warmup": a.warmup, "layout_launch": list(lay.last_layout_launch()),
           "composed_plans": [list(h.last_conv_plan()) for h in pairs], "routes_relative_rms": rel}
    for n in ms:
        v = ms[n]
        rec[n] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                  "all_ms": [round(t, 4) for t in v]}
    rec["layout_median_over_composed_min"] = round(rec["layout"]["median_ms"] / rec["composed"]["min_ms"], 4)
    rec["layout_median_over_composed_median"] = round(rec["layout"]["median_ms"] / rec["composed"]["median_ms"], 4)
    rec["layout_median_below_composed_min"] = rec["layout"]["median_ms"] < rec["composed"]["min_ms"]
    return rec


def bench_scheduled(a, name, K):
    import numpy as np
    import torch
    import open_headstage_amd as ohs
    from open_headstage_amd import synth

    dev = torch.device("cuda:0")
    S, nb, seg, n_sets = a.streams, a.blocks, a.seg_blocks, a.sets
    frames = nb * 512
    P = (K + 1) // 2
    n_segs = -(-nb // seg)
    base = synth.hrir_set(a.taps)
    table = np.zeros((n_sets, K, 2, a.taps), np.float32)
    for j in range(n_sets):
        for c in range(K):
            for e in range(2):
                table[j, c, e] = np.roll(base[(2 * c + e + j) % 4], (5 * c + e + 3 * j) % 23) * np.float32(1.0 - 0.02 * c)
        table[j] /= np.abs(table[j]).sum(axis=(0, 2), keepdims=True)
    # every stream its own row, a new set in every segment
    idx = np.zeros((S, n_segs), np.uint32)
    for s in range(S):
        idx[s] = (7 * s + np.arange(n_segs) * (1 + s % 5)) % n_sets
    assert (idx[:, 1:] != idx[:, :-1]).all()

    sched = ohs.BatchProcessor(S, num_bands=10)
    sched.set_layout_table(table)
    plain = ohs.BatchProcessor(S, num_bands=10)
    plain.set_layout_irs(table[0])
    pairs = []
    zero = np.zeros((n_sets, a.taps), np.float32)
    for p in range(P):
        h = ohs.BatchProcessor(S, num_bands=10)
        odd = 2 * p + 1 >= K
        h.set_schedule_irs(np.stack([table[:, 2 * p, 0], table[:, 2 * p, 1], zero if odd else table[:, 2 * p + 1, 0],
                                     zero if odd else table[:, 2 * p + 1, 1]], axis=1))
        pairs.append(h)

    Kp = 2 * P
    x = torch.empty((S, Kp, frames), dtype=torch.float32, device=dev)
    for c in range(Kp):
        x[:, c] = synth.white_noise_torch(1000 * c, S, frames, dev)[:, 0] if c < K else 0.0
    y = {n: torch.empty((S, 2, frames), dtype=torch.float32, device=dev) for n in ("sched_xf", "composed", "sched_ro", "plain")}
    scratch = torch.empty((S, Kp, frames), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(dev)
    hs = stream.cuda_stream

    def sched_call(fade, out):
        sched.process_layout_scheduled_ptr(x.data_ptr(), out.data_ptr(), nb, Kp * frames, frames, 2 * frames, frames, seg, idx, None,
                                           fade, hs)

    def composed():
        for p, h in enumerate(pairs):
            off = 4 * 2 * p * frames
            h.process_ir_crossfaded_ptr(x.data_ptr() + off, scratch.data_ptr() + off, nb, Kp * frames, frames, seg, idx, None, hs)
        if P == 1:
            y["composed"].copy_(scratch[:, 0:2])
        else:
            torch.add(scratch[:, 0:2], scratch[:, 2:4], out=y["composed"])
        for p in range(2, P):
            y["composed"].add_(scratch[:, 2 * p:2 * p + 2])

    routes = [("sched_xf", lambda: sched_call(True, y["sched_xf"])), ("composed", composed),
              ("sched_ro", lambda: sched_call(False, y["sched_ro"])),
              ("plain", lambda: plain.process_layout_ptr(x.data_ptr(), y["plain"].data_ptr(), nb, Kp * frames, frames, 2 * frames,
                                                         frames, hs))]
    ms = {n: [] for n, _ in routes}
    launches = {}
    torch.cuda.synchronize(dev)     # (the inputs were filled on torch's own stream; `stream` does not wait for it by itself)
    with torch.cuda.stream(stream):
        for _ in range(a.warmup):
            for n, fn in routes:
                fn()
                if n.startswith("sched"):
                    launches[n] = [int(sched.last_layout_scheduled())] + list(sched.last_layout_launch())
        stream.synchronize()
        d = (y["sched_xf"].double() - y["composed"].double())
        rel = float(torch.sqrt((d * d).mean()) / torch.sqrt((y["composed"].double() ** 2).mean()))
        for _ in range(a.reps):
            for n, fn in routes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                stream.synchronize()
                ms[n].append(e0.elapsed_time(e1))
    rec = {"name": name, "channels": K, "pairs": P, "streams": S, "blocks": nb, "taps": a.taps, "eq": 0, "sets": n_sets,
           "seg_blocks": seg, "reps": a.reps, "warmup": a.warmup, "scheduled_and_launch": launches,
           "plain_launch": list(plain.last_layout_launch()), "sched_xf_vs_composed_relative_rms": rel}
    for n in ms:
        v = ms[n]
        rec[n] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                  "all_ms": [round(t, 4) for t in v]}
    rec["sched_xf_median_over_composed_min"] = round(rec["sched_xf"]["median_ms"] / rec["composed"]["min_ms"], 4)
    rec["sched_xf_median_below_composed_min"] = rec["sched_xf"]["median_ms"] < rec["composed"]["min_ms"]
    rec["sched_xf_median_over_plain_median"] = round(rec["sched_xf"]["median_ms"] / rec["plain"]["median_ms"], 4)
    rec["sched_ro_median_over_plain_median"] = round(rec["sched_ro"]["median_ms"] / rec["plain"]["median_ms"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=938)          # 480 256 frames
    ap.add_argument("--taps", type=int, default=512)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layouts", type=str, default="5.1,7.1")
    ap.add_argument("--tag", type=str, default="")
    ap.add_argument("--scheduled", action="store_true")         # ohs_batch_process_layout_scheduled and its routes
    ap.add_argument("--sets", type=int, default=72)
    ap.add_argument("--seg-blocks", type=int, default=2)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    assert a.reps >= 1 and a.warmup >= 1
    sys.path.insert(0, ROOT)
    from open_headstage_amd import build
    known = {"5.1": 6, "7.1": 8}
    kernel = "k_conv_p1_layout_irs" if a.scheduled else "k_conv_p1_layout"
    res = build.resources().get(kernel, {})
    out = {"tag": a.tag, "kernel": {"name": kernel, **res}, "results": []}
    for name in a.layouts.split(","):
        rec = (bench_scheduled if a.scheduled else bench_one)(a, name, known[name] if name in known else int(name))
        print(json.dumps(rec), flush=True)
        out["results"].append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Prices ohs_batch_process_ir_scheduled at the headline's shape: 256 streams x 480 256 frames per step, 4 x 512 taps,
seg_blocks = 2 with a DIFFERENT set of impulse responses in every segment, out of a table of 72 sets.  Variants, alternated
round by round in one session:

  plain    one ohs_batch_process of the same frames (the handle's one set): what the schedule costs on top of
  shared   one ohs_batch_process_ir_scheduled, one row of set indices for all streams
  streams  the same with a row per stream (every stream its own pseudo-random walk through the table)
  xf_shared, xf_streams   ohs_batch_process_ir_crossfaded on the same rows: the first block of every segment fades from the
           previous segment's set (prev_idx: the row's last entry, so the call's first block fades too)
  loop     the per-segment call loop the new call replaces: four ohs_batch_set_ir and one 2-block ohs_batch_process per
           segment -- one set for all streams, the tail cut at every change (--loop-steps of them per round; 0 leaves it out)

--eq 1 runs the ten-band EQ in front (the headline), --eq 0 the convolution alone.  --mode ring_out | cut.
Device time per step by HIP events around `--steps` back-to-back steps on a stream of the tool's own, after a warm-up of every
variant.  Prints one JSON line per round and a summary (median, min, max per variant, the ratios of the medians).

    python tools/bench_ir_scheduled.py [--eq 1] [--rounds 5] [--steps 5] [--out profiles/NAME.jsonl]

--package-root DIR imports open_headstage_amd from another checkout (the parent commit's tree with its own build): `plain` and
`loop` only, the entry points that exist there -- for the plain headline of both builds alternating in one session, and for the
loop as the parent commit runs it.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=938)          # 480 256 frames
    ap.add_argument("--taps", type=int, default=512)
    ap.add_argument("--seg-blocks", type=int, default=2)
    ap.add_argument("--sets", type=int, default=72)
    ap.add_argument("--eq", type=int, default=1)
    ap.add_argument("--mode", type=str, default="ring_out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--loop-steps", type=int, default=1)
    ap.add_argument("--only", type=str, default="", help="comma-separated variants to run (default: all there are)")
    ap.add_argument("--package-root", type=str, default="")
    ap.add_argument("--tag", type=str, default="")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root) if a.package_root else ROOT)
    import numpy as np
    import torch
    import open_headstage_amd as ohs
    from open_headstage_amd import synth

    dev = torch.device("cuda:0")
    S, nb, sb = a.streams, a.blocks, a.seg_blocks
    n_segs = -(-nb // sb)
    # the table: synth's set, every set with its direct taps moved and its noise part scaled -- all different
    base = synth.hrir_set(a.taps)
    sets = np.zeros((a.sets, 4, a.taps), np.float32)
    for i in range(a.sets):
        for p in range(4):
            sets[i, p] = np.roll(base[p], i % 17) * np.float32(1.0 - 0.003 * i)
    idx = (np.arange(n_segs) * 7 % a.sets).astype(np.uint32)
    assert a.sets < 2 or np.all(idx[1:] != idx[:-1])
    rng = np.random.default_rng(8)
    idx_s = np.zeros((S, n_segs), np.uint32)
    idx_s[:, 0] = rng.integers(0, a.sets, S)
    for k in range(1, n_segs):          # (a new set in every segment of every stream)
        idx_s[:, k] = (idx_s[:, k - 1] + rng.integers(1, max(a.sets, 2), S)) % a.sets
    assert a.sets < 2 or np.all(idx_s[:, 1:] != idx_s[:, :-1])

    bands = synth.eq_table()
    bp = ohs.BatchProcessor(S, num_bands=len(bands))
    for p in range(4):
        bp.set_ir(p, sets[0][p])
    for i, b in enumerate(bands):
        bp.update_band_coeffs(i, synth.FS, b)
    bp.set_eq_enabled(bool(a.eq))
    new_api = hasattr(bp, "process_ir_scheduled")
    xf_api = hasattr(bp, "process_ir_crossfaded")
    if new_api:
        bp.set_schedule_irs(sets)
    x = synth.white_noise_torch(0, S, nb * 512, dev)
    y = torch.empty_like(x)
    stream = torch.cuda.Stream(dev)
    hs = stream.cuda_stream

    def plain():
        bp.process(x, out=y, hip_stream=hs)

    def shared():
        bp.process_ir_scheduled(x, sb, idx, a.mode, out=y, hip_stream=hs)

    def streams():
        bp.process_ir_scheduled(x, sb, idx_s, a.mode, out=y, hip_stream=hs)

    def xf_shared():
        bp.process_ir_crossfaded(x, sb, idx, int(idx[-1]), out=y, hip_stream=hs)

    def xf_streams():
        bp.process_ir_crossfaded(x, sb, idx_s, idx_s[:, -1], out=y, hip_stream=hs)

    def loop():
        f = sb * 512
        for k in range(n_segs):
            for p in range(4):
                bp.set_ir(p, sets[idx[k]][p])
            b0, b1 = k * f, min((k + 1) * f, nb * 512)
            bp.process_ptr(x.data_ptr() + 4 * b0, y.data_ptr() + 4 * b0, (b1 - b0) // 512, 2 * nb * 512, nb * 512, hs)

    variants = [("plain", plain, a.steps)]
    if new_api:
        variants += [("shared", shared, a.steps), ("streams", streams, a.steps)]
    if xf_api:
        variants += [("xf_shared", xf_shared, a.steps), ("xf_streams", xf_streams, a.steps)]
    if a.loop_steps > 0:
        variants.append(("loop", loop, a.loop_steps))
    if a.only:
        keep = set(a.only.split(","))
        variants = [v for v in variants if v[0] in keep]
    with torch.cuda.stream(stream):
        for name, fn, _ in variants:       # warm-up: every shape the timed windows use, every staging slot grown
            for _ in range(1 if name == "loop" else 5):
                fn()
        stream.synchronize()
        forms = {}
        for name, fn, _ in variants:
            if name == "loop":
                continue
            fn(); stream.synchronize()
            forms[name] = list(bp.last_conv_plan()) + ([bp.last_conv_ir_scheduled()] if new_api else []) + \
                ([bp.last_conv_ir_crossfaded()] if xf_api else [])
        if any(v[0] == "loop" for v in variants):       # (the loop leaves another set loaded: plain runs on set 0 again)
            for p in range(4):
                bp.set_ir(p, sets[0][p])
        ms = {name: [] for name, _, _ in variants}
        lines = []
        for r in range(a.rounds):
            rec = {"round": r}
            for name, fn, steps in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                stream.synchronize()
                e0.record(stream)
                t0 = time.perf_counter()
                for _ in range(steps):
                    fn()
                e1.record(stream)
                stream.synchronize()
                t_wall = (time.perf_counter() - t0) * 1e3 / steps
                t = e0.elapsed_time(e1) / steps
                ms[name].append(t)
                rec[name + "_ms_per_step"] = round(t, 4)
                rec[name + "_wall_ms_per_step"] = round(t_wall, 4)
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    frames = S * nb * 512
    summ = {"tag": a.tag, "shape": {"streams": S, "blocks": nb, "taps": a.taps, "eq": int(bool(a.eq)), "seg_blocks": sb, "segments": n_segs,
                                    "sets": a.sets, "mode": a.mode}, "forms": forms}
    for name in ms:
        v = ms[name]
        med = statistics.median(v)
        summ[name] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                      "msamples_per_s": round(frames / med / 1e3, 1)}
    if "plain" in ms:
        for name in ("shared", "streams", "xf_shared", "xf_streams"):
            if name in ms:
                summ[name + "_over_plain"] = round(summ[name]["median_ms"] / summ["plain"]["median_ms"], 4)
    for name, base in (("xf_shared", "shared"), ("xf_streams", "streams"), ("xf_shared", "streams")):
        if name in ms and base in ms:
            summ[name + "_over_" + base] = round(summ[name]["median_ms"] / summ[base]["median_ms"], 4)
    if "loop" in ms:
        for name in ("shared", "streams", "xf_shared", "xf_streams"):
            if name in ms:
                summ["loop_over_" + name] = round(summ["loop"]["median_ms"] / summ[name]["median_ms"], 2)
        summ["loop_us_per_segment"] = round(summ["loop"]["median_ms"] * 1e3 / n_segs, 2)
    print(json.dumps(summ), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for rec in lines + [summ]:
                f.write(json.dumps(dict(rec, tag=a.tag)) + "\n")


if __name__ == "__main__":
    main()

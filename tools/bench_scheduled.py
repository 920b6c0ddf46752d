#!/usr/bin/env python3
"""Prices ohs_batch_process_scheduled at the headline's shape: 256 streams x 480 256 frames per step, 4 x 512 taps, ten bands,
seg_blocks = 2 with a DIFFERENT table index and gain in every segment -- the reference's cadence, all bands and the master
gain refreshed once per 1 024-frame host block.  Three variants, alternated round by round in one session:

  plain      one ohs_batch_process of the same frames (one table, one gain): what the schedule costs on top of
  scheduled  one ohs_batch_process_scheduled
  loop       the per-segment call loop the scheduled call replaces: ten ohs_batch_set_eq_band_coeffs, one ohs_batch_set_gain
             and one 2-block ohs_batch_process per segment (--loop-steps of them per round; 0 leaves it out)

Device time per step by HIP events around `--steps` back-to-back steps on a stream of the tool's own, after a warm-up of every
variant.  Prints one JSON line per round and a summary (median, min, max per variant, the ratios of the medians).

    python tools/bench_scheduled.py [--rounds 5] [--steps 5] [--out profiles/NAME.jsonl]

--per-stream prices ohs_batch_process_scheduled_streams instead: every stream its own pseudo-random index row over the pool of
tables (one set of flags) and its own gain row, a new table and gain in every segment of every stream.  The yardstick is
`scheduled` (ohs_batch_process_scheduled, one row for all) on the same handle and buffers, alternating with the new call round
by round; `stage` is the larger staging copy alone (streams x segments x 8 bytes, pinned host memory to the device), the margin
the new call is allowed on top of the yardstick's own spread.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import open_headstage_amd as ohs  # noqa: E402
from open_headstage_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=938)          # 480 256 frames
    ap.add_argument("--taps", type=int, default=512)
    ap.add_argument("--seg-blocks", type=int, default=2)
    ap.add_argument("--tables", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--loop-steps", type=int, default=2)
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--per-stream", action="store_true", help="ohs_batch_process_scheduled_streams against ohs_batch_process_scheduled")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    S, nb, sb = a.streams, a.blocks, a.seg_blocks
    n_segs = -(-nb // sb)
    bands = synth.eq_table()
    coeffs = np.zeros((a.tables, len(bands), 5), np.float32)
    for t in range(a.tables):
        for i, b in enumerate(bands):
            coeffs[t, i] = ohs.biquad_coefficients(b.filter_type, synth.FS, b.center_freq * (1.0 + 0.004 * t), b.q, b.gain_db - 0.05 * t)
    en = np.ones((a.tables, len(bands)), bool)
    idx = (np.arange(n_segs) * 7 % a.tables).astype(np.uint32)
    assert a.tables < 2 or np.all(idx[1:] != idx[:-1])
    gains = (0.5 + 0.4 * np.sin(np.arange(n_segs) * 0.013) + 1e-4 * np.arange(n_segs)).astype(np.float32)
    assert np.all(gains[1:] != gains[:-1])

    bp = ohs.BatchProcessor(S, num_bands=len(bands))
    irs = synth.hrir_set(a.taps)
    for p in range(4):
        bp.set_ir(p, irs[p])
    bp.set_eq_enabled(True)
    bp.set_schedule_tables(coeffs, en)
    x = synth.white_noise_torch(0, S, nb * 512, dev)
    y = torch.empty_like(x)
    stream = torch.cuda.Stream(dev)
    hs = stream.cuda_stream

    def plain():
        bp.process(x, out=y, hip_stream=hs)

    def scheduled():
        bp.process_scheduled(x, sb, idx, gains, out=y, hip_stream=hs)

    def loop():
        f = sb * 512
        for k in range(n_segs):
            for i in range(len(bands)):
                bp.set_band_coeffs(i, coeffs[idx[k], i], True)
            bp.set_gain(float(gains[k]))
            b0, b1 = k * f, min((k + 1) * f, nb * 512)
            bp.process_ptr(x.data_ptr() + 4 * b0, y.data_ptr() + 4 * b0, (b1 - b0) // 512, 2 * nb * 512, nb * 512, hs)

    # --per-stream: a row per stream; stream s starts elsewhere in the pool and walks it with its own odd step
    rng = np.random.default_rng(8)
    idx_s = np.zeros((S, n_segs), np.uint32)
    idx_s[:, 0] = rng.integers(0, a.tables, S)
    for k in range(1, n_segs):          # (a new table in every segment of every stream)
        idx_s[:, k] = (idx_s[:, k - 1] + rng.integers(1, max(a.tables, 2), S)) % a.tables
    assert a.tables < 2 or np.all(idx_s[:, 1:] != idx_s[:, :-1])
    gains_s = (gains[None, :] * (1.0 + 0.001 * np.arange(S)[:, None])).astype(np.float32)
    assert np.all(gains_s[:, 1:] != gains_s[:, :-1])
    pinned = torch.empty(2 * S * n_segs, dtype=torch.int32).pin_memory()
    staged = torch.empty(2 * S * n_segs, dtype=torch.int32, device=dev)

    def streams():
        bp.process_scheduled_streams(x, sb, idx_s, gains_s, out=y, hip_stream=hs)

    def stage():
        staged.copy_(pinned, non_blocking=True)

    variants = [("plain", plain, a.steps), ("scheduled", scheduled, a.steps)]
    if a.per_stream:
        variants += [("streams", streams, a.steps), ("stage", stage, a.steps)]
    elif a.loop_steps > 0:
        variants.append(("loop", loop, a.loop_steps))
    with torch.cuda.stream(stream):
        for _, fn, _ in variants:       # warm-up: every shape the timed windows use, every staging slot of the scheduled calls grown
            for _ in range(5):
                fn()
        stream.synchronize()
        forms = {}
        plain(); stream.synchronize(); forms["plain"] = list(bp.last_eq_form()) + list(bp.last_conv_plan())
        scheduled(); stream.synchronize(); forms["scheduled"] = list(bp.last_eq_form()) + list(bp.last_conv_plan())
        if a.per_stream:
            streams(); stream.synchronize(); forms["streams"] = list(bp.last_eq_form()) + list(bp.last_conv_plan())
        prep = {}
        if a.per_stream:        # host time of ONE call on an idle stream (no staging slot to wait for): the device idles that long
            for name, fn in (("scheduled", scheduled), ("streams", streams)):
                v = []
                for _ in range(5):
                    stream.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    v.append((time.perf_counter() - t0) * 1e3)
                prep[name] = round(statistics.median(v), 4)
            stream.synchronize()
        ms = {name: [] for name, _, _ in variants}
        lines = []
        for r in range(a.rounds):
            rec = {"round": r}
            for name, fn, steps in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                t0 = time.perf_counter()
                for _ in range(steps):
                    fn()
                t_host = (time.perf_counter() - t0) * 1e3 / steps
                e1.record(stream)
                stream.synchronize()
                t = e0.elapsed_time(e1) / steps
                ms[name].append(t)
                rec[name + "_ms_per_step"] = round(t, 4)
                if a.per_stream:        # (host time until the call returns: the device idles for the first call's share of it)
                    rec[name + "_host_ms_per_call"] = round(t_host, 4)
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    frames = S * nb * 512
    summ = {"shape": {"streams": S, "blocks": nb, "taps": a.taps, "bands": len(bands), "seg_blocks": sb, "segments": n_segs,
                      "tables": a.tables}, "forms": forms}
    for name in ms:
        v = ms[name]
        med = statistics.median(v)
        summ[name] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                      "msamples_per_s": round(frames / med / 1e3, 1)}
    summ["scheduled_over_plain"] = round(summ["scheduled"]["median_ms"] / summ["plain"]["median_ms"], 4)
    if "loop" in ms:
        summ["loop_over_scheduled"] = round(summ["loop"]["median_ms"] / summ["scheduled"]["median_ms"], 3)
        summ["loop_us_per_call"] = round(summ["loop"]["median_ms"] * 1e3 / n_segs, 2)
    if prep:
        summ["host_ms_per_call_on_an_idle_stream"] = prep
    if "streams" in ms:
        summ["streams_over_scheduled"] = round(summ["streams"]["median_ms"] / summ["scheduled"]["median_ms"], 4)
        summ["margin_ms"] = round(summ["scheduled"]["max_ms"] - summ["scheduled"]["min_ms"] + summ["stage"]["median_ms"], 4)
        summ["streams_minus_scheduled_ms"] = round(summ["streams"]["median_ms"] - summ["scheduled"]["median_ms"], 4)
    summ["scheduled_extra_us_per_boundary"] = round((summ["scheduled"]["median_ms"] - summ["plain"]["median_ms"]) * 1e3 / max(n_segs - 1, 1), 4)
    print(json.dumps(summ), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines + [summ]:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

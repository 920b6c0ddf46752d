#!/usr/bin/env python3
"""Prices short batch calls on long impulse responses: BASELINE config-4 shape -- 64 streams,
4 x 16 384 taps -- driven with calls of 1, 2, 3, 4, 8, 32 and 256 blocks of 512 frames.  Device time per call by HIP
events around a run of back-to-back calls on one stream (so launch gaps between a call's kernels count, host
enqueue time does not unless it is the bound), and host wall time per call beside it.  One JSON line per call size.

    python tools/bench_short_calls.py [--streams 64] [--taps 16384] [--plan 0]

--eq: the reference's cadence through the existing setters -- ten bands on, and in front of EVERY call a changed table (ten
ohs_batch_set_eq_band_coeffs) and a changed gain (ohs_batch_set_gain), as a host that refreshes per block does.  The per-segment
call loop ohs_batch_process_scheduled replaces; `--streams 256 --taps 512 --sizes 2 --eq` is the headline's shape.

--stream-eq: the same cadence with every stream on a table of its own -- streams x ten ohs_batch_set_stream_eq_band_coeffs and
one ohs_batch_set_gain in front of EVERY call: the per-host-block loop ohs_batch_process_scheduled_streams replaces (one gain
per call is all this loop can do: the handle has no gain per stream).  The setters are host work and the next launch uploads
the tables synchronously, so the figure to read is wall_us_per_call.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import open_headstage_amd as ohs  # noqa: E402
from open_headstage_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--taps", type=int, default=16384)
    ap.add_argument("--plan", type=int, default=0)
    ap.add_argument("--sizes", type=str, default="1,2,3,4,8,32,256")
    ap.add_argument("--eq", action="store_true", help="ten bands on; a changed table and gain in front of every call")
    ap.add_argument("--stream-eq", action="store_true", help="as --eq, with streams x ten per-stream setters in front of every call")
    ap.add_argument("--max-calls", type=int, default=400)
    a = ap.parse_args()
    a.eq = a.eq or a.stream_eq
    dev = torch.device("cuda:0")
    S = a.streams
    bp = ohs.BatchProcessor(S, num_bands=10)
    irs = synth.hrir_set(a.taps)
    for p in range(4):
        bp.set_ir(p, irs[p])
    bp.set_eq_enabled(a.eq)
    bp.set_conv_plan(a.plan)
    tables = []
    if a.eq:        # six ten-band tables whose coefficients all differ
        bands = synth.eq_table()
        for t in range(6):
            tables.append([ohs.biquad_coefficients(b.filter_type, synth.FS, b.center_freq * (1.0 + 0.01 * t), b.q, b.gain_db - 0.1 * t)
                           for b in bands])
        for i, c in enumerate(tables[0]):
            bp.set_band_coeffs(i, c, True)
    turn = [0]

    def call(xs, ys):
        if a.eq:
            turn[0] += 1
            if a.stream_eq:
                for s in range(S):
                    for i, c in enumerate(tables[(turn[0] + s) % 6]):
                        bp.set_stream_band_coeffs(s, i, c, True)
            else:
                for i, c in enumerate(tables[turn[0] % 6]):
                    bp.set_band_coeffs(i, c, True)
            bp.set_gain(0.5 + 0.01 * (turn[0] % 32))
        bp.process(xs, out=ys)
    frames_total = 256 * 512
    x = synth.white_noise_torch(0, S, frames_total, dev)
    y = torch.empty_like(x)
    # a long call first: every path is then older than its own impulse response (the steady state of a running job)
    bp.process(x, out=y)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream(dev)
    steady = None
    for nb in [int(v) for v in a.sizes.split(",")]:
        n = nb * 512
        calls = max(8, min(a.max_calls, 4096 // nb))
        xs = x[:, :, :n].contiguous()
        ys = torch.empty_like(xs)
        for _ in range(3):
            call(xs, ys)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(st)
        for _ in range(calls):
            call(xs, ys)
        e1.record(st)
        t_host = time.perf_counter() - t0
        torch.cuda.synchronize()
        t_wall = time.perf_counter() - t0
        dev_us = e0.elapsed_time(e1) * 1e3 / calls
        rec = {"streams": S, "taps": a.taps, "plan": a.plan, "eq": bool(a.eq), "stream_eq": bool(a.stream_eq), "blocks_per_call": nb, "calls": calls,
               "msamples_per_s": round(S * n / dev_us, 1),
               "device_us_per_call": round(dev_us, 2), "host_enqueue_us_per_call": round(t_host * 1e6 / calls, 2),
               "wall_us_per_call": round(t_wall * 1e6 / calls, 2),
               "us_per_block": round(dev_us / nb, 3)}
        if nb == 256:
            steady = dev_us
        print(json.dumps(rec), flush=True)
    if steady:
        print(json.dumps({"steady_256_block_call_us": round(steady, 2), "per_2_blocks_us": round(steady / 128, 3),
                          "target_3x_us": round(3 * steady / 128, 3)}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cycles and shader clock inside k_eq_ring (experiment build: OHS_BUILD_TAG=eqstamps OHS_EXTRA_DEFS=-DOHS_EQ_STAMPS): s_memtime
(shader clock) against s_memrealtime (100 MHz) over every wave of EVERY EQ launch of one steady-state headline step, with
and without the convolution running beside it, for the quad ring's loops: the library's (one merged store per group; in a
library from before round 17 the one below), round 15's with store, store, load in one cluster per group
(Tuning::eq_quad_cluster_port), round 12's with the port's memory instructions each alone in its slot
(Tuning::eq_quad_lone_port; the only loop of a library from before round 15, "v_nop" there) and that one with the fill
instruction (Tuning::eq_quad_fill).  Per launch: shader-clock ticks per sample (independent of the clock), the clock, and how far the
slowest wave ends behind the median one (a launch ends with its slowest wave); per step the line through the six launches'
median ticks over their samples: slope = the loop's ticks per sample, intercept = a launch's fixed ticks.
    OHS_LIB=open_headstage_amd/libohs_hip_eqstamps.so python tools/eq_clock.py [--json FILE] [streams ...]"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import open_headstage_amd as ohs  # noqa: E402
from open_headstage_amd import _ffi, synth  # noqa: E402

FRAMES = 480256
RECORDS = 16384
dev = torch.device("cuda:0")
L = _ffi.lib()
L.ohs_debug_eq_stamps.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_uint)]
L.ohs_debug_eq_stamps_reset.argtypes = []
L.ohs_debug_set_tuning.argtypes = [C.c_char_p, C.c_char_p]


def launches(st):
    """records [k][6] = (wave, n, rt0, rt1, ck0, ck1) -> one array per launch: the launches of a stream follow one another, so
    a wave that starts behind every end seen so far opens the next one"""
    st = st[np.argsort(st[:, 2], kind="stable")]
    out, lo, end = [], 0, st[0, 3]
    for i in range(1, len(st)):
        if st[i, 2] >= end:
            out.append(st[lo:i])
            lo = i
        end = max(end, st[i, 3])
    out.append(st[lo:])
    return out


HAS_LONE = L.ohs_debug_set_tuning(b"eq_quad_lone_port", b"0") == 0
HAS_CLUSTER = L.ohs_debug_set_tuning(b"eq_quad_cluster_port", b"0") == 0
LOOPS = ("merged", "cluster", "lone", "fill") if HAS_CLUSTER else ("cluster", "lone", "fill") if HAS_LONE else ("v_nop", "fill")
if os.environ.get("EQ_CLOCK_LOOPS"):        # a subset, in this order
    LOOPS = tuple(l for l in os.environ["EQ_CLOCK_LOOPS"].split(",") if l in LOOPS)


def run(S, conv_on, loop, sink):
    assert L.ohs_debug_set_tuning(b"eq_quad_fill", str(int(loop == "fill")).encode()) == 0
    if HAS_LONE:
        assert L.ohs_debug_set_tuning(b"eq_quad_lone_port", str(int(loop == "lone")).encode()) == 0
    if HAS_CLUSTER:
        assert L.ohs_debug_set_tuning(b"eq_quad_cluster_port", str(int(loop == "cluster")).encode()) == 0
    bp = ohs.BatchProcessor(S, num_bands=10)
    irs = synth.hrir_set(512)
    for p in range(4):
        bp.set_ir(p, irs[p] if conv_on else irs[p][:0])
    for i, b in enumerate(synth.eq_table()):
        bp.update_band_coeffs(i, synth.FS, b)
    bp.set_eq_enabled(True)
    x = synth.white_noise_torch(0, S, FRAMES, dev)
    y = torch.empty_like(x)
    for _ in range(4):
        bp.process(x, out=y)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(4):
        bp.process(x, out=y)
    b.record()
    torch.cuda.synchronize()
    assert L.ohs_debug_eq_stamps_reset() == 0
    bp.process(x, out=y)            # the step that is read
    torch.cuda.synchronize()
    buf, count = (C.c_ulonglong * (6 * RECORDS))(), C.c_uint(0)
    assert L.ohs_debug_eq_stamps(buf, RECORDS, C.byref(count)) == 0
    assert 0 < count.value <= RECORDS, count.value
    st = np.frombuffer(buf, dtype=np.uint64).reshape(RECORDS, 6)[:count.value].astype(np.int64)
    st = st[st[:, 0] < 2 * S]       # (waves behind the last chain leave at once)
    print(f"streams {S}, loop {loop}, convolution {'on' if conv_on else 'muted (empty IRs: general path, no P = 1 kernel)'}: "
          f"{a.elapsed_time(b) / 4:.3f} ms per step, {count.value} wave records", flush=True)
    t0 = st[:, 2].min()
    fit = []
    for k, l in enumerate(launches(st)):
        n = int(l[0, 1])
        ticks = (l[:, 5] - l[:, 4]) / n
        ghz = (l[:, 5] - l[:, 4]) / ((l[:, 3] - l[:, 2]) * 10.0)
        life = (l[:, 3] - l[:, 2]) / 100.0
        end = (l[:, 3] - t0) / 100.0
        rec = {"streams": S, "loop": loop, "conv_on": bool(conv_on), "launch": k, "samples": n, "waves": len(l),
               "start_us": round(float((l[:, 2].min() - t0) / 100.0), 1), "span_us": round(float(end.max() - (l[:, 2].min() - t0) / 100.0), 1),
               "ticks_per_sample": [round(float(v), 3) for v in (np.median(ticks), ticks.min(), ticks.max())],
               "ghz": [round(float(v), 4) for v in (np.median(ghz), ghz.min(), ghz.max())],
               "life_us": [round(float(v), 1) for v in (np.median(life), life.min(), life.max())],
               "last_end_behind_median_us": round(float(end.max() - np.median(end)), 1),
               "end_spread_us": round(float(end.max() - end.min()), 1)}
        sink.append(rec)
        fit.append((n, float(np.median(l[:, 5] - l[:, 4]))))
        print(f"  launch {k}: {n:7d} samples, {len(l):4d} waves, start {rec['start_us']:8.1f} us, span {rec['span_us']:7.1f} us; "
              f"ticks per sample median {rec['ticks_per_sample'][0]:.3f} (min {rec['ticks_per_sample'][1]:.3f}, max "
              f"{rec['ticks_per_sample'][2]:.3f}); clock {rec['ghz'][0]:.3f} GHz (min {rec['ghz'][1]:.3f}, max {rec['ghz'][2]:.3f}); "
              f"last wave ends {rec['last_end_behind_median_us']:.1f} us behind the median one, ends spread over {rec['end_spread_us']:.1f} us",
              flush=True)
    if len(fit) >= 2:
        slope, icpt = np.polyfit([f[0] for f in fit], [f[1] for f in fit], 1)
        sink.append({"streams": S, "loop": loop, "conv_on": bool(conv_on), "fit_ticks_per_sample": round(float(slope), 3),
                     "fit_ticks_per_launch": round(float(icpt))})
        print(f"  fit over {len(fit)} launches: {slope:.3f} ticks per sample + {icpt:.0f} ticks per launch", flush=True)
    del bp, x, y
    torch.cuda.empty_cache()


if __name__ == "__main__":
    args = sys.argv[1:]
    out = None
    if "--json" in args:
        i = args.index("--json")
        out = args[i + 1]
        del args[i:i + 2]
    sink = []
    for S in [int(a) for a in args] or [256]:
        for conv_on in (True, False):
            for loop in LOOPS:
                run(S, conv_on, loop, sink)
    if out:
        with open(out, "w") as f:
            for r in sink:
                f.write(json.dumps(r) + "\n")

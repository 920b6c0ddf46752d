#!/usr/bin/env python3
"""Prices the direction lookup (libohs_lookup.so) against the numpy helpers it stands in for and against the scene call it feeds.

Shape (tools/bench_objects_blend.py's): 256 streams x 256 blocks, seg_blocks 2 -> 128 segments, K = 6, 8, 16 objects, a table of 1 024
directions; and K = 16 on a table of 65 536.  Sources move from segment to segment and are shared by the streams ([segs][K]); every
stream has a head pose of its own per segment ([streams][segs]: yaw, pitch, roll).  Per case:

  rows      DirectionLookup.rows' C call (ohs_lookup_rows) on the packed sources and matrices, nearest only and bracketed
  points    ohs_lookup_points on the same head-relative queries, computed on the host beforehand, nearest only and bracketed
  host      scene.nearest_directions and scene2.bracket_directions on the first `--host-sample` of those queries, microseconds per query
  call      the BlendSceneProcessor.process_ptr call the bracketed rows feed, as HIP events on a stream of the tool's own see it

The lookup's calls are synchronous and take host pointers, so their figure is the call as the host's clock sees it: checking and packing,
the copy up, the kernel, the copy down.  `--warmup` untimed rounds first, then the median and min - max of `--rounds`.  Two ratios per
case, neither a condition: the bracketed rows call over the helper's time for as many queries, and over the call it feeds.

    python tools/bench_lookup.py [--rounds 7] [--warmup 3] [--out profiles/lookup_bench.json]
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


def bench_one(a, K, n_dirs):
    import numpy as np
    import torch
    import open_headstage_amd as ohs
    from open_headstage_amd import lookup, synth

    dev = torch.device("cuda:0")
    S, nb, seg = a.streams, a.blocks, a.seg_blocks
    n_segs, frames = -(-nb // seg), nb * 512
    n = S * n_segs * K
    rng = np.random.default_rng(1000 * K + n_dirs % 997)
    pos = np.stack([rng.uniform(0, 360, n_dirs), np.degrees(np.arcsin(rng.uniform(-1, 1, n_dirs))), np.ones(n_dirs)], 1).astype(np.float32)
    src_az = (rng.uniform(-180, 180, (1, K)) + np.cumsum(rng.uniform(-3, 3, (n_segs, K)), 0)).astype(np.float32)
    src_el = rng.uniform(-50, 70, (n_segs, K)).astype(np.float32)
    yaw = np.cumsum(rng.uniform(-4, 4, (S, n_segs)), 1).astype(np.float32)
    pitch, roll = rng.uniform(-20, 20, (S, n_segs)).astype(np.float32), rng.uniform(-10, 10, (S, n_segs)).astype(np.float32)

    lk = ohs.DirectionLookup(pos)
    L = lookup.lookup_lib()
    v, sss, sks, R, rss, S_, segs_, K_ = lookup.rows_host_half(src_az, src_el, yaw, pitch, roll)
    assert (S_, segs_, K_, sss, sks, rss) == (S, n_segs, K, 0, 1, n_segs)
    q = np.ascontiguousarray(np.einsum("skji,kcj->skci", R, v.reshape(n_segs, K, 3)).reshape(n, 3))
    i0, i1, w = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.float32)
    p = lambda arr, t: arr.ctypes.data_as(t)      # noqa: E731

    def rows(blend):
        lookup.lookup_check(L.ohs_lookup_rows(lk._h, S, n_segs, K, p(v, lookup.dp), sss, sks, p(R, lookup.dp), rss, p(i0, lookup.u32p),
                                              p(i1, lookup.u32p) if blend else None, p(w, lookup.fp) if blend else None))

    def points(blend):
        lookup.lookup_check(L.ohs_lookup_points(lk._h, n, p(q, lookup.dp), p(i0, lookup.u32p), p(i1, lookup.u32p) if blend else None,
                                                p(w, lookup.fp) if blend else None))

    rec = {"objects": K, "streams": S, "segments": n_segs, "directions": n_dirs, "queries": n, "rounds": a.rounds, "warmup": a.warmup}
    for name, fn in (("rows", rows), ("points", points)):
        for blend in (False, True):
            for _ in range(a.warmup):
                fn(blend)
            ms = []
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                fn(blend)
                ms.append(1e3 * (time.perf_counter() - t0))
            rec[f"{name}_{'bracketed' if blend else 'nearest'}"] = _stats(ms)
    rec["last_launch"] = list(lk.last_launch())
    out_bytes = {"nearest": 4 * n, "bracketed": 12 * n}
    rec["bytes"] = {"rows_h2d": v.nbytes + R.nbytes, "points_h2d": q.nbytes, "d2h_nearest": out_bytes["nearest"], "d2h_bracketed": out_bytes["bracketed"]}
    rows(True)
    r0, r1, rw = i0.reshape(S, n_segs, K).copy(), i1.reshape(S, n_segs, K).copy(), w.reshape(S, n_segs, K).copy()

    # the helpers on a sample of the same head-relative directions
    ns = min(a.host_sample, n, max(64, (1 << 24) // n_dirs))      # (the helpers' temporaries are [sample][directions][3] f64)
    sk = np.arange(ns) // K
    az2, el2 = ohs.rotate_sources(src_az[sk % n_segs, np.arange(ns) % K], src_el[sk % n_segs, np.arange(ns) % K], yaw.reshape(-1)[sk],
                                  pitch.reshape(-1)[sk], roll.reshape(-1)[sk])
    t0 = time.perf_counter()
    h0 = ohs.nearest_directions(pos, -az2, el2)
    t1 = time.perf_counter()
    ohs.bracket_directions(pos, -az2, el2)
    t2 = time.perf_counter()
    rec["host"] = {"sample_queries": ns, "nearest_us_per_query": round(1e6 * (t1 - t0) / ns, 3), "bracket_us_per_query": round(1e6 * (t2 - t1) / ns, 3),
                   "sample_idx0_equal_share": float((h0 == r0.reshape(-1)[:ns]).mean())}

    # the call the rows feed
    sc = ohs.BlendSceneProcessor(S, num_bands=10)
    sc.set_directions((rng.standard_normal((n_dirs, 2, a.taps)) * (0.05 / K)).astype(np.float32))
    x = torch.empty((S, K, frames), dtype=torch.float32, device=dev)
    for c in range(K):
        x[:, c] = synth.white_noise_torch(1000 * c, S, frames, dev)[:, 0]
    y = torch.empty((S, 2, frames), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    ms = []
    with torch.cuda.stream(stream):
        for r in range(a.warmup + a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            sc.process_ptr(x.data_ptr(), y.data_ptr(), nb, K * frames, frames, 2 * frames, frames, K, seg, r0, None, None, None, True,
                           stream.cuda_stream, r1, rw, None, None)
            e1.record(stream)
            stream.synchronize()
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1))
    rec["scene_call"] = dict(_stats(ms), launch=list(sc.last_launch()))
    helper_ms = rec["host"]["bracket_us_per_query"] * n / 1e3
    rec["rows_bracketed_over_host_helper"] = round(rec["rows_bracketed"]["median_ms"] / helper_ms, 8)
    rec["rows_bracketed_over_scene_call"] = round(rec["rows_bracketed"]["median_ms"] / rec["scene_call"]["median_ms"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--seg-blocks", type=int, default=2)
    ap.add_argument("--taps", type=int, default=512)
    ap.add_argument("--cases", type=str, nargs="+", default=["6:1024", "8:1024", "16:1024", "16:65536"], help="objects:directions")
    ap.add_argument("--host-sample", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_lookup.py needs a GPU")
    from open_headstage_amd import build
    res = build.resources()
    out = {"tool": "tools/bench_lookup.py", "device": torch.cuda.get_device_name(0),
           "kernel_resources": {k: res.get(k, {}) for k in ("k_lookup<0>", "k_lookup<1>")}, "cases": []}
    for case in a.cases:
        K, n_dirs = (int(t) for t in case.split(":"))
        rec = bench_one(a, K, n_dirs)
        out["cases"].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

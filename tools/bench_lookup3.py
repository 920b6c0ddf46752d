#!/usr/bin/env python3
"""Prices the three-direction lookup (libohs_lookup3.so) against the numpy helper it stands in for and against the scene call it feeds.

Shape (tools/bench_lookup.py's): 256 streams x 256 blocks, seg_blocks 2 -> 128 segments, K = 6, 8, 16 objects over the octahedron
subdivided four times (1 026 directions, 2 048 triangles; lookup3.octahedron_mesh, no scipy); and K = 16 over the octahedron subdivided
six times (16 386 directions, 32 768 triangles).  Sources move from segment to segment and are shared by the streams ([segs][K]); every
stream has a head pose of its own per segment ([streams][segs]: yaw, pitch, roll).  Per case:

  rows      TriangleLookup.rows' C call (ohs_lookup3_rows) on the packed sources and matrices, tri == NULL
  points    ohs_lookup3_points on the same head-relative queries, computed on the host beforehand
  host      scene3.triangle_directions on the first `--host-sample` of those queries, microseconds per query
  call      the TriSceneProcessor.process_ptr call the rows feed, as HIP events on a stream of the tool's own see it

The lookup's calls are synchronous and take host pointers, so their figure is the call as the host's clock sees it: checking and packing,
the copy up, the kernel, the copy down.  `--warmup` untimed rounds first, then the median and min - max of `--rounds`.  Two ratios per
case, neither a condition: the rows call over the helper's time for as many queries, and over the call it feeds.

    python tools/bench_lookup3.py [--rounds 7] [--warmup 3] [--out profiles/lookup3_bench.json]
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


def bench_one(a, K, levels):
    import numpy as np
    import torch
    import open_headstage_amd as ohs
    from open_headstage_amd import lookup, lookup3, synth

    dev = torch.device("cuda:0")
    S, nb, seg = a.streams, a.blocks, a.seg_blocks
    n_segs, frames = -(-nb // seg), nb * 512
    n = S * n_segs * K
    pos, tri = lookup3.octahedron_mesh(levels)
    n_dirs = len(pos)
    rng = np.random.default_rng(1000 * K + levels)
    src_az = (rng.uniform(-180, 180, (1, K)) + np.cumsum(rng.uniform(-3, 3, (n_segs, K)), 0)).astype(np.float32)
    src_el = rng.uniform(-50, 70, (n_segs, K)).astype(np.float32)
    yaw = np.cumsum(rng.uniform(-4, 4, (S, n_segs)), 1).astype(np.float32)
    pitch, roll = rng.uniform(-20, 20, (S, n_segs)).astype(np.float32), rng.uniform(-10, 10, (S, n_segs)).astype(np.float32)

    lk = ohs.TriangleLookup(pos, tri)
    L = lookup3.lookup3_lib()
    v, sss, sks, R, rss, S_, segs_, K_ = lookup.rows_host_half(src_az, src_el, yaw, pitch, roll)
    assert (S_, segs_, K_, sss, sks, rss) == (S, n_segs, K, 0, 1, n_segs)
    q = np.ascontiguousarray(np.einsum("skji,kcj->skci", R, v.reshape(n_segs, K, 3)).reshape(n, 3))
    out = [np.empty(n, np.uint32) for _ in range(3)] + [np.empty(n, np.float32) for _ in range(2)]
    ptrs = [arr.ctypes.data_as(t) for arr, t in zip(out, lookup3._OUT)] + [None]
    p = lambda arr: arr.ctypes.data_as(lookup.dp)      # noqa: E731

    def rows():
        lookup3.lookup3_check(L.ohs_lookup3_rows(lk._h, S, n_segs, K, p(v), sss, sks, p(R), rss, *ptrs))

    def points():
        lookup3.lookup3_check(L.ohs_lookup3_points(lk._h, n, p(q), *ptrs))

    rec = {"objects": K, "streams": S, "segments": n_segs, "directions": n_dirs, "triangles": int(len(tri)), "queries": n,
           "rounds": a.rounds, "warmup": a.warmup}
    for name, fn in (("rows", rows), ("points", points)):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            fn()
            ms.append(1e3 * (time.perf_counter() - t0))
        rec[name] = _stats(ms)
    rec["last_launch"] = list(lk.last_launch())
    rec["bytes"] = {"rows_h2d": v.nbytes + R.nbytes, "points_h2d": q.nbytes, "d2h": 20 * n, "inverses_on_device": 72 * int(len(tri))}
    rows()
    r = [arr.reshape(S, n_segs, K).copy() for arr in out]
    rec["rows_with_w2_above_zero_share"] = float((r[4] > 0).mean())

    # the helper on a sample of the same head-relative directions
    ns = min(a.host_sample, n, max(64, (1 << 24) // len(tri)))
    sk = np.arange(ns) // K
    az2, el2 = ohs.rotate_sources(src_az[sk % n_segs, np.arange(ns) % K], src_el[sk % n_segs, np.arange(ns) % K], yaw.reshape(-1)[sk],
                                  pitch.reshape(-1)[sk], roll.reshape(-1)[sk])
    t0 = time.perf_counter()
    h = ohs.triangle_directions(pos, tri, -az2, el2)
    t1 = time.perf_counter()
    rec["host"] = {"sample_queries": ns, "triangle_us_per_query": round(1e6 * (t1 - t0) / ns, 3),
                   "sample_idx0_equal_share": float((h[0] == r[0].reshape(-1)[:ns]).mean())}

    # the call the rows feed
    sc = ohs.TriSceneProcessor(S, num_bands=10)
    sc.set_directions((rng.standard_normal((n_dirs, 2, a.taps)) * (0.05 / K)).astype(np.float32))
    x = torch.empty((S, K, frames), dtype=torch.float32, device=dev)
    for c in range(K):
        x[:, c] = synth.white_noise_torch(1000 * c, S, frames, dev)[:, 0]
    y = torch.empty((S, 2, frames), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    ms = []
    with torch.cuda.stream(stream):
        for i in range(a.warmup + a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            sc.process_ptr(x.data_ptr(), y.data_ptr(), nb, K * frames, frames, 2 * frames, frames, K, seg, r[0], None, None, None, True,
                           stream.cuda_stream, r[1], r[3], None, None, r[2], r[4], None, None)
            e1.record(stream)
            stream.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
    rec["scene_call"] = dict(_stats(ms), launch=list(sc.last_launch()))
    helper_ms = rec["host"]["triangle_us_per_query"] * n / 1e3
    rec["rows_over_host_helper"] = round(rec["rows"]["median_ms"] / helper_ms, 8)
    rec["rows_over_scene_call"] = round(rec["rows"]["median_ms"] / rec["scene_call"]["median_ms"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--seg-blocks", type=int, default=2)
    ap.add_argument("--taps", type=int, default=512)
    ap.add_argument("--cases", type=str, nargs="+", default=["6:4", "8:4", "16:4", "16:6"], help="objects:subdivisions of the octahedron")
    ap.add_argument("--host-sample", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup3_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_lookup3.py needs a GPU")
    from open_headstage_amd import build
    res = build.resources()
    out = {"tool": "tools/bench_lookup3.py", "device": torch.cuda.get_device_name(0),
           "kernel_resources": {k: res.get(k, {}) for k in ("k_lookup_tri",)}, "cases": []}
    for case in a.cases:
        K, levels = (int(t) for t in case.split(":"))
        rec = bench_one(a, K, levels)
        out["cases"].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Prices the tracked scene call (libohs_tracked.so) against the two calls it joins -- ohs_lookup3p_rows, then
ohs_scene3_process_blended3 -- on identical inputs in one session.

Shape: the scene benchmarks' -- 256 streams x 256 blocks, seg_blocks 2 -> 128 segments, K = 6, 8, 16 objects, 512 taps, CROSSFADE, every
object moving in every segment (sources shared by the streams, a head pose per stream and segment: every row differs) -- over
lookup3.octahedron_mesh at 2 048 triangles (level 4) and at 32 768 (level 6).  Two legs alternate inside every round; `--warmup` untimed
rounds first, then the median and min - max of `--rounds`, on the host's clock around call + sync:

  tracked    ohs_tracked_process, then ohs_tracked_sync
  composed   ohs_lookup3p_rows, then ohs_scene3_process_blended3 with prev_* by hand, then ohs_scene3_sync

and, for each leg, `held`: how long the caller's thread was held before the (last) call returned.  Every round carries the round
before it on both legs, so both render the same signal: the last round's outputs, rows and launch records are compared.
The one condition: the tracked leg's median is not above the composed leg's at any case (exit status 1 otherwise).

    python tools/bench_tracked.py [--rounds 5] [--warmup 2] [--out profiles/tracked_bench.json]
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


def bench_one(a, K, level):
    import numpy as np
    import torch
    import open_headstage_amd as ohs
    from open_headstage_amd import lookup, lookup3, lookup3p, synth

    dev = torch.device("cuda:0")
    S, nb, seg = a.streams, a.blocks, a.seg_blocks
    n_segs, frames = -(-nb // seg), nb * 512
    n = S * n_segs * K
    pos, tri = lookup3.octahedron_mesh(level)
    n_dirs = len(pos)
    rng = np.random.default_rng(1000 * K + n_dirs)
    src_az = (rng.uniform(-180, 180, (1, K)) + np.cumsum(rng.uniform(-3, 3, (n_segs, K)), 0)).astype(np.float32)
    src_el = rng.uniform(-50, 70, (n_segs, K)).astype(np.float32)
    yaw = np.cumsum(rng.uniform(-4, 4, (S, n_segs)), 1).astype(np.float32)
    pitch, roll = rng.uniform(-20, 20, (S, n_segs)).astype(np.float32), rng.uniform(-10, 10, (S, n_segs)).astype(np.float32)
    v, sss, sks, R, rss, S_, segs_, K_ = lookup.rows_host_half(src_az, src_el, yaw, pitch, roll)
    assert (S_, segs_, K_, sss, sks, rss) == (S, n_segs, K, 0, 1, n_segs)
    dirs = (rng.standard_normal((n_dirs, 2, a.taps)) * (0.05 / K)).astype(np.float32)

    tr = ohs.TrackedSceneProcessor(S, pos, tri, num_bands=10)
    tr.set_directions(dirs)
    lk = ohs.PrunedTriangleLookup(pos, tri)
    sc = ohs.TriSceneProcessor(S, num_bands=10)
    sc.set_directions(dirs)
    L3P = lookup3p.lookup3p_lib()
    rows = [np.empty(n, np.uint32) for _ in range(3)] + [np.empty(n, np.float32) for _ in range(2)]
    ptrs = [arr.ctypes.data_as(t) for arr, t in zip(rows, lookup3._OUT)] + [None]
    shaped = [arr.reshape(S, n_segs, K) for arr in rows]
    p = lambda arr: arr.ctypes.data_as(lookup.dp)      # noqa: E731

    x = torch.empty((S, K, frames), dtype=torch.float32, device=dev)
    for c in range(K):
        x[:, c] = synth.white_noise_torch(1000 * c, S, frames, dev)[:, 0]
    y = {name: torch.empty((S, 2, frames), dtype=torch.float32, device=dev) for name in ("tracked", "composed")}
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    prev = [None] * 5
    geometry = (nb, K * frames, frames, 2 * frames, frames, K, seg)

    def tracked():
        t0 = time.perf_counter()
        tr.process_ptr(x.data_ptr(), y["tracked"].data_ptr(), *geometry, v, sss, sks, R, rss, None, True, None, stream.cuda_stream)
        t1 = time.perf_counter()
        tr.sync(stream.cuda_stream)
        return t1 - t0, time.perf_counter() - t0

    def composed():
        t0 = time.perf_counter()
        lookup3p.lookup3p_check(L3P.ohs_lookup3p_rows(lk._h, S, n_segs, K, p(v), sss, sks, p(R), rss, *ptrs))
        sc.process_ptr(x.data_ptr(), y["composed"].data_ptr(), *geometry, shaped[0], None, prev[0], None, True, stream.cuda_stream, shaped[1],
                       shaped[3], prev[1], prev[3], shaped[2], shaped[4], prev[2], prev[4])
        t1 = time.perf_counter()
        sc.sync(stream.cuda_stream)
        t2 = time.perf_counter()
        prev[:] = [arr[:, -1, :].copy() for arr in shaped]
        return t1 - t0, t2 - t0

    legs = {"tracked": tracked, "composed": composed}
    total, held = {name: [] for name in legs}, {name: [] for name in legs}
    for i in range(a.warmup + a.rounds):
        for name, fn in legs.items():
            h, t = fn()
            if i >= a.warmup:
                held[name].append(1e3 * h)
                total[name].append(1e3 * t)
    torch.cuda.synchronize(dev)
    same_rows = all((got.view(np.uint32) == want.view(np.uint32)).all() for got, want in zip(tr.rows(), shaped))
    rec = {"objects": K, "streams": S, "blocks": nb, "segments": n_segs, "taps": a.taps, "directions": n_dirs, "triangles": int(len(tri)),
           "entries": n, "rounds": a.rounds, "warmup": a.warmup,
           "tracked": dict(_stats(total["tracked"]), held=_stats(held["tracked"])),
           "composed": dict(_stats(total["composed"]), held=_stats(held["composed"])),
           "outputs_bit_equal": bool(torch.equal(y["tracked"].view(torch.int32), y["composed"].view(torch.int32))),
           "rows_bit_equal": bool(same_rows),
           "launch": {"tracked": list(tr.last_launch()), "composed": list(sc.last_launch()) + [lk.last_launch()[2]]}}
    rec["tracked_over_composed"] = round(rec["tracked"]["median_ms"] / rec["composed"]["median_ms"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--seg-blocks", type=int, default=2)
    ap.add_argument("--taps", type=int, default=512)
    ap.add_argument("--cases", type=str, nargs="+", default=["6:4", "8:4", "16:4", "6:6", "8:6", "16:6"],
                    help="objects:subdivisions of the octahedron (4: 2 048 triangles, 6: 32 768)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracked_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_tracked.py needs a GPU")
    from open_headstage_amd import build
    res = build.resources()
    out = {"tool": "tools/bench_tracked.py", "device": torch.cuda.get_device_name(0),
           "kernel_resources": {k: res.get(k, {}) for k in ("k_scene_rows_seal<1>", "k_scene_rows_seal<4>", "k_lookup_tri_cells",
                                                            "k_lookup_tri_rest", "k_conv_p1_objects_blend3")}, "cases": []}
    slower = []
    for case in a.cases:
        K, level = (int(t) for t in case.split(":"))
        rec = bench_one(a, K, level)
        out["cases"].append(rec)
        print(json.dumps(rec), flush=True)
        if rec["tracked"]["median_ms"] > rec["composed"]["median_ms"]:
            slower.append(case)
    fmt = lambda s: f"{s['median_ms']:.2f} ({s['min_ms']:.2f} - {s['max_ms']:.2f})"       # noqa: E731
    print("| triangles | K | tracked, call + sync, ms | composed, ms | tracked / composed | thread held: tracked, ms | composed, ms | bits equal |")
    print("|---|---|---|---|---|---|---|---|")
    for r in out["cases"]:
        print(f"| {r['triangles']} | {r['objects']} | {fmt(r['tracked'])} | {fmt(r['composed'])} | {r['tracked_over_composed']:.2f} | "
              f"{fmt(r['tracked']['held'])} | {fmt(r['composed']['held'])} | {r['outputs_bit_equal'] and r['rows_bit_equal']} |", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if slower:
        sys.exit(f"the tracked call's median is above the composed path's at {slower}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Prices the pruned three-direction lookup (libohs_lookup3p.so) against the brute-force one (libohs_lookup3.so) on identical inputs, and
both against the scene call the rows feed.

Shape, method and clock are tools/bench_lookup3.py's: 256 streams x 256 blocks, seg_blocks 2 -> 128 segments; K = 6, 8, 16 objects over
the octahedron subdivided four times (2 048 triangles), K = 16 over the octahedron subdivided six times (32 768), and -- where scipy is
installed -- K = 16 over the hull of 65 536 random points (131 068 triangles).  Sources move from segment to segment and are shared by
the streams, every stream has a head pose of its own per segment.  Both calls are synchronous and take host pointers: the figure is the
call as the host's clock sees it.  `--warmup` untimed rounds first, then the median and min - max of `--rounds`; the two libraries' legs
alternate inside every round.  Per case:

  moving    PrunedTriangleLookup.rows' C call against TriangleLookup.rows' on the moving sources (a handful of queries reach pass 2)
  worst     the same calls with every source on a measurement and identity poses: every query reaches pass 2
  create    seconds to create each handle (inverses on both; the index on the pruned one), once each
  index     ohs_lookup3p_index's figures for the mesh
  call      the TriSceneProcessor.process_ptr call the rows feed, as HIP events on a stream of the tool's own see it

Nothing here is a condition.

    python tools/bench_lookup3p.py [--rounds 7] [--warmup 3] [--out profiles/lookup3p_bench.json]
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


def _mesh(case):
    import numpy as np
    from open_headstage_amd import lookup3, scene3
    if case == "hull":
        rng = np.random.default_rng(65536)
        pos = np.stack([rng.uniform(0, 360, 65536), np.degrees(np.arcsin(rng.uniform(-1, 1, 65536))), np.ones(65536)], 1).astype(np.float32)
        return pos, scene3.triangulate_directions(pos)
    return lookup3.octahedron_mesh(int(case))


def _alternate(a, legs):
    """legs: name -> fn; -> name -> stats, the legs run one after the other inside every round"""
    ms = {name: [] for name in legs}
    for i in range(a.warmup + a.rounds):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            if i >= a.warmup:
                ms[name].append(1e3 * (time.perf_counter() - t0))
    return {name: _stats(v) for name, v in ms.items()}


def bench_one(a, K, case):
    import numpy as np
    import torch
    import open_headstage_amd as ohs
    from open_headstage_amd import lookup, lookup3, lookup3p, synth

    dev = torch.device("cuda:0")
    S, nb, seg = a.streams, a.blocks, a.seg_blocks
    n_segs, frames = -(-nb // seg), nb * 512
    n = S * n_segs * K
    pos, tri = _mesh(case)
    n_dirs = len(pos)
    rng = np.random.default_rng(1000 * K + n_dirs)
    src_az = (rng.uniform(-180, 180, (1, K)) + np.cumsum(rng.uniform(-3, 3, (n_segs, K)), 0)).astype(np.float32)
    src_el = rng.uniform(-50, 70, (n_segs, K)).astype(np.float32)
    yaw = np.cumsum(rng.uniform(-4, 4, (S, n_segs)), 1).astype(np.float32)
    pitch, roll = rng.uniform(-20, 20, (S, n_segs)).astype(np.float32), rng.uniform(-10, 10, (S, n_segs)).astype(np.float32)

    t0 = time.perf_counter()
    brute = ohs.TriangleLookup(pos, tri)
    t1 = time.perf_counter()
    pruned = ohs.PrunedTriangleLookup(pos, tri)
    t2 = time.perf_counter()
    L3, L3P = lookup3.lookup3_lib(), lookup3p.lookup3p_lib()
    v, sss, sks, R, rss, S_, segs_, K_ = lookup.rows_host_half(src_az, src_el, yaw, pitch, roll)
    assert (S_, segs_, K_, sss, sks, rss) == (S, n_segs, K, 0, 1, n_segs)
    # the worst case: every source on a measurement, identity poses
    xyz = lookup.table_xyz(pos)
    v_on = np.ascontiguousarray(xyz[rng.integers(0, n_dirs, (n_segs, K))].astype(np.float64))
    R_eye = np.ascontiguousarray(np.broadcast_to(np.eye(3), (S, n_segs, 3, 3)))
    outs = {name: [np.empty(n, np.uint32) for _ in range(3)] + [np.empty(n, np.float32) for _ in range(2)] for name in ("pruned", "brute")}
    ptrs = {name: [arr.ctypes.data_as(t) for arr, t in zip(o, lookup3._OUT)] + [None] for name, o in outs.items()}
    p = lambda arr: arr.ctypes.data_as(lookup.dp)      # noqa: E731

    def call(name, src, rot):
        if name == "pruned":
            lookup3p.lookup3p_check(L3P.ohs_lookup3p_rows(pruned._h, S, n_segs, K, p(src), sss, sks, p(rot), rss, *ptrs[name]))
        else:
            lookup3.lookup3_check(L3.ohs_lookup3_rows(brute._h, S, n_segs, K, p(src), sss, sks, p(rot), rss, *ptrs[name]))

    rec = {"objects": K, "streams": S, "segments": n_segs, "directions": n_dirs, "triangles": int(len(tri)), "queries": n,
           "rounds": a.rounds, "warmup": a.warmup,
           "create_s": {"brute": round(t1 - t0, 4), "pruned": round(t2 - t1, 4)},
           "index": dict(zip(("grid", "cells", "entries", "longest_list", "everywhere"), pruned.index()))}
    for shape, src, rot in (("moving", v, R), ("worst", v_on, R_eye)):
        st = _alternate(a, {"pruned": lambda: call("pruned", src, rot), "brute": lambda: call("brute", src, rot)})
        same = all((np.ascontiguousarray(x).view(np.uint32) == np.ascontiguousarray(y).view(np.uint32)).all()
                   for x, y in zip(outs["pruned"], outs["brute"]))
        rec[shape] = dict(st, fallback_queries=pruned.last_launch()[2], rows_bit_equal=bool(same),
                          pruned_over_brute=round(st["pruned"]["median_ms"] / st["brute"]["median_ms"], 4))
    call("pruned", v, R)
    r = [arr.reshape(S, n_segs, K).copy() for arr in outs["pruned"]]

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
    for shape in ("moving", "worst"):
        for name in ("pruned", "brute"):
            rec[shape][f"{name}_over_scene_call"] = round(rec[shape][name]["median_ms"] / rec["scene_call"]["median_ms"], 4)
    return rec


def create_only(n_tris):
    """create times at a mesh size the cases above may not reach: the level-6 mesh, stored four times for 131 072 triangles"""
    import numpy as np
    import open_headstage_amd as ohs
    from open_headstage_amd import lookup3
    pos, tri = lookup3.octahedron_mesh(6)
    tri = np.ascontiguousarray(np.tile(tri, (n_tris // len(tri), 1)))
    t0 = time.perf_counter()
    ohs.TriangleLookup(pos, tri)
    t1 = time.perf_counter()
    lk = ohs.PrunedTriangleLookup(pos, tri)
    t2 = time.perf_counter()
    return {"triangles": int(len(tri)), "mesh": "lookup3.octahedron_mesh(6)" + (f" stored {n_tris // 32768} times" if n_tris > 32768 else ""),
            "create_s": {"brute": round(t1 - t0, 4), "pruned": round(t2 - t1, 4)},
            "index": dict(zip(("grid", "cells", "entries", "longest_list", "everywhere"), lk.index()))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--seg-blocks", type=int, default=2)
    ap.add_argument("--taps", type=int, default=512)
    ap.add_argument("--cases", type=str, nargs="+", default=["6:4", "8:4", "16:4", "16:6", "16:hull"],
                    help="objects:subdivisions of the octahedron, or objects:hull (the hull of 65 536 random points; needs scipy)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup3p_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_lookup3p.py needs a GPU")
    from open_headstage_amd import build
    res = build.resources()
    out = {"tool": "tools/bench_lookup3p.py", "device": torch.cuda.get_device_name(0),
           "kernel_resources": {k: res.get(k, {}) for k in ("k_lookup_tri_cells", "k_lookup_tri_rest", "k_lookup_tri")}, "cases": [],
           "skipped": [], "create_only": []}
    # (a first handle of each kind, untimed: the libraries load and the device wakes outside the create figures)
    import open_headstage_amd as ohs
    from open_headstage_amd import lookup3
    warm = lookup3.octahedron_mesh(1)
    ohs.TriangleLookup(*warm), ohs.PrunedTriangleLookup(*warm)
    for case in a.cases:
        K, mesh = case.split(":")
        if mesh == "hull":
            try:
                import scipy  # noqa: F401
            except ImportError:
                out["skipped"].append({"case": case, "why": "scipy is not installed"})
                continue
        rec = bench_one(a, int(K), mesh)
        out["cases"].append(rec)
        print(json.dumps(rec), flush=True)
    for n_tris in (32768, 131072):
        rec = create_only(n_tris)
        out["create_only"].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

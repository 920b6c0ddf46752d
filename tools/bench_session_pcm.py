#!/usr/bin/env python3
"""Prices SessionRenderer.render_pcm -- integer PCM over the link, the codec on the device -- against the host codec around
SessionRenderer.render, host memory to host memory.

Shape: the one of profiles/session_bench.json -- 256 streams, 5.1 (6 channels), 72 sets of 512 taps, every stream a row of its own
with a new set every two blocks, 938 blocks (480 256 frames), chunks of 64 blocks, crossfade on, EQ off.  If the pinned staging
buffers cannot be had for 256 streams, the stream count is halved until they can, and recorded.  Input: int16, interleaved
[S][frames][6], from a fixed seed.

Three forms, alternating run by run in one process, `--runs` (5) timed runs each after one untimed run of all:

  host_codec  per stream pcm_decode, render on the float array, per stream pcm_encode: what render_files did per call before the
              PCM path, without the file I/O -- the same int16-to-int16 job
  float       render on the float array decoded beforehand, float result: the renderer without any codec, an easier job
  pcm         render_pcm

Wall time by perf_counter around the blocking call.  The results of host_codec and pcm are compared byte for byte once.
Criteria:  1. the SLOWEST pcm run is faster than the FASTEST host_codec run;  2. the median of pcm is at or below the median of
float.  Also recorded, without a threshold: link_bytes per form, GB/s each way, Msamples/s (stream-frames per second), and the time
of every stage of a SERIAL loop over the same chunks for the pcm and the float form (host copy into pinned memory and the drain by
perf_counter; copy-in, decode + kernels + encode, copy-out by HIP events): where criterion 2 fails, the stage to look at is the
one that grew.

--files: the other mode.  64 streams of 5.1, 16-bit, 480 256 frames, written to a temporary directory that is removed afterwards;
render_files(pcm=False) against the default path, alternating, three timed runs each after one untimed.  Criterion: the default
path's slowest run is faster than the pcm=False path's fastest; the output files are compared byte for byte.  Its record goes under
"files" into the same JSON file, beside what is there.

    python tools/bench_session_pcm.py [--files] [--out profiles/session_pcm_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(np, synth, n_sets, K, taps):
    base = synth.hrir_set(taps)
    table = np.zeros((n_sets, K, 2, taps), np.float32)
    for j in range(n_sets):
        for c in range(K):
            for e in range(2):
                table[j, c, e] = np.roll(base[(2 * c + e + j) % 4], (5 * c + e + 3 * j) % 23) * np.float32(1.0 - 0.02 * c)
        table[j] /= np.abs(table[j]).sum(axis=(0, 2), keepdims=True)
    return table, np.arange(n_sets) * (360.0 / n_sets) - 180.0


def _stats(v):
    return {"median_s": round(statistics.median(v), 4), "min_s": round(min(v), 4), "max_s": round(max(v), 4),
            "all_s": [round(t, 4) for t in v]}


def _save(path, key, rec):
    print(json.dumps(rec), flush=True)
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    doc = {}
    if os.path.exists(path):
        try:
            doc = json.load(open(path))
        except ValueError:
            doc = {}
    if key is None:
        doc = {**rec, **({"files": doc["files"]} if "files" in doc else {})}
    else:
        doc[key] = rec
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def _stages(torch, np, ohs, r, ref, x16, xf, idx, calls, K, seg, pcm):
    """one SERIAL pass over the chunks, every stage waited for and timed on its own -> seconds per stage, summed over the chunks"""
    from open_headstage_amd.session import call_rows
    S, chunk = r.n_streams, r.chunk_blocks * 512
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    w = 2 if pcm else 4
    h_in = torch.empty(S * K * chunk * w, dtype=torch.uint8, pin_memory=True)
    h_out = torch.empty(S * 2 * chunk * w, dtype=torch.uint8, pin_memory=True)
    d_raw_in = torch.empty(S * K * chunk * w, dtype=torch.uint8, device=dev)
    d_raw_out = torch.empty(S * 2 * chunk * w, dtype=torch.uint8, device=dev)
    d_in = torch.empty(S * K * chunk, dtype=torch.float32, device=dev) if pcm else d_raw_in.view(torch.float32)
    d_out = torch.empty(S * 2 * chunk, dtype=torch.float32, device=dev) if pcm else d_raw_out.view(torch.float32)
    f64 = torch.empty(S * 2 * chunk, dtype=torch.float64, device=dev) if pcm else None
    dt = torch.int16 if pcm else torch.float32
    src = torch.from_numpy(x16 if pcm else xf)
    res = torch.empty((S, calls[-1][0] * 512 + calls[-1][1] * 512, 2) if pcm else (S, 2, calls[-1][0] * 512 + calls[-1][1] * 512), dtype=dt)
    t = {"host_copy_into_pinned": 0.0, "copy_in": 0.0, "decode_kernels_encode" if pcm else "kernels": 0.0, "copy_out": 0.0, "drain": 0.0}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ref.reset()
    with torch.cuda.stream(stream):
        for start, n, g, _ in calls:
            nf, f0 = n * 512, start * 512
            shape_in, shape_out = ((S, nf, K), (S, nf, 2)) if pcm else ((S, K, nf), (S, 2, nf))
            hi = h_in[:S * K * nf * w].view(dt).view(shape_in)
            ho = h_out[:S * 2 * nf * w].view(dt).view(shape_out)
            ri = d_raw_in[:S * K * nf * w].view(dt).view(shape_in)
            ro = d_raw_out[:S * 2 * nf * w].view(dt).view(shape_out)
            di, do = d_in[:S * K * nf].view(S, K, nf), d_out[:S * 2 * nf].view(S, 2, nf)
            t0 = time.perf_counter()
            hi.copy_(src[:, f0:f0 + nf] if pcm else src[:, :, f0:f0 + nf])
            t["host_copy_into_pinned"] += time.perf_counter() - t0
            ev[0].record(stream)
            ri.copy_(hi, non_blocking=True)
            ev[1].record(stream)
            if pcm:
                ohs.pcm_decode_device(ri, 16, di)
            ref.process_layout_scheduled_ptr(di.data_ptr(), do.data_ptr(), n, K * nf, nf, 2 * nf, nf, g,
                                             call_rows(idx, 0, start, n, g, seg),
                                             None if start == 0 else np.ascontiguousarray(idx[:, (start - 1) // seg]), True,
                                             stream.cuda_stream)
            if pcm:
                ohs.pcm_encode_device(do, 16, ro, f64[:S * 2 * nf].view(S, 2, nf))
            ev[2].record(stream)
            ho.copy_(ro, non_blocking=True)
            ev[3].record(stream)
            stream.synchronize()
            t["copy_in"] += ev[0].elapsed_time(ev[1]) / 1e3
            t["decode_kernels_encode" if pcm else "kernels"] += ev[1].elapsed_time(ev[2]) / 1e3
            t["copy_out"] += ev[2].elapsed_time(ev[3]) / 1e3
            t0 = time.perf_counter()
            (res[:, f0:f0 + nf] if pcm else res[:, :, f0:f0 + nf]).copy_(ho)
            t["drain"] += time.perf_counter() - t0
    return {k: round(v, 4) for k, v in t.items()}, res.numpy()


def bench_render(a):
    import numpy as np
    import torch
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    from open_headstage_amd.session import pcm_decode, pcm_encode, plan_calls

    K, nb, seg, n_sets, chunk = 6, a.blocks, a.seg_blocks, a.sets, a.chunk_blocks
    assert nb % seg == 0, "the session is one call that is not final"
    frames, n_segs = nb * 512, nb // seg
    table, grid = _table(np, synth, n_sets, K, a.taps)
    S, r, requested = a.streams, None, a.streams
    while r is None:
        try:
            r = ohs.SessionRenderer.layout(S, table, grid, seg_blocks=seg, chunk_blocks=chunk)
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
    x16 = rng.integers(-16384, 16384, (S, frames, K), dtype=np.int16)
    xf = np.empty((S, K, frames), np.float32)
    for s in range(S):
        xf[s] = pcm_decode(x16[s].tobytes(), 16, K)
    x_tmp = np.empty((S, K, frames), np.float32)
    y_tmp = np.empty((S, 2, frames), np.float32)
    y_float = np.empty((S, 2, frames), np.float32)
    y_host = np.zeros((S, frames, 2), np.int16)
    y_pcm = np.zeros((S, frames, 2), np.int16)
    link = {}

    def host_codec():
        r.reset()
        for s in range(S):
            x_tmp[s] = pcm_decode(x16[s].tobytes(), 16, K)
        r.render(x_tmp, rows=idx, out=y_tmp)
        for s in range(S):
            y_host[s] = np.frombuffer(pcm_encode(y_tmp[s], 16), np.int16).reshape(frames, 2)

    def float_form():
        r.reset()
        r.render(xf, rows=idx, out=y_float)

    def pcm_form():
        r.reset()
        r.render_pcm(x16, rows=idx, out=y_pcm)

    forms = [("host_codec", host_codec), ("float", float_form), ("pcm", pcm_form)]
    for n, fn in forms:
        fn()
        link[n] = list(r.link_bytes)
    same = bool(y_host.tobytes() == y_pcm.tobytes()) and int(np.abs(y_pcm.astype(np.int32)).max()) > 300
    sec = {n: [] for n, _ in forms}
    for _ in range(a.runs):
        for n, fn in forms:
            t0 = time.perf_counter()
            fn()
            sec[n].append(time.perf_counter() - t0)

    rec = {"shape": {"streams": S, "streams_requested": requested, "channels": K, "sets": n_sets, "taps": a.taps, "seg_blocks": seg,
                     "blocks": nb, "frames": frames, "chunk_blocks": chunk, "calls": len(list(plan_calls(0, nb, seg, chunk))),
                     "crossfade": 1, "eq": 0, "input": "int16 interleaved"},
           "pinned_bytes_of_the_renderer": 2 * 4 * (S * K + S * 2) * chunk * 512,
           "device_bytes_of_the_renderer_float_only": (8 * K + 16) * S * chunk * 512,
           "device_bytes_of_the_renderer_with_pcm": (20 * K + 56) * S * chunk * 512,
           "device_bytes_measured": int(torch.cuda.memory_allocated()),
           "torch_threads": torch.get_num_threads(), "runs": a.runs, "host_codec_and_pcm_same_bytes": same}
    for n in sec:
        t = statistics.median(sec[n])
        rec[n] = _stats(sec[n])
        rec[n].update({"link_bytes": link[n], "link_GBps_in": round(link[n][0] / t / 1e9, 3),
                       "link_GBps_out": round(link[n][1] / t / 1e9, 3), "Msamples_s": round(S * frames / t / 1e6, 1)})
    rec["criterion_1_pcm_max_below_host_codec_min"] = rec["pcm"]["max_s"] < rec["host_codec"]["min_s"]
    rec["criterion_2_pcm_median_at_or_below_float_median"] = rec["pcm"]["median_s"] <= rec["float"]["median_s"]
    rec["pcm_median_over_float_median"] = round(statistics.median(sec["pcm"]) / statistics.median(sec["float"]), 4)
    rec["pcm_median_over_host_codec_median"] = round(statistics.median(sec["pcm"]) / statistics.median(sec["host_codec"]), 4)

    del x_tmp, y_tmp, y_float
    calls = list(plan_calls(0, nb, seg, chunk))
    ref = ohs.BatchProcessor(S, num_bands=10)
    ref.set_layout_table(table)
    try:
        st_pcm, res = _stages(torch, np, ohs, r, ref, x16, xf, idx, calls, K, seg, True)
        st_pcm["same_bytes_as_render_pcm"] = bool(res.tobytes() == y_pcm.tobytes())
        st_float, _ = _stages(torch, np, ohs, r, ref, x16, xf, idx, calls, K, seg, False)
        rec["serial_stages_s"] = {"pcm": st_pcm, "float": st_float}
        grew = {k: st_pcm[k2] - st_float[k] for k, k2 in [("host_copy_into_pinned",) * 2, ("copy_in",) * 2,
                                                          ("kernels", "decode_kernels_encode"), ("copy_out",) * 2, ("drain",) * 2]}
        rec["serial_stage_that_grew_most_from_float_to_pcm"] = max(grew, key=grew.get)
    except RuntimeError as e:
        rec["serial_stages_s"] = {"error": str(e)}
    _save(a.out, None, rec)
    return 0 if rec["criterion_1_pcm_max_below_host_codec_min"] and rec["criterion_2_pcm_median_at_or_below_float_median"] and same else 1


def bench_files(a):
    import numpy as np
    import open_headstage_amd as ohs
    from open_headstage_amd import synth

    K, S, nb, seg, chunk, runs = 6, a.file_streams, a.blocks, a.seg_blocks, a.chunk_blocks, 3
    frames = nb * 512
    table, grid = _table(np, synth, a.sets, K, a.taps)
    r = ohs.SessionRenderer.layout(S, table, grid, seg_blocks=seg, chunk_blocks=chunk)
    T = frames / 48000.0
    tracks = [ohs.HeadTrack([0.0, T], [-170.0 + 3.0 * s, 170.0 - 5.0 * s]) for s in range(S)]
    with tempfile.TemporaryDirectory() as d:
        rng = np.random.default_rng(2)
        ins = []
        for s in range(S):
            p = os.path.join(d, f"in{s}.wav")
            with wave.open(p, "wb") as w:
                w.setnchannels(K); w.setsampwidth(2); w.setframerate(48000)
                w.writeframes(rng.integers(-16384, 16384, (frames, K), dtype=np.int16))
            ins.append(p)
        outs = {n: [os.path.join(d, f"{n}{s}.wav") for s in range(S)] for n in ("float_path", "default_path")}
        forms = [("float_path", lambda: ohs.render_files(ins, outs["float_path"], r, tracks, pcm=False)),
                 ("default_path", lambda: ohs.render_files(ins, outs["default_path"], r, tracks))]
        link, written = {}, {}
        for n, fn in forms:
            written[n] = fn()
            link[n] = list(r.link_bytes)
        same = written["float_path"] == written["default_path"] and all(
            open(p, "rb").read() == open(q, "rb").read() for p, q in zip(outs["float_path"], outs["default_path"]))
        sec = {n: [] for n, _ in forms}
        for _ in range(runs):
            for n, fn in forms:
                t0 = time.perf_counter()
                fn()
                sec[n].append(time.perf_counter() - t0)
    rec = {"shape": {"streams": S, "channels": K, "bits": 16, "frames": frames, "sets": a.sets, "taps": a.taps, "seg_blocks": seg,
                     "chunk_blocks": chunk, "call_chunks": ohs.session.CALL_CHUNKS, "ring_out": 1, "a head track per stream": 1},
           "runs": runs, "frames_written_per_output": written["default_path"][0], "both_paths_same_file_bytes": bool(same)}
    for n in sec:
        rec[n] = _stats(sec[n])
        rec[n]["link_bytes"] = link[n]
        rec[n]["Msamples_s"] = round(S * frames / statistics.median(sec[n]) / 1e6, 1)
    rec["criterion_default_max_below_float_path_min"] = rec["default_path"]["max_s"] < rec["float_path"]["min_s"]
    rec["default_median_over_float_path_median"] = round(rec["default_path"]["median_s"] / rec["float_path"]["median_s"], 4)
    _save(a.out, "files", rec)
    return 0 if rec["criterion_default_max_below_float_path_min"] and same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--file-streams", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=938)
    ap.add_argument("--taps", type=int, default=512)
    ap.add_argument("--sets", type=int, default=72)
    ap.add_argument("--seg-blocks", type=int, default=2)
    ap.add_argument("--chunk-blocks", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--files", action="store_true", help="the file mode: render_files(pcm=False) against the default path")
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    return bench_files(a) if a.files else bench_render(a)


if __name__ == "__main__":
    sys.exit(main())

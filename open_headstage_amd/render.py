"""python -m open_headstage_amd.render: WAV stems, a SOFA file and head-tracker logs -> binaural WAVs.

    python -m open_headstage_amd.render --sofa F --layout 5.1|7.1|stereo --yaw-step 5 [--track T.csv ...] [--late late.wav]
                                        [--out-bits 16|24|32] -o OUTDIR IN.wav ...

One input file per stream (PCM 16 / 24 / 32, all of one rate; 6, 8 or 2 channels in WAV order), one output file of the same name in
OUTDIR, of its input's sample width or of --out-bits.  --track: `time_s,yaw_deg` lines, yaw positive to the right; one file for all streams or one per input; none: the head
looks ahead.  --late: a four-channel WAV [Lsl, Lsr, Rsl, Rsr] holding the static late part of the room's response from tap 512 on
(stereo only).  The table holds one set per --yaw-step degrees around the circle."""
from __future__ import annotations

import argparse
import os
import sys


def _parser():
    p = argparse.ArgumentParser(prog="python -m open_headstage_amd.render", description=__doc__.split("\n\n")[0])
    p.add_argument("inputs", nargs="+", metavar="IN.wav", help="one PCM WAV per stream")
    p.add_argument("--sofa", required=True, help="the SOFA file the responses come from")
    p.add_argument("--layout", required=True, choices=["5.1", "7.1", "stereo"])
    p.add_argument("--yaw-step", type=float, default=5.0, help="degrees between two sets of the table (default 5)")
    p.add_argument("--track", action="append", default=[], metavar="T.csv", help="tracker log: time_s,yaw_deg per line")
    p.add_argument("--late", metavar="late.wav", help="static late part, four channels (stereo only)")
    p.add_argument("-o", "--outdir", required=True)
    p.add_argument("--seg-blocks", type=int, default=2, help="blocks of 512 frames per yaw segment (default 2)")
    p.add_argument("--chunk-blocks", type=int, default=64, help="blocks per pipeline chunk (default 64)")
    p.add_argument("--no-crossfade", action="store_true", help="let the old set ring out instead of fading")
    p.add_argument("--no-ring-out", action="store_true", help="cut every output at its input's length")
    p.add_argument("--out-bits", type=int, choices=[16, 24, 32], help="bits per sample of the outputs (default: the inputs' width)")
    p.add_argument("--device", type=int, default=0)
    return p


def main(argv=None) -> int:
    a = _parser().parse_args(argv)
    import numpy as np

    from . import session
    from .batch import LAYOUT_5_1, LAYOUT_7_1
    from .sofa import MySofa

    if not 0 < a.yaw_step <= 360:
        raise SystemExit("--yaw-step: between 0 and 360 degrees")
    if a.track and len(a.track) not in (1, len(a.inputs)):
        raise SystemExit("--track: one log for all streams, or one per input")
    with session.WavReader(a.inputs[0]) as w:
        fs = float(w.rate)
    grid = np.arange(-180.0, 180.0, a.yaw_step)
    kw = dict(seg_blocks=a.seg_blocks, chunk_blocks=a.chunk_blocks, crossfade=not a.no_crossfade, fs=fs, device=a.device)
    sofa = MySofa(a.sofa)
    S = len(a.inputs)
    if a.layout == "stereo":
        late = None
        if a.late:
            late, late_fs, _ = session.read_wav(a.late)
            if late_fs != fs or late.shape[0] != 4:
                raise SystemExit(f"--late: four channels at {fs:g} Hz, got {late.shape[0]} at {late_fs}")
        r = session.SessionRenderer.stereo_from_sofa(S, sofa, grid, late_irs=late, **kw)
    else:
        if a.late:
            raise SystemExit("--late: a late part is available with --layout stereo only")
        r = session.SessionRenderer.layout_from_sofa(S, sofa, LAYOUT_5_1 if a.layout == "5.1" else LAYOUT_7_1, grid, **kw)
    tracks = [session.read_track_csv(t) for t in a.track]
    tracks = None if not tracks else tracks[0] if len(tracks) == 1 else tracks
    os.makedirs(a.outdir, exist_ok=True)
    outs = [os.path.join(a.outdir, os.path.basename(p)) for p in a.inputs]
    if len(set(outs)) != len(outs):
        raise SystemExit("two inputs share a file name: their outputs would collide")
    n = session.render_files(a.inputs, outs, r, tracks, ring_out=not a.no_ring_out, out_bits=a.out_bits)
    for p, k in zip(outs, n):
        print(f"{p}: {k} frames")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Extracts the two-speaker HRIR set (azimuth +/-30 deg, elevation 0) of the reference's DATA asset
data/hrtf/subject_003.sofa (CIPIC subject 003; a data file, not source) into
tests/golden/cipic003_pm30.npz with this repo's SOFA reader, for the GPU tests (the GPU box has no
/root/reference).  Also stores the 48 kHz resampled set used as the realistic-HRIR input of
SURVEY section 8d.  Run from the repo root:  python tools/make_sofa_fixture.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from open_headstage_amd import sofa  # noqa: E402

SRC = "/root/reference/data/hrtf/subject_003.sofa"
s = sofa.MySofa(SRC)
il, ir = s.nearest(30.0, 0.0), s.nearest(-30.0, 0.0)
irs441 = sofa.speaker_hrirs(s)
irs48 = sofa.speaker_hrirs(s, target_samplerate=48000.0)
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "cipic003_pm30.npz"),
                    index_left=il, index_right=ir, pos_left=s.position(il), pos_right=s.position(ir),
                    fs=s.source_samplerate, irs_44100=np.stack(irs441), irs_48000=np.stack(irs48))
print("indices", il, ir, "taps", irs441[0].size, irs48[0].size)

# The reference's second data asset, data/hrtf/processed_hrir.wav (a data file: 16-bit PCM, 4 channels, 200 frames,
# 44.1 kHz): its channels are measurements 355 and 171 of the same SOFA file, receivers 0 and 1, quantised to int16
# (channels 0 / 2 clip).  Kept as a fixture: it pins ohs_sofa_get_ir against data the reference itself holds.
import struct  # noqa: E402

raw = open("/root/reference/data/hrtf/processed_hrir.wav", "rb").read()
assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE"
fmt_tag, channels, rate, _, _, bits = struct.unpack("<HHIIHH", raw[20:36])
assert (fmt_tag, channels, bits) == (1, 4, 16)
i = raw.index(b"data")
nbytes = struct.unpack("<I", raw[i + 4:i + 8])[0]
pcm = np.frombuffer(raw[i + 8:i + 8 + nbytes], dtype="<i2").reshape(-1, channels).copy()
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "processed_hrir_wav.npz"), pcm=pcm, fs=np.float32(rate),
                    measurement=np.array([355, 355, 171, 171]), receiver=np.array([0, 1, 0, 1]))
print("processed_hrir.wav:", pcm.shape, rate)

# subject_003.sofa itself, for the SOFA reader's tests (tests/test_cpu_sofa.py, tests/test_cpu_parsers_asan.py): the file
# byte for byte except Data.IR, whose one deflate + shuffle chunk is rewritten with every measurement those tests do not
# read set to zero.  The new, shorter chunk sits at the same offset (the chunk B-tree's size field updated, the rest of
# the old chunk zero-filled), so every other offset in the file holds; gzip then packs the zeros away.
import gzip  # noqa: E402
import zlib  # noqa: E402

IR_CHUNK_OFF, IR_CHUNK_SIZE_FIELD, IR_CHUNK_ADDR_FIELD = 60771, 35582, 35622
src = bytearray(open(SRC, "rb").read())
old_len = struct.unpack_from("<I", src, IR_CHUNK_SIZE_FIELD)[0]
assert struct.unpack_from("<Q", src, IR_CHUNK_ADDR_FIELD)[0] == IR_CHUNK_OFF and old_len == 1776593
full = np.frombuffer(zlib.decompress(bytes(src[IR_CHUNK_OFF:IR_CHUNK_OFF + old_len])), np.uint8)
full = full.reshape(8, -1).T.copy().view("<f8").reshape(s.num_measurements, s.num_receivers, s.filter_length)
si = sofa.MySofa(SRC, sofa.SOFA_INTERPOLATE)
pos = np.stack([s.position(m) for m in range(s.num_measurements)])
keep = {0, 1, 13, 308, 355, 356, 171, 172, 400, 908, 1249, int(np.argmin(pos[:, 0] + pos[:, 1]))}
# every direction the tests query (AES69 azimuths: the plugin's speaker angles negated), with two rings of neighbours
for az, el in ((30, 0), (-30, 0), (75, 20), (-10, -15), (-12.5, 44), (-88, -44), (-90, 0), (90, 0), (31.7, 1.2)):
    ring = {s.nearest(az, el)}
    for _ in range(2):
        ring |= {int(j) for m in ring for j in si.neighbors(m)[:4] if j >= 0}
    keep |= ring
part = np.zeros_like(full)
part[sorted(keep)] = full[sorted(keep)]
chunk = zlib.compress(np.frombuffer(part.tobytes(), np.uint8).reshape(-1, 8).T.tobytes(), 9)
assert len(chunk) <= old_len
src[IR_CHUNK_OFF:IR_CHUNK_OFF + old_len] = chunk + bytes(old_len - len(chunk))
struct.pack_into("<I", src, IR_CHUNK_SIZE_FIELD, len(chunk))
with open(os.path.join(ROOT, "tests", "golden", "subject_003_subset.sofa.gz"), "wb") as f:
    f.write(gzip.compress(bytes(src), 9, mtime=0))
print("subject_003_subset.sofa.gz:", len(keep), "of", s.num_measurements, "measurements kept:", sorted(keep))

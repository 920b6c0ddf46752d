"""PCM beside the session renderer, the part that needs no GPU: the device codec on torch CPU tensors and the RIFF reader.

The yardsticks are session.pcm_decode / session.pcm_encode (numpy, pinned by tests/test_cpu_session.py) and the stdlib `wave`
module; every comparison is on bytes.  The EXTENSIBLE headers are built by hand here, field by field."""
import os
import struct
import subprocess
import sys
import wave

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_INT = {16: np.int16, 24: np.uint8, 32: np.int32}


def to_pcm(v, bits):
    """integers [...] (int64, in range) -> the PCM array of that width: int16 / int32 [...], 24-bit packed uint8 [...][3]"""
    v = np.asarray(v, np.int64)
    if bits == 24:
        return np.stack([(v >> (8 * i)) & 0xFF for i in range(3)], axis=-1).astype(np.uint8)
    return v.astype(NP_INT[bits])


def host_decode(raw, bits):
    """pcm_decode per stream: PCM [S][n][C](+[3]) -> float32 [S][C][n]"""
    from open_headstage_amd.session import pcm_decode
    return np.stack([pcm_decode(raw[s].tobytes(), bits, raw.shape[2]) for s in range(raw.shape[0])])


def host_encode(y, bits):
    """pcm_encode per stream: float [S][2][n] -> PCM [S][n][2](+[3])"""
    from open_headstage_amd.session import pcm_encode
    S, C, n = y.shape
    shape = (n, C, 3) if bits == 24 else (n, C)
    return np.stack([np.frombuffer(pcm_encode(y[s], bits), NP_INT[bits]).reshape(shape) for s in range(S)])


def device_decode(raw, bits):
    import torch
    from open_headstage_amd import pcm_decode_device
    S, n, C = raw.shape[:3]
    out = torch.full((S, C, n), float("nan"))
    word = torch.zeros((S, n, C), dtype=torch.int32) if bits == 24 else None
    got = pcm_decode_device(torch.from_numpy(raw), bits, out, word)
    assert got is out
    if bits == 24:
        assert (word.numpy() & 0xFF == 0).all()                 # (the contract that lets the scratch be used again)
    return out.numpy()


def device_encode(y, bits):
    import torch
    from open_headstage_amd import pcm_encode_device
    S, C, n = y.shape
    shape = (S, n, C, 3) if bits == 24 else (S, n, C)
    out = torch.zeros(shape, dtype={16: torch.int16, 24: torch.uint8, 32: torch.int32}[bits])
    word = torch.full((S, n, C), 0x55555555, dtype=torch.int32) if bits == 24 else None
    pcm_encode_device(torch.from_numpy(y), bits, out, torch.full((S, C, n), float("nan"), dtype=torch.float64), word)
    return out.numpy()


def _edge_ints(bits, count):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    v = [lo, hi, 0, -1]
    for k in range(bits - 1):
        for d in (-1, 0, 1):
            v += [(1 << k) + d, -(1 << k) + d]
    v = [a for a in v if lo <= a <= hi]
    rng = np.random.default_rng(bits)
    v = np.concatenate([np.array(v, np.int64), rng.integers(lo, hi + 1, 4096, dtype=np.int64)])
    return np.resize(v, count) if count > v.size else v


# ---- the codec ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C", [(1, 1), (3, 2), (1, 6), (3, 6)])
def test_decode_16_of_every_value(S, C):
    v = np.arange(-32768, 32768, dtype=np.int64)
    n = -(-v.size // (S * C)) + 3
    v = np.resize(np.random.default_rng(S * 10 + C).permutation(v), (S, n, C))
    assert set(v.reshape(-1).tolist()) == set(range(-32768, 32768))
    raw = to_pcm(v, 16)
    got, want = device_decode(raw, 16), host_decode(raw, 16)
    assert got.shape == (S, C, n) and got.dtype == np.float32
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert (got.astype(np.float64) * 32768.0 == v.transpose(0, 2, 1)).all()


@pytest.mark.parametrize("bits", [24, 32])
@pytest.mark.parametrize("S,C", [(1, 1), (3, 2), (1, 6), (3, 6)])
def test_decode_24_and_32_at_the_edges_and_at_random(bits, S, C):
    v = _edge_ints(bits, 0)
    n = -(-v.size // (S * C)) + 1
    v = np.resize(v, (S, n, C))
    raw = to_pcm(v, bits)
    got, want = device_decode(raw, bits), host_decode(raw, bits)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    exact = got.astype(np.float64) * float(1 << (bits - 1)) == v.transpose(0, 2, 1)
    if bits == 24:
        assert exact.all()
    else:
        assert not exact.all() and exact.any()                  # (values no float32 holds are among them: the rounding is tested)


def _encode_inputs(bits):
    full = float(1 << (bits - 1))
    lsb = 1.0 / full
    special = [1.0, -1.0, 1.0 - lsb, -(1.0 - lsb), 1.0 + lsb, -1.0 - lsb, 1.2, -1.2, 2.5, -3.0, 8.0, -8.0, 0.0, -0.0,
               1e-45, -1e-45, 1e-39, -1e-39, 1.17549435e-38, 0.4 * lsb, -0.6 * lsb]
    special += [(k + 0.5) * lsb for k in range(-3, 4)]
    special += [0.5 + (k + 0.5) * lsb for k in range(-3, 4)] + [-0.25 + (k + 0.5) * lsb for k in range(-3, 4)]
    # the values of tests/test_cpu_session.py::test_pcm_encode_clips_and_rounds_half_to_even
    special += [1.0, 2.5, -1.0, -3.0, 0.5 / full, 1.5 / full, 2.5 / full, -0.5 / full, -1.5 / full, 0.4 / full, -0.6 / full]
    rng = np.random.default_rng(100 + bits)
    return np.concatenate([np.array(special, np.float64).astype(np.float32), rng.uniform(-1.2, 1.2, 6000).astype(np.float32)])


@pytest.mark.parametrize("bits", [16, 24, 32])
@pytest.mark.parametrize("S", [1, 3])
def test_encode_against_the_host_encode(bits, S):
    v = _encode_inputs(bits)
    n = -(-v.size // (S * 2)) + 1
    y = np.ascontiguousarray(np.resize(v, (S, 2, n)))
    got, want = device_encode(y, bits), host_encode(y, bits)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert got.tobytes() == want.tobytes()
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    for i in range(40):                                         # the special values again, in Python integers (round: half to even)
        exact = float(y[0, 0, i]) * float(1 << (bits - 1))      # (a float32 times a power of two: exact in float64)
        assert int.from_bytes(got[0, i, 0].tobytes(), "little", signed=True) == max(lo, min(hi, round(exact))), float(y[0, 0, i])
    assert int.from_bytes(got[0, 0, 0].tobytes(), "little", signed=True) == hi      # 1.0 is the positive rail


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_encode_of_the_ties_written_out(bits):
    """the values and the expectations of test_pcm_encode_clips_and_rounds_half_to_even, as Python integers"""
    full = float(1 << (bits - 1))
    x = np.array([1.0, 2.5, -1.0, -3.0, 0.5 / full, 1.5 / full, 2.5 / full, -0.5 / full, -1.5 / full, 0.4 / full, -0.6 / full], np.float64)
    want = [(1 << (bits - 1)) - 1, (1 << (bits - 1)) - 1, -(1 << (bits - 1)), -(1 << (bits - 1)), 0, 2, 2, 0, -2, 0, -1]
    y = np.zeros((1, 2, x.size), np.float32)
    y[0, 1] = x.astype(np.float32)
    got = device_encode(y, bits)
    assert [int.from_bytes(got[0, i, 1].tobytes(), "little", signed=True) for i in range(x.size)] == want
    assert not got[0, :, 0].any()


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_decode_then_encode_is_the_identity_on_the_bytes(bits):
    v = _edge_ints(bits, 0)
    if bits == 32:
        v = v & ~np.int64(0xFF)                                 # the values a float32 sample can hold
    v = np.resize(v, (3, -(-v.size // 6), 2))
    raw = to_pcm(v, bits)
    assert device_encode(device_decode(raw, bits), bits).tobytes() == raw.tobytes()


def test_codec_works_on_views_and_refuses_what_does_not_fit():
    import torch
    from open_headstage_amd import pcm_decode_device, pcm_encode_device
    raw = to_pcm(np.resize(_edge_ints(16, 0), (2, 40, 6)), 16)
    big = torch.zeros((2, 6, 64))
    pcm_decode_device(torch.from_numpy(raw), 16, big[:, :, :40])            # a strided output, as the renderer's ragged chunk
    assert (big[:, :, :40].numpy() == host_decode(raw, 16)).all() and not big[:, :, 40:].any()
    out = torch.empty((2, 6, 40))
    with pytest.raises(ValueError):
        pcm_decode_device(torch.from_numpy(raw), 12, out)
    with pytest.raises(ValueError):
        pcm_decode_device(torch.from_numpy(raw), 32, out)                   # int16 samples called 32-bit
    with pytest.raises(ValueError):
        pcm_decode_device(torch.from_numpy(raw[:, :39]), 16, out)
    with pytest.raises(ValueError):
        pcm_decode_device(torch.from_numpy(to_pcm(np.zeros((2, 40, 6)), 24)), 24, out)      # 24 bits without the word
    y = torch.zeros((2, 2, 40))
    with pytest.raises(ValueError):
        pcm_encode_device(y, 16, torch.empty((2, 40, 2), dtype=torch.int16), torch.empty((2, 2, 40)))       # a float32 scratch
    with pytest.raises(ValueError):
        pcm_encode_device(y, 16, torch.empty((2, 40, 2), dtype=torch.int32), torch.empty((2, 2, 40), dtype=torch.float64))
    with pytest.raises(ValueError):
        pcm_encode_device(y, 8, torch.empty((2, 40, 2), dtype=torch.int16), torch.empty((2, 2, 40), dtype=torch.float64))


# ---- the RIFF reader ------------------------------------------------------------------------------------------------------------
PCM_GUID = struct.pack("<H", 1) + bytes.fromhex("000000001000800000aa00389b71")
FLOAT_GUID = struct.pack("<H", 3) + bytes.fromhex("000000001000800000aa00389b71")


def extensible_wav(data, channels, bits, rate=48000, valid=None, guid=PCM_GUID, extra=(), cut=None):
    """a WAVE_FORMAT_EXTENSIBLE file by hand: RIFF, fmt (40 bytes), the `extra` chunks (id, payload) with their pad bytes, data"""
    align = channels * bits // 8
    fmt = struct.pack("<HHIIHH", 0xFFFE, channels, rate, rate * align, align, bits)
    fmt += struct.pack("<HHI", 22, bits if valid is None else valid, (1 << channels) - 1) + guid
    assert len(fmt) == 40
    body = b"WAVE" + b"fmt " + struct.pack("<I", 40) + fmt
    for cid, payload in extra:
        body += cid + struct.pack("<I", len(payload)) + payload + (b"\x00" if len(payload) & 1 else b"")
    if data is not None:
        body += b"data" + struct.pack("<I", len(data)) + data + (b"\x00" if len(data) & 1 else b"")
    blob = b"RIFF" + struct.pack("<I", len(body)) + body
    return blob if cut is None else blob[:cut]


@pytest.mark.parametrize("bits", [16, 24, 32])
@pytest.mark.parametrize("channels", [1, 2, 6])
def test_reader_gives_the_frames_wave_gives(tmp_path, bits, channels):
    from open_headstage_amd import WavReader
    from open_headstage_amd.session import read_wav
    frames = 333
    raw = to_pcm(np.resize(_edge_ints(bits, 0), (frames, channels)), bits).tobytes()
    p = tmp_path / "a.wav"
    with wave.open(str(p), "wb") as w:
        w.setnchannels(channels); w.setsampwidth(bits // 8); w.setframerate(44100)
        w.writeframes(raw)
    with wave.open(str(p), "rb") as w:
        want = w.readframes(w.getnframes())
        assert want == raw
    with WavReader(p) as r:
        assert (r.channels, r.bits, r.rate, r.frames, r.frame_bytes) == (channels, bits, 44100, frames, channels * bits // 8)
        assert r.readframes(frames) == want
        assert r.readframes(5) == b""
    x, rate, b = read_wav(p)
    assert rate == 44100 and b == bits and x.shape == (channels, frames)


def test_reader_takes_an_extensible_header_behind_an_odd_list_chunk(tmp_path):
    from open_headstage_amd import WavReader
    from open_headstage_amd.session import pcm_decode, read_wav
    channels, frames = 6, 100
    v = np.resize(_edge_ints(24, 0), (frames, channels))
    raw = to_pcm(v, 24).tobytes()
    p = tmp_path / "x.wav"
    p.write_bytes(extensible_wav(raw, channels, 24, extra=[(b"LIST", b"INFOabc")]))         # 7 bytes: a pad byte follows
    if sys.version_info < (3, 12):
        with pytest.raises(wave.Error):                         # (the gap this reader closes)
            wave.open(str(p), "rb")
    with WavReader(p) as r:
        assert (r.channels, r.bits, r.rate, r.frames) == (channels, 24, 48000, frames)
        one = r.readframes(frames)
    assert one == raw
    with WavReader(p) as r:                                     # readinto in three pieces, into slices of one array
        a = np.zeros((frames, channels, 3), np.uint8)
        assert r.readinto(a[:30], 30) == 30
        assert r.readinto(a[30:31], 1) == 1
        assert r.readinto(a[31:], 500) == frames - 31           # (asks for more than is left: what is left)
        assert r.readinto(a[:0], 4) == 0
    assert a.tobytes() == raw
    x, rate, bits = read_wav(p)
    assert (rate, bits) == (48000, 24) and (x == pcm_decode(raw, 24, channels)).all()
    with WavReader(p) as r, pytest.raises(ValueError):
        r.readinto(np.zeros((10, channels, 3), np.uint8), 11)   # a buffer that is too small


def test_reader_refusals(tmp_path):
    from open_headstage_amd import WavReader
    data = bytes(6 * 3 * 10)
    p = tmp_path / "bad.wav"
    cases = {
        "a float sub-format": extensible_wav(bytes(6 * 4 * 10), 6, 32, guid=FLOAT_GUID),
        "20 valid bits in 24": extensible_wav(data, 6, 24, valid=20),
        "8-bit extensible": extensible_wav(bytes(60), 6, 8),
        "no data chunk": extensible_wav(None, 6, 24, extra=[(b"LIST", b"INFOabc")]),
        "cut inside fmt": extensible_wav(data, 6, 24, cut=12 + 8 + 20),
        "cut inside a chunk header": extensible_wav(data, 6, 24, cut=12 + 8 + 40 + 3),
        "not RIFF": b"RIFX" + extensible_wav(data, 6, 24)[4:],
    }
    for what, blob in cases.items():
        p.write_bytes(blob)
        with pytest.raises(ValueError):
            WavReader(p)
            pytest.fail(what)
    for tag, bits, what in [(3, 32, "float, tag 3"), (1, 8, "8-bit, tag 1"), (0x11, 16, "ADPCM")]:
        fmt = struct.pack("<HHIIHH", tag, 2, 48000, 48000 * 2 * bits // 8, 2 * bits // 8, bits)
        body = b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", 16) + bytes(16)
        p.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)
        with pytest.raises(ValueError):
            WavReader(p)
            pytest.fail(what)
    body = b"WAVE" + b"fmt " + struct.pack("<I", 0x7FFFFFF0) + bytes(64)   # a fmt chunk that claims 2 GiB is not read to find out
    p.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)
    with pytest.raises(ValueError, match="fmt chunk of"):
        WavReader(p)
    p.write_bytes(extensible_wav(data, 6, 24))                   # ... and the file they were all made from is read
    with WavReader(p) as r:
        assert r.frames == 10


# ---- command line and package surface -------------------------------------------------------------------------------------------
def test_render_command_line_help_names_out_bits_and_keeps_its_words():
    r = subprocess.run([sys.executable, "-m", "open_headstage_amd.render", "--help"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for word in ("--out-bits", "--sofa", "--layout", "--yaw-step", "--track", "--late", "--outdir"):
        assert word in r.stdout, word
    from open_headstage_amd.render import _parser
    base = ["--sofa", "f", "--layout", "5.1", "-o", "d", "in.wav"]
    assert _parser().parse_args(base).out_bits is None
    assert _parser().parse_args(base + ["--out-bits", "24"]).out_bits == 24
    with pytest.raises(SystemExit):
        _parser().parse_args(base + ["--out-bits", "12"])


def test_package_exports_the_pcm_names():
    import inspect

    import open_headstage_amd as ohs
    for name in ("pcm_decode_device", "pcm_encode_device", "WavReader"):
        assert hasattr(ohs, name) and name in ohs.__all__, name
    assert callable(ohs.SessionRenderer.render_pcm) and isinstance(ohs.SessionRenderer.link_bytes, property)
    p = inspect.signature(ohs.SessionRenderer.render_pcm).parameters
    assert list(p)[1:] == ["x", "yaw", "rows", "prev", "final", "ring_out", "out", "out_bits"]
    p = inspect.signature(ohs.render_files).parameters
    assert list(p) == ["inputs", "outputs", "renderer", "tracks", "ring_out", "out_bits", "pcm"] and p["pcm"].default is None


# ---- render_files around a stand-in renderer: the two paths, the threads ------------------------------------------------------------
class _StandIn:
    """what render_files asks of a renderer, without a GPU: two of the channels, halved, behind `reach` frames of delay; render_pcm
    is by definition the host codec around render"""
    n_streams, channels, reach, fs, seg_blocks, chunk_blocks = 3, 6, 5, 48000.0, 2, 1

    def __init__(self, fail_at_call=None):
        self.calls, self.fail_at_call = 0, fail_at_call

    def reset(self):
        self.calls = 0

    def render(self, x, yaw=None, final=False, ring_out=False, out=None):
        self.calls += 1
        if self.calls == self.fail_at_call:
            raise RuntimeError("the stand-in fails here")
        assert final or x.shape[2] % (self.seg_blocks * 512) == 0
        y = np.zeros((x.shape[0], 2, x.shape[2] + (self.reach if ring_out else 0)), np.float32)
        y[:, :, :x.shape[2]] = 0.5 * x[:, 1:3] + 0.25 * x[:, 4:6]
        return y

    def render_pcm(self, x, yaw=None, final=False, ring_out=False, out=None, out_bits=None):
        bits = {np.dtype(np.int16): 16, np.dtype(np.uint8): 24, np.dtype(np.int32): 32}[x.dtype]
        out[...] = host_encode(self.render(host_decode(x, bits), final=final, ring_out=ring_out), out_bits)
        return out


def _stand_in_files(tmp_path, bits, lens=(1400, 2500, 700)):
    paths = []
    for s, n in enumerate(lens):
        raw = to_pcm(np.resize(_edge_ints(bits, 0)[s:], (n, 6)), bits).tobytes()
        p = tmp_path / f"in{bits}_{s}.wav"
        if s == 1:
            p.write_bytes(extensible_wav(raw, 6, bits, extra=[(b"LIST", b"INFOabc")]))
        else:
            with wave.open(str(p), "wb") as w:
                w.setnchannels(6); w.setsampwidth(bits // 8); w.setframerate(48000)
                w.writeframes(raw)
        paths.append(p)
    return paths


@pytest.mark.parametrize("bits,out_bits", [(16, None), (24, None), (32, None), (24, 16), (16, 32)])
def test_render_files_paths_write_the_same_bytes_around_a_stand_in(tmp_path, monkeypatch, bits, out_bits):
    import threading

    from open_headstage_amd import render_files, session
    monkeypatch.setattr(session, "CALL_CHUNKS", 2)              # calls of 1 024 frames: three calls, the last one ragged
    ins = _stand_in_files(tmp_path, bits)
    outs = {n: [tmp_path / f"{n}{s}.wav" for s in range(3)] for n in ("float", "default", "pcm")}
    r = _StandIn()
    want = [n + 5 for n in (1400, 2500, 700)]
    assert render_files(ins, outs["float"], r, out_bits=out_bits, pcm=False) == want and r.calls == 3
    assert render_files(ins, outs["default"], r, out_bits=out_bits) == want and r.calls == 3
    assert render_files(ins, outs["pcm"], r, out_bits=out_bits, pcm=True) == want
    assert threading.active_count() == 1                        # reader and writer are gone on return
    for s in range(3):
        a, b, c = (outs[n][s].read_bytes() for n in ("float", "default", "pcm"))
        assert a == b == c and len(a) == 44 + want[s] * 2 * (out_bits or bits) // 8
    assert render_files(ins, outs["pcm"], r, ring_out=False) == [1400, 2500, 700]


def test_render_files_mixed_widths_and_a_failure_midway(tmp_path, monkeypatch):
    import threading

    from open_headstage_amd import render_files, session
    monkeypatch.setattr(session, "CALL_CHUNKS", 2)
    in16, in24 = _stand_in_files(tmp_path, 16), _stand_in_files(tmp_path, 24)
    mixed = [in16[0], in24[1], in16[2]]
    outs = [tmp_path / f"o{s}.wav" for s in range(3)]
    ref = [tmp_path / f"r{s}.wav" for s in range(3)]
    r = _StandIn()
    monkeypatch.setattr(r, "render_pcm", None)                  # the fallback does not touch it
    assert render_files(mixed, outs, r) == render_files(mixed, ref, r, pcm=False)
    assert [o.read_bytes() for o in outs] == [o.read_bytes() for o in ref]
    with wave.open(str(outs[1]), "rb") as w:
        assert w.getsampwidth() == 3
    with pytest.raises(ValueError):
        render_files(mixed, outs, r, pcm=True)
    with pytest.raises(ValueError):
        render_files(in16, outs, r, out_bits=20)
    broken = _StandIn(fail_at_call=2)                           # the second call fails while the reader is ahead of it
    with pytest.raises(RuntimeError, match="stand-in"):
        render_files(in16, outs, broken)
    assert threading.active_count() == 1
    for o in outs:                                              # every file was closed: the header was patched on close
        with wave.open(str(o), "rb") as w:
            assert w.getnframes() <= 1024

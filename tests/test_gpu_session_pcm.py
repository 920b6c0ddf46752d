"""SessionRenderer.render_pcm and the PCM path of render_files: integer PCM over the link, the codec on the device.

The yardstick is the float path with the HOST codec around it: per stream pcm_encode(render(pcm_decode(x))) on a twin renderer of
the same construction (session.pcm_decode / pcm_encode are pinned by tests/test_cpu_session.py, render by
tests/test_gpu_session.py, whose builders and fixtures are imported, not restated).  Every comparison is on bytes.  Three streams,
5.1 and stereo, 24-tap responses, seg_blocks 2, chunks of 4 and 3 blocks, unless said otherwise."""
import struct
import wave

import numpy as np
import pytest

from tests.test_cpu_ir_schedule import make_rows
from tests.test_cpu_layout import BLOCK
from tests.test_cpu_session_pcm import NP_INT, extensible_wav, host_decode, host_encode, to_pcm
from tests.test_gpu_session import FS, K, N_SETS, S, TAPS, _late_irs, _layout_renderer, _stereo_renderer
from tests.test_gpu_session import lib, sets, table          # noqa: F401  (module-scoped fixtures)

pytestmark = pytest.mark.gpu


def pcm_noise(bits, channels, frames, seed, streams=S, square=False):
    """interleaved PCM drawn over the full integer range, [streams][frames][channels](+[3]); square: the two ends only (the
    loudest noise the format holds)"""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    rng = np.random.default_rng(seed)
    v = rng.integers(lo, hi + 1, (streams, frames, channels), dtype=np.int64)
    if square:
        v = np.where(v < 0, lo, hi)
    v[0, :2, 0] = [lo, hi]
    return to_pcm(v, bits)


def via_host_codec(r, x, bits, out_bits=None, **kw):
    """the definition: per stream pcm_encode(render(pcm_decode(x)), out_bits)"""
    return host_encode(r.render(host_decode(x, bits), **kw), out_bits or bits)


def same_bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.dtype} {want.shape}"
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        pytest.fail(f"{what}: {len(bad)} of {got.size} entries differ, the first at {bad[0].tolist()}: {got[tuple(bad[0])]} "
                    f"against {want[tuple(bad[0])]}")


# ---- 1. render_pcm is the encode of render on the decode ------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [16, 24, 32])
@pytest.mark.parametrize("fade", [True, False])
def test_layout_render_pcm_is_the_host_codec_around_render(lib, table, bits, fade):
    x = pcm_noise(bits, K, 11 * BLOCK, 8000 + bits)
    rows = make_rows(S, 6, N_SETS)
    for chunk in (4, 3):
        want = via_host_codec(_layout_renderer(lib, table, chunk, fade), x, bits, rows=rows, final=True)
        assert len(np.unique(want)) > 100
        r = _layout_renderer(lib, table, chunk, fade)
        y = r.render_pcm(x, rows=rows, final=True)
        assert isinstance(y, np.ndarray) and r.position_blocks == 11
        same_bytes(y, want, f"layout, {bits} bits, chunks of {chunk}, crossfade {fade}")


@pytest.mark.parametrize("bits", [16, 24, 32])
@pytest.mark.parametrize("fade", [True, False])
@pytest.mark.parametrize("late", [False, True])
def test_stereo_render_pcm_is_the_host_codec_around_render(lib, sets, bits, fade, late):
    x = pcm_noise(bits, 2, 11 * BLOCK, 8100 + bits)
    rows = make_rows(S, 6, N_SETS)
    irs = _late_irs() if late else None
    for chunk in (4, 3):
        want = via_host_codec(_stereo_renderer(lib, sets, chunk, fade, irs), x, bits, rows=rows, final=True)
        y = _stereo_renderer(lib, sets, chunk, fade, irs).render_pcm(x, rows=rows, final=True)
        same_bytes(y, want, f"stereo, {bits} bits, chunks of {chunk}, crossfade {fade}, late part {late}")


# ---- 2. two calls and a ragged final one; the two paths in one session ----------------------------------------------------------
@pytest.mark.parametrize("bits", [16, 24])
def test_two_calls_and_a_ragged_final_with_ring_out(lib, table, bits):
    frames = 11 * BLOCK + 700                                   # 6 blocks, then 5 blocks + 700 frames, then the reach
    x = pcm_noise(bits, K, frames, 8200 + bits)
    rows = make_rows(S, 7, N_SETS)
    a, b = np.ascontiguousarray(x[:, :6 * BLOCK]), np.ascontiguousarray(x[:, 6 * BLOCK:])
    ref = _layout_renderer(lib, table, 4)
    want = [via_host_codec(ref, a, bits, rows=rows[:, :3]), via_host_codec(ref, b, bits, rows=rows[:, 3:], final=True, ring_out=True)]
    r = _layout_renderer(lib, table, 4)
    ya = r.render_pcm(a, rows=rows[:, :3])
    assert r.position_blocks == 6
    yb = r.render_pcm(b, rows=rows[:, 3:], final=True, ring_out=True)
    assert yb.shape[1] == 5 * BLOCK + 700 + TAPS - 1 and r.position_blocks == 13
    same_bytes(ya, want[0], "the first call")
    same_bytes(yb, want[1], "the ragged final call with its reach")
    assert yb[:, 5 * BLOCK + 700:].any()                        # (the reach holds the response's tail)
    with pytest.raises(ValueError):
        r.render_pcm(a, rows=rows[:, :3])                       # the session is over
    r.reset()
    same_bytes(r.render_pcm(a, rows=rows[:, :3]), want[0], "behind reset()")


def test_render_and_render_pcm_alternate_within_one_session(lib, sets):
    """16-bit input is exact in float32, so the float results of the mixed session are those of the all-float one, and the PCM
    results their encode"""
    x = pcm_noise(16, 2, 12 * BLOCK, 8300)
    xf = host_decode(x, 16)
    rows = make_rows(S, 6, N_SETS)
    cut = [slice(0, 4 * BLOCK), slice(4 * BLOCK, 8 * BLOCK), slice(8 * BLOCK, 12 * BLOCK)]
    ref = _stereo_renderer(lib, sets, 3)
    want = [ref.render(np.ascontiguousarray(xf[:, :, c]), rows=rows[:, 2 * i:2 * i + 2]) for i, c in enumerate(cut)]
    r = _stereo_renderer(lib, sets, 3)
    y0 = r.render_pcm(np.ascontiguousarray(x[:, cut[0]]), rows=rows[:, 0:2])
    y1 = r.render(np.ascontiguousarray(xf[:, :, cut[1]]), rows=rows[:, 2:4])
    y2 = r.render_pcm(np.ascontiguousarray(x[:, cut[2]]), rows=rows[:, 4:6])
    assert r.position_blocks == 12
    same_bytes(y0, host_encode(want[0], 16), "render_pcm at the session's start")
    same_bytes(y1.view(np.uint32), want[1].view(np.uint32), "render behind render_pcm")
    same_bytes(y2, host_encode(want[2], 16), "render_pcm behind render")


# ---- 3. clipping and out_bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,out_bits", [(24, 16), (16, 24), (16, 32)])
def test_clipping_and_out_bits(lib, table, bits, out_bits):
    x = pcm_noise(bits, K, 6 * BLOCK, 8400 + bits, square=True)
    rows = make_rows(S, 3, N_SETS)
    ref = _layout_renderer(lib, table, 4)
    ref.set_gain(4.0)
    want = via_host_codec(ref, x, bits, out_bits, rows=rows)
    r = _layout_renderer(lib, table, 4)
    r.set_gain(4.0)
    y = r.render_pcm(x, rows=rows, out_bits=out_bits)
    same_bytes(y, want, f"{bits} bits in, {out_bits} out, gain 4")
    lo, hi = -(1 << (out_bits - 1)), (1 << (out_bits - 1)) - 1
    v = y.astype(np.int64)
    if out_bits == 24:
        v = v[..., 0] | (v[..., 1] << 8) | (v[..., 2] << 16)
        v = v - ((v & 0x800000) << 1)
    assert (v == hi).sum() > 10 and (v == lo).sum() > 10, "the result reaches both rails"
    assert ((v > lo) & (v < hi)).sum() > 1000


# ---- 4. both slots turn over; pinned input --------------------------------------------------------------------------------------
def test_nine_chunks_and_a_pinned_tensor(lib, table):
    import torch
    x = pcm_noise(16, K, 9 * BLOCK, 8500)
    rows = make_rows(S, 5, N_SETS)
    want = via_host_codec(_layout_renderer(lib, table, 1), x, 16, rows=rows, final=True)
    r = _layout_renderer(lib, table, 1)
    same_bytes(r.render_pcm(x, rows=rows, final=True), want, "nine chunks of one block")
    r.reset()
    xp = torch.from_numpy(x.copy()).pin_memory()
    yp = r.render_pcm(xp, rows=rows, final=True)
    assert isinstance(yp, torch.Tensor) and not yp.is_cuda and yp.dtype == torch.int16
    same_bytes(yp.numpy(), want, "a pinned tensor through nine chunks")
    big = _layout_renderer(lib, table, 16)                      # one chunk: the pinned tensor is copied to the device as it is
    same_bytes(big.render_pcm(xp, rows=rows, final=True).numpy(), want, "a pinned tensor in one chunk")
    out = np.zeros((S, 9 * BLOCK, 2), np.int16)
    big.reset()
    assert big.render_pcm(x, rows=rows, final=True, out=out) is out
    same_bytes(out, want, "into out=")


def test_first_24_bit_call_behind_a_busy_default_stream(lib, table):
    """the first render_pcm allocates and zeroes the decode scratch: that fill is ordered in front of the decode even while the
    caller's own work keeps the default stream busy"""
    import torch
    x = pcm_noise(24, K, 8 * BLOCK, 8550)
    rows = make_rows(S, 4, N_SETS)
    want = via_host_codec(_layout_renderer(lib, table, 4), x, 24, rows=rows)
    r = _layout_renderer(lib, table, 4)
    busy = torch.empty(1 << 26, device="cuda")
    for _ in range(20):
        busy.normal_()                                          # (queued, not waited for)
    y = r.render_pcm(x, rows=rows)
    torch.cuda.synchronize()
    same_bytes(y, want, "the first 24-bit call of a renderer")


# ---- 5. integers cross the link -------------------------------------------------------------------------------------------------
def test_link_bytes_count_half_and_three_quarters_of_the_float_path(lib, table):
    frames = 8 * BLOCK
    rows = make_rows(S, 4, N_SETS)
    r = _layout_renderer(lib, table, 3)
    assert r.link_bytes == (0, 0)
    r.render(host_decode(pcm_noise(16, K, frames, 8600), 16), rows=rows)
    fin, fout = r.link_bytes
    assert (fin, fout) == (4 * S * K * frames, 4 * S * 2 * frames)          # every sample of the call, four bytes each
    r.reset()
    assert r.link_bytes == (0, 0)
    r.render_pcm(pcm_noise(16, K, frames, 8600), rows=rows)
    assert r.link_bytes == (fin // 2, fout // 2)
    r.reset()
    r.render_pcm(pcm_noise(24, K, frames, 8601), rows=rows)
    assert r.link_bytes == (3 * fin // 4, 3 * fout // 4)
    r.render_pcm(pcm_noise(24, K, frames, 8602), rows=rows, out_bits=16)    # ... and they add up until reset()
    assert r.link_bytes == (3 * fin // 2, 3 * fout // 4 + fout // 2)


# ---- 6. memory ------------------------------------------------------------------------------------------------------------------
def test_device_memory_is_allocated_once_and_render_alone_allocates_what_it_did(lib, table):
    import gc

    import torch
    chunk = 2
    gc.collect()                                                # (no earlier renderer is freed between the readings below)
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    r = _layout_renderer(lib, table, chunk)
    x = pcm_noise(16, K, 32 * BLOCK, 8700)
    rows = make_rows(S, 16, N_SETS)
    r.render(host_decode(x[:, :8 * BLOCK], 16), rows=rows[:, :4])
    torch.cuda.synchronize()
    float_only = 2 * 4 * (S * K + 2 * S) * chunk * BLOCK                   # DESIGN section 4.5g's formula
    assert float_only % 512 == 0                                            # (no rounding by the allocator to account for)
    assert torch.cuda.memory_allocated() - m0 == float_only
    r.reset()
    r.render_pcm(np.ascontiguousarray(x[:, :8 * BLOCK]), rows=rows[:, :4])  # 4 chunks
    torch.cuda.synchronize()
    m4 = torch.cuda.memory_allocated()
    assert m4 - m0 == (20 * K + 56) * S * chunk * BLOCK                     # render_pcm's docstring
    r.reset()
    r.render_pcm(x, rows=rows)                                              # 16 chunks
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == m4
    r.reset()
    r.render_pcm(pcm_noise(24, K, 8 * BLOCK, 8701), rows=rows[:, :4], out_bits=32)      # another width in, the widest out
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == m4


# ---- 7. files -------------------------------------------------------------------------------------------------------------------
LENS = [1400, 2048, 700]


def _write_inputs(tmp_path, bits, tag, extensible=None):
    rng = np.random.default_rng(90 + bits)
    ints = [rng.integers(-(1 << (bits - 2)), 1 << (bits - 2), (n, K), dtype=np.int64) for n in LENS]
    paths = []
    for s, v in enumerate(ints):
        p = tmp_path / f"{tag}{s}.wav"
        raw = to_pcm(v, bits).tobytes()
        if s == extensible:
            p.write_bytes(extensible_wav(raw, K, bits, rate=int(FS), extra=[(b"LIST", b"INFOabc")]))
        else:
            with wave.open(str(p), "wb") as w:
                w.setnchannels(K); w.setsampwidth(bits // 8); w.setframerate(int(FS))
                w.writeframes(raw)
        paths.append(p)
    return paths, ints


def _read_outputs(paths):
    got = []
    for p in paths:
        with wave.open(str(p), "rb") as w:
            got.append(((w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()), w.readframes(w.getnframes())))
    return got


def _tracks():
    from open_headstage_amd import HeadTrack
    T = 2048 / FS
    return [HeadTrack([0.0, T], [-20.0, 20.0]), HeadTrack([0.0, T], [15.0, -15.0]), HeadTrack([0.0, T / 4], [0.0, 20.0])]


@pytest.mark.parametrize("bits,out_bits", [(16, None), (24, None), (24, 16)])
def test_render_files_pcm_path_writes_the_bytes_of_the_float_path(lib, table, tmp_path, monkeypatch, bits, out_bits):
    from open_headstage_amd import render_files, session
    monkeypatch.setattr(session, "CALL_CHUNKS", 2)              # two calls of two chunks each
    ins, ints = _write_inputs(tmp_path, bits, "in", extensible=1 if bits == 24 else None)
    r = _layout_renderer(lib, table, 1)
    outs_f = [tmp_path / f"float{s}.wav" for s in range(S)]
    outs_p = [tmp_path / f"pcm{s}.wav" for s in range(S)]
    written_f = render_files(ins, outs_f, r, _tracks(), ring_out=True, out_bits=out_bits, pcm=False)
    assert r.link_bytes == (4 * S * K * 5 * BLOCK, 4 * S * 2 * 5 * BLOCK)   # 2 048 frames + the reach: five chunks of floats
    written_p = render_files(ins, outs_p, r, _tracks(), ring_out=True, out_bits=out_bits)
    w_in, w_out = bits // 8, (out_bits or bits) // 8
    assert r.link_bytes == (w_in * S * K * 2048, w_out * S * 2 * (2048 + TAPS - 1))     # the files' own bytes and no more
    assert written_f == written_p == [n + TAPS - 1 for n in LENS]
    got_f, got_p = _read_outputs(outs_f), _read_outputs(outs_p)
    # ... against the host encode of render on the padded array, the check of tests/test_gpu_session.py
    xpad = np.zeros((S, K, 2048), np.float32)
    for s, v in enumerate(ints):
        xpad[s, :, :LENS[s]] = (v.T / float(1 << (bits - 1))).astype(np.float32)
    r.reset()
    y = r.render(xpad, yaw=_tracks(), final=True, ring_out=True)
    for s in range(S):
        n = LENS[s] + TAPS - 1
        assert got_p[s][0] == got_f[s][0] == (2, w_out, int(FS), n)
        assert got_p[s][1] == got_f[s][1], f"output {s}: the two paths differ"
        assert got_p[s][1] == session.pcm_encode(y[s, :, :n], 8 * w_out), f"output {s} against the host encode"
    # without the reach, and pcm=True said aloud: every output ends where its input ends
    assert render_files(ins, outs_p, r, _tracks(), ring_out=False, pcm=True) == LENS
    r.reset()
    y = r.render(xpad, yaw=_tracks(), final=True)
    assert [g[1] for g in _read_outputs(outs_p)] == [session.pcm_encode(y[s, :, :LENS[s]], bits) for s in range(S)]


def test_render_files_with_mixed_widths_falls_back_or_refuses(lib, table, tmp_path, monkeypatch):
    from open_headstage_amd import render_files, session
    monkeypatch.setattr(session, "CALL_CHUNKS", 2)
    in16, _ = _write_inputs(tmp_path, 16, "a")
    in24, _ = _write_inputs(tmp_path, 24, "b")
    ins = [in16[0], in24[1], in16[2]]
    r = _layout_renderer(lib, table, 1)
    outs_f = [tmp_path / f"float{s}.wav" for s in range(S)]
    outs_d = [tmp_path / f"default{s}.wav" for s in range(S)]
    written = render_files(ins, outs_f, r, _tracks(), pcm=False)
    assert render_files(ins, outs_d, r, _tracks()) == written == [n + TAPS - 1 for n in LENS]
    assert r.link_bytes[0] == 4 * S * K * 5 * BLOCK             # (floats crossed the link: the fallback)
    got_f, got_d = _read_outputs(outs_f), _read_outputs(outs_d)
    assert got_f == got_d and [g[0][1] for g in got_d] == [2, 3, 2]
    with pytest.raises(ValueError):
        render_files(ins, outs_d, r, _tracks(), pcm=True)
    with pytest.raises(ValueError):
        render_files(in16, outs_d, r, _tracks(), out_bits=12)
    bad = tmp_path / "float.wav"
    guid = struct.pack("<H", 3) + bytes.fromhex("000000001000800000aa00389b71")
    bad.write_bytes(extensible_wav(bytes(K * 4 * 10), K, 32, rate=int(FS), guid=guid))
    with pytest.raises(ValueError):
        render_files([in16[0], bad, in16[2]], outs_d, r, _tracks())
    assert render_files(in16, outs_d, r, _tracks()) == written  # the renderer and the paths are usable behind the refusals


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_renderer_usable(lib, table):
    import torch
    x = pcm_noise(16, K, 4 * BLOCK, 8800)
    rows = make_rows(S, 2, N_SETS)
    want = _layout_renderer(lib, table, 4).render_pcm(x, rows=rows)
    r = _layout_renderer(lib, table, 4)
    with pytest.raises(TypeError):
        r.render_pcm(host_decode(x, 16), rows=rows)             # float audio is render()'s
    with pytest.raises(TypeError):
        r.render_pcm(x.astype(np.float64), rows=rows)
    with pytest.raises(ValueError):
        r.render_pcm(np.zeros((S, 4 * BLOCK, K, 3), np.int16), rows=rows)   # int16 with a trailing axis of 3
    with pytest.raises(ValueError):
        r.render_pcm(np.zeros((S, 4 * BLOCK, K, 4), np.uint8), rows=rows)   # four bytes per sample
    with pytest.raises(ValueError):
        r.render_pcm(x.astype(np.int64), rows=rows)
    with pytest.raises(ValueError):
        r.render_pcm(x[:, :, :5], rows=rows)                    # a wrong channel count
    with pytest.raises(ValueError):
        r.render_pcm(np.ascontiguousarray(x.transpose(0, 2, 1)), rows=rows)         # planar
    with pytest.raises(ValueError):
        r.render_pcm(x[:2], rows=rows)                          # a wrong stream count
    with pytest.raises(ValueError):
        r.render_pcm(x, rows=rows, out_bits=12)
    with pytest.raises(ValueError):
        r.render_pcm(x, rows=rows, out=np.zeros((S, 4 * BLOCK, 2), np.int32))       # an out of the wrong dtype
    with pytest.raises(ValueError):
        r.render_pcm(x, rows=rows, out=np.zeros((S, 4 * BLOCK, 2), np.int16), out_bits=24)
    with pytest.raises(ValueError):
        r.render_pcm(x, rows=rows, out=np.zeros((S, 4 * BLOCK + 1, 2), np.int16))
    with pytest.raises(ValueError):
        r.render_pcm(x, rows=rows, out=torch.zeros((S, 4 * BLOCK, 2), dtype=torch.int16))   # a tensor for a numpy call
    with pytest.raises((ValueError, TypeError)):
        r.render_pcm(x, rows=rows, out=np.zeros((S, 4 * BLOCK, 2), np.float32))
    with pytest.raises(ValueError):
        r.render_pcm(x[:, :3 * BLOCK], rows=rows)               # off the segment grid, as render refuses it
    with pytest.raises(ValueError):
        r.render_pcm(x)                                         # neither yaw nor rows
    assert r.position_blocks == 0 and r.link_bytes == (0, 0)    # nothing was queued
    same_bytes(r.render_pcm(x, rows=rows), want, "the valid call behind the refused ones")

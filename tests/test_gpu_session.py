"""SessionRenderer: host audio of any length and head yaw per stream -> binaural audio, cut into pipelined chunks.

The yardstick is never the code under test: EXISTING entry points driven by hand on a second handle, the f64 models of
tests/test_cpu_ir_crossfade.py and tests/test_cpu_layout_schedule.py (imported, not restated), or brute-force numpy.  Bars: bit for
bit where the header promises bits or where the same calls are issued by hand, 1e-6 relative RMS per stream -- the project's FFT
bar, DESIGN section 2 -- everywhere else.  Plan 1, gain 0.7; three streams, 24-tap responses, five sets, a row per stream that
changes in every segment, unless said otherwise.

Measured on an MI355X (worst stream, relative RMS): see DESIGN section 4.5g."""
import wave

import numpy as np
import pytest

from tests.test_cpu_ir_crossfade import model_ir_crossfade
from tests.test_cpu_ir_schedule import RING_OUT, make_rows, make_sets, model_ir_schedule
from tests.test_cpu_layout import BAR, BLOCK, make_input, rel_rms_per_stream
from tests.test_cpu_layout_schedule import make_table, model_layout_schedule_f64
from tests.test_gpu_layout import GAIN, NB, _batch, _eq_bands, _oracle_eq, _same_bits, _within_bar
from tests.test_gpu_layout import _run as _run_layout

pytestmark = pytest.mark.gpu

S = 3
TAPS = 24
N_SETS = 5
K = 6
GRID = np.array([-20.0, -10.0, 0.0, 10.0, 20.0])
FS = 48000.0
# the planner's cuts of 11 blocks at seg_blocks 2 (pinned in tests/test_cpu_session.py), written out: (start, blocks, g)
CUTS = {4: [(0, 4, 2), (4, 4, 2), (8, 3, 2)], 3: [(0, 3, 1), (3, 3, 1), (6, 3, 1), (9, 2, 1)]}


@pytest.fixture(scope="module")
def lib():
    from open_headstage_amd import _ffi
    return _ffi.lib()


@pytest.fixture(scope="module")
def table():
    return make_table(N_SETS, K, TAPS)


@pytest.fixture(scope="module")
def sets():
    return make_sets(N_SETS, TAPS)


def _layout_renderer(lib, table, chunk, fade=True, streams=S, seg=2):
    import open_headstage_amd as ohs
    r = ohs.SessionRenderer.layout(streams, table, GRID, seg_blocks=seg, chunk_blocks=chunk, crossfade=fade, fs=FS, num_bands=NB,
                                   library=lib)
    r.batch.set_conv_plan(1)
    r.set_gain(GAIN)
    return r


def _stereo_renderer(lib, sets, chunk, fade=True, late=None, streams=S, grid=GRID):
    import open_headstage_amd as ohs
    r = ohs.SessionRenderer.stereo(streams, sets, grid, late_irs=late, seg_blocks=2, chunk_blocks=chunk, crossfade=fade, fs=FS,
                                   num_bands=NB, library=lib)
    r.batch.set_conv_plan(1)
    r.set_gain(GAIN)
    return r


def _stereo_input(streams, blocks, seed):
    from open_headstage_amd import synth
    return synth.white_noise(range(seed, seed + streams), blocks * BLOCK)


def _three_bands(target):
    """synth's table with its first three bands enabled, through target's setters"""
    for i, (c, _) in enumerate(_eq_bands()):
        target.set_band_coeffs(i, c, i < 3)
    target.set_eq_enabled(True)


# ---- 1. layouts: the whole session against ONE call of the existing entry ---------------------------------------------------------
@pytest.mark.parametrize("fade", [True, False])
def test_layout_session_is_one_scheduled_call_bit_for_bit(lib, table, fade):
    """11 blocks, seg_blocks 2: chunks of 4 run with g = 2, chunks of 3 with g = 1 and segments that straddle the cuts; the last
    call is short.  The header promises bits that do not depend on the cuts."""
    import torch
    x = make_input(S, K, 11, seed=7000)
    rows = make_rows(S, 6, N_SETS)
    ref = _batch(lib, None, S)
    ref.set_layout_table(table)
    want = ref.process_layout_scheduled(torch.from_numpy(x.copy()).cuda(), rows, 2, None, fade)
    torch.cuda.synchronize()
    want = want.cpu().numpy()
    for chunk in (4, 3):
        r = _layout_renderer(lib, table, chunk, fade)
        y = r.render(x, rows=rows, final=True)
        assert isinstance(y, np.ndarray) and y.dtype == np.float32 and r.position_blocks == 11
        assert r.batch.last_layout_scheduled()
        _same_bits(y, want, f"layout session in chunks of {chunk}, crossfade {fade}")


# ---- 2. stereo: the planner's calls issued by hand on a second handle, and the f64 model ------------------------------------------
def _by_hand(lib, sets, x, rows, cuts, eq):
    import open_headstage_amd as ohs
    import torch
    ref = ohs.BatchProcessor(S, num_bands=NB, library=lib)
    ref.set_conv_plan(1)
    ref.set_gain(GAIN)
    ref.set_schedule_irs(sets)
    if eq:
        _three_bands(ref)
    per_block = np.repeat(rows, 2, axis=1)                      # the session's set of every block
    out = []
    for start, n, g in cuts:
        idx = np.ascontiguousarray(per_block[:, start:start + n:g])
        prev = None if start == 0 else np.ascontiguousarray(per_block[:, start - 1])
        d = torch.from_numpy(np.ascontiguousarray(x[:, :, start * BLOCK:(start + n) * BLOCK])).cuda()
        ref.process_ir_crossfaded_ptr(d.data_ptr(), d.data_ptr(), n, 2 * n * BLOCK, n * BLOCK, g, idx, prev,
                                      torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out.append(d.cpu().numpy())
    return np.concatenate(out, axis=2)


@pytest.mark.parametrize("chunk", [4, 3])
def test_stereo_session_is_the_hand_driven_sequence_bit_for_bit(lib, oracle, sets, chunk):
    x = _stereo_input(S, 11, 7100)
    rows = make_rows(S, 6, N_SETS)
    r = _stereo_renderer(lib, sets, chunk)
    _three_bands(r)
    y = r.render(x, rows=rows, final=True)
    assert r.batch.last_conv_ir_crossfaded()
    _same_bits(y, _by_hand(lib, sets, x, rows, CUTS[chunk], True), f"stereo session in chunks of {chunk}, EQ on")
    r = _stereo_renderer(lib, sets, chunk)
    y = r.render(x, rows=rows, final=True)
    _same_bits(y, _by_hand(lib, sets, x, rows, CUTS[chunk], False), f"stereo session in chunks of {chunk}, EQ off")
    ref, _ = model_ir_crossfade(oracle, x, sets, rows, 2)
    _within_bar(y, GAIN * ref, f"stereo session in chunks of {chunk} against the f64 model")


def test_stereo_session_without_crossfade_against_the_ring_out_model(lib, oracle, sets):
    x = _stereo_input(S, 11, 7150)
    rows = make_rows(S, 6, N_SETS)
    r = _stereo_renderer(lib, sets, 3, fade=False)
    y = r.render(x, rows=rows, final=True)
    assert r.batch.last_conv_ir_scheduled() and not r.batch.last_conv_ir_crossfaded()
    ref, _ = model_ir_schedule(oracle, x, sets, rows, 2, RING_OUT)
    _within_bar(y, GAIN * ref, "stereo session, crossfade off")


# ---- 3. two render calls and a ragged final one -----------------------------------------------------------------------------------
def test_two_renders_and_a_ragged_final_equal_one_render(lib, oracle, table):
    frames = 10 * BLOCK + 300
    x = make_input(S, K, 11, seed=7200)[:, :, :frames]
    rows = make_rows(S, 6, N_SETS)
    one = _layout_renderer(lib, table, 4).render(x, rows=rows, final=True, ring_out=True)
    assert one.shape == (S, 2, frames + TAPS - 1)
    r = _layout_renderer(lib, table, 4)
    assert r.reach == TAPS - 1
    a = r.render(np.ascontiguousarray(x[:, :, :6 * BLOCK]), rows=rows[:, :3])          # (fills both staging pairs with noise)
    assert a.shape == (S, 2, 6 * BLOCK) and r.position_blocks == 6
    b = r.render(np.ascontiguousarray(x[:, :, 6 * BLOCK:]), rows=rows[:, 3:], final=True, ring_out=True)
    assert b.shape == (S, 2, 4 * BLOCK + 300 + TAPS - 1) and r.position_blocks == 11
    _same_bits(np.concatenate([a, b], axis=2), one, "6 blocks, then 4 blocks + 300 frames, against one render")
    # ... and that render is the model on the zero-padded input: whatever the staging buffers held behind the ragged end stayed there
    xpad = np.zeros((S, K, 11 * BLOCK), np.float32)
    xpad[:, :, :frames] = x
    ref = model_layout_schedule_f64(oracle, xpad, table, rows, 2, None, True, GAIN)
    _within_bar(one, ref[:, :, :frames + TAPS - 1], "ragged final render against the f64 model")
    tail = ref[:, :, frames:frames + TAPS - 1]
    assert (np.abs(one[:, :, frames:] - tail).max(axis=(1, 2)) <= 1e-5 * np.abs(ref).max()).all()
    assert (ref[:, :, frames + TAPS - 1:] == 0).all()           # (the reach is exactly TAPS - 1 frames)
    with pytest.raises(ValueError):
        r.render(x[:, :, :2 * BLOCK], rows=rows[:, :1])         # the session is over
    r.reset()
    _same_bits(r.render(x, rows=rows, final=True, ring_out=True), one, "behind reset()")


# ---- 4. both staging pairs turn over, pinned input -------------------------------------------------------------------------------
def test_nine_chunks_turn_the_staging_over_and_a_pinned_tensor_gives_the_same_bits(lib, oracle, table):
    import torch
    blocks = 18
    x = make_input(S, K, blocks, seed=7300)                     # distinct noise in every chunk
    rows = make_rows(S, 9, N_SETS)
    r = _layout_renderer(lib, table, 2)
    y = r.render(x, rows=rows)
    ref = model_layout_schedule_f64(oracle, x, table, rows, 2, None, True, GAIN)
    for c in range(9):
        sl = slice(c * 2 * BLOCK, (c + 1) * 2 * BLOCK)
        err = rel_rms_per_stream(y[:, :, sl], ref[:, :, sl])
        assert (err <= BAR).all(), f"chunk {c}: relative RMS per stream {err}"
    _within_bar(y, ref, "nine chunks of two blocks")
    r.reset()
    xp = torch.from_numpy(x.copy()).pin_memory()
    yp = r.render(xp, rows=rows)
    assert isinstance(yp, torch.Tensor) and not yp.is_cuda
    _same_bits(yp.numpy(), y, "a pinned tensor through nine chunks")
    big = _layout_renderer(lib, table, 32)                      # one chunk: the pinned tensor is copied to the device as it is
    _same_bits(big.render(xp, rows=rows).numpy(), y, "a pinned tensor in one chunk")


# ---- 5. the late part -------------------------------------------------------------------------------------------------------------
def _late_irs(L=988):
    rng = np.random.default_rng(77)
    k = np.arange(L, dtype=np.float64)
    return (0.02 * rng.standard_normal((4, L)) * np.exp(-k / 400.0)).astype(np.float32)


def _late_model(oracle, x, late):
    """gain * (x conv (zeros(512) ++ late)) in f64 by direct convolution: Lsl, Rsl -> left ear, Lsr, Rsr -> right ear"""
    full = np.concatenate([np.zeros((4, BLOCK), np.float32), late], axis=1)
    y = np.zeros(x.shape, np.float64)
    for s in range(x.shape[0]):
        for p, (src, ear) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
            y[s, ear] += oracle.direct_conv_f64(np.ascontiguousarray(x[s, src]), np.ascontiguousarray(full[p]))
    return GAIN * y


@pytest.mark.parametrize("eq", [False, True])
def test_late_part_against_the_f64_model(lib, oracle, eq):
    streams, n_sets = 2, 3
    head = make_sets(n_sets, 64)
    late = _late_irs()
    x = _stereo_input(streams, 9, 7400)
    rows = make_rows(streams, 5, n_sets)
    r = _stereo_renderer(lib, head, 3, late=late, streams=streams, grid=GRID[:n_sets])
    assert r.reach == BLOCK + 988 - 1 and r.late_batch is not None
    if eq:
        for i, (c, en) in enumerate(_eq_bands()):
            r.set_band_coeffs(i, c, en)
        r.set_eq_enabled(True)
    y = r.render(x, rows=rows, final=True)
    assert r.late_batch.last_conv_plan()[0] != "block512_p1", r.late_batch.last_conv_plan()      # (a long-response plan served it)
    xe = _oracle_eq(oracle, x)[0] if eq else x                   # the EQ is bit-exact and runs in front of both convolutions
    ref_head, _ = model_ir_crossfade(oracle, xe, head, rows, 2)
    ref = GAIN * ref_head + _late_model(oracle, xe, late)
    assert (rel_rms_per_stream(ref, GAIN * ref_head) > 1e-3).all()       # (the late part is far above the bar)
    _within_bar(y, ref, f"head + late, EQ {'on' if eq else 'off'}")


# ---- 6. device memory does not grow with the session -----------------------------------------------------------------------------
def test_device_memory_does_not_depend_on_the_session_length(lib, table):
    import torch
    r = _layout_renderer(lib, table, 2)
    x = make_input(S, K, 32, seed=7500)
    rows = make_rows(S, 16, N_SETS)
    r.render(np.ascontiguousarray(x[:, :, :8 * BLOCK]), rows=rows[:, :4])
    torch.cuda.synchronize()
    m4 = torch.cuda.memory_allocated()
    r.reset()
    r.render(x, rows=rows)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == m4 and m4 > 0


# ---- 7. yaw in, sets out ----------------------------------------------------------------------------------------------------------
def test_yaw_tracks_are_their_rows_and_a_still_head_takes_the_plain_kernel(lib, table):
    from open_headstage_amd import HeadTrack, yaw_rows
    blocks = 12
    x = make_input(S, K, blocks, seed=7600)
    T = blocks * BLOCK / FS
    tracks = [HeadTrack([0.0, T], [-24.0, 24.0]), HeadTrack([0.0, T / 2, T], [20.0, -20.0, 14.0]), HeadTrack([0.0, T], [170.0, 190.0 + 360.0])]
    rows = yaw_rows(tracks, 0, blocks, 2, FS, GRID)
    assert rows.shape == (S, 6) and all(len(set(row.tolist())) >= 3 for row in rows[:2])
    r = _layout_renderer(lib, table, 4)
    y = r.render(x, yaw=tracks)
    assert r.batch.last_layout_scheduled()
    r.reset()
    _same_bits(r.render(x, rows=rows), y, "yaw= per-stream tracks against rows=yaw_rows(...)")
    r.reset()
    deg = np.stack([tr.at(np.arange(6) * 2 * BLOCK / FS) for tr in tracks])
    _same_bits(r.render(x, yaw=deg), y, "yaw= degrees per segment")
    # a head that sits between two grid yaws all session: one shared constant row, the plain layout kernel on that set
    r.reset()
    still = r.render(x, yaw=HeadTrack([0.0, 1.0], [4.0, 4.9]))
    assert not r.batch.last_layout_scheduled()
    _same_bits(still, _run_layout(_batch(lib, table[2], S), x), "a still head against process_layout on set 2")


# ---- 8. files ---------------------------------------------------------------------------------------------------------------------
def test_render_files_is_the_encode_of_render_on_the_padded_array(lib, table, tmp_path, monkeypatch):
    from open_headstage_amd import HeadTrack, render_files, session
    monkeypatch.setattr(session, "CALL_CHUNKS", 2)              # two render calls of two chunks each
    from open_headstage_amd.session import pcm_encode
    lens = [1400, 2048, 700]
    rng = np.random.default_rng(5)
    ints = [rng.integers(-12000, 12000, (K, n), dtype=np.int64) for n in lens]
    ins, outs = [], []
    for s, v in enumerate(ints):
        p = tmp_path / f"in{s}.wav"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(K); w.setsampwidth(2); w.setframerate(int(FS))
            w.writeframes(np.ascontiguousarray(v.T).astype("<i2").tobytes())
        ins.append(p)
        outs.append(tmp_path / f"out{s}.wav")
    T = 2048 / FS
    tracks = [HeadTrack([0.0, T], [-20.0, 20.0]), HeadTrack([0.0, T], [15.0, -15.0]), HeadTrack([0.0, T / 4], [0.0, 20.0])]
    r = _layout_renderer(lib, table, 1)
    written = render_files(ins, outs, r, tracks, ring_out=True)
    assert written == [n + TAPS - 1 for n in lens]
    xpad = np.zeros((S, K, 2048), np.float32)
    for s, v in enumerate(ints):
        xpad[s, :, :lens[s]] = (v / 32768.0).astype(np.float32)
    r.reset()
    y = r.render(xpad, yaw=tracks, final=True, ring_out=True)
    assert float(np.abs(y).max()) > 0.01
    for s, p in enumerate(outs):
        with wave.open(str(p), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (2, 2, int(FS), lens[s] + TAPS - 1)
            raw = w.readframes(w.getnframes())
        assert raw == pcm_encode(y[s, :, :lens[s] + TAPS - 1], 16), f"output {s}"


# ---- 9. refusals leave the renderer usable ---------------------------------------------------------------------------------------
def test_refusals_are_value_errors_and_leave_the_renderer_usable(lib, table, sets, tmp_path):
    import open_headstage_amd as ohs
    from open_headstage_amd import render_files
    x = make_input(S, K, 4, seed=7700)
    rows = make_rows(S, 2, N_SETS)
    twin = _layout_renderer(lib, table, 4)
    want = twin.render(x, rows=rows)
    r = _layout_renderer(lib, table, 4)
    with pytest.raises(ValueError):
        r.render(x[:, :, :3 * BLOCK], rows=rows)                # a non-final call off the segment grid
    with pytest.raises(ValueError):
        r.render(x[:, :, :4 * BLOCK - 7], rows=rows)
    with pytest.raises(ValueError):
        r.render(x, yaw=np.zeros(2), rows=rows)                 # both
    with pytest.raises(ValueError):
        r.render(x)                                             # neither
    with pytest.raises(ValueError):
        r.render(x[:, :5], rows=rows)                           # a wrong channel count
    with pytest.raises(ValueError):
        r.render(x[:, :2], rows=rows)
    with pytest.raises(ValueError):
        r.render(x[:2], rows=rows)                              # a wrong stream count
    with pytest.raises(ValueError):
        r.render(x, rows=rows[:, :1])                           # too few segments
    bad = rows.copy(); bad[1, 1] = N_SETS
    with pytest.raises(ValueError):
        r.render(x, rows=bad)                                   # an index beyond the table
    with pytest.raises(ValueError):
        ohs.SessionRenderer.layout(S, table, GRID, late_irs=np.zeros((4, 100), np.float32), library=lib)      # late part, layout mode
    with pytest.raises(ValueError):
        ohs.SessionRenderer.layout(S, table, GRID[:4], library=lib)                    # a grid that is not the table's
    st = _stereo_renderer(lib, sets, 4)
    with pytest.raises(ValueError):
        st.render(x, rows=rows)                                 # six channels into the stereo mode
    p = tmp_path / "in.wav"
    with wave.open(str(p), "wb") as w:
        w.setnchannels(K); w.setsampwidth(2); w.setframerate(44100)
        w.writeframes(np.zeros((100, K), "<i2").tobytes())
    with pytest.raises(ValueError):
        render_files([p] * S, [tmp_path / f"o{s}.wav" for s in range(S)], r)           # a file rate different from fs
    assert r.position_blocks == 0
    _same_bits(r.render(x, rows=rows), want, "the valid call behind the refused ones")
    sx = _stereo_input(S, 4, 7750)
    _same_bits(st.render(sx, rows=rows), _stereo_renderer(lib, sets, 4).render(sx, rows=rows), "the stereo renderer behind its refusal")

"""ohs_batch_process_layout_scheduled: a table of speaker layouts walked per stream and segment inside one kernel, with a crossfade
over the first block of every segment that changes the set.

The yardstick is never the code under test: the f64 model of tests/test_cpu_layout_schedule.py (checked there against the layout
model and the stereo crossfade model), the oracle's StereoParametricEQ, or EXISTING entry points on a second handle --
ohs_batch_process_layout, ohs_batch_process_ir_scheduled, ohs_batch_process_ir_crossfaded.  Bars: bit for bit where the header
promises bits, 1e-6 relative RMS per stream -- the project's FFT bar, DESIGN section 2 -- everywhere else.  Plan 1, gain 0.7,
five streams, 13 blocks unless said otherwise."""
import ctypes as C

import numpy as np
import pytest

from tests.test_cpu_ir_schedule import make_rows
from tests.test_cpu_ir_crossfade import fade_plan
from tests.test_cpu_layout import BAR, BLOCK, make_input, make_layout, model_layout_f64, rel_rms_per_stream
from tests.test_cpu_layout_schedule import CROSSFADE, RING_OUT, make_table, model_layout_schedule_f64
from tests.test_gpu_layout import GAIN, NB, S, _batch, _eq_bands, _oracle_eq, _same_bits, _within_bar  # noqa: F401
from tests.test_gpu_layout import _run as _run_layout

pytestmark = pytest.mark.gpu

BLOCKS = 13
N_SETS = 5


@pytest.fixture(scope="module")
def lib():
    from open_headstage_amd import _ffi
    return _ffi.lib()


def _handle(lib, table=None, streams=S, eq=False):
    bp = _batch(lib, None, streams, eq)
    if table is not None:
        bp.set_layout_table(table)
    return bp


def _run(bp, x, idx, seg_blocks, prev=None, crossfade=True):
    import torch
    y = bp.process_layout_scheduled(torch.from_numpy(np.ascontiguousarray(x).copy()).cuda(), idx, seg_blocks, prev, crossfade)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _stereo_handle(lib, sets, streams=S):
    """a second handle for the EXISTING stereo schedule calls: plan 1, the same gain, the set table [n_sets][4][len]"""
    import open_headstage_amd as ohs
    bp = ohs.BatchProcessor(streams, num_bands=NB, library=lib)
    bp.set_conv_plan(1)
    bp.set_gain(GAIN)
    bp.set_schedule_irs(sets)
    return bp


# ---- a. a shared constant row is the layout call on that set, served by its kernel ----------------------------------------------
def test_shared_constant_row_is_the_layout_call_bit_for_bit(lib):
    K = 6
    table = make_table(N_SETS, K)
    x = make_input(S, K, BLOCKS, seed=4000)
    want = _run_layout(_batch(lib, table[3]), x)
    for prev, fade in [(None, True), (3, True), (1, False)]:
        bp = _handle(lib, table)
        y = _run(bp, x, np.full(7, 3, np.uint32), 2, prev, fade)
        assert not bp.last_layout_scheduled() and bp.last_layout_launch()[0] == 3
        _same_bits(y, want, f"shared constant row, prev {prev}, crossfade {fade}")


# ---- b. constant rows per stream: every stream its own set, the scheduled kernel, the layout call's bits ------------------------
@pytest.mark.parametrize("fade", [True, False])
def test_constant_rows_per_stream_have_the_layout_calls_bits(lib, fade):
    K = 6
    table = make_table(N_SETS, K)
    x = make_input(S, K, BLOCKS, seed=4100)
    row = np.array([2, 0, 4, 1, 3], np.uint32)
    idx = np.repeat(row[:, None], 7, axis=1)
    bp = _handle(lib, table)
    y = _run(bp, x, idx, 2, row if fade else None, fade)
    assert bp.last_layout_scheduled() and bp.last_layout_launch()[0] == 3
    for j in sorted(set(int(v) for v in row)):
        want = _run_layout(_batch(lib, table[j]), x)
        for s in np.flatnonzero(row == j):
            _same_bits(y[s:s + 1], want[s:s + 1], f"stream {s} on set {j}")


# ---- c. two channels under RING_OUT: the bits of the IR-scheduled stereo call ----------------------------------------------------
@pytest.mark.parametrize("seg_blocks", [2, 3])
def test_two_channels_ring_out_are_the_ir_scheduled_call_bit_for_bit(lib, seg_blocks):
    table = make_table(N_SETS, 2)
    x = make_input(S, 2, BLOCKS, seed=4200)
    idx = make_rows(S, -(-BLOCKS // seg_blocks), N_SETS)
    ref = _stereo_handle(lib, table.reshape(N_SETS, 4, -1))      # [Lsl, Lsr, Rsl, Rsr] = [0][0], [0][1], [1][0], [1][1]
    import torch
    want = ref.process_ir_scheduled(torch.from_numpy(x.copy()).cuda(), seg_blocks, idx, "ring_out")
    torch.cuda.synchronize()
    assert ref.last_conv_ir_scheduled()
    bp = _handle(lib, table)
    y = _run(bp, x, idx, seg_blocks, None, False)
    assert bp.last_layout_scheduled()
    _same_bits(y, want.cpu().numpy(), f"K = 2 RING_OUT, seg_blocks {seg_blocks}")


# ---- d. against the f64 model ----------------------------------------------------------------------------------------------------
def _against_model(lib, oracle, K, taps, seg_blocks, with_prev=True, shared=False, fade=True, seed=4300):
    table = make_table(N_SETS, K, taps)
    x = make_input(S, K, BLOCKS, seed=seed)
    n_segs = -(-BLOCKS // seg_blocks)
    idx = make_rows(S, n_segs, N_SETS)
    prev = (idx[:, 0] + 2) % N_SETS if with_prev else None
    if shared:
        idx = idx[1]
        prev = int(prev[1]) if with_prev else None
    bp = _handle(lib, table)
    y = _run(bp, x, idx, seg_blocks, prev, fade)
    assert bp.last_layout_scheduled() and bp.last_layout_launch()[0] == (K + 1) // 2
    ref = model_layout_schedule_f64(oracle, x, table, idx, seg_blocks, prev, fade, GAIN)
    _within_bar(y, ref, f"K = {K}, {taps} taps, seg_blocks {seg_blocks}, prev {with_prev}, shared {shared}, crossfade {fade}")


@pytest.mark.parametrize("K,taps", [(1, 512), (3, 512), (6, 512), (8, 512), (16, 512), (6, 1), (6, 200)])
def test_crossfaded_layouts_against_the_f64_model(lib, oracle, K, taps):
    _against_model(lib, oracle, K, taps, 2)


@pytest.mark.parametrize("seg_blocks", [1, 5])
def test_every_block_fading_and_long_segments_against_the_f64_model(lib, oracle, seg_blocks):
    _against_model(lib, oracle, 6, 512, seg_blocks)


def test_without_prev_idx_against_the_f64_model(lib, oracle):
    _against_model(lib, oracle, 6, 512, 2, with_prev=False)


def test_shared_row_against_the_f64_model(lib, oracle):
    _against_model(lib, oracle, 6, 512, 2, shared=True)


def test_ring_out_against_the_f64_model(lib, oracle):
    _against_model(lib, oracle, 6, 512, 2, fade=False)


# ---- e. two channels under CROSSFADE against the existing stereo crossfade ----------------------------------------------------------
def test_two_channels_crossfade_against_the_ir_crossfaded_call(lib):
    """Within the bar, NOT bit for bit: ohs_batch_process_ir_crossfaded runs a fading block as two blocks and sums two inverse
    transforms in the time domain, this call sums the two products in the spectrum in front of one inverse transform."""
    import torch
    table = make_table(N_SETS, 2)
    x = make_input(S, 2, BLOCKS, seed=4400)
    idx = make_rows(S, 7, N_SETS)
    prev = (idx[:, 0] + 1) % N_SETS
    ref = _stereo_handle(lib, table.reshape(N_SETS, 4, -1))
    want = ref.process_ir_crossfaded(torch.from_numpy(x.copy()).cuda(), 2, idx, prev)
    torch.cuda.synchronize()
    assert ref.last_conv_ir_crossfaded()
    bp = _handle(lib, table)
    _within_bar(_run(bp, x, idx, 2, prev), want.cpu().numpy(), "K = 2 CROSSFADE against ohs_batch_process_ir_crossfaded")


# ---- f. the bits do not depend on where the signal is cut into calls ---------------------------------------------------------------
def test_call_cuts_do_not_change_the_bits(lib):
    K = 6
    table = make_table(N_SETS, K)
    x = make_input(S, K, BLOCKS, seed=4500)
    idx = make_rows(S, 7, N_SETS)
    prev0 = (idx[:, 0] + 1) % N_SETS
    whole = _run(_handle(lib, table), x, idx, 2, prev0)
    bp = _handle(lib, table)
    out, pos = [], 0
    for nb in [2, 4, 6, 1]:                 # (cuts at segment boundaries)
        k0 = pos // 2
        out.append(_run(bp, x[:, :, pos * BLOCK:(pos + nb) * BLOCK], np.ascontiguousarray(idx[:, k0:]), 2,
                        prev0 if pos == 0 else np.ascontiguousarray(idx[:, k0 - 1])))
        pos += nb
    assert pos == BLOCKS
    _same_bits(np.concatenate(out, axis=2), whole, "2 + 4 + 6 + 1 blocks against 13")


# ---- g. ... nor on the number of chunks per stream ---------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_blocks", [3, 5])
def test_chunks_per_stream_do_not_change_the_bits(lib, seg_blocks):
    K, streams, blocks = 6, 2, 40
    table = make_table(N_SETS, K)
    x = make_input(streams, K, blocks, seed=4600)
    idx = make_rows(streams, -(-blocks // seg_blocks), N_SETS)
    prev = (idx[:, 0] + 1) % N_SETS
    bp = _handle(lib, table, streams)
    whole = _run(bp, x, idx, seg_blocks, prev)
    assert bp.last_layout_scheduled() and bp.last_layout_launch()[1] > 1, bp.last_layout_launch()
    cur, old = fade_plan(streams, blocks, idx, seg_blocks, prev)
    one = _handle(lib, table, streams)
    single = [_run(one, x[:, :, t * BLOCK:(t + 1) * BLOCK], cur[:, t:t + 1].astype(np.uint32), 1, old[:, t].astype(np.uint32))
              for t in range(blocks)]
    assert one.last_layout_launch() == (3, 1)
    _same_bits(whole, np.concatenate(single, axis=2), f"2 streams x 40 blocks in chunks (seg_blocks {seg_blocks}) against forty 1-block calls")


# ---- h. odd K: the channel behind the last one is never read, fading or not ----------------------------------------------------------
@pytest.mark.parametrize("K", [3, 5])
def test_odd_layouts_do_not_read_the_channel_behind_the_last(lib, oracle, K):
    table = make_table(N_SETS, K)
    x = make_input(S, K, BLOCKS, seed=4700)
    xn = np.concatenate([x, np.full((S, 1, x.shape[2]), np.nan, np.float32)], axis=1)      # [S][K + 1][frames]
    idx = make_rows(S, 7, N_SETS)
    prev = (idx[:, 0] + 1) % N_SETS
    y = _run(_handle(lib, table), xn, idx, 2, prev)
    assert np.isfinite(y).all()
    _within_bar(y, model_layout_schedule_f64(oracle, x, table, idx, 2, prev, True, GAIN), f"K = {K} with a NaN channel behind it")


# ---- i. EQ on: the oracle's EQ on the ear signals of the same call ------------------------------------------------------------------
def test_eq_filters_the_ear_signals_after_the_convolution(lib, oracle):
    K = 6
    table = make_table(N_SETS, K)
    x = make_input(S, K, 12, seed=4800)
    idx = make_rows(S, 6, N_SETS)
    off, on = _handle(lib, table), _handle(lib, table, eq=True)
    pos, eqs = 0, None
    for call, nb in enumerate([4, 8]):
        xc = x[:, :, pos * BLOCK:(pos + nb) * BLOCK]
        rows = np.ascontiguousarray(idx[:, pos // 2:])
        prev = None if pos == 0 else np.ascontiguousarray(idx[:, pos // 2 - 1])
        dry = _run(off, xc, rows, 2, prev)
        ref, eqs = _oracle_eq(oracle, dry, eqs)
        got = _run(on, xc, rows, 2, prev)
        assert (rel_rms_per_stream(got, dry) > 1e-3).all()          # (the EQ does something)
        _same_bits(got, ref, f"EQ on, call {call}")
        pos += nb


# ---- j. state ----------------------------------------------------------------------------------------------------------------------
def test_layout_call_and_scheduled_call_continue_one_another(lib, oracle):
    K = 6
    table = make_table(N_SETS, K)
    x = make_input(S, K, BLOCKS, seed=4900)
    idx = make_rows(S, 4, N_SETS)
    prev = np.zeros(S, np.uint32)           # (the layout call in front ran on set 0)
    bp = _handle(lib, table)
    bp.set_layout_irs(table[0])
    bp.set_layout_table(table)              # (either order: the overlap is one)
    y1 = _run_layout(bp, x[:, :, :5 * BLOCK])
    assert not bp.last_layout_scheduled()
    y2 = _run(bp, x[:, :, 5 * BLOCK:], idx, 2, prev)
    assert bp.last_layout_scheduled()
    full_idx = np.concatenate([np.zeros((S, 5), np.uint32), np.repeat(idx, 2, axis=1)], axis=1)[:, :BLOCKS]
    ref = model_layout_schedule_f64(oracle, x, table, full_idx, 1, None, True, GAIN)
    _within_bar(np.concatenate([y1, y2], axis=2), ref, "process_layout, then the scheduled call")
    y3 = _run_layout(bp, x[:, :, :2 * BLOCK])      # ... and back: the scheduled call's overlap rings into the layout call
    tail_ref = model_layout_schedule_f64(oracle, np.concatenate([x, x[:, :, :2 * BLOCK]], axis=2), table,
                                         np.concatenate([full_idx, np.zeros((S, 2), np.uint32)], axis=1), 1, None, False, GAIN)
    _within_bar(y3, tail_ref[:, :, BLOCKS * BLOCK:], "the layout call behind the scheduled call")


def test_reset_and_a_new_upload_zero_the_overlap(lib):
    K = 6
    table, other = make_table(N_SETS, K), make_table(N_SETS, K, seed=50)
    x = make_input(S, K, 9, seed=5000)
    idx = make_rows(S, 5, N_SETS)
    fresh = _run(_handle(lib, table), x, idx, 2)
    bp = _handle(lib, table)
    _same_bits(_run(bp, x, idx, 2), fresh, "first call")
    again = _run(bp, x, idx, 2)             # (the overlap of the first call rings into this one)
    assert (rel_rms_per_stream(again[:, :, :BLOCK], fresh[:, :, :BLOCK]) > 1e-3).all()
    bp.reset()
    _same_bits(_run(bp, x, idx, 2), fresh, "behind ohs_batch_reset")
    bp.set_layout_table(other)
    bp.set_layout_table(table)
    _same_bits(_run(bp, x, idx, 2), fresh, "behind a second upload")
    bp.set_layout_table(other)
    _same_bits(_run(bp, x, idx, 2), _run(_handle(lib, other), x, idx, 2), "another table")
    # the single layout comes and goes beside the table; the table stays
    bp.set_layout_irs(table[1])
    bp.set_layout_irs(np.zeros((0, 2, 1), np.float32))
    _same_bits(_run(bp, x, idx, 2), _run(_handle(lib, other), x, idx, 2), "the table behind a freed single layout")


def test_scheduled_layout_and_stereo_calls_do_not_touch_each_other(lib):
    import torch
    from tests.test_cpu_ir_schedule import make_sets
    K = 6
    table = make_table(N_SETS, K)
    own = make_sets(1)[0]
    x = make_input(S, K, 14, seed=5100)
    xs = make_input(S, 2, 7, seed=5150)
    idx = make_rows(S, 7, N_SETS)

    def handle():
        bp = _handle(lib, table)
        for p in range(4):
            bp.set_ir(p, own[p])
        return bp

    def plain(bp):
        y = bp.process(torch.from_numpy(xs.copy()).cuda())
        torch.cuda.synchronize()
        return y.cpu().numpy()

    mixed, alone, stereo = handle(), handle(), handle()
    a1 = _run(mixed, x[:, :, :6 * BLOCK], np.ascontiguousarray(idx[:, :3]), 2)
    st = plain(mixed)
    a2 = _run(mixed, x[:, :, 6 * BLOCK:], np.ascontiguousarray(idx[:, 3:]), 2, np.ascontiguousarray(idx[:, 2]))
    st2 = plain(mixed)
    b1 = _run(alone, x[:, :, :6 * BLOCK], np.ascontiguousarray(idx[:, :3]), 2)
    b2 = _run(alone, x[:, :, 6 * BLOCK:], np.ascontiguousarray(idx[:, 3:]), 2, np.ascontiguousarray(idx[:, 2]))
    _same_bits(np.concatenate([a1, a2], axis=2), np.concatenate([b1, b2], axis=2), "scheduled, stereo, scheduled against the scheduled calls alone")
    _same_bits(st, plain(stereo), "the stereo call between the scheduled calls")
    _same_bits(st2, plain(stereo), "the second stereo call")


# ---- k. padded strides on both sides ------------------------------------------------------------------------------------------------
def test_padded_strides_and_untouched_padding(lib):
    import torch
    K, blocks = 6, 7
    table = make_table(N_SETS, K)
    x = make_input(S, K, blocks, seed=5200)
    idx = make_rows(S, 4, N_SETS)
    prev = (idx[:, 0] + 1) % N_SETS
    frames = blocks * BLOCK
    want = _run(_handle(lib, table), x, idx, 2, prev)
    in_cs, in_ss = frames + 96, (K + 1) * (frames + 96) + 32        # (a surplus channel's worth of room per stream: NaN there)
    out_cs, out_ss = frames + 160, 2 * (frames + 160) + 64
    SENT = np.float32(-777.25)
    xin = np.full(S * in_ss, np.nan, np.float32)
    for s in range(S):
        for c in range(K):
            xin[s * in_ss + c * in_cs: s * in_ss + c * in_cs + frames] = x[s, c]
    d_in = torch.from_numpy(xin).cuda()
    d_out = torch.full((S * out_ss,), float(SENT), dtype=torch.float32, device="cuda")
    bp = _handle(lib, table)
    bp.process_layout_scheduled_ptr(d_in.data_ptr(), d_out.data_ptr(), blocks, in_ss, in_cs, out_ss, out_cs, 2, idx, prev, True,
                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    mask = np.ones(S * out_ss, bool)
    y = np.empty_like(want)
    for s in range(S):
        for e in range(2):
            sl = slice(s * out_ss + e * out_cs, s * out_ss + e * out_cs + frames)
            y[s, e] = got[sl]
            mask[sl] = False
    assert (got[mask] == SENT).all(), "the output padding was written"
    assert d_in.cpu().numpy().tobytes() == xin.tobytes(), "the input was written"
    assert np.isfinite(y).all(), "a surplus input channel or the input padding was read"
    _same_bits(y, want, "padded strides against the contiguous run")


# ---- l. every refused call leaves the handle usable ---------------------------------------------------------------------------------
def test_argument_errors_leave_the_handle_usable(lib):
    import torch
    from open_headstage_amd import _ffi
    K, blocks = 6, 4
    table = make_table(N_SETS, K)
    x = make_input(S, K, blocks, seed=5300)
    frames = blocks * BLOCK
    d = torch.from_numpy(x.copy()).cuda()
    out = torch.empty((S, 2, frames), dtype=torch.float32, device="cuda")
    INV, OK = _ffi.OHS_ERR_INVALID_ARG, _ffi.OHS_OK
    idx = make_rows(S, 2, N_SETS)
    prev = ((idx[:, 0] + 1) % N_SETS).astype(np.uint32)
    up = C.POINTER(C.c_uint32)
    f = lib.ohs_batch_process_layout_scheduled

    def call(bp, d_in=None, d_out=None, n_blocks=blocks, in_ss=K * frames, in_cs=frames, out_ss=2 * frames, out_cs=frames, seg=2,
             rows=idx, stride=2, pv=prev, mode=CROSSFADE):
        rows = None if rows is None else np.ascontiguousarray(rows, np.uint32)
        pv = None if pv is None else np.ascontiguousarray(pv, np.uint32)
        return f(bp._h if bp is not None else None, C.c_void_p(d.data_ptr() if d_in is None else d_in),
                 C.c_void_p(out.data_ptr() if d_out is None else d_out), n_blocks, in_ss, in_cs, out_ss, out_cs, seg,
                 None if rows is None else rows.ctypes.data_as(up), stride, None if pv is None else pv.ctypes.data_as(up), mode, None)

    bp, twin = _handle(lib, table), _handle(lib, table)
    ip = idx.ctypes.data_as(up)
    assert call(None) == INV
    assert f(bp._h, None, C.c_void_p(out.data_ptr()), blocks, K * frames, frames, 2 * frames, frames, 2, ip, 2, None, 1, None) == INV
    assert f(bp._h, C.c_void_p(d.data_ptr()), None, blocks, K * frames, frames, 2 * frames, frames, 2, ip, 2, None, 1, None) == INV
    v = C.c_int(7)
    assert lib.ohs_batch_last_layout_scheduled(bp._h, None) == INV
    assert lib.ohs_batch_last_layout_scheduled(bp._h, C.byref(v)) == OK and v.value == 0
    assert call(_handle(lib)) == INV                                # no table uploaded
    assert call(_batch(lib, table[0])) == INV                       # ... a single layout is not a table
    fp = _ffi.fp
    sl = lib.ohs_batch_set_layout_schedule_irs
    assert sl(bp._h, 2, 17, np.zeros((2, 17, 2, 8), np.float32).ctypes.data_as(fp), 8) == INV       # n_channels > 16
    assert sl(bp._h, 2, 0, table.ctypes.data_as(fp), 8) == INV                                        # n_channels == 0
    assert sl(bp._h, N_SETS, K, table.ctypes.data_as(fp), 0) == INV                                   # len == 0
    assert sl(bp._h, 1, 2, np.zeros((1, 2, 2, 513), np.float32).ctypes.data_as(fp), 513) == INV       # len > 512
    assert sl(bp._h, 65537, 1, table.ctypes.data_as(fp), 1) == INV                                    # n_sets > 65536
    assert sl(bp._h, N_SETS, K, None, 512) == INV
    assert call(bp, seg=0) == INV
    assert call(bp, rows=None) == INV
    assert call(bp, mode=2) == INV and call(bp, mode=-1) == INV
    assert call(bp, stride=1) == INV                                # a non-zero idx_stride below the number of segments
    bad = idx.copy(); bad[S - 1, 1] = N_SETS
    assert call(bp, rows=bad) == INV                                # an index >= n_sets
    badp = prev.copy(); badp[2] = N_SETS
    assert call(bp, pv=badp) == INV
    assert call(bp, pv=badp, mode=RING_OUT) == OK                   # (prev_idx is read under CROSSFADE only)
    torch.cuda.synchronize()
    twin_y = _run(twin, x, idx, 2, None, False)
    _same_bits(out.cpu().numpy(), twin_y, "RING_OUT with an unread prev_idx")
    bp.reset(); twin.reset()
    assert call(bp, in_cs=frames - 1) == INV and call(bp, out_cs=frames - 1) == INV          # strides below the region
    assert call(bp, in_ss=K * frames - 1) == INV and call(bp, out_ss=2 * frames - 1) == INV
    assert call(bp, in_ss=frames) == INV
    assert call(bp, d_out=d.data_ptr()) == INV                      # in place
    assert call(bp, d_out=d.data_ptr() + 4 * (S * K * frames - 1)) == INV                    # the regions meet in one frame
    assert call(bp, n_blocks=(1 << 24) + 1, in_cs=1 << 40, in_ss=1 << 50, out_cs=1 << 40, out_ss=1 << 50) == INV
    assert call(bp, n_blocks=0) == OK                               # a no-op
    # ... and none of them queued anything or touched the state: the table uploaded first still serves, as on the twin
    assert call(bp) == OK
    torch.cuda.synchronize()
    got = out.cpu().numpy().copy()
    assert lib.ohs_batch_last_layout_scheduled(bp._h, C.byref(v)) == OK and v.value == 1
    _same_bits(got, _run(twin, x, idx, 2, prev), "the valid call behind the refused ones")
    _same_bits(_run(bp, x, idx, 2, prev), _run(twin, x, idx, 2, prev), "and the call after it")

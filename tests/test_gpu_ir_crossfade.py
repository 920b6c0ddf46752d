"""ohs_batch_process_ir_crossfaded: the schedule of HRIR sets with a crossfade over the first block of every segment that changes
the set.

The yardstick is never the code under test: it is the f64 model of tests/test_cpu_ir_crossfade.py (built from the direct f64
convolution of tests/test_cpu_ir_schedule.py and checked there), or the EXISTING entry points on further handles
(ohs_batch_process_ir_scheduled under RING_OUT on the two halves of the split input).  Bars: bit for bit where the header
promises bits, 1e-6 relative RMS per stream -- the project's FFT bar, DESIGN section 2 -- everywhere else."""
import ctypes as C

import numpy as np
import pytest

from tests.test_cpu_ir_crossfade import fade_plan, model_ir_crossfade, split_input
from tests.test_cpu_ir_schedule import BLOCK, RING_OUT, make_rows, make_sets, rel_rms_per_stream, render_f64
from tests.test_gpu_ir_schedule import (N_SETS, S, _batch, _conv_launches, _oracle_eq, _plain, _same_bits, _shared_row,
                                        _within_bar)
from tests.test_gpu_ir_schedule import _run as _run_scheduled

pytestmark = pytest.mark.gpu

BLOCKS = [13, 9]


@pytest.fixture(scope="module")
def lib():
    from open_headstage_amd import _ffi
    return _ffi.lib()


def _run(bp, x, seg_blocks, idx, prev=None, in_place=False):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()
    y = bp.process_ir_crossfaded(d, seg_blocks, idx, prev, out=d if in_place else None)
    torch.cuda.synchronize()
    return y.cpu().numpy()


# ---- 1. rows per stream, a change in every segment, two calls -------------------------------------------------------------------
@pytest.mark.parametrize("seg_blocks", [1, 2, 3])
def test_rows_per_stream_two_calls_against_the_f64_model(lib, oracle, seg_blocks):
    from open_headstage_amd import synth
    sets = make_sets(N_SETS)
    a, b = _batch(lib, sets=sets), _batch(lib, sets=sets)
    x = synth.white_noise(range(500, 500 + S), sum(BLOCKS) * BLOCK)
    x1, x2 = x[:, :, :BLOCKS[0] * BLOCK], x[:, :, BLOCKS[0] * BLOCK:]
    idx1 = make_rows(S, -(-BLOCKS[0] // seg_blocks), N_SETS, 0)
    idx2 = make_rows(S, -(-BLOCKS[1] // seg_blocks), N_SETS, 1)
    prev = idx1[:, -1].copy()
    assert (prev != idx2[:, 0]).any()                   # the second call's first block fades in some stream
    ref1, tails = model_ir_crossfade(oracle, x1, sets, idx1, seg_blocks)
    for bp in (a, b):
        y1 = _run(bp, x1, seg_blocks, idx1)
        assert bp.last_conv_ir_crossfaded() and bp.last_conv_ir_scheduled() and bp.last_conv_plan()[0] == "block512_p1"
        _within_bar(y1, ref1, f"call 0 (seg_blocks {seg_blocks})")
    ref2, _ = model_ir_crossfade(oracle, x2, sets, idx2, seg_blocks, prev=prev, tail_in=tails)
    _within_bar(_run(a, x2, seg_blocks, idx2, prev), ref2, "call 1 with prev_idx")
    assert a.last_conv_ir_crossfaded()
    ref3, _ = model_ir_crossfade(oracle, x2, sets, idx2, seg_blocks, tail_in=tails)
    assert (rel_rms_per_stream(ref3, ref2)[prev != idx2[:, 0]] > 1e-3).all()
    _within_bar(_run(b, x2, seg_blocks, idx2, None), ref3, "call 1 without prev_idx")


# ---- 2. one row for all streams, in place and not, EQ on and off ----------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("eq", [False, True])
def test_shared_row_against_the_f64_model(lib, oracle, in_place, eq):
    from open_headstage_amd import synth
    sets = make_sets(N_SETS)
    bp = _batch(lib, sets=sets, eq=eq)
    xin = synth.white_noise(range(510, 510 + S), sum(BLOCKS) * BLOCK)
    # (the EQ runs in front of the convolution: the model takes the equalised input)
    x, eqs = _oracle_eq(oracle, xin) if eq else (xin, None)
    pos, tails, prev = 0, None, None
    for call, nb in enumerate(BLOCKS):
        row = _shared_row(-(-nb // 2), call)
        assert prev is None or prev != int(row[0])      # the second call's first block fades
        sl = slice(pos, pos + nb * BLOCK)
        y = _run(bp, xin[:, :, sl], 2, row, prev, in_place)
        assert bp.last_conv_ir_crossfaded()
        ref, tails = model_ir_crossfade(oracle, x[:, :, sl], sets, row, 2, prev=prev, tail_in=tails)
        _within_bar(y, ref, f"shared row, call {call}")
        prev = int(row[-1])
        pos += nb * BLOCK
    # the handle adopted the last segment's set: a plain call continues with it
    last = sets[prev]
    x3 = synth.white_noise(range(515, 515 + S), 4 * BLOCK)
    x3e = _oracle_eq(oracle, x3, eqs)[0] if eq else x3
    ref3, _ = render_f64(oracle, x3e, lambda s, t: last, tail_in=tails)
    _within_bar(_plain(bp, x3), ref3, "plain call behind the shared row")


# ---- 3. bits ---------------------------------------------------------------------------------------------------------------------
def test_constant_row_among_changing_rows_and_third_blocks_are_ring_outs_bits(lib):
    from open_headstage_amd import synth
    sets = make_sets(N_SETS)
    a, b = _batch(lib, sets=sets), _batch(lib, sets=sets)
    nb, seg = 13, 3
    x = synth.white_noise(range(520, 520 + S), nb * BLOCK)
    idx = make_rows(S, -(-nb // seg), N_SETS)
    idx[2, :] = 4                                       # one stream never changes its set
    y = _run(a, x, seg, idx)
    assert a.last_conv_ir_crossfaded()
    r = _run_scheduled(b, x, seg, idx, RING_OUT)
    _same_bits(y[2:3], r[2:3], "the stream with a constant row")
    third = np.concatenate([np.arange(t * BLOCK, (t + 1) * BLOCK) for t in range(2, nb, seg)])
    _same_bits(np.ascontiguousarray(y[:, :, third]), np.ascontiguousarray(r[:, :, third]), "the third block of every segment")
    others = [s for s in range(S) if s != 2]
    assert (rel_rms_per_stream(y[others], r[others]) > 1e-3).all()      # (and the fading streams are not RING_OUT's)


def test_a_call_without_any_boundary_is_the_ring_out_call(lib):
    from open_headstage_amd import synth
    sets = make_sets(N_SETS)
    x = synth.white_noise(range(530, 530 + S), 11 * BLOCK)
    for idx, prev, says in [(np.full(4, 3, np.uint32), None, 0), (np.full(4, 3, np.uint32), 3, 0),
                            (np.tile(np.array([[1], [2], [3], [4], [5]], np.uint32), (1, 4)), None, 1),
                            (np.tile(np.array([[1], [2], [3], [4], [5]], np.uint32), (1, 4)), np.arange(1, 6), 1)]:
        a, b = _batch(lib, sets=sets, own=sets[0]), _batch(lib, sets=sets, own=sets[0])
        for call in range(2):
            y, r = _run(a, x, 3, idx, prev), _run_scheduled(b, x, 3, idx, RING_OUT)
            _same_bits(y, r, f"no boundary, call {call}")
            v, w = C.c_int(-1), C.c_int(-1)
            assert lib.ohs_batch_last_conv_ir_scheduled(a._h, C.byref(v)) == 0 and lib.ohs_batch_last_conv_ir_scheduled(b._h, C.byref(w)) == 0
            assert v.value == w.value == says and not a.last_conv_ir_crossfaded()
    # ... and one differing prev_idx entry is a boundary
    a = _batch(lib, sets=sets)
    _run(a, x, 3, np.full(4, 3, np.uint32), 2)
    v = C.c_int(-1)
    assert lib.ohs_batch_last_conv_ir_scheduled(a._h, C.byref(v)) == 0 and v.value == 2


def test_rows_per_stream_are_single_stream_handles_and_one_row_is_that_row_tiled_bit_for_bit(lib):
    from open_headstage_amd import synth
    sets = make_sets(N_SETS)
    bp = _batch(lib, sets=sets)
    singles = [_batch(lib, streams=1, sets=sets) for _ in range(S)]
    one, tiled = _batch(lib, sets=sets), _batch(lib, sets=sets)
    x = synth.white_noise(range(540, 540 + S), sum(BLOCKS) * BLOCK)
    pos, prev, prev_row = 0, None, None
    for call, nb in enumerate(BLOCKS):
        idx = make_rows(S, -(-nb // 2), N_SETS, call)
        xc = x[:, :, pos:pos + nb * BLOCK]
        y = _run(bp, xc, 2, idx, prev)
        ref = np.concatenate([_run(singles[s], xc[s:s + 1], 2, idx[s], None if prev is None else prev[s]) for s in range(S)])
        _same_bits(y, ref, f"rows per stream, call {call}")
        row = _shared_row(-(-nb // 2), call)
        _same_bits(_run(one, xc, 2, row, prev_row), _run(tiled, xc, 2, np.tile(row, (S, 1)), None if prev_row is None else [prev_row] * S),
                   f"one row, call {call}")
        prev, prev_row = idx[:, -1].copy(), int(row[-1])
        pos += nb * BLOCK


# ---- 4. the yardstick of existing entry points: RING_OUT on both halves of the split input ---------------------------------------
@pytest.mark.parametrize("seg_blocks", [1, 2])
def test_crossfade_is_the_sum_of_two_ring_out_calls(lib, seg_blocks):
    from open_headstage_amd import synth
    sets = make_sets(N_SETS)
    bp, h_new, h_old = _batch(lib, sets=sets), _batch(lib, sets=sets), _batch(lib, sets=sets)
    x = synth.white_noise(range(550, 550 + S), sum(BLOCKS) * BLOCK)
    pos, prev = 0, None
    for call, nb in enumerate(BLOCKS):
        n_segs = -(-nb // seg_blocks)
        idx = make_rows(S, n_segs, N_SETS, call)
        xc = x[:, :, pos:pos + nb * BLOCK]
        cur, old = fade_plan(S, nb, idx, seg_blocks, prev)
        x_new, x_old = split_input(xc, cur, old)
        shifted = np.empty_like(idx)            # segment k fades from segment k - 1's set (x_old is zero off the fading blocks)
        shifted[:, 1:] = idx[:, :-1]
        shifted[:, 0] = idx[:, 0] if prev is None else prev
        want = _run_scheduled(h_new, x_new, seg_blocks, idx, RING_OUT).astype(np.float64) + \
            _run_scheduled(h_old, x_old, seg_blocks, shifted, RING_OUT).astype(np.float64)
        _within_bar(_run(bp, xc, seg_blocks, idx, prev), want, f"sum of two RING_OUT calls, call {call}")
        prev = idx[:, -1].copy()
        pos += nb * BLOCK


# ---- 5. state at rest behind a call whose last block fades ------------------------------------------------------------------------
def test_set_ir_of_one_path_behind_a_faded_last_block_drops_that_paths_tail_only(lib, oracle):
    from open_headstage_amd import synth
    sets = make_sets(N_SETS + 1)
    own, new1 = sets[N_SETS], make_sets(1, seed=99)[0][1]
    x = synth.white_noise(range(560, 560 + S), 12 * BLOCK)
    x1, x2 = x[:, :, :7 * BLOCK], x[:, :, 7 * BLOCK:]
    first = slice(0, BLOCK)

    # rows per stream, seg_blocks 1: every stream's last block fades
    bp = _batch(lib, sets=sets[:N_SETS], own=own)
    idx = make_rows(S, 7, N_SETS)
    y1 = _run(bp, x1, 1, idx)
    bp.set_ir(1, new1)
    y2 = _plain(bp, x2)
    ref1, tails = model_ir_crossfade(oracle, x1, sets, idx, 1)
    after = [own[0], new1, own[2], own[3]]              # the handle's own responses were untouched by the call
    dropped = tails.copy()
    dropped[:, 1] = 0.0
    ref2, _ = render_f64(oracle, x2, lambda s, t: after, tail_in=dropped)
    _within_bar(y1, ref1, "rows per stream: the crossfaded call")
    _within_bar(y2, ref2, "rows per stream: the plain call behind set_ir of path 1")
    # teeth: keeping path 1's tail, or tails rebuilt from the last input through the last set alone, is far off
    keep, _ = render_f64(oracle, x2, lambda s, t: after, tail_in=tails)
    _, rebuilt = render_f64(oracle, x1[:, :, 6 * BLOCK:], lambda s, t: sets[int(idx[s, 6])])
    rebuilt[:, 1] = 0.0
    wrong, _ = render_f64(oracle, x2, lambda s, t: after, tail_in=rebuilt)
    assert (rel_rms_per_stream(keep[:, :, first], ref2[:, :, first]) > 1e-3).all()
    assert (rel_rms_per_stream(wrong[:, :, first], ref2[:, :, first]) > 1e-3).all()

    # one row for all streams: the handle adopts the last set; a plain call continues, with and without a set_ir in between
    row = np.array([1, 4, 2, 5, 0, 3, 1], np.uint32)
    ref1, tails = model_ir_crossfade(oracle, x1, sets, row, 1)
    last = sets[int(row[-1])]
    for with_set_ir in (False, True):
        bp = _batch(lib, sets=sets[:N_SETS], own=own)
        _within_bar(_run(bp, x1, 1, row), ref1, "one row: the crossfaded call")
        t_in, after = tails.copy(), list(last)
        if with_set_ir:
            bp.set_ir(1, new1)
            t_in[:, 1] = 0.0
            after[1] = new1
        ref2, _ = render_f64(oracle, x2, lambda s, t: after, tail_in=t_in)
        _within_bar(_plain(bp, x2), ref2, f"one row: the plain call behind it (set_ir of path 1: {with_set_ir})")
        _, rebuilt = render_f64(oracle, x1[:, :, 6 * BLOCK:], lambda s, t: last)
        if with_set_ir:
            rebuilt[:, 1] = 0.0
        wrong, _ = render_f64(oracle, x2, lambda s, t: after, tail_in=rebuilt)
        assert (rel_rms_per_stream(wrong[:, :, first], ref2[:, :, first]) > 1e-3).all()


def test_one_block_call_with_prev_idx_leaves_the_faded_state(lib, oracle):
    from open_headstage_amd import synth
    sets = make_sets(N_SETS)
    new2 = make_sets(1, seed=98)[0][2]
    bp = _batch(lib, sets=sets, own=sets[0])
    x = synth.white_noise(range(565, 565 + S), 4 * BLOCK)
    idx, prev = np.array([[1], [2], [3], [4], [5]], np.uint32), np.array([0, 2, 5, 1, 3], np.uint32)
    y1 = _run(bp, x[:, :, :BLOCK], 1, idx, prev)
    assert bp.last_conv_ir_crossfaded()
    bp.set_ir(2, new2)
    y2 = _plain(bp, x[:, :, BLOCK:])
    ref1, tails = model_ir_crossfade(oracle, x[:, :, :BLOCK], sets, idx, 1, prev=prev)
    tails[:, 2] = 0.0
    after = [sets[0][0], sets[0][1], new2, sets[0][3]]
    ref2, _ = render_f64(oracle, x[:, :, BLOCK:], lambda s, t: after, tail_in=tails)
    _within_bar(y1, ref1, "a one-block call with prev_idx")
    _within_bar(y2, ref2, "the plain call behind set_ir of path 2")


# ---- 6. several time chunks: fading blocks that are a chunk's dry block -----------------------------------------------------------
@pytest.mark.parametrize("streams,blocks,seg_blocks", [(6, 130, 3), (300, 70, 2)])
def test_overlapped_calls_one_launch_per_time_chunk(lib, oracle, streams, blocks, seg_blocks):
    from open_headstage_amd import synth
    sets = make_sets(N_SETS)
    bp, twin = _batch(lib, streams=streams, sets=sets, eq=True, plan=0), _batch(lib, streams=streams, own=sets[0], eq=True, plan=1)
    x = synth.white_noise(range(600, 600 + streams), blocks * BLOCK)
    idx = make_rows(streams, -(-blocks // seg_blocks), N_SETS)
    prev = (idx[:, 0] + 1) % N_SETS
    _plain(twin, x)
    chunks = _conv_launches(twin)                    # the plain call's time chunks for this shape
    assert chunks > 1
    before = _conv_launches(bp)
    y = _run(bp, x, seg_blocks, idx, prev, in_place=True)
    assert bp.last_conv_ir_crossfaded() and bp.last_conv_plan()[0] == "block512_p1"
    assert _conv_launches(bp) - before == chunks, (bp.conv_plan_counts(), chunks)
    check = list(range(streams)) if streams <= 8 else [0, 1, streams // 2, streams - 1]
    xe, _ = _oracle_eq(oracle, x[check])
    ref, _ = model_ir_crossfade(oracle, xe, sets, idx[check], seg_blocks, prev=prev[check])
    _within_bar(y[check], ref, f"{streams} streams x {blocks} blocks")


# ---- 7. every refused call leaves the handle usable -------------------------------------------------------------------------------
def test_argument_errors_leave_the_handle_usable(lib):
    import torch
    from open_headstage_amd import _ffi, synth
    sets = make_sets(N_SETS)
    x = synth.white_noise(range(640, 640 + S), 12 * BLOCK)
    d = torch.from_numpy(x.copy()).cuda()
    out = torch.empty_like(d)
    frames = x.shape[2]
    u32p = C.POINTER(C.c_uint32)
    row = np.array([0, 1, 2, 3, 4, 5], np.uint32)
    rp = row.ctypes.data_as(u32p)
    one_prev = np.array([3], np.uint32)

    def call(bp, d_in=None, d_out=None, n_blocks=12, ss=2 * frames, cs=frames, seg=2, idx=rp, stride=0, prev=one_prev):
        pp = None if prev is None else prev.ctypes.data_as(u32p)
        return lib.ohs_batch_process_ir_crossfaded(bp._h if bp is not None else None, C.c_void_p(d.data_ptr() if d_in is None else d_in),
                                                   C.c_void_p(out.data_ptr() if d_out is None else d_out), n_blocks, ss, cs, seg, idx,
                                                   stride, pp, None)

    INV = _ffi.OHS_ERR_INVALID_ARG
    bp, twin = _batch(lib, sets=sets, own=sets[1]), _batch(lib, own=sets[1])
    assert call(None) == INV
    assert lib.ohs_batch_process_ir_crossfaded(bp._h, None, C.c_void_p(out.data_ptr()), 12, 2 * frames, frames, 2, rp, 0, None, None) == INV
    assert lib.ohs_batch_process_ir_crossfaded(bp._h, C.c_void_p(d.data_ptr()), None, 12, 2 * frames, frames, 2, rp, 0, None, None) == INV
    assert call(bp, idx=None) == INV
    assert call(bp, seg=0) == INV
    bad = row.copy(); bad[3] = N_SETS
    assert call(bp, idx=bad.ctypes.data_as(u32p)) == INV
    rows = np.tile(row, (S, 1)); rows[S - 1, 5] = N_SETS + 7
    prevs = np.arange(S, dtype=np.uint32)
    assert call(bp, idx=rows.ctypes.data_as(u32p), stride=6, prev=prevs) == INV         # ... in the last stream's row
    assert call(bp, prev=np.array([N_SETS], np.uint32)) == INV                          # a prev_idx entry out of range
    good = np.tile(row, (S, 1)); bad_prev = prevs.copy(); bad_prev[S - 1] = N_SETS
    assert call(bp, idx=good.ctypes.data_as(u32p), stride=6, prev=bad_prev) == INV      # ... the last stream's
    assert call(bp, stride=5) == INV                    # a non-zero stride below n_segments
    assert call(bp, cs=frames - 1) == INV and call(bp, ss=frames) == INV
    fresh = _batch(lib, own=sets[1])
    assert call(fresh) == INV                           # no set table uploaded
    assert call(bp) == _ffi.OHS_OK
    torch.cuda.synchronize()
    assert bp.last_conv_ir_crossfaded()
    # the handle behaves as one that never saw the refused calls: same calls on a twin that made only the accepted one
    twin.set_schedule_irs(sets)
    assert call(twin) == _ffi.OHS_OK
    torch.cuda.synchronize()
    _same_bits(_plain(bp, x), _plain(twin, x), "plain call behind the refused calls")

    # a response longer than one partition on the handle
    rng = np.random.default_rng(1)
    long_ir = (0.02 * rng.standard_normal(1100)).astype(np.float32)
    lp, lt = _batch(lib, sets=sets, own=sets[1], plan=0), _batch(lib, own=sets[1], plan=0)
    for h in (lp, lt):
        h.set_ir(0, long_ir)
    assert call(lp) == INV
    y8 = [_plain(h, x[:, :, :8 * BLOCK]) for h in (lp, lt)]
    _same_bits(y8[0], y8[1], "long response")

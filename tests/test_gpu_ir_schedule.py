"""ohs_batch_process_ir_scheduled: a schedule of HRIR sets per stream inside one batch call.

The yardstick is never the code under test: it is the oracle's engine driven the reference's way (set_ir x 4 in front of every
run), the f64 model of tests/test_cpu_ir_schedule.py (checked there against the oracle), or the EXISTING entry points on a
second handle (ohs_batch_set_ir x 4 + ohs_batch_process per run).  Bars: bit for bit where the header promises bits (plan 1),
1e-6 relative RMS per stream -- the project's FFT bar, DESIGN section 2 -- everywhere else."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.test_cpu_ir_schedule import (BLOCK, CUT, RING_OUT, engine_cut_reference, make_rows, make_sets, model_ir_schedule,
                                        rel_rms_per_stream, render_f64, runs_of)
from tests.util import write_minimal_sofa

pytestmark = pytest.mark.gpu

S = 5
NB = 10
N_SETS = 6
BAR = 1e-6
MODES = {RING_OUT: "ring_out", CUT: "cut"}


@pytest.fixture(scope="module")
def lib():
    from open_headstage_amd import _ffi
    return _ffi.lib()


def _batch(lib, streams=S, sets=None, plan=1, eq=False, own=None):
    """a batch handle; sets: the schedule's table; own: the handle's own four responses (set_ir); eq: synth's table, enabled"""
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    bp = ohs.BatchProcessor(streams, num_bands=NB, library=lib)
    bp.set_conv_plan(plan)
    if own is not None:
        for p in range(4):
            bp.set_ir(p, own[p])
    if sets is not None:
        bp.set_schedule_irs(sets)
    if eq:
        for i, (c, en) in enumerate(_eq_bands()):
            bp.set_band_coeffs(i, c, en)
        bp.set_eq_enabled(True)
    return bp


def _eq_bands():
    """synth's EQ table as (coefficients, enabled) per band: the same five floats go to the GPU and to the oracle"""
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    bands = synth.eq_table()[:NB]
    assert len(bands) == NB
    return [(ohs.biquad_coefficients(b.filter_type, synth.FS, b.center_freq, b.q, b.gain_db), bool(b.enabled)) for b in bands]


def _oracle_eq(oracle, x, eqs=None):
    """x through the oracle's EQ (synth's table), per stream; eqs: the instances of an earlier call (state carried)"""
    from open_headstage_amd import synth
    if eqs is None:
        eqs = []
        for _ in range(x.shape[0]):
            q = oracle.StereoParametricEQ(NB, synth.FS)
            for i, (c, en) in enumerate(_eq_bands()):
                q.set_band_coeffs(i, c, en)
            eqs.append(q)
    y = np.array(x, np.float32)
    for s, q in enumerate(eqs):
        l, r = y[s, 0].copy(), y[s, 1].copy()
        q.process_block(l, r)
        y[s, 0], y[s, 1] = l, r
    return y, eqs


def _same_bits(y, ref, what):
    assert float(np.abs(ref).max()) > 0.01, what
    for s in range(y.shape[0]):
        bad = np.flatnonzero(y[s].view(np.uint32).ravel() != ref[s].view(np.uint32).ravel())
        assert bad.size == 0, f"{what}: stream {s}, {bad.size} samples differ, first at {bad[:4]}"


def _within_bar(y, ref, what):
    err = rel_rms_per_stream(y, ref)
    print(f"{what}: relative RMS per stream, worst {err.max():.3e}")
    assert (err <= BAR).all(), f"{what}: relative RMS per stream {err} (bar {BAR:.0e})"


def _run(bp, x, seg_blocks, idx, mode, in_place=False):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()
    y = bp.process_ir_scheduled(d, seg_blocks, idx, MODES[mode], out=d if in_place else None)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _plain(bp, x):
    import torch
    y = bp.process(torch.from_numpy(np.ascontiguousarray(x).copy()).cuda())
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _per_run_reference(ref, x, sets, row, seg_blocks):
    """the existing entry points: ohs_batch_set_ir x 4 in front of every run of equal indices, ohs_batch_process per run"""
    frames = x.shape[2]
    out = np.empty_like(x)
    for k0, k1, i in runs_of(list(row)):
        for p in range(4):
            ref.set_ir(p, sets[i][p])
        sl = slice(k0 * seg_blocks * BLOCK, min(k1 * seg_blocks * BLOCK, frames))
        out[:, :, sl] = _plain(ref, x[:, :, sl])
    return out


def _shared_row(n_segs, call):
    """one row for all streams: a new set in most segments, one run of two equal segments"""
    row = np.array([(1 + 2 * call + 5 * k) % N_SETS for k in range(n_segs)], np.uint32)
    if n_segs >= 3:
        row[2] = row[1]
    return row


# ---- a. CUT, one row, against set_ir x 4 + process per run on a second handle: bit for bit -------------------------------------
@pytest.mark.parametrize("seg_blocks", [1, 2, 3, 7])
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("eq", [False, True])
def test_cut_shared_row_is_set_ir_and_process_per_run_bit_for_bit(lib, seg_blocks, in_place, eq):
    from open_headstage_amd import synth
    sets = make_sets(N_SETS)
    bp, ref = _batch(lib, sets=sets, eq=eq), _batch(lib, eq=eq)
    blocks = [23, 17]
    assert all(nb % seg_blocks for nb in blocks if seg_blocks > 1)
    x = synth.white_noise(range(500, 500 + S), sum(blocks) * BLOCK)
    pos = 0
    for call, nb in enumerate(blocks):
        n_segs = -(-nb // seg_blocks)
        row = _shared_row(n_segs, call)
        if call == 1:
            row[0] = last            # the call's start is a boundary even where the index stays
        xc = x[:, :, pos:pos + nb * BLOCK]
        y = _run(bp, xc, seg_blocks, row, CUT, in_place)
        assert bp.last_conv_ir_scheduled() and bp.last_conv_plan()[0] == "block512_p1"
        _same_bits(y, _per_run_reference(ref, xc, sets, row, seg_blocks), f"call {call} ({nb} blocks, seg_blocks {seg_blocks})")
        last = row[-1]
        pos += nb * BLOCK


# ---- b. CUT against the oracle's engine with set_ir between runs ---------------------------------------------------------------
def test_cut_rows_per_stream_against_the_oracle_engine(lib, oracle):
    from open_headstage_amd import synth
    sets = make_sets(N_SETS)
    bp = _batch(lib, streams=4, sets=sets)
    x = synth.white_noise(range(520, 524), 19 * BLOCK)
    idx = make_rows(4, 10, N_SETS)
    idx[1, 4] = idx[1, 3]
    y = _run(bp, x, 2, idx, CUT)
    _within_bar(y, engine_cut_reference(oracle, x, sets, idx, 2), "CUT vs oracle engine")


# ---- c. RING_OUT against the f64 model, a new set in every segment, every stream its own row ------------------------------------
@pytest.mark.parametrize("seg_blocks", [1, 2])
def test_ring_out_rows_per_stream_against_the_f64_model(lib, oracle, seg_blocks):
    from open_headstage_amd import synth
    sets = make_sets(N_SETS)
    bp = _batch(lib, sets=sets)
    blocks = [13, 9]
    x = synth.white_noise(range(530, 530 + S), sum(blocks) * BLOCK)
    pos, tails = 0, None
    for call, nb in enumerate(blocks):
        idx = make_rows(S, -(-nb // seg_blocks), N_SETS, call)
        assert len({tuple(r) for r in idx.tolist()}) == S
        xc = x[:, :, pos:pos + nb * BLOCK]
        y = _run(bp, xc, seg_blocks, idx, RING_OUT)
        assert bp.last_conv_ir_scheduled()
        ref, tails = model_ir_schedule(oracle, xc, sets, idx, seg_blocks, RING_OUT, tail_in=tails)
        _within_bar(y, ref, f"RING_OUT call {call}")
        cut, _ = model_ir_schedule(oracle, xc, sets, idx, seg_blocks, CUT)
        assert (rel_rms_per_stream(y, cut) > 1e-3).all()        # (and it is not the other mode)
        pos += nb * BLOCK


# ---- d. rows per stream = one single-stream handle per stream on that row; one row = that row repeated ------------------------
@pytest.mark.parametrize("mode", [RING_OUT, CUT])
def test_rows_per_stream_are_single_stream_handles_bit_for_bit(lib, mode):
    from open_headstage_amd import synth
    sets = make_sets(N_SETS)
    bp = _batch(lib, sets=sets)
    singles = [_batch(lib, streams=1, sets=sets) for _ in range(S)]
    blocks = [14, 11]
    x = synth.white_noise(range(540, 540 + S), sum(blocks) * BLOCK)
    pos = 0
    for call, nb in enumerate(blocks):
        idx = make_rows(S, -(-nb // 2), N_SETS, call)
        xc = x[:, :, pos:pos + nb * BLOCK]
        y = _run(bp, xc, 2, idx, mode)
        ref = np.concatenate([_run(singles[s], xc[s:s + 1], 2, idx[s], mode) for s in range(S)])
        _same_bits(y, ref, f"mode {mode}, call {call}")
        pos += nb * BLOCK


@pytest.mark.parametrize("mode", [RING_OUT, CUT])
def test_one_row_is_that_row_repeated_per_stream_bit_for_bit(lib, mode):
    from open_headstage_amd import synth
    sets = make_sets(N_SETS)
    a, b = _batch(lib, sets=sets), _batch(lib, sets=sets)
    blocks = [14, 11]
    x = synth.white_noise(range(550, 550 + S), sum(blocks) * BLOCK)
    pos = 0
    for call, nb in enumerate(blocks):
        row = _shared_row(-(-nb // 2), call)
        xc = x[:, :, pos:pos + nb * BLOCK]
        _same_bits(_run(a, xc, 2, row, mode), _run(b, xc, 2, np.tile(row, (S, 1)), mode), f"mode {mode}, call {call}")
        pos += nb * BLOCK


# ---- e. a constant schedule is the plain call on a handle that loaded the set ---------------------------------------------------
@pytest.mark.parametrize("mode", [RING_OUT, CUT])
def test_constant_schedule_is_the_plain_call_bit_for_bit(lib, mode):
    from open_headstage_amd import synth
    sets = make_sets(N_SETS)
    x = synth.white_noise(range(560, 560 + S), 21 * BLOCK)
    ref = _batch(lib, own=sets[4])
    want = _plain(ref, x)
    a = _batch(lib, sets=sets)
    _same_bits(_run(a, x, 3, np.full(7, 4, np.uint32), mode), want, "one constant row")
    assert not a.last_conv_ir_scheduled()           # the plain kernel served it
    # the same set named by every stream's own row goes through the scheduled kernel: the same bits
    b = _batch(lib, sets=sets)
    _same_bits(_run(b, x, 3, np.full((S, 7), 4, np.uint32), mode), want, "constant rows per stream")
    assert b.last_conv_ir_scheduled()


# ---- f. scheduled -> plain -> scheduled: the plain call continues with the last set ---------------------------------------------
def test_scheduled_plain_scheduled_shared_row_against_the_f64_model(lib, oracle):
    from open_headstage_amd import synth
    sets = make_sets(N_SETS)
    bp = _batch(lib, sets=sets, own=sets[0])
    x = synth.white_noise(range(570, 570 + S), 30 * BLOCK)
    row1, row3 = np.array([2, 5, 1, 3], np.uint32), np.array([0, 4, 4, 2, 1], np.uint32)
    y1 = _run(bp, x[:, :, :8 * BLOCK], 2, row1, RING_OUT)
    y2 = _plain(bp, x[:, :, 8 * BLOCK:20 * BLOCK])
    assert not bp.last_conv_ir_scheduled()
    y3 = _run(bp, x[:, :, 20 * BLOCK:], 2, row3, RING_OUT)
    per_block = [int(row1[t // 2]) for t in range(8)] + [int(row1[-1])] * 12 + [int(row3[t // 2]) for t in range(10)]
    ref, _ = render_f64(oracle, x, lambda s, t: sets[per_block[t]])
    _within_bar(np.concatenate([y1, y2, y3], axis=2), ref, "scheduled -> plain -> scheduled")


# ---- g. rows per stream, then set_ir of ONE path, then a plain call -------------------------------------------------------------
def test_set_ir_of_one_path_after_rows_per_stream_drops_that_paths_tail_only(lib, oracle):
    from open_headstage_amd import synth
    sets = make_sets(N_SETS + 1)
    own, new1 = sets[N_SETS], make_sets(1, seed=99)[0][1]
    bp = _batch(lib, sets=sets[:N_SETS], own=own)
    x = synth.white_noise(range(580, 580 + S), 18 * BLOCK)
    idx = make_rows(S, 5, N_SETS)
    assert len(set(idx[:, -1].tolist())) > 1            # the streams end on different sets
    y1 = _run(bp, x[:, :, :10 * BLOCK], 2, idx, RING_OUT)
    bp.set_ir(1, new1)
    y2 = _plain(bp, x[:, :, 10 * BLOCK:])
    ref1, tails = model_ir_schedule(oracle, x[:, :, :10 * BLOCK], sets, idx, 2, RING_OUT)
    after = [own[0], new1, own[2], own[3]]              # the handle's own responses were untouched by the call
    dropped = tails.copy()
    dropped[:, 1] = 0.0
    ref2, _ = render_f64(oracle, x[:, :, 10 * BLOCK:], lambda s, t: after, tail_in=dropped)
    _within_bar(y1, ref1, "the scheduled call")
    _within_bar(y2, ref2, "the plain call behind set_ir of path 1")
    # teeth: keeping path 1's tail, or ringing out with the handle's own responses instead of each stream's last set, is far off
    keep, _ = render_f64(oracle, x[:, :, 10 * BLOCK:], lambda s, t: after, tail_in=tails)
    _, own_tails = render_f64(oracle, x[:, :, 9 * BLOCK:10 * BLOCK], lambda s, t: own)
    own_tails[:, 1] = 0.0
    wrong, _ = render_f64(oracle, x[:, :, 10 * BLOCK:], lambda s, t: after, tail_in=own_tails)
    first = slice(0, BLOCK)
    assert (rel_rms_per_stream(keep[:, :, first], ref2[:, :, first]) > 1e-3).all()
    assert (rel_rms_per_stream(wrong[:, :, first], ref2[:, :, first]) > 1e-3).all()


# ---- h. shapes: several time chunks, one and several chunks per stream, where plan 0 would take hop 1536 -----------------------
def _conv_launches(bp):
    return sum(bp.conv_plan_counts().values())


@pytest.mark.parametrize("streams,blocks,seg_blocks,mode", [(6, 130, 3, RING_OUT), (6, 97, 2, CUT), (300, 70, 2, RING_OUT)])
def test_overlapped_calls_one_launch_per_time_chunk(lib, oracle, streams, blocks, seg_blocks, mode):
    """EQ on, 64 blocks or more: the call is cut into time chunks at block positions that are no segment boundaries; the long
    chunks run several waves per stream, the short last one a single wave"""
    from open_headstage_amd import synth
    sets = make_sets(N_SETS)
    bp, twin = _batch(lib, streams=streams, sets=sets, eq=True, plan=0), _batch(lib, streams=streams, own=sets[0], eq=True, plan=1)
    x = synth.white_noise(range(600, 600 + streams), blocks * BLOCK)
    idx = make_rows(streams, -(-blocks // seg_blocks), N_SETS)
    _plain(twin, x)
    chunks = _conv_launches(twin)                    # the plain call's time chunks for this shape
    assert chunks > 1
    before = _conv_launches(bp)
    y = _run(bp, x, seg_blocks, idx, mode, in_place=True)
    assert bp.last_conv_ir_scheduled() and bp.last_conv_plan()[0] == "block512_p1"
    assert _conv_launches(bp) - before == chunks, (bp.conv_plan_counts(), chunks)
    check = list(range(streams)) if streams <= 8 else [0, 1, streams // 2, streams - 1]
    xe, _ = _oracle_eq(oracle, x[check])
    ref, _ = model_ir_schedule(oracle, xe, sets, idx[check], seg_blocks, mode)
    _within_bar(y[check], ref, f"{streams} streams x {blocks} blocks")


@pytest.mark.parametrize("in_place", [False, True])
def test_512_streams_48_blocks_stay_with_block_512_under_plan_0(lib, oracle, in_place):
    from open_headstage_amd import synth
    streams, blocks = 512, 48
    sets = make_sets(N_SETS)
    bp, twin = _batch(lib, streams=streams, sets=sets, plan=0), _batch(lib, streams=streams, own=sets[0], plan=0)
    x = synth.white_noise(range(900, 900 + streams), blocks * BLOCK)
    import torch
    d = torch.from_numpy(x.copy()).cuda()
    twin.process(d, out=d if in_place else None)
    torch.cuda.synchronize()
    assert twin.last_conv_plan()[0] == "hop1536_p1"        # what plan 0 picks for the plain call of this shape
    idx = make_rows(streams, blocks // 2, N_SETS)
    before = _conv_launches(bp)
    y = _run(bp, x, 2, idx, RING_OUT, in_place)
    assert bp.last_conv_ir_scheduled() and bp.last_conv_plan()[0] == "block512_p1"
    assert _conv_launches(bp) - before == 1
    check = [0, 7, 255, 511]
    ref, _ = model_ir_schedule(oracle, x[check], sets, idx[check], 2, RING_OUT)
    _within_bar(y[check], ref, "512 streams x 48 blocks")


# ---- the speaker-angle front end ------------------------------------------------------------------------------------------------
def test_set_schedule_speakers_builds_the_sets_set_speakers_loads(lib, tmp_path):
    import open_headstage_amd as ohs
    from open_headstage_amd import sofa, synth
    rng = np.random.default_rng(5)
    az = np.arange(0.0, 360.0, 10.0)
    pos = np.stack([az, np.zeros_like(az), np.ones_like(az)], 1)
    ir = 0.05 * rng.standard_normal((len(pos), 2, 160)) * np.exp(-np.arange(160) / 40.0)
    path = write_minimal_sofa(str(tmp_path / "ring.sofa"), ir, pos, synth.FS)
    sf = sofa.MySofa(path)
    angles = [[-30.0, 0.0, 30.0, 0.0], [-60.0, 0.0, 60.0, 0.0], [-90.0, 0.0, 20.0, 0.0]]
    bp, ref = _batch(lib), _batch(lib)
    up = bp.set_schedule_speakers(sf, angles, 1.0, synth.FS)
    assert up.shape[:2] == (3, 4) and up.shape[2] <= BLOCK and len({up[i].tobytes() for i in range(3)}) == 3
    x = synth.white_noise(range(620, 620 + S), 12 * BLOCK)
    row = np.array([1, 1, 2, 0], np.uint32)
    y = _run(bp, x, 3, row, CUT)
    out = np.empty_like(x)
    for k0, k1, i in runs_of(list(row)):
        ref.set_speakers(sf, *angles[i], 1.0, synth.FS)
        sl = slice(k0 * 3 * BLOCK, k1 * 3 * BLOCK)
        out[:, :, sl] = _plain(ref, x[:, :, sl])
    # (set_speakers re-loads only the paths whose response changed; the angles above change every path at every run, so it is four
    # set_ir per run, what CUT promises)
    _same_bits(y, out, "schedule built from speaker angles")
    with pytest.raises(ValueError):
        long_ir = 0.05 * rng.standard_normal((len(pos), 2, 600))
        bp.set_schedule_speakers(sofa.MySofa(write_minimal_sofa(str(tmp_path / "long.sofa"), long_ir, pos, synth.FS)), angles, 1.0, synth.FS)


# ---- i. every refused call leaves the handle usable ---------------------------------------------------------------------------
def test_argument_errors_leave_the_handle_usable(lib):
    import torch
    from open_headstage_amd import _ffi, synth
    sets = make_sets(N_SETS)
    x = synth.white_noise(range(640, 640 + S), 12 * BLOCK)
    d = torch.from_numpy(x.copy()).cuda()
    out = torch.empty_like(d)
    frames = x.shape[2]
    row = np.array([0, 1, 2, 3, 4, 5], np.uint32)
    rp = row.ctypes.data_as(C.POINTER(C.c_uint32))

    def call(bp, d_in=None, d_out=None, n_blocks=12, ss=2 * frames, cs=frames, seg=2, idx=rp, stride=0, mode=0):
        return lib.ohs_batch_process_ir_scheduled(bp._h if bp is not None else None, C.c_void_p(d.data_ptr() if d_in is None else d_in),
                                                  C.c_void_p(out.data_ptr() if d_out is None else d_out), n_blocks, ss, cs, seg, idx,
                                                  stride, mode, None)

    INV = _ffi.OHS_ERR_INVALID_ARG
    bp, twin = _batch(lib, sets=sets, own=sets[1]), _batch(lib, own=sets[1])
    assert call(None) == INV
    assert lib.ohs_batch_process_ir_scheduled(bp._h, None, C.c_void_p(out.data_ptr()), 12, 2 * frames, frames, 2, rp, 0, 0, None) == INV
    assert lib.ohs_batch_process_ir_scheduled(bp._h, C.c_void_p(d.data_ptr()), None, 12, 2 * frames, frames, 2, rp, 0, 0, None) == INV
    assert call(bp, idx=None) == INV
    assert call(bp, seg=0) == INV
    bad = row.copy(); bad[3] = N_SETS
    assert call(bp, idx=bad.ctypes.data_as(C.POINTER(C.c_uint32))) == INV
    rows = np.tile(row, (S, 1)); rows[S - 1, 5] = N_SETS + 7
    assert call(bp, idx=rows.ctypes.data_as(C.POINTER(C.c_uint32)), stride=6) == INV           # ... in the last stream's row
    assert call(bp, stride=5) == INV                    # a non-zero stride below n_segments
    assert call(bp, mode=2) == INV and call(bp, mode=-1) == INV
    assert call(bp, cs=frames - 1) == INV and call(bp, ss=frames) == INV
    fresh = _batch(lib, own=sets[1])
    assert call(fresh) == INV                           # no set table uploaded
    with pytest.raises(_ffi.OhsError):
        bp.set_schedule_irs(np.zeros((2, 4, 513), np.float32))          # len > 512
    assert lib.ohs_batch_set_schedule_irs(bp._h, 2, sets.ctypes.data_as(_ffi.fp), 0) == INV
    assert call(bp) == _ffi.OHS_OK                      # ... the table uploaded earlier still serves
    torch.cuda.synchronize()
    # the handle behaves as one that never saw the refused calls: same calls on a twin that made only the accepted one
    twin.set_schedule_irs(sets)
    assert call(twin) == _ffi.OHS_OK
    torch.cuda.synchronize()
    _same_bits(_plain(bp, x), _plain(twin, x), "plain call behind the refused calls")

    # a response longer than one partition on the handle; and tails of one still pending
    rng = np.random.default_rng(1)
    long_ir = (0.02 * rng.standard_normal(1100)).astype(np.float32)
    lp, lt = _batch(lib, sets=sets, own=sets[1], plan=0), _batch(lib, own=sets[1], plan=0)
    for h in (lp, lt):
        h.set_ir(0, long_ir)
    assert call(lp) == INV
    y8 = [_plain(h, x[:, :, :8 * BLOCK]) for h in (lp, lt)]
    _same_bits(y8[0], y8[1], "long response")
    for h in (lp, lt):
        h.set_ir(0, sets[1][0])                         # one partition again, the long response's tails pending
    assert call(lp) == INV
    a, b = _plain(lp, x), _plain(lt, x)
    _same_bits(a, b, "plain call with pending tails behind the refused call")
    for h in (lp, lt):
        _plain(h, x)                                    # (the tails have run out: 8192 frames)
    assert call(lp) == _ffi.OHS_OK
    torch.cuda.synchronize()

"""ohs_batch_process_scheduled_streams: a schedule of EQ tables and gains PER STREAM inside one batch call -- every stream a plugin
instance whose host refreshes its own bands and its own master gain in front of every block (parametric_eq.rs:125-129,
lib.rs:1180-1207; update_coefficients keeps s1, s2, parametric_eq.rs:85-114).

The yardstick is the oracle driven the reference's way and existing entry points, never the code under test (the manner of
test_gpu_schedule.py).  Per stream s an oracle StereoParametricEQ gets set_band_coeffs for every band from table idx[s][k] in
front of segment k; the EQ output of all streams goes through an EQ-off batch of the same stream count under plan 1, called once
per segment with set_gain(gain[s][k]) in front, of whose output only row s is kept -- one such reference batch PER STREAM, so
nothing is assumed about bits across batch shapes.  Taps <= 512, plan 1: the scheduled call must equal that BIT FOR BIT.  Every
case makes two consecutive calls, so that EQ state, overlaps and pending state carry over."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S = 5
NB = 10


def _tables(n_tables, nb=NB, seed=11):
    """n_tables tables of nb bands whose coefficients all differ; every band enabled"""
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    from open_headstage_amd.dsp import FilterType
    rng = np.random.default_rng(seed)
    types = [FilterType.Peak, FilterType.LowShelf, FilterType.HighShelf]
    coeffs = np.zeros((n_tables, nb, 5), np.float32)
    for t in range(n_tables):
        for b in range(nb):
            fc = min(38.0 * 2.0 ** (b * 0.88 + 0.05 * t), 18000.0)
            coeffs[t, b] = ohs.biquad_coefficients(types[(t + b) % 3], synth.FS, fc, float(0.5 + 0.25 * ((t + 2 * b) % 6)),
                                                   float(rng.uniform(-9, 9)))
    flat = coeffs.reshape(-1, 5)
    assert len({tuple(r) for r in flat.view(np.uint32).tolist()}) == flat.shape[0]      # all different
    return coeffs, np.ones((n_tables, nb), bool)


def _batch(lib, irs, nb=NB, plan=1, streams=S):
    import open_headstage_amd as ohs
    bp = ohs.BatchProcessor(streams, num_bands=nb, library=lib)
    for p in range(4):
        bp.set_ir(p, irs[p])
    bp.set_conv_plan(plan)
    return bp


class _Reference:
    """per stream: an oracle EQ refreshed per segment from that stream's row + an EQ-off batch of its own, called once per
    segment with that stream's gain, of which only that stream's row is kept"""

    def __init__(self, oracle, lib, irs, coeffs, en, streams=S, setup=None):
        from open_headstage_amd import synth
        self.coeffs, self.en, self.n = coeffs, en, streams
        self.eqs = [oracle.StereoParametricEQ(coeffs.shape[1], synth.FS) for _ in range(streams)]
        self.convs = [_batch(lib, irs, coeffs.shape[1], 1, streams) for _ in range(streams)]
        for c in self.convs:
            c.set_eq_enabled(False)
            if setup:
                setup(c)

    def refresh(self, s, table):
        for b in range(self.coeffs.shape[1]):
            self.eqs[s].set_band_coeffs(b, self.coeffs[table, b], bool(self.en[table, b]))

    def set_band(self, s, band, c, enabled):
        self.eqs[s].set_band_coeffs(band, c, bool(enabled))

    def set_gain(self, g):
        for c in self.convs:
            c.set_gain(float(g))

    def call(self, x, seg_blocks, idx, gains):
        """idx [S][n_segs] / [n_segs] / None (no refresh: the tables the EQs hold); gains likewise (None: the batches' gain)"""
        import torch
        n_blocks = x.shape[2] // 512
        n_segs = -(-n_blocks // seg_blocks)
        if idx is not None:
            idx = np.broadcast_to(np.asarray(idx), (self.n, n_segs))
        if gains is not None:
            gains = np.broadcast_to(np.asarray(gains, np.float32), (self.n, n_segs))
        xe = np.empty_like(x)
        out = np.empty_like(x)
        for k, b0 in enumerate(range(0, n_blocks, seg_blocks)):
            sl = slice(b0 * 512, min(b0 + seg_blocks, n_blocks) * 512)
            for s, q in enumerate(self.eqs):
                if idx is not None:
                    self.refresh(s, int(idx[s, k]))
                l, r = x[s, 0, sl].copy(), x[s, 1, sl].copy()
                q.process_block(l, r)
                xe[s, 0, sl], xe[s, 1, sl] = l, r
            d = torch.from_numpy(np.ascontiguousarray(xe[:, :, sl])).cuda()
            for s, c in enumerate(self.convs):
                if gains is not None:
                    c.set_gain(float(gains[s, k]))
                out[s, :, sl] = c.process(d)[s].cpu().numpy()
        return out


def _rows(n_blocks, seg_blocks, n_tables, call, streams=S, pool=None):
    """every stream its own index row and gain row; runs of different lengths: stream 0 constant throughout, stream 1 a new
    table every segment, stream 2 every third, the others every second / every segment with another phase"""
    n_segs = -(-n_blocks // seg_blocks)
    pool = list(range(n_tables)) if pool is None else pool
    idx = np.zeros((streams, n_segs), np.uint32)
    period = [0, 1, 3, 2, 1]
    for s in range(streams):
        p = period[s % len(period)]
        for k in range(n_segs):
            step = 0 if p == 0 else k // p
            idx[s, k] = pool[(s + 2 * call + step * (1 + s % 2)) % len(pool)] if len(pool) > 2 else pool[(s + call + step) % len(pool)]
    for s in range(streams):            # a run really ends where its period says
        p = period[s % len(period)]
        for k in range(1, n_segs):
            if p and k % p == 0 and idx[s, k] == idx[s, k - 1]:
                idx[s, k] = pool[(pool.index(int(idx[s, k])) + 1) % len(pool)]
    gains = (0.35 + 0.0137 * np.arange(n_segs)[None, :] + 0.00519 * np.arange(streams)[:, None] + 0.211 * call).astype(np.float32)
    assert len(set(gains.ravel().tolist())) == gains.size
    return idx, gains


def _same_bits(y, ref, what):
    for s in range(y.shape[0]):
        bad = np.flatnonzero(y[s].view(np.uint32).ravel() != ref[s].view(np.uint32).ravel())
        assert bad.size == 0, f"{what}: stream {s}, {bad.size} samples differ, first at {bad[:4]}"


def _two_calls(oracle, lib, blocks, seg_blocks, coeffs, en, in_place=False, setup=None, expect=None, rows_fn=None,
               expect_calls=None):
    import torch
    from open_headstage_amd import synth
    irs = synth.hrir_set(512)
    bp = _batch(lib, irs, coeffs.shape[1])
    bp.set_eq_enabled(True)
    bp.set_schedule_tables(coeffs, en)
    if setup:
        setup(bp)
    ref = _Reference(oracle, lib, irs, coeffs, en, setup=setup)
    x = synth.white_noise(range(500, 500 + S), sum(blocks) * 512)
    pos = 0
    for call, nb in enumerate(blocks):
        idx, gains = (rows_fn or _rows)(nb, seg_blocks, coeffs.shape[0], call)
        xc = np.ascontiguousarray(x[:, :, pos:pos + nb * 512])
        d = torch.from_numpy(xc.copy()).cuda()
        y = bp.process_scheduled_streams(d, seg_blocks, idx, gains, out=d if in_place else None)
        torch.cuda.synchronize()
        want = expect_calls[call] if expect_calls is not None else expect
        if want is not None:
            assert bp.last_eq_form() == want, bp.last_eq_form()
        _same_bits(y.cpu().numpy(), ref.call(xc, seg_blocks, idx, gains), f"call {call} ({nb} blocks, seg_blocks {seg_blocks})")
        pos += nb * 512
    return bp, ref


# ---- 1. every stream its own rows, runs of different lengths ----------------------------------------------------------------
@pytest.mark.parametrize("seg_blocks", [1, 2, 3])
def test_rows_per_stream_in_the_scheduled_wave_ring(oracle, seg_blocks):
    """five streams, six tables, a new table in every segment of stream 1, every third of stream 2, none of stream 0; a gain per
    stream and segment.  The handle must report the wave ring AND tables changing inside the launch: not the fallback."""
    from open_headstage_amd import _ffi
    coeffs, en = _tables(6)
    idx, _ = _rows(24, seg_blocks, 6, 0)
    assert len(set(idx[0].tolist())) == 1 and all(idx[1, k] != idx[1, k - 1] for k in range(1, idx.shape[1]))
    assert len({tuple(r) for r in idx.tolist()}) == S
    _two_calls(oracle, _ffi.lib(), [24, 17], seg_blocks, coeffs, en, expect=("wave_ring", True))


# ---- 2. different flags per stream in ONE launch ----------------------------------------------------------------------------
def _two_groups():
    """tables 0 - 3 enable all ten bands, 4 - 7 leave three out"""
    coeffs, en = _tables(8)
    en[4:, [1, 4, 8]] = False
    return coeffs, en


def test_streams_on_different_flags_share_one_launch(oracle):
    from open_headstage_amd import _ffi
    coeffs, en = _two_groups()

    def rows_fn(n_blocks, seg_blocks, n_tables, call):
        idx, gains = _rows(n_blocks, seg_blocks, 4, call)
        idx[1] += 4         # streams 1 and 3 live in the group of seven bands
        idx[3] += 4
        return idx, gains

    _two_calls(oracle, _ffi.lib(), [24, 17], 2, coeffs, en, rows_fn=rows_fn, expect=("wave_ring", True))


# ---- 3. flags that change in mid-call ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_flags_changing_for_one_stream_end_the_launch_for_all(oracle, in_place):
    """stream 1 changes groups in mid-call; band 4 goes off and on again for stream 2 only; stream 3 meets a table with no band
    at all (the fallback for that span); the other streams carry on through their own rows"""
    from open_headstage_amd import _ffi
    coeffs, en = _two_groups()
    coeffs = np.concatenate([coeffs, coeffs[:2]])
    en = np.concatenate([en, en[:2]])
    en[8, 4] = False            # table 8: table 0's coefficients, band 4 off
    en[9, :] = False            # table 9: no band

    def rows_fn(n_blocks, seg_blocks, n_tables, call):
        idx, gains = _rows(n_blocks, seg_blocks, 4, call)
        n_segs = idx.shape[1]
        idx[1, n_segs // 2:] += 4                   # to the group of seven bands, for good
        idx[2, n_segs // 3:n_segs // 3 + 2] = 8     # band 4 off for two segments, then on again
        idx[3, (2 * n_segs) // 3] = 9               # one segment without any band
        return idx, gains

    _two_calls(oracle, _ffi.lib(), [40, 23], 2, coeffs, en, rows_fn=rows_fn, in_place=in_place)


@pytest.mark.parametrize("exact", [False, True], ids=["ring_forms", "exact_specials"])
def test_segments_without_any_band_arrive_in_the_output(oracle, exact):
    """out of place, every stream on one table of its own, stream 3 on the table without bands (ring forms: its rows hand the
    samples on; exact-specials mode: that stream's launch sequence is a copy).  First call: two segments of 8 blocks = one span
    of 8 192 frames, the wave ring's threshold, then a segment in which NO stream has a band: copied through for all streams at
    once.  Second call: 1 024 frames, the rows."""
    from open_headstage_amd import _ffi
    coeffs, en = _tables(6)
    en[5, :] = False

    def rows_fn(n_blocks, seg_blocks, n_tables, call):
        n_segs = -(-n_blocks // seg_blocks)
        idx = np.repeat((np.arange(S, dtype=np.uint32) % 5)[:, None], n_segs, axis=1)
        idx[3] = 5
        if call == 0:
            idx[:, -1] = 5
        return idx, _rows(n_blocks, seg_blocks, 5, call)[1]

    _two_calls(oracle, _ffi.lib(), [24, 2], 8, coeffs, en, rows_fn=rows_fn,
               setup=(lambda bp: bp.set_eq_exact_specials(True)) if exact else None,
               expect_calls=[("conveyor" if exact else "wave_ring", False), ("conveyor" if exact else "row_ring", False)])


# ---- 4. call lengths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_blocks", [2, 3])
@pytest.mark.parametrize("blocks", [[16, 17], [18, 19], [70, 19]], ids=lambda b: "x".join(map(str, b)))
def test_call_lengths(oracle, blocks, seg_blocks):
    """16 .. 19 blocks: every tail of the four-group loop; 70 blocks: the overlap's time chunks cut between segment boundaries"""
    from open_headstage_amd import _ffi
    coeffs, en = _tables(6)
    _two_calls(oracle, _ffi.lib(), blocks, seg_blocks, coeffs, en)


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("blocks", [[70, 66], [7, 3]], ids=lambda b: "x".join(map(str, b)))
def test_overlapped_and_short_calls(oracle, blocks, in_place):
    from open_headstage_amd import _ffi
    coeffs, en = _tables(6)
    _two_calls(oracle, _ffi.lib(), blocks, 2, coeffs, en, in_place=in_place)


# ---- 5. the fallback forms ----------------------------------------------------------------------------------------------------
def test_row_form_forced(oracle, exp_tuning):
    from open_headstage_amd import _ffi
    exp_tuning.DEFAULTS.setdefault("eq_form", "0")
    exp_tuning("eq_form", 1)
    coeffs, en = _tables(6)
    _two_calls(oracle, _ffi.experiments_lib(), [24, 17], 2, coeffs, en, expect=("row_ring", False))


def test_wave_ring_forced_for_short_launches(oracle, exp_tuning):
    """(the experiments library: the wave ring whatever the launch's length, so 7-block calls take the scheduled kernel too)"""
    from open_headstage_amd import _ffi
    exp_tuning.DEFAULTS.setdefault("eq_form", "0")
    exp_tuning("eq_form", 2)
    coeffs, en = _tables(6)
    _two_calls(oracle, _ffi.experiments_lib(), [7, 4], 1, coeffs, en, expect=("wave_ring", True))


def test_exact_specials_mode(oracle):
    from open_headstage_amd import _ffi
    coeffs, en = _tables(6)
    _two_calls(oracle, _ffi.lib(), [24, 17], 2, coeffs, en, setup=lambda bp: bp.set_eq_exact_specials(True),
               expect=("conveyor", False))


def test_fourteen_bands(oracle):
    """more than 12 enabled bands: two passes of the per-stream ring form per span, never the scheduled kernel"""
    from open_headstage_amd import _ffi
    coeffs, en = _tables(4, nb=14)
    bp, _ = _two_calls(oracle, _ffi.lib(), [20, 17], 3, coeffs, en)
    assert bp.last_eq_form()[1] is False


@pytest.mark.parametrize("mode", [1, 2])
def test_denormal_modes(oracle, mode):
    from open_headstage_amd import _ffi
    coeffs, en = _tables(6)
    _two_calls(oracle, _ffi.lib(), [24, 17], 2, coeffs, en, setup=lambda bp: bp.set_flush_denormals(mode),
               expect=("wave_ring", True))


# ---- 6. one row for all streams == ohs_batch_process_scheduled; the handle's table and gain are not adopted -------------------
def test_shared_rows_are_the_scheduled_call_and_nothing_is_adopted(oracle):
    import torch
    from open_headstage_amd import _ffi, synth
    irs = synth.hrir_set(512)
    coeffs, en = _tables(6)
    nb1, nb2 = 20, 17
    x = synth.white_noise(range(40, 40 + S), (nb1 + nb2) * 512)
    a, b = _batch(_ffi.lib(), irs), _batch(_ffi.lib(), irs)
    ref = _Reference(oracle, _ffi.lib(), irs, coeffs, en)
    for bp in (a, b):
        bp.set_eq_enabled(True)
        bp.set_schedule_tables(coeffs, en)
        for band in range(NB):
            bp.set_band_coeffs(band, coeffs[5, band], True)
        bp.set_gain(0.8)
    for s in range(S):
        ref.refresh(s, 5)
    ref.set_gain(0.8)
    idx, gains = _rows(nb1, 2, 6, 0)
    idx, gains = idx[1].copy(), gains[1].copy()
    x1 = torch.from_numpy(np.ascontiguousarray(x[:, :, :nb1 * 512])).cuda()
    ya = a.process_scheduled_streams(x1, 2, idx, gains)              # idx_stride == 0, gain_stride == 0
    yb = b.process_scheduled(x1, 2, idx, gains)
    torch.cuda.synchronize()
    assert torch.equal(ya.view(torch.int32), yb.view(torch.int32))
    assert a.last_eq_form() == b.last_eq_form() == ("wave_ring", True)
    _same_bits(ya.cpu().numpy(), ref.call(x[:, :, :nb1 * 512], 2, idx, gains), "shared rows against the oracle")
    # a plain call: `a` continues with the table and gain it had BEFORE the call, the twin with the last segment's
    x2 = np.ascontiguousarray(x[:, :, nb1 * 512:])
    y2a = a.process(torch.from_numpy(x2).cuda())
    y2b = b.process(torch.from_numpy(x2).cuda())
    torch.cuda.synchronize()
    for s in range(S):
        ref.refresh(s, 5)
    ref.set_gain(0.8)
    want_a = ref.call(x2, nb2, None, None)
    _same_bits(y2a.cpu().numpy(), want_a, "plain call behind a per-stream scheduled one")
    assert not np.array_equal(y2b.cpu().numpy().view(np.uint32), want_a.view(np.uint32))       # (the twin adopted table and gain)


# ---- 7. gains only over static per-stream tables; tables only ---------------------------------------------------------------
def test_gains_only_over_static_stream_tables_and_tables_only(oracle):
    import torch
    from open_headstage_amd import _ffi, synth
    irs = synth.hrir_set(512)
    coeffs, en = _tables(6)
    nb1, nb2 = 20, 17
    x = synth.white_noise(range(60, 60 + S), (nb1 + nb2) * 512)
    bp = _batch(_ffi.lib(), irs)
    bp.set_eq_enabled(True)
    ref = _Reference(oracle, _ffi.lib(), irs, coeffs, en)
    for band in range(NB):                       # all streams start from table 0, streams 1 and 3 get bands of their own
        bp.set_band_coeffs(band, coeffs[0, band], True)
    for s in range(S):
        ref.refresh(s, 0)
    for s, band, t in [(1, 2, 3), (1, 7, 4), (3, 0, 2), (3, 5, 5)]:
        bp.set_stream_band_coeffs(s, band, coeffs[t, band], True)
        ref.set_band(s, band, coeffs[t, band], True)
    bp.set_stream_band_coeffs(3, 9, coeffs[0, 9], False)
    ref.set_band(3, 9, coeffs[0, 9], False)
    _, gains = _rows(nb1, 2, 6, 0)
    x1 = np.ascontiguousarray(x[:, :, :nb1 * 512])
    y = bp.process_scheduled_streams(torch.from_numpy(x1).cuda(), 2, None, gains)
    torch.cuda.synchronize()
    _same_bits(y.cpu().numpy(), ref.call(x1, 2, None, gains), "gains only over static per-stream tables")
    # tables only, on a handle back on the shared table
    bp.share_eq_table()
    bp.set_schedule_tables(coeffs, en)
    bp.set_gain(0.7)
    ref.set_gain(0.7)
    idx, _ = _rows(nb2, 2, 6, 1)
    x2 = np.ascontiguousarray(x[:, :, nb1 * 512:])
    y = bp.process_scheduled_streams(torch.from_numpy(x2).cuda(), 2, idx, None)
    torch.cuda.synchronize()
    assert bp.last_eq_form() == ("wave_ring", True)
    _same_bits(y.cpu().numpy(), ref.call(x2, 2, idx, None), "tables only")


# ---- 8. guard bands -----------------------------------------------------------------------------------------------------------
SENT_IN = np.uint32(0x7FA5A5A5)         # a NaN: an input gap that leaked into a chain would poison its output
SENT_OUT = np.uint32(0xDEADBEEF)


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("blocks", [17, 19, 70])
def test_guard_bands(oracle, blocks, in_place):
    import torch
    from open_headstage_amd import _ffi, synth
    frames = blocks * 512
    lead, cgap, sgap = 64, 61, 129
    cs = frames + cgap
    ss = 2 * cs + sgap
    total = lead + (S - 1) * ss + cs + frames
    mask = np.zeros(total, bool)
    for s in range(S):
        for c in range(2):
            mask[lead + s * ss + c * cs:lead + s * ss + c * cs + frames] = True
    irs = synth.hrir_set(512)
    coeffs, en = _tables(6)
    idx, gains = _rows(blocks, 2, 6, 0)
    x = synth.white_noise(range(70, 70 + S), frames)
    hin = np.full(total, SENT_IN, np.uint32).view(np.float32)
    for s in range(S):
        for c in range(2):
            hin[lead + s * ss + c * cs:lead + s * ss + c * cs + frames] = x[s, c]
    d_in = torch.from_numpy(hin.copy()).cuda()
    d_out = d_in if in_place else torch.from_numpy(np.full(total, SENT_OUT, np.uint32).view(np.float32)).cuda()
    bp = _batch(_ffi.lib(), irs)
    bp.set_eq_enabled(True)
    bp.set_schedule_tables(coeffs, en)
    bp.process_scheduled_streams_ptr(d_in.data_ptr() + 4 * lead, d_out.data_ptr() + 4 * lead, blocks, ss, cs, 2, idx, gains,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if blocks < 64:         # (an overlapped call's last time chunk is a few blocks: the row form)
        assert bp.last_eq_form() == ("wave_ring", True)
    out = d_out.cpu().numpy()
    sent = SENT_IN if in_place else SENT_OUT
    assert np.all(out.view(np.uint32)[~mask] == sent), np.flatnonzero(out.view(np.uint32)[~mask] != sent)[:8]
    if not in_place:
        assert np.array_equal(d_in.cpu().numpy().view(np.uint32), hin.view(np.uint32))       # the input is only read
    y = np.stack([np.stack([out[lead + s * ss + c * cs:lead + s * ss + c * cs + frames] for c in range(2)]) for s in range(S)])
    ref = _Reference(oracle, _ffi.lib(), irs, coeffs, en)
    _same_bits(y, ref.call(x, 2, idx, gains), f"{blocks} blocks")


# ---- 9. the whole chain against the reference's arithmetic --------------------------------------------------------------------
@pytest.mark.parametrize("taps,kernel", [(512, None), (2048, "block2048")])
def test_chain_against_the_oracle_per_segment_and_stream(oracle, taps, kernel):
    """oracle.chain_process per segment and stream with the refresh in front, <= 1e-6 RMS: 4 x 512 taps under the library's own
    plan, 4 x 2 048 taps (block 2048: the per-stream scale pass behind the launch)"""
    import torch
    from open_headstage_amd import _ffi, synth
    from tests.util import assert_parity
    irs = synth.hrir_set(taps)
    coeffs, en = _tables(6)
    bp = _batch(_ffi.lib(), irs, plan=0)
    bp.set_eq_enabled(True)
    bp.set_schedule_tables(coeffs, en)
    blocks, seg_blocks = [24, 17], 2
    x = synth.white_noise(range(90, 90 + S), sum(blocks) * 512)
    engines = []
    for s in range(S):
        eng = oracle.ConvolutionEngine()
        for p in range(4):
            eng.set_ir(p, irs[p])
        engines.append((eng, oracle.StereoParametricEQ(NB, synth.FS)))
    pos = 0
    for call, nb in enumerate(blocks):
        idx, gains = _rows(nb, seg_blocks, 6, call)
        xc = np.ascontiguousarray(x[:, :, pos:pos + nb * 512])
        y = bp.process_scheduled_streams(torch.from_numpy(xc).cuda(), seg_blocks, idx, gains).cpu().numpy()
        if kernel:
            assert bp.last_conv_plan()[0] == kernel, bp.last_conv_plan()
        ref = np.empty_like(xc)
        for k, b0 in enumerate(range(0, nb, seg_blocks)):
            sl = slice(b0 * 512, min(b0 + seg_blocks, nb) * 512)
            for s, (eng, eq) in enumerate(engines):
                for b in range(NB):
                    eq.set_band_coeffs(b, coeffs[idx[s, k], b], True)
                l, r = xc[s, 0, sl].copy(), xc[s, 1, sl].copy()
                oracle.chain_process(eng, eq, l, r, eq_enable=True, gain=float(gains[s, k]))
                ref[s, 0, sl], ref[s, 1, sl] = l, r
        for s in range(S):
            a, r = assert_parity(y[s], ref[s], f"{taps} taps, call {call}, stream {s}")
            print(f"taps {taps} call {call} stream {s}: abs RMS {a:.3e} rel RMS {r:.3e}")
        pos += nb * 512


# ---- 10. argument errors ------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_handle_usable(oracle):
    import ctypes as C
    import torch
    import open_headstage_amd as ohs
    from open_headstage_amd import _ffi, synth
    irs = synth.hrir_set(512)
    coeffs, en = _tables(4)
    bp = _batch(_ffi.lib(), irs)
    bp.set_eq_enabled(True)
    n_blocks, n_segs = 8, 4
    x = torch.from_numpy(synth.white_noise(range(S), n_blocks * 512)).cuda()
    idx = np.tile(np.array([0, 1, 2, 3], np.uint32), (S, 1))
    for s in range(S):
        idx[s] = np.roll(idx[s], s)
    gains = (0.5 + 0.05 * np.arange(S * n_segs, dtype=np.float32)).reshape(S, n_segs)
    L = _ffi.lib()
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)

    def raw(handle=True, d_in=True, d_out=True, seg_blocks=2, t=idx, ts=n_segs, g=gains, gs=n_segs, ss=2 * n_blocks * 512,
            cs=n_blocks * 512):
        y = torch.empty_like(x)
        return L.ohs_batch_process_scheduled_streams(
            bp._h if handle else None, C.c_void_p(x.data_ptr()) if d_in else None, C.c_void_p(y.data_ptr()) if d_out else None,
            n_blocks, ss, cs, seg_blocks, t.ctypes.data_as(u32p) if t is not None else None, ts,
            g.ctypes.data_as(f32p) if g is not None else None, gs, None)

    def refused(*a, **k):
        with pytest.raises(ohs.OhsError) as e:
            bp.process_scheduled_streams(*a, **k)
        assert e.value.status == _ffi.OHS_ERR_INVALID_ARG, e.value
        return str(e.value)

    refused(x, 2, idx, None)                                    # table_idx with no tables uploaded
    bp.set_schedule_tables(coeffs, en)
    assert raw(handle=False) == _ffi.OHS_ERR_INVALID_ARG        # NULL handle, NULL buffers
    assert raw(d_in=False) == _ffi.OHS_ERR_INVALID_ARG
    assert raw(d_out=False) == _ffi.OHS_ERR_INVALID_ARG
    refused(x, 0, None, None)                                   # seg_blocks == 0
    bad = idx.copy()
    bad[S - 1, n_segs - 1] = 4
    refused(x, 2, bad, None)                                    # an index out of range in the last row
    assert raw(ts=n_segs - 1) == _ffi.OHS_ERR_INVALID_ARG       # non-zero strides below n_segments
    assert raw(gs=n_segs - 1) == _ffi.OHS_ERR_INVALID_ARG
    assert raw(cs=n_blocks * 512 - 1) == _ffi.OHS_ERR_INVALID_ARG           # strides smaller than the processed region
    assert raw(ss=n_blocks * 512) == _ffi.OHS_ERR_INVALID_ARG
    bp.set_stream_band_coeffs(1, 2, coeffs[1, 2], True)
    assert "per-stream" in refused(x, 2, idx, None)             # table_idx on a handle with static per-stream tables
    bp.share_eq_table()
    bp.set_schedule_tables(np.zeros((0, NB, 5), np.float32), np.zeros((0, NB), bool))       # frees the set
    refused(x, 2, idx, None)
    bp.set_schedule_tables(coeffs, en)
    # ... and the handle still works: a correct call against the reference
    y = bp.process_scheduled_streams(x, 2, idx, gains)
    torch.cuda.synchronize()
    ref = _Reference(oracle, _ffi.lib(), irs, coeffs, en)
    _same_bits(y.cpu().numpy(), ref.call(x.cpu().numpy(), 2, idx, gains), "after the refused calls")


# ---- 11. the staging slots under mixed traffic ----------------------------------------------------------------------------------
def test_mixed_scheduled_calls_share_the_staging_slots():
    """One handle, no host synchronisation: three rounds of {per-stream EQ + gain schedule, crossfaded IR schedule with rows per
    stream and prev_idx, crossfaded layout schedule with rows per stream and prev_idx}, seg_blocks 1, 64 / 128 / 384 blocks.  Nine
    calls are more than two turns of the four staging slots, and the last round's EQ call stages 3 x 384 x 2 = 2304 entries -- more
    than a fresh slot's 2048 --, so a slot earlier calls used is regrown while others are in flight.  The yardstick: the same calls
    with a sync() behind each, the six stereo calls on one handle and the three layout calls on another (the two states are
    independent: test_gpu_layout_schedule.py's test_scheduled_layout_and_stereo_calls_do_not_touch_each_other).  Bit for bit.
    (The handle's own table has no band enabled here; the EQ state that layout and stereo calls SHARE is checked against the oracle in
    tests/test_gpu_fuzz_call_kinds.py.)"""
    import torch
    from open_headstage_amd import _ffi, synth
    from tests.test_cpu_ir_schedule import make_sets
    from tests.test_cpu_layout import make_input
    from tests.test_cpu_layout_schedule import make_table
    streams, K, n_choices, rounds = 3, 3, 4, [64, 128, 384]
    coeffs, en = _tables(n_choices)
    sets, table, irs = make_sets(n_choices), make_table(n_choices, K), synth.hrir_set(512)
    total = sum(rounds) * 512
    x_eq = torch.from_numpy(synth.white_noise(range(900, 900 + streams), total)).cuda()
    x_ir = torch.from_numpy(synth.white_noise(range(920, 920 + streams), total)).cuda()
    x_lay = torch.from_numpy(make_input(streams, K, sum(rounds), seed=6000)).cuda()
    rng = np.random.default_rng(2718)
    calls, pos = [], 0
    for nb in rounds:
        sl = slice(pos * 512, (pos + nb) * 512)
        rows = lambda: rng.integers(0, n_choices, (streams, nb)).astype(np.uint32)      # noqa: E731
        prev = lambda: rng.integers(0, n_choices, streams).astype(np.uint32)            # noqa: E731
        calls.append(("eq", x_eq[:, :, sl].contiguous(), rows(), rng.uniform(0.3, 0.9, (streams, nb)).astype(np.float32)))
        calls.append(("ir", x_ir[:, :, sl].contiguous(), rows(), prev()))
        calls.append(("layout", x_lay[:, :, sl].contiguous(), rows(), prev()))
        pos += nb
    assert calls[6][2].size + calls[6][3].size == 2304

    def handle():
        bp = _batch(_ffi.lib(), irs, streams=streams)
        bp.set_schedule_tables(coeffs, en)
        bp.set_schedule_irs(sets)
        bp.set_layout_table(table)
        bp.set_eq_enabled(True)         # (the handle's own table has no band enabled: the EQ state is the EQ-scheduled calls' alone)
        return bp

    def run(bp, kinds, sync):
        out = []
        for kind, x, idx, extra in calls:
            if kind not in kinds:
                continue
            if kind == "eq":
                out.append(bp.process_scheduled_streams(x, 1, idx, extra))
            elif kind == "ir":
                out.append(bp.process_ir_crossfaded(x, 1, idx, extra))
            else:
                out.append(bp.process_layout_scheduled(x, idx, 1, extra, True))
            if sync:
                bp.sync()
        torch.cuda.synchronize()
        return out

    mixed = run(handle(), ("eq", "ir", "layout"), False)
    stereo = iter(run(handle(), ("eq", "ir"), True))
    layout = iter(run(handle(), ("layout",), True))
    for i, (y, (kind, _, _, _)) in enumerate(zip(mixed, calls)):
        want = next(layout if kind == "layout" else stereo)
        assert torch.equal(y.view(torch.int32), want.view(torch.int32)), f"call {i} ({kind}, {y.shape[2] // 512} blocks)"

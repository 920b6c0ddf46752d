"""ohs_batch_process_scheduled: a schedule of EQ tables and gains inside ONE batch call -- what the reference does when its host
refreshes all bands and the master gain in front of every block (lib.rs:1180-1207; update_coefficients keeps s1, s2,
parametric_eq.rs:85-114).

The yardstick is the oracle driven the reference's way, never the code under test (the technique of test_gpu_stream_eq.py):
per stream an oracle StereoParametricEQ gets set_band_coeffs for every band from table table_idx[k] in front of segment k and
filters that segment; its output goes through a second batch with the EQ OFF, plan 1, called once per segment with
set_gain(gain[k]) in front -- existing, trusted entry points.  The convolution is a deterministic function of the bits it is
fed, and under plan 1 with taps <= 512 its bits do not depend on where calls cut the signal: the scheduled call (plan 1) must
equal that BIT FOR BIT.  Every case makes two consecutive scheduled calls, so that EQ state, overlaps and the handle's table
carry over."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S = 3
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
    """the oracle EQs refreshed per segment + the EQ-off batch called once per segment"""

    def __init__(self, oracle, lib, irs, coeffs, en, streams=S):
        from open_headstage_amd import synth
        self.coeffs, self.en = coeffs, en
        self.eqs = [oracle.StereoParametricEQ(coeffs.shape[1], synth.FS) for _ in range(streams)]
        self.conv = _batch(lib, irs, coeffs.shape[1], 1, streams)
        self.conv.set_eq_enabled(False)

    def refresh(self, table):
        for q in self.eqs:
            for b in range(self.coeffs.shape[1]):
                q.set_band_coeffs(b, self.coeffs[table, b], bool(self.en[table, b]))

    def eq_call(self, x, seg_blocks, table_idx):
        """x [S][2][n] -> the oracle's EQ output; table_idx None: no refresh (the tables the EQs hold)"""
        n_blocks = x.shape[2] // 512
        xe = np.empty_like(x)
        for k, b0 in enumerate(range(0, n_blocks, seg_blocks)):
            sl = slice(b0 * 512, min(b0 + seg_blocks, n_blocks) * 512)
            if table_idx is not None:
                self.refresh(int(table_idx[k]))
            for s, q in enumerate(self.eqs):
                l, r = x[s, 0, sl].copy(), x[s, 1, sl].copy()
                q.process_block(l, r)
                xe[s, 0, sl], xe[s, 1, sl] = l, r
        return xe

    def call(self, x, seg_blocks, table_idx, gains):
        import torch
        xe = self.eq_call(x, seg_blocks, table_idx)
        n_blocks = x.shape[2] // 512
        out = np.empty_like(x)
        for k, b0 in enumerate(range(0, n_blocks, seg_blocks)):
            sl = slice(b0 * 512, min(b0 + seg_blocks, n_blocks) * 512)
            if gains is not None:
                self.conv.set_gain(float(gains[k]))
            y = self.conv.process(torch.from_numpy(np.ascontiguousarray(xe[:, :, sl])).cuda())
            out[:, :, sl] = y.cpu().numpy()
        return out


def _schedule(n_blocks, seg_blocks, n_tables, call):
    n_segs = -(-n_blocks // seg_blocks)
    idx = np.array([(2 * call + (n_tables - 1) * k + k // n_tables) % n_tables for k in range(n_segs)], np.uint32)
    for k in range(1, n_segs):          # a new table in every segment
        if idx[k] == idx[k - 1]:
            idx[k] = (idx[k] + 1) % n_tables
    gains = (0.35 + 0.0137 * np.arange(n_segs) + 0.211 * call).astype(np.float32)
    assert len(set(gains.tolist())) == n_segs
    return idx, gains


def _same_bits(y, ref, what):
    for s in range(y.shape[0]):
        bad = np.flatnonzero(y[s].view(np.uint32).ravel() != ref[s].view(np.uint32).ravel())
        assert bad.size == 0, f"{what}: stream {s}, {bad.size} samples differ, first at {bad[:4]}"


def _two_calls(oracle, lib, blocks, seg_blocks, coeffs, en, in_place=False, setup=None, expect=None, idx_fn=None):
    import torch
    from open_headstage_amd import synth
    irs = synth.hrir_set(512)
    bp = _batch(lib, irs, coeffs.shape[1])
    bp.set_eq_enabled(True)
    bp.set_schedule_tables(coeffs, en)
    if setup:
        setup(bp)
    ref = _Reference(oracle, lib, irs, coeffs, en)
    if setup:
        setup(ref.conv)
    x = synth.white_noise(range(500, 500 + S), sum(blocks) * 512)
    pos = 0
    for call, nb in enumerate(blocks):
        idx, gains = (idx_fn or _schedule)(nb, seg_blocks, coeffs.shape[0], call)
        xc = np.ascontiguousarray(x[:, :, pos:pos + nb * 512])
        d = torch.from_numpy(xc.copy()).cuda()
        y = bp.process_scheduled(d, seg_blocks, idx, gains, out=d if in_place else None)
        torch.cuda.synchronize()
        if expect is not None:
            assert bp.last_eq_form() == expect, bp.last_eq_form()
        _same_bits(y.cpu().numpy(), ref.call(xc, seg_blocks, idx, gains), f"call {call} ({nb} blocks, seg_blocks {seg_blocks})")
        pos += nb * 512
    return bp, ref


# ---- 1. the wave-ring form: the tables change INSIDE the launch -------------------------------------------------------------
@pytest.mark.parametrize("seg_blocks", [1, 2, 3])
def test_wave_ring_scheduled_kernel_bit_exact(oracle, seg_blocks):
    """launches of 8 192 samples or more, six distinct tables, a new table and a new gain in every segment; the handle must
    report the wave ring AND the scheduled kernel, so the case cannot pass through the fallback"""
    from open_headstage_amd import _ffi
    coeffs, en = _tables(6)
    _two_calls(oracle, _ffi.lib(), [24, 17], seg_blocks, coeffs, en, expect=("wave_ring", True))


# ---- 2. call lengths: not a multiple of seg_blocks, around the ring's group of 48 and its four-group loop -------------------
@pytest.mark.parametrize("seg_blocks", [2, 3])
@pytest.mark.parametrize("blocks", [[16, 17], [18, 19], [70, 19]], ids=lambda b: "x".join(map(str, b)))
def test_call_lengths(oracle, blocks, seg_blocks):
    """16 .. 19 blocks: 170 .. 202 groups (every tail of the four-group loop); 70 blocks: the EQ || convolution overlap cuts
    the call into six EQ launches at block positions that are no segment boundaries"""
    from open_headstage_amd import _ffi
    coeffs, en = _tables(6)
    _two_calls(oracle, _ffi.lib(), blocks, seg_blocks, coeffs, en)


# ---- 3. enabled flags that change -------------------------------------------------------------------------------------------
def test_band_off_and_on_again_and_a_table_without_bands(oracle):
    """band 4 off in one segment and on again two segments later (its state frozen in between); a table with no band enabled
    in the middle of a call: the launch ends where the flags change, state travels through the state slots"""
    from open_headstage_amd import _ffi
    coeffs, en = _tables(6)
    en[2, 4] = False
    en[3, 4] = False
    en[5, :] = False

    def idx_fn(n_blocks, seg_blocks, n_tables, call):
        n_segs = -(-n_blocks // seg_blocks)
        base = [0, 1, 2, 3, 4, 0, 5, 1, 2, 4]           # 4 on | 2, 3: off | 4: on again ... 5: nothing enabled ... 2: off again
        idx = np.array([base[(k + 3 * call) % len(base)] for k in range(n_segs)], np.uint32)
        return idx, _schedule(n_blocks, seg_blocks, n_tables, call)[1]

    _two_calls(oracle, _ffi.lib(), [40, 23], 2, coeffs, en, idx_fn=idx_fn)
    _two_calls(oracle, _ffi.lib(), [20, 9], 1, coeffs, en, idx_fn=idx_fn, in_place=True)


# ---- 4. overlapped and short calls, in place and out of place ---------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("blocks", [[70, 66], [7, 3]], ids=lambda b: "x".join(map(str, b)))
def test_overlapped_and_short_calls(oracle, blocks, in_place):
    from open_headstage_amd import _ffi
    coeffs, en = _tables(6)
    _two_calls(oracle, _ffi.lib(), blocks, 2, coeffs, en, in_place=in_place)


# ---- 5. the fallback forms: one plain launch per run of equal tables --------------------------------------------------------
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
    """more than 12 enabled bands: not the ring form"""
    from open_headstage_amd import _ffi
    coeffs, en = _tables(4, nb=14)
    _two_calls(oracle, _ffi.lib(), [20, 17], 3, coeffs, en, expect=("conveyor", False))


@pytest.mark.parametrize("mode", [1, 2])
def test_denormal_modes(oracle, mode):
    """FTZ / FTZ | DAZ in the EQ and the convolution of both sides; the oracle EQ runs under the same MXCSR bits (the data are
    ordinary audio: no denormal arises, the modes' launches are what is exercised)"""
    from open_headstage_amd import _ffi
    coeffs, en = _tables(6)
    _two_calls(oracle, _ffi.lib(), [24, 17], 2, coeffs, en, setup=lambda bp: bp.set_flush_denormals(mode),
               expect=("wave_ring", True))


# ---- 6. constant schedules and mixing with plain calls ----------------------------------------------------------------------
def test_constant_schedule_is_the_plain_call_and_a_plain_call_continues(oracle):
    import torch
    from open_headstage_amd import _ffi, synth
    irs = synth.hrir_set(512)
    coeffs, en = _tables(6)
    nb1, nb2, nb3 = 20, 18, 17
    x = synth.white_noise(range(40, 40 + S), (nb1 + nb2 + nb3) * 512)
    a, b = _batch(_ffi.lib(), irs), _batch(_ffi.lib(), irs)
    for bp in (a, b):
        bp.set_eq_enabled(True)
        bp.set_schedule_tables(coeffs, en)
    x1 = torch.from_numpy(np.ascontiguousarray(x[:, :, :nb1 * 512])).cuda()
    # a constant schedule == the plain call with that table and gain
    ya = a.process_scheduled(x1, 2, np.full(nb1 // 2, 3, np.uint32), np.full(nb1 // 2, 0.6, np.float32))
    for band in range(NB):
        b.set_band_coeffs(band, coeffs[3, band], True)
    b.set_gain(0.6)
    yb = b.process(x1)
    torch.cuda.synchronize()
    assert torch.equal(ya.view(torch.int32), yb.view(torch.int32))
    assert a.last_eq_form() == ("wave_ring", False) and a.last_conv_plan() == b.last_conv_plan()
    # a scheduled call, then a plain one: it continues with the last segment's table and gain
    ref = _Reference(oracle, _ffi.lib(), irs, coeffs, en)
    ref.refresh(3)
    ref.conv.set_gain(0.6)
    _same_bits(ya.cpu().numpy(), ref.call(x[:, :, :nb1 * 512], nb1, None, None), "constant schedule against the oracle")
    idx, gains = _schedule(nb2, 2, 6, 1)
    x2 = np.ascontiguousarray(x[:, :, nb1 * 512:(nb1 + nb2) * 512])
    y2 = a.process_scheduled(torch.from_numpy(x2).cuda(), 2, idx, gains)
    torch.cuda.synchronize()
    _same_bits(y2.cpu().numpy(), ref.call(x2, 2, idx, gains), "scheduled call behind a plain one")
    x3 = np.ascontiguousarray(x[:, :, (nb1 + nb2) * 512:])
    y3 = a.process(torch.from_numpy(x3).cuda())
    torch.cuda.synchronize()
    _same_bits(y3.cpu().numpy(), ref.call(x3, nb3, None, None), "plain call behind a scheduled one")       # (last table, last gain)
    # gains alone (table_idx None: the handle's table throughout), then tables alone
    x4 = x2
    g4 = _schedule(nb2, 3, 6, 0)[1]
    y4 = a.process_scheduled(torch.from_numpy(x4).cuda(), 3, None, g4)
    torch.cuda.synchronize()
    _same_bits(y4.cpu().numpy(), ref.call(x4, 3, None, g4), "gains only")
    i5 = _schedule(nb2, 3, 6, 1)[0]
    y5 = a.process_scheduled(torch.from_numpy(x4).cuda(), 3, i5, None)
    torch.cuda.synchronize()
    _same_bits(y5.cpu().numpy(), ref.call(x4, 3, i5, None), "tables only")


# ---- 7. guard bands -------------------------------------------------------------------------------------------------------
SENT_IN = np.uint32(0x7FA5A5A5)         # a NaN: an input gap that leaked into a chain would poison its output
SENT_OUT = np.uint32(0xDEADBEEF)


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("blocks", [17, 19, 70])
def test_guard_bands(oracle, blocks, in_place):
    """sentinels in front of, between and behind every chain's frames (the last chain ends exactly at the end of its
    allocation): nothing outside is written, every sample inside is bit-exact"""
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
    idx, gains = _schedule(blocks, 2, 6, 0)
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
    bp.process_scheduled_ptr(d_in.data_ptr() + 4 * lead, d_out.data_ptr() + 4 * lead, blocks, ss, cs, 2, idx, gains,
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


# ---- the whole chain against the reference's arithmetic -------------------------------------------------------------------
@pytest.mark.parametrize("taps,kernel", [(512, None), (2048, "block2048")])
def test_chain_against_the_oracle_per_segment(oracle, taps, kernel):
    """oracle.chain_process (EQ -> convolution -> gain, lib.rs:1169-1207) called per segment with the refresh in front, <= 1e-6
    RMS: 4 x 512 taps under the library's own plan, 4 x 2 048 taps (block 2048: the gain's scale pass behind the launch)"""
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
        idx, gains = _schedule(nb, seg_blocks, 6, call)
        xc = np.ascontiguousarray(x[:, :, pos:pos + nb * 512])
        y = bp.process_scheduled(torch.from_numpy(xc).cuda(), seg_blocks, idx, gains).cpu().numpy()
        if kernel:
            assert bp.last_conv_plan()[0] == kernel, bp.last_conv_plan()
        ref = np.empty_like(xc)
        for k, b0 in enumerate(range(0, nb, seg_blocks)):
            sl = slice(b0 * 512, min(b0 + seg_blocks, nb) * 512)
            for s, (eng, eq) in enumerate(engines):
                for b in range(NB):
                    eq.set_band_coeffs(b, coeffs[idx[k], b], True)
                l, r = xc[s, 0, sl].copy(), xc[s, 1, sl].copy()
                oracle.chain_process(eng, eq, l, r, eq_enable=True, gain=float(gains[k]))
                ref[s, 0, sl], ref[s, 1, sl] = l, r
        for s in range(S):
            a, r = assert_parity(y[s], ref[s], f"{taps} taps, call {call}, stream {s}")
            print(f"taps {taps} call {call} stream {s}: abs RMS {a:.3e} rel RMS {r:.3e}")
        pos += nb * 512


# ---- argument errors ------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_handle_usable(oracle):
    import torch
    import open_headstage_amd as ohs
    from open_headstage_amd import _ffi, synth
    irs = synth.hrir_set(512)
    coeffs, en = _tables(4)
    bp = _batch(_ffi.lib(), irs)
    bp.set_eq_enabled(True)
    x = torch.from_numpy(synth.white_noise(range(S), 8 * 512)).cuda()
    idx = np.array([0, 1, 2, 3], np.uint32)

    def refused(*a, **k):
        with pytest.raises(ohs.OhsError) as e:
            bp.process_scheduled(*a, **k)
        assert e.value.status == _ffi.OHS_ERR_INVALID_ARG, e.value
        return str(e.value)

    refused(x, 2, idx, None)                                    # no tables uploaded
    bp.set_schedule_tables(coeffs, en)
    refused(x, 0, None, None)                                   # seg_blocks == 0
    refused(x, 2, np.array([0, 1, 4, 3], np.uint32), None)      # index out of range
    bp.set_stream_band_coeffs(1, 2, coeffs[1, 2], True)
    assert "per-stream" in refused(x, 2, idx, None)
    bp.share_eq_table()
    bp.set_schedule_tables(np.zeros((0, NB, 5), np.float32), np.zeros((0, NB), bool))       # frees the set
    refused(x, 2, idx, None)
    bp.set_schedule_tables(coeffs, en)
    # ... and the handle still works: the same call against the reference
    gains = np.array([0.5, 0.25, 1.0, 0.75], np.float32)
    y = bp.process_scheduled(x, 2, idx, gains)
    torch.cuda.synchronize()
    ref = _Reference(oracle, _ffi.lib(), irs, coeffs, en)
    _same_bits(y.cpu().numpy(), ref.call(x.cpu().numpy(), 2, idx, gains), "after the refused calls")

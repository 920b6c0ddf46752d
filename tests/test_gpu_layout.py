"""ohs_batch_process_layout: K input channels (5.1, 7.1, up to 16) to a binaural pair in one kernel.

The yardstick is never the code under test: the f64 model of tests/test_cpu_layout.py (direct convolution per channel and ear,
summed), the oracle's ConvolutionEngine per pair of channels summed in f32 (checked against the model there), the oracle's
StereoParametricEQ, or the EXISTING ohs_batch_process on a second handle.  Bars: bit for bit where the header promises bits,
1e-6 relative RMS per stream -- the project's FFT bar, DESIGN section 2 -- everywhere else.  Gain 0.7 throughout."""
import ctypes as C

import numpy as np
import pytest

from tests.test_cpu_layout import BAR, BLOCK, engines_layout, make_input, make_layout, model_layout_f64, rel_rms_per_stream

pytestmark = pytest.mark.gpu

S = 5
NB = 10
GAIN = 0.7


@pytest.fixture(scope="module")
def lib():
    from open_headstage_amd import _ffi
    return _ffi.lib()


def _batch(lib, irs=None, streams=S, eq=False):
    import open_headstage_amd as ohs
    bp = ohs.BatchProcessor(streams, num_bands=NB, library=lib)
    bp.set_conv_plan(1)
    bp.set_gain(GAIN)
    if irs is not None:
        bp.set_layout_irs(irs)
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
    """x [S][2][frames] through the oracle's EQ (synth's table), per stream; eqs: the instances of an earlier call (state carried)"""
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
    assert y.shape == ref.shape, what
    assert float(np.abs(ref).max()) > 0.01, what
    for s in range(y.shape[0]):
        bad = np.flatnonzero(y[s].view(np.uint32).ravel() != ref[s].view(np.uint32).ravel())
        assert bad.size == 0, f"{what}: stream {s}, {bad.size} samples differ, first at {bad[:4]}"


def _within_bar(y, ref, what):
    err = rel_rms_per_stream(y, ref)
    print(f"{what}: relative RMS per stream, worst {err.max():.3e}")
    assert (err <= BAR).all(), f"{what}: relative RMS per stream {err} (bar {BAR:.0e})"


def _run(bp, x):
    import torch
    y = bp.process_layout(torch.from_numpy(np.ascontiguousarray(x).copy()).cuda())
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _run_calls(bp, x, cuts):
    """x in consecutive calls of `cuts` blocks each"""
    out, pos = [], 0
    for nb in cuts:
        out.append(_run(bp, x[:, :, pos:pos + nb * BLOCK]))
        pos += nb * BLOCK
    assert pos == x.shape[2]
    return np.concatenate(out, axis=2)


def _plain(bp, x):
    import torch
    y = bp.process(torch.from_numpy(np.ascontiguousarray(x).copy()).cuda())
    torch.cuda.synchronize()
    return y.cpu().numpy()


# ---- a. two channels are the stereo call under plan 1, bit for bit --------------------------------------------------------------
@pytest.mark.parametrize("taps", [512, 200])
def test_two_channels_are_the_stereo_call_bit_for_bit(lib, taps):
    irs = make_layout(2, taps)
    x = make_input(S, 2, 13, seed=1000)
    bp, ref = _batch(lib, irs), _batch(lib)
    for path, h in enumerate([irs[0, 0], irs[0, 1], irs[1, 0], irs[1, 1]]):       # Lsl, Lsr, Rsl, Rsr
        ref.set_ir(path, h)
    want = _plain(ref, x)
    assert ref.last_conv_plan()[0] == "block512_p1"
    _same_bits(_run(bp, x), want, f"K = 2, {taps} taps")
    assert bp.last_layout_launch()[0] == 1


# ---- b. against the f64 model and against the summed oracle engines -----------------------------------------------------------
@pytest.mark.parametrize("K,taps", [(1, 512), (3, 512), (6, 512), (8, 512), (16, 512), (6, 1), (6, 200)])
def test_layouts_against_the_f64_model_and_the_summed_engines(lib, oracle, K, taps):
    irs = make_layout(K, taps)
    x = make_input(S, K, 13, seed=1100)
    bp = _batch(lib, irs)
    y = _run(bp, x)
    assert bp.last_layout_launch()[0] == (K + 1) // 2
    _within_bar(y, model_layout_f64(oracle, x, irs, GAIN), f"K = {K}, {taps} taps vs the f64 model")
    _within_bar(y, engines_layout(oracle, x, irs, GAIN)[0], f"K = {K}, {taps} taps vs the summed oracle engines")


# ---- c. odd K: the channel behind the last one is never read -------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 5])
def test_odd_layouts_do_not_read_the_channel_behind_the_last(lib, oracle, K):
    irs = make_layout(K)
    x = make_input(S, K, 13, seed=1200)
    xn = np.concatenate([x, np.full((S, 1, x.shape[2]), np.nan, np.float32)], axis=1)      # [S][K + 1][frames]
    bp = _batch(lib, irs)
    y = _run(bp, xn)
    assert np.isfinite(y).all()
    _within_bar(y, model_layout_f64(oracle, x, irs, GAIN), f"K = {K} with a NaN channel behind it")


# ---- d. the bits do not depend on where the signal is cut into calls -------------------------------------------------------------
def test_call_cuts_do_not_change_the_bits(lib):
    irs = make_layout(6)
    x = make_input(S, 6, 13, seed=1300)
    whole = _run(_batch(lib, irs), x)
    _same_bits(_run_calls(_batch(lib, irs), x, [1, 5, 7]), whole, "1 + 5 + 7 blocks against 13")


# ---- e. ... nor on the number of chunks per stream ------------------------------------------------------------------------------
def test_chunks_per_stream_do_not_change_the_bits(lib):
    irs = make_layout(6)
    x = make_input(2, 6, 40, seed=1400)
    bp = _batch(lib, irs, streams=2)
    whole = _run(bp, x)
    assert bp.last_layout_launch()[1] > 1, bp.last_layout_launch()
    one = _batch(lib, irs, streams=2)
    single = _run_calls(one, x, [1] * 40)
    assert one.last_layout_launch() == (3, 1)
    _same_bits(whole, single, "2 streams x 40 blocks in chunks against forty 1-block calls")


# ---- f. reset and a second set_layout_irs zero the overlap -----------------------------------------------------------------------
def test_reset_and_a_new_layout_zero_the_overlap(lib):
    irs, other = make_layout(6), make_layout(6, seed=12)
    x = make_input(S, 6, 9, seed=1500)
    fresh = _run(_batch(lib, irs), x)
    bp = _batch(lib, irs)
    first = _run(bp, x)
    _same_bits(first, fresh, "first call")
    again = _run(bp, x)                 # (the overlap of the first call rings into this one)
    assert (rel_rms_per_stream(again[:, :, :BLOCK], fresh[:, :, :BLOCK]) > 1e-3).all()
    bp.reset()
    _same_bits(_run(bp, x), fresh, "behind ohs_batch_reset")
    bp.set_layout_irs(other)
    bp.set_layout_irs(irs)
    _same_bits(_run(bp, x), fresh, "behind a second set_layout_irs")
    bp.set_layout_irs(other)
    _same_bits(_run(bp, x), _run(_batch(lib, other), x), "another layout")


# ---- g. the layout's overlap and the stereo state are independent ----------------------------------------------------------------
def test_layout_and_stereo_calls_do_not_touch_each_other(lib):
    from tests.test_cpu_ir_schedule import make_sets
    irs = make_layout(6)
    own = make_sets(1)[0]
    x = make_input(S, 6, 14, seed=1600)
    xs = make_input(S, 2, 7, seed=1650)

    def handle():
        bp = _batch(lib, irs)
        for p in range(4):
            bp.set_ir(p, own[p])
        return bp

    mixed, alone, stereo = handle(), handle(), handle()
    a1 = _run(mixed, x[:, :, :6 * BLOCK])
    st = _plain(mixed, xs)
    a2 = _run(mixed, x[:, :, 6 * BLOCK:])
    st2 = _plain(mixed, xs)
    _same_bits(np.concatenate([a1, a2], axis=2), _run_calls(alone, x, [6, 8]), "layout, stereo, layout against the layout calls alone")
    _same_bits(st, _plain(stereo, xs), "the stereo call between the layout calls")
    _same_bits(st2, _plain(stereo, xs), "the second stereo call")


# ---- h. EQ on: the oracle's EQ on the ear signals, state carried across calls ---------------------------------------------------
def test_eq_filters_the_ear_signals_after_the_convolution(lib, oracle):
    irs = make_layout(6)
    x = make_input(S, 6, 12, seed=1700)
    cuts = [5, 7]
    off, on = _batch(lib, irs), _batch(lib, irs, eq=True)
    pos, eqs = 0, None
    for call, nb in enumerate(cuts):
        xc = x[:, :, pos:pos + nb * BLOCK]
        dry = _run(off, xc)
        ref, eqs = _oracle_eq(oracle, dry, eqs)
        got = _run(on, xc)
        assert (rel_rms_per_stream(got, dry) > 1e-3).all()          # (the EQ does something)
        _same_bits(got, ref, f"EQ on, call {call}")
        pos += nb * BLOCK


# ---- i. padded strides on both sides --------------------------------------------------------------------------------------------
def test_padded_strides_and_untouched_padding(lib):
    import torch
    K, blocks = 6, 7
    irs = make_layout(K)
    x = make_input(S, K, blocks, seed=1800)
    frames = blocks * BLOCK
    want = _run(_batch(lib, irs), x)
    in_cs, in_ss = frames + 96, (K + 1) * (frames + 96) + 32
    out_cs, out_ss = frames + 160, 2 * (frames + 160) + 64
    SENT = np.float32(-777.25)
    xin = np.full(S * in_ss, SENT, np.float32)
    for s in range(S):
        for c in range(K):
            xin[s * in_ss + c * in_cs: s * in_ss + c * in_cs + frames] = x[s, c]
    d_in = torch.from_numpy(xin).cuda()
    d_out = torch.full((S * out_ss,), float(SENT), dtype=torch.float32, device="cuda")
    bp = _batch(lib, irs)
    bp.process_layout_ptr(d_in.data_ptr(), d_out.data_ptr(), blocks, in_ss, in_cs, out_ss, out_cs,
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
    assert (d_in.cpu().numpy() == xin).all(), "the input was written"
    _same_bits(y, want, "padded strides against the contiguous run")


# ---- j. every refused call leaves the handle usable ------------------------------------------------------------------------------
def test_argument_errors_leave_the_handle_usable(lib):
    import torch
    from open_headstage_amd import _ffi
    K, blocks = 6, 4
    irs = make_layout(K)
    x = make_input(S, K, blocks, seed=1900)
    frames = blocks * BLOCK
    d = torch.from_numpy(x.copy()).cuda()
    out = torch.empty((S, 2, frames), dtype=torch.float32, device="cuda")
    INV, OK = _ffi.OHS_ERR_INVALID_ARG, _ffi.OHS_OK

    def call(bp, d_in=None, d_out=None, n_blocks=blocks, in_ss=K * frames, in_cs=frames, out_ss=2 * frames, out_cs=frames):
        return lib.ohs_batch_process_layout(bp._h if bp is not None else None, C.c_void_p(d.data_ptr() if d_in is None else d_in),
                                            C.c_void_p(out.data_ptr() if d_out is None else d_out), n_blocks, in_ss, in_cs,
                                            out_ss, out_cs, None)

    bp, twin = _batch(lib, irs), _batch(lib, irs)
    assert call(None) == INV
    assert lib.ohs_batch_process_layout(bp._h, None, C.c_void_p(out.data_ptr()), blocks, K * frames, frames, 2 * frames, frames, None) == INV
    assert lib.ohs_batch_process_layout(bp._h, C.c_void_p(d.data_ptr()), None, blocks, K * frames, frames, 2 * frames, frames, None) == INV
    p, r = C.c_int(), C.c_int()
    assert lib.ohs_batch_last_layout_launch(bp._h, None, C.byref(r)) == INV
    assert lib.ohs_batch_last_layout_launch(bp._h, C.byref(p), C.byref(r)) == OK and (p.value, r.value) == (0, 0)
    assert call(_batch(lib)) == INV                                 # no layout uploaded
    fp = _ffi.fp
    big = np.zeros((17, 2, 8), np.float32)
    assert lib.ohs_batch_set_layout_irs(bp._h, 17, big.ctypes.data_as(fp), 8) == INV          # n_channels > 16
    assert lib.ohs_batch_set_layout_irs(bp._h, K, irs.ctypes.data_as(fp), 0) == INV           # len == 0
    assert lib.ohs_batch_set_layout_irs(bp._h, 2, np.zeros((2, 2, 513), np.float32).ctypes.data_as(fp), 513) == INV    # len > 512
    assert lib.ohs_batch_set_layout_irs(bp._h, K, None, 512) == INV
    assert call(bp, in_cs=frames - 1) == INV and call(bp, out_cs=frames - 1) == INV          # strides below the region
    assert call(bp, in_ss=K * frames - 1) == INV and call(bp, out_ss=2 * frames - 1) == INV
    assert call(bp, in_ss=frames) == INV
    assert call(bp, d_out=d.data_ptr()) == INV                      # in place
    assert call(bp, d_out=d.data_ptr() + 4 * (S * K * frames - 1)) == INV                    # the regions meet in one frame
    assert call(bp, d_in=out.data_ptr() + 4 * frames, n_blocks=1, in_ss=K * BLOCK, in_cs=BLOCK, out_ss=2 * frames) == INV   # ... the other way round
    assert call(bp, n_blocks=(1 << 24) + 1, in_cs=1 << 40, in_ss=1 << 50, out_cs=1 << 40, out_ss=1 << 50) == INV
    # ... and none of them queued anything or touched the state: the layout uploaded first still serves, as on the twin
    assert call(bp) == OK
    torch.cuda.synchronize()
    got = out.cpu().numpy().copy()
    assert lib.ohs_batch_last_layout_launch(bp._h, C.byref(p), C.byref(r)) == OK and p.value == 3 and r.value >= 1
    _same_bits(got, _run(twin, x), "the valid call behind the refused ones")
    _same_bits(_run(bp, x), _run(twin, x), "and the call after it")

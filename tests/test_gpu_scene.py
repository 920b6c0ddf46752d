"""ohs_scene_process (libohs_scene.so): K independently moving sources per stream to a binaural pair in one kernel.

The yardstick is never the code under test: the f64 model of tests/scene_model.py (checked against a direct time-domain evaluation in
tests/test_cpu_scene.py), the EXISTING layout calls of the product library on a second handle, the oracle's StereoParametricEQ.  Bars:
bit for bit where include/ohs_scene.h promises bits, 1e-6 relative RMS -- the project's FFT bar, DESIGN section 2 -- per stream AND per
512-frame block everywhere else.  3 streams, 7 directions, gain 0.7 throughout."""
import ctypes as C

import numpy as np
import pytest

from tests import guard_bands as gb
from tests import scene_model as sm
from tests.test_cpu_layout import BAR, BLOCK, make_input, make_layout, rel_rms_per_stream
from tests.test_cpu_scene import rel_rms_per_block
from tests.test_gpu_layout import _batch, _eq_bands, _oracle_eq, _same_bits

pytestmark = pytest.mark.gpu

S = 3
NB = 10
GAIN = 0.7
N_DIRS = 7
# (K, taps, seg_blocks, a shared row, blocks): odd K and K = 1, 8 and 512 taps, a shared row and rows per stream
TRAJECTORY_CASES = [(1, 512, 1, False, 6), (2, 8, 2, False, 7), (3, 512, 2, False, 8), (5, 512, 3, True, 12), (8, 512, 2, False, 6)]


def trajectory_case(K, taps, seg_blocks, shared, blocks):
    """-> (x, dirs, idx, seg_blocks, gains, prev_idx, prev_gains) of one case (tests/test_cpu_scene.py runs the mutants on these)"""
    dirs = make_layout(N_DIRS, taps)
    x = make_input(S, K, blocks, seed=6000 + 10 * K)
    idx, gains, pi, pg = sm.make_scene(S, K, blocks, seg_blocks, N_DIRS, seed=K, shared=shared)
    return x, dirs, idx, seg_blocks, gains, pi, pg


@pytest.fixture(scope="module")
def lib():
    from open_headstage_amd import _ffi
    return _ffi.lib()


def _scene(dirs=None, streams=S, eq=False):
    import open_headstage_amd as ohs
    sc = ohs.SceneProcessor(streams, num_bands=NB)
    sc.set_gain(GAIN)
    if dirs is not None:
        sc.set_directions(dirs)
    if eq:
        for i, (c, en) in enumerate(_eq_bands()):
            sc.set_band_coeffs(i, c, en)
        sc.set_eq_enabled(True)
    return sc


def _run(sc, x, idx, seg_blocks, gains=None, prev_idx=None, prev_gains=None, crossfade=True):
    import torch
    y = sc.process(torch.from_numpy(np.ascontiguousarray(x).copy()).cuda(), idx, seg_blocks, gains, prev_idx, prev_gains, crossfade)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _within_bar(y, ref, what):
    e, eb = rel_rms_per_stream(y, ref), rel_rms_per_block(y, ref)
    print(f"{what}: relative RMS per stream, worst {e.max():.3e}; per 512-frame block, worst {eb.max():.3e}")
    assert np.isfinite(y).all(), what
    assert (e <= BAR).all(), f"{what}: relative RMS per stream {e} (bar {BAR:.0e})"
    assert (eb <= BAR).all(), f"{what}: relative RMS per block, worst {eb.max():.3e} at {np.unravel_index(eb.argmax(), eb.shape)} (bar {BAR:.0e})"


# ---- a. a static scene is the layout call on those directions, bit for bit -------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 5])
def test_static_scene_is_the_layout_call_bit_for_bit(lib, K):
    import torch
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S, K, 9, seed=6100 + K)
    row = np.array([4, 0, 6, 2, 4], np.uint32)[:K]
    ref = _batch(lib, dirs[row], S)
    sc = _scene(dirs)
    pos = 0
    for call, nb in enumerate([4, 5]):          # (the second call continues the first one's overlap)
        xc = np.ascontiguousarray(x[:, :, pos * BLOCK:(pos + nb) * BLOCK])
        want = ref.process_layout(torch.from_numpy(xc.copy()).cuda())
        torch.cuda.synchronize()
        y = _run(sc, xc, np.repeat(row[None], 3, axis=0), 2)
        assert sc.last_launch()[0] == (K + 1) // 2 and sc.last_launch()[2] == 0
        _same_bits(y, want.cpu().numpy(), f"K = {K}, static scene, call {call}")
        pos += nb


# ---- b. every object switching in every segment is the scheduled layout call on the table of those sets ---------------------------
@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("fade", [True, False])
def test_all_objects_switching_is_the_scheduled_layout_call_bit_for_bit(lib, K, fade):
    import torch
    blocks, seg = 9, 2
    n_segs = 5
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S, K, blocks, seed=6200 + K)
    idx, prev = sm.make_switching_rows(S, K, n_segs, N_DIRS, seed=K)
    assert (idx[:, 1:] != idx[:, :-1]).all() and (idx[:, 0] != prev).all()
    # one set of the layout table per (stream, segment), and one per stream for what stood in front
    combos = np.concatenate([prev[:, None], idx], axis=1)                       # [S][n_segs + 1][K]
    table = dirs[combos.reshape(-1, K)]                                         # [S * (n_segs + 1)][K][2][512]
    set_idx = (np.arange(S)[:, None] * (n_segs + 1) + 1 + np.arange(n_segs)[None, :]).astype(np.uint32)
    set_prev = (np.arange(S) * (n_segs + 1)).astype(np.uint32)
    ref = _batch(lib, None, S)
    ref.set_layout_table(table)
    want = ref.process_layout_scheduled(torch.from_numpy(x.copy()).cuda(), set_idx, seg, set_prev if fade else None, fade)
    torch.cuda.synchronize()
    assert ref.last_layout_scheduled()
    sc = _scene(dirs)
    y = _run(sc, x, idx, seg, None, prev if fade else None, None, fade)
    pairs = (K + 1) // 2
    assert sc.last_launch()[0] == pairs and sc.last_launch()[2] == (S * n_segs * pairs if fade else 0), sc.last_launch()
    _same_bits(y, want.cpu().numpy(), f"K = {K}, every object switching, crossfade {fade}")


# ---- c. independent trajectories with gains, against the f64 model ------------------------------------------------------------------
_model_cache = {}


def _model(case, fade=True):
    if (case, fade) not in _model_cache:
        x, dirs, idx, seg, gains, pi, pg = trajectory_case(*case)
        _model_cache[(case, fade)] = sm.model_scene_f64(x, dirs, idx, seg, gains, pi, pg, fade, GAIN)
    return _model_cache[(case, fade)]


@pytest.mark.parametrize("case", TRAJECTORY_CASES, ids=lambda c: f"K{c[0]}-taps{c[1]}-seg{c[2]}-{'shared' if c[3] else 'rows'}")
def test_independent_trajectories_against_the_f64_model(case):
    x, dirs, idx, seg, gains, pi, pg = trajectory_case(*case)
    K = case[0]
    sc = _scene(dirs)
    y = _run(sc, x, idx, seg, gains, pi, pg)
    pairs, ranges, fading = sc.last_launch()
    assert pairs == (K + 1) // 2 and fading > 0
    _within_bar(y, _model(case), f"case {case}, CROSSFADE")
    if K > 2:
        assert not (gains if gains.ndim == 2 else gains[0])[:, K - 1].any()      # (the silent object)


def test_ring_out_against_the_f64_model():
    case = TRAJECTORY_CASES[2]
    x, dirs, idx, seg, gains, pi, pg = trajectory_case(*case)
    sc = _scene(dirs)
    y = _run(sc, x, idx, seg, gains, pi, pg, crossfade=False)
    assert sc.last_launch()[2] == 0
    _within_bar(y, _model(case, False), f"case {case}, RING_OUT")
    assert (rel_rms_per_stream(_model(case, False), _model(case, True)) > 1e-3).all()


# ---- d. the bits do not depend on cuts, chunks or the neighbours -----------------------------------------------------------------------
def test_cuts_chunks_and_neighbours_do_not_change_the_bits():
    K, blocks, seg = 3, 24, 2
    dirs = make_layout(N_DIRS, 512)
    x3 = make_input(S, K, blocks, seed=6400)
    idx3, gains3, pi3, pg3 = sm.make_scene(S, K, blocks, seg, N_DIRS, seed=40)
    x, idx, gains, pi, pg = x3[1:2], idx3[1:2], gains3[1:2], pi3[1:2], pg3[1:2]       # (stream 1 alone)
    one = _scene(dirs, 1)
    whole = _run(one, x, idx, seg, gains, pi, pg)
    assert one.last_launch()[1] > 1, one.last_launch()         # many ranges, each with a dry block in front
    _within_bar(whole, sm.model_scene_f64(x, dirs, idx, seg, gains, pi, pg, True, GAIN), "one stream, 24 blocks in one call")
    # per block: the entries of the block's segment, and in front of it the previous block's (prev_* in front of the first)
    bi, bg = np.repeat(idx, seg, axis=1), np.repeat(gains, seg, axis=1)         # [1][blocks][K]
    for cuts in ([1, 5, 7, 11], [1] * blocks):
        sc = _scene(dirs, 1)
        out, pos = [], 0
        for nb in cuts:
            p_i, p_g = (pi, pg) if pos == 0 else (bi[:, pos - 1], bg[:, pos - 1])
            out.append(_run(sc, x[:, :, pos * BLOCK:(pos + nb) * BLOCK], np.ascontiguousarray(bi[:, pos:pos + nb]), 1,
                            np.ascontiguousarray(bg[:, pos:pos + nb]), p_i, p_g))
            pos += nb
        assert pos == blocks
        _same_bits(np.concatenate(out, axis=2), whole, f"calls of {cuts if len(cuts) < 5 else 'one block each'} against one call")
    y3 = _run(_scene(dirs, S), x3, idx3, seg, gains3, pi3, pg3)
    _same_bits(y3[1:2], whole, "the same stream inside a 3-stream handle")
    # without prev_* a cut at a change of direction does not fade: far off
    cut = next(t for t in range(2, blocks, 2) if (bi[0, t] != bi[0, t - 1]).any())
    sc = _scene(dirs, 1)
    a = _run(sc, x[:, :, :cut * BLOCK], np.ascontiguousarray(bi[:, :cut]), 1, np.ascontiguousarray(bg[:, :cut]), pi, pg)
    b = _run(sc, x[:, :, cut * BLOCK:], np.ascontiguousarray(bi[:, cut:]), 1, np.ascontiguousarray(bg[:, cut:]))
    _same_bits(a, whole[:, :, :cut * BLOCK], "the call in front of the cut")
    d = rel_rms_per_stream(b[:, :, :BLOCK], whole[:, :, cut * BLOCK:(cut + 1) * BLOCK])
    print(f"the block behind a cut at block {cut} without prev_*: relative RMS {d}")
    assert (d > 1e3 * BAR).all(), d


# ---- e. EQ on, and reset ----------------------------------------------------------------------------------------------------------------
def test_eq_filters_the_ear_signals_and_reset_gives_a_new_handles_bits(oracle):
    case = TRAJECTORY_CASES[2]
    x, dirs, idx, seg, gains, pi, pg = trajectory_case(*case)
    off, on = _scene(dirs), _scene(dirs, eq=True)
    dry = _run(off, x, idx, seg, gains, pi, pg)
    _within_bar(dry, _model(case), "EQ off")
    ref, _ = _oracle_eq(oracle, dry)
    got = _run(on, x, idx, seg, gains, pi, pg)
    assert (rel_rms_per_stream(got, dry) > 1e-3).all()          # (the EQ does something)
    _same_bits(got, ref, "EQ(gain * conv): the oracle's EQ over the ear signals")
    again = _run(on, x, idx, seg, gains, pi, pg)                # (overlap and EQ state ring into this one)
    assert (rel_rms_per_stream(again[:, :, :BLOCK], got[:, :, :BLOCK]) > 1e-3).all()
    on.reset()
    _same_bits(_run(on, x, idx, seg, gains, pi, pg), got, "behind ohs_scene_reset")
    on.set_directions(dirs)                                     # (an upload zeroes the overlap; the EQ state is reset's)
    off.set_directions(dirs)
    _same_bits(_run(off, x, idx, seg, gains, pi, pg), dry, "behind a second upload")


# ---- f. guard bands on both sides ---------------------------------------------------------------------------------------------------------
def test_guard_bands_and_surplus_channels():
    import torch
    K, blocks, seg = 3, 5, 2
    frames = blocks * BLOCK
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S, K, blocks, seed=6600)
    idx, gains, pi, pg = sm.make_scene(S, K, blocks, seg, N_DIRS, seed=60)
    want = _run(_scene(dirs), x, idx, seg, gains, pi, pg)
    # input: K chains and one surplus channel's worth of room per stream, every word that is no sample of a chain the NaN sentinel
    lead, cgap, sgap = 64, 96, 32
    in_cs = frames + cgap
    in_ss = (K + 1) * in_cs + sgap
    xin = gb.filled(lead + S * in_ss + 64, gb.SENT_IN).copy()
    for s in range(S):
        for c in range(K):
            o = lead + s * in_ss + c * in_cs
            xin[o:o + frames] = x[s, c]
    out_ss, out_cs, total, mask = gb.layout(S, frames, 48, 160, 64, 80)
    d_in = torch.from_numpy(xin).cuda()
    d_out = torch.from_numpy(gb.filled(total, gb.SENT_OUT).copy()).cuda()
    sc = _scene(dirs)
    sc.process_ptr(d_in.data_ptr() + 4 * lead, d_out.data_ptr() + 4 * 48, blocks, in_ss, in_cs, out_ss, out_cs, K, seg, idx, gains, pi, pg,
                   True, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    gb.gaps_intact(got.view(np.uint32), mask, gb.SENT_OUT, "the scene call's output")
    assert d_in.cpu().numpy().tobytes() == xin.tobytes(), "the input was written"
    y = gb.take(got, S, frames, 48, out_ss, out_cs)
    assert np.isfinite(y).all(), "a surplus input channel or an input gap was read"
    _same_bits(y, want, "guard-banded strides against the contiguous run")


# ---- g. containment ---------------------------------------------------------------------------------------------------------------------------
def test_a_nan_in_one_object_of_one_stream_stays_in_that_stream():
    case = TRAJECTORY_CASES[2]
    x, dirs, idx, seg, gains, pi, pg = trajectory_case(*case)
    clean = _run(_scene(dirs), x, idx, seg, gains, pi, pg)
    xn = x.copy()
    xn[1, 1, 3 * BLOCK + 17] = np.nan
    y = _run(_scene(dirs), xn, idx, seg, gains, pi, pg)
    assert np.isnan(y[1]).any()
    _same_bits(y[[0, 2]], clean[[0, 2]], "the streams beside the poisoned one")
    _same_bits(y[1:2, :, :3 * BLOCK], clean[1:2, :, :3 * BLOCK], "the poisoned stream in front of the NaN")


# ---- h. every refused call leaves the handle usable ------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_handle_usable():
    import torch
    from open_headstage_amd import _ffi, scene
    L = scene.scene_lib()
    K, blocks, seg = 3, 4, 2
    frames = blocks * BLOCK
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S, K, blocks, seed=6800)
    idx, gains, pi, pg = sm.make_scene(S, K, blocks, seg, N_DIRS, seed=80)
    d = torch.from_numpy(x.copy()).cuda()
    out = torch.empty((S, 2, frames), dtype=torch.float32, device="cuda")
    INV, OK = _ffi.OHS_ERR_INVALID_ARG, _ffi.OHS_OK
    up, fp = C.POINTER(C.c_uint32), _ffi.fp
    f = L.ohs_scene_process

    def call(sc, d_in=None, d_out=None, n_blocks=blocks, in_ss=K * frames, in_cs=frames, out_ss=2 * frames, out_cs=frames, n_obj=K,
             sg=seg, rows=idx, stride=2, pv=pi, mode=1):
        rows = None if rows is None else np.ascontiguousarray(rows, np.uint32)
        pv = None if pv is None else np.ascontiguousarray(pv, np.uint32)
        g, pgc = np.ascontiguousarray(gains, np.float32), np.ascontiguousarray(pg, np.float32)
        return f(sc._h if sc is not None else None, C.c_void_p(d.data_ptr() if d_in is None else d_in),
                 C.c_void_p(out.data_ptr() if d_out is None else d_out), n_blocks, in_ss, in_cs, out_ss, out_cs, n_obj, sg,
                 None if rows is None else rows.ctypes.data_as(up), g.ctypes.data_as(fp), stride,
                 None if pv is None else pv.ctypes.data_as(up), pgc.ctypes.data_as(fp), mode, None)

    sc, twin = _scene(dirs), _scene(dirs)
    assert call(None) == INV
    assert call(_scene()) == INV                                    # no table
    sd = L.ohs_scene_set_direction_irs
    scratch = _scene(dirs)
    assert sd(scratch._h, N_DIRS, dirs.ctypes.data_as(fp), 0) == INV                                  # len 0
    assert sd(scratch._h, 1, np.zeros((1, 2, 513), np.float32).ctypes.data_as(fp), 513) == INV        # len 513
    assert sd(scratch._h, 65537, dirs.ctypes.data_as(fp), 1) == INV                                   # n_dirs 65537
    assert sd(scratch._h, N_DIRS, None, 512) == INV
    assert call(sc, d_in=0) == INV and call(sc, d_out=0) == INV and call(sc, rows=None) == INV
    assert call(sc, n_obj=0) == INV and call(sc, n_obj=65) == INV
    assert call(sc, sg=0) == INV
    assert call(sc, stride=1) == INV                                # a non-zero idx_stride below the number of segments
    assert call(sc, mode=2) == INV and call(sc, mode=-1) == INV
    for where in [(0, 0, 0), (S - 1, 1, K - 1), (1, 1, 0)]:         # anywhere in a row that would be read
        bad = idx.copy(); bad[where] = N_DIRS
        assert call(sc, rows=bad) == INV, where
    badp = pi.copy(); badp[S - 1, K - 1] = N_DIRS
    assert call(sc, pv=badp) == INV
    assert b"prev_idx" in L.ohs_scene_last_error()
    assert call(sc, in_cs=frames - 1) == INV and call(sc, out_cs=frames - 1) == INV          # strides below the region
    assert call(sc, in_ss=K * frames - 1) == INV and call(sc, out_ss=2 * frames - 1) == INV
    assert call(sc, d_out=d.data_ptr()) == INV                      # in place
    assert call(sc, d_out=d.data_ptr() + 4 * (S * K * frames - 1)) == INV                    # the regions meet in one frame
    assert call(sc, n_blocks=(1 << 24) + 1, in_cs=1 << 40, in_ss=1 << 50, out_cs=1 << 40, out_ss=1 << 50) == INV
    assert call(sc, n_blocks=0) == OK                               # a no-op
    assert sc.last_launch() == (0, 0, 0)                            # none of them launched anything
    # ... nor touched the state: the handle serves as its twin does
    assert call(sc) == OK
    torch.cuda.synchronize()
    got = out.cpu().numpy().copy()
    _same_bits(got, _run(twin, x, idx, seg, gains, pi, pg), "the valid call behind the refused ones")
    _same_bits(_run(sc, x, idx, seg, gains, pi, pg), _run(twin, x, idx, seg, gains, pi, pg), "and the call after it")
    # a refused upload leaves the table that was there
    _same_bits(_run(scratch, x, idx, seg, gains, pi, pg), got, "the table behind refused uploads")

"""ohs_scene2_process_blended (libohs_scene2.so): every object of a scene between two measured directions, blended inside the kernel.

The yardstick is never the code under test: the f64 model of tests/scene_blend_model.py (checked against a direct time-domain
evaluation and against the existing one-direction model in tests/test_cpu_scene_blend.py), and the UNCHANGED libohs_scene.so on a
second handle -- by bits where include/ohs_scene2.h promises bits, and as 2 K objects on duplicated channels
(conv(u h0 + w h1, x) = conv(h0, u x) + conv(h1, w x)) elsewhere.  Bars: bit for bit, or 1e-6 relative RMS -- the project's FFT bar,
DESIGN section 2 -- per stream AND per 512-frame block.  3 streams, 7 directions, gain 0.7 throughout."""
import ctypes as C

import numpy as np
import pytest

from tests import guard_bands as gb
from tests import scene_blend_model as bm
from tests.test_cpu_layout import BAR, BLOCK, make_input, make_layout, rel_rms_per_stream
from tests.test_cpu_scene import rel_rms_per_block
from tests.test_gpu_layout import _eq_bands, _oracle_eq, _same_bits
from tests.test_gpu_scene import _within_bar

pytestmark = pytest.mark.gpu

S = 3
NB = 10
GAIN = 0.7
N_DIRS = 7
# (K, taps, seg_blocks, a shared row, blocks): K = 1; K = 2, a pair of a blended and a w = 0 object, 8 taps; K = 3, odd, the last object
# blended; K = 5 on a shared row; K = 8
BLEND_CASES = [(1, 512, 1, False, 6), (2, 8, 2, False, 7), (3, 512, 2, False, 8), (5, 512, 3, True, 12), (8, 512, 2, False, 6)]
_IDS = [f"K{c[0]}-taps{c[1]}-seg{c[2]}-{'shared' if c[3] else 'rows'}" for c in BLEND_CASES]


def blend_case(K, taps, seg_blocks, shared, blocks):
    """-> (x, dirs, seg_blocks, scene dict) of one case (tests/test_cpu_scene_blend.py runs the mutants on these)"""
    dirs = make_layout(N_DIRS, taps)
    x = make_input(S, K, blocks, seed=6500 + 10 * K)
    return x, dirs, seg_blocks, bm.make_blend_scene(S, K, blocks, seg_blocks, N_DIRS, seed=K, shared=shared)


def _setup(sc, dirs, eq):
    sc.set_gain(GAIN)
    if dirs is not None:
        sc.set_directions(dirs)
    if eq:
        for i, (c, en) in enumerate(_eq_bands()):
            sc.set_band_coeffs(i, c, en)
        sc.set_eq_enabled(True)
    return sc


def _blend(dirs=None, streams=S, eq=False):
    import open_headstage_amd as ohs
    return _setup(ohs.BlendSceneProcessor(streams, num_bands=NB), dirs, eq)


def _plain(dirs=None, streams=S, eq=False):
    import open_headstage_amd as ohs
    return _setup(ohs.SceneProcessor(streams, num_bands=NB), dirs, eq)


def _run(h, x, seg_blocks, sc, crossfade=True, **over):
    """one call of a BlendSceneProcessor on the scene dict (entries overridden by name)"""
    import torch
    a = dict(sc, **over)
    y = h.process(torch.from_numpy(np.ascontiguousarray(x).copy()).cuda(), a["idx"], seg_blocks, a["gains"], a["prev_idx"], a["prev_gains"],
                  crossfade, a["idx1"], a["weights"], a["prev_idx1"], a["prev_weights"])
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _run_plain(h, x, idx, seg_blocks, gains=None, prev_idx=None, prev_gains=None, crossfade=True):
    import torch
    y = h.process(torch.from_numpy(np.ascontiguousarray(x).copy()).cuda(), idx, seg_blocks, gains, prev_idx, prev_gains, crossfade)
    torch.cuda.synchronize()
    return y.cpu().numpy()


_cache = {}


def _model(case, fade=True):
    if (case, fade) not in _cache:
        x, dirs, seg, sc = blend_case(*case)
        m = bm.model_blend_f64(x, dirs, sc["idx"], sc["idx1"], sc["weights"], seg, sc["gains"], sc["prev_idx"], sc["prev_idx1"],
                               sc["prev_weights"], sc["prev_gains"], fade, GAIN)
        m.setflags(write=False)
        _cache[(case, fade)] = m
    return _cache[(case, fade)]


def _plan(case, fade=True):
    x, dirs, seg, sc = blend_case(*case)
    return bm.blend_plan(S, case[0], case[4], sc["idx"], sc["idx1"], sc["weights"], seg, sc["gains"], sc["prev_idx"], sc["prev_idx1"],
                         sc["prev_weights"], sc["prev_gains"], fade)


# ---- a. weights all +0.0: the one-direction call's bits, whatever idx1 names ---------------------------------------------------
@pytest.mark.parametrize("K", [2, 3])
def test_zero_weights_have_the_bits_of_the_unchanged_scene_call(K):
    from tests import scene_model as sm
    blocks, seg = 9, 2
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S, K, blocks, seed=6510 + K)
    idx, gains, pi, pg = sm.make_scene(S, K, blocks, seg, N_DIRS, seed=K)
    rng = np.random.default_rng(K)
    # arbitrary and valid: a new one per object and BLOCK, and one more in front of the first call (beside +0.0 it is never read)
    idx1 = rng.integers(0, N_DIRS, (S, blocks, K)).astype(np.uint32)
    before = ((idx1[:, 0] + 1 + rng.integers(0, N_DIRS - 1, (S, K))) % N_DIRS).astype(np.uint32)
    assert (idx1[:, 1:] != idx1[:, :-1]).any(axis=(0, 2)).all() and (before != idx1[:, 0]).all()
    zero = np.zeros((S, blocks, K), np.float32)
    ref, with_zero, with_none = _plain(dirs), _blend(dirs), _blend(dirs)
    pos = 0
    bi, bg = np.repeat(idx, seg, axis=1), np.repeat(gains, seg, axis=1)
    assert (bi[:, 1:] == bi[:, :-1]).all(axis=(0, 2)).any()     # (blocks in which nothing but idx1 moves)
    for call, nb in enumerate([4, 5]):          # (the second call continues the first one's overlap, prev_* handed on)
        sl = slice(pos, pos + nb)
        xc = np.ascontiguousarray(x[:, :, pos * BLOCK:(pos + nb) * BLOCK])
        ci, cg = np.ascontiguousarray(bi[:, sl]), np.ascontiguousarray(bg[:, sl])
        p_i, p_g = (pi, pg) if pos == 0 else (bi[:, pos - 1], bg[:, pos - 1])
        want = _run_plain(ref, xc, ci, 1, cg, p_i, p_g)
        sc = dict(idx=ci, idx1=np.ascontiguousarray(idx1[:, sl]), weights=np.ascontiguousarray(zero[:, sl]), gains=cg, prev_idx=p_i,
                  prev_idx1=before if pos == 0 else idx1[:, pos - 1], prev_weights=zero[:, 0], prev_gains=p_g)
        y = _run(with_zero, xc, 1, sc)
        assert with_zero.last_launch()[:3] == ref.last_launch() and with_zero.last_launch()[3] == 0, with_zero.last_launch()
        _same_bits(y, want, f"K = {K}, weights +0.0, call {call}")
        y = _run(with_none, xc, 1, sc, idx1=None, weights=None)
        assert with_none.last_launch() == ref.last_launch() + (0,)
        _same_bits(y, want, f"K = {K}, idx1 and weights None, call {call}")
        pos += nb


# ---- b. w = 1 everywhere: the plain call on idx1 -------------------------------------------------------------------------------
def test_unit_weights_are_the_plain_call_on_idx1():
    case = BLEND_CASES[2]
    x, dirs, seg, sc = blend_case(*case)
    fixed = np.broadcast_to(sc["idx"][:, :1], sc["idx"].shape).copy()           # (idx constant: only idx1 and the gains change)
    one = np.ones_like(sc["weights"])
    y = _run(_blend(dirs), x, seg, sc, idx=fixed, weights=one, prev_idx=None, prev_weights=None)
    want = _run_plain(_plain(dirs), x, sc["idx1"], seg, sc["gains"], sc["prev_idx1"], sc["prev_gains"])
    diff = int((y.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"w = 1 everywhere against the plain call on idx1: {diff} of {y.size} samples differ in bits")
    _within_bar(y, want.astype(np.float64), "w = 1 against the plain call on idx1")
    # 0 A[d0] + 1 A[d1] is A[d1], each operation rounded by itself: equal as numbers (a zero's sign may differ)
    ne = np.argwhere(~(y == want))
    assert ne.size == 0, f"w = 1: {len(ne)} samples differ from the plain call on idx1 as numbers, first (stream, ear, frame) {ne[0].tolist()}: " \
                         f"{y[tuple(ne[0])]!r} against {want[tuple(ne[0])]!r}"


def test_negative_zero_weights_are_the_plain_call_on_idx():
    """w = -0.0 everywhere is not +0.0: every pass loads four rows, and 1 A[d0] + (-0) A[d1] is A[d0] -- the four-row pass against the
    two-row pass, operation for operation, equal as numbers.  idx1 is held per object, so the blended call fades where the plain one does."""
    case = BLEND_CASES[2]
    x, dirs, seg, sc = blend_case(*case)
    K = case[0]
    held = np.broadcast_to(sc["idx1"][:, :1], sc["idx1"].shape).copy()
    neg = np.full_like(sc["weights"], -0.0)
    assert np.signbit(neg).all() and (held != sc["idx"]).any()
    h, ref = _blend(dirs), _plain(dirs)
    y = _run(h, x, seg, sc, idx1=held, weights=neg, prev_idx1=None, prev_weights=None)
    want = _run_plain(ref, x, sc["idx"], seg, sc["gains"], sc["prev_idx"], sc["prev_gains"])
    pairs, _, fading, blended = h.last_launch()
    # every pass is a blended one: per stream and block one per pair, and one more per pair with an old half
    assert (pairs, fading) == (ref.last_launch()[0], ref.last_launch()[2]) and fading > 0, (h.last_launch(), ref.last_launch())
    assert blended == S * case[4] * ((K + 1) // 2) + fading, h.last_launch()
    diff = int((y.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"w = -0.0 everywhere against the plain call on idx: {diff} of {y.size} samples differ in bits")
    ne = np.argwhere(~(y == want))
    assert ne.size == 0, f"w = -0.0: {len(ne)} samples differ from the plain call on idx as numbers, first (stream, ear, frame) {ne[0].tolist()}: " \
                         f"{y[tuple(ne[0])]!r} against {want[tuple(ne[0])]!r}"


# ---- c. trajectories against the f64 model -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BLEND_CASES, ids=_IDS)
def test_blended_trajectories_against_the_f64_model(case):
    x, dirs, seg, sc = blend_case(*case)
    K = case[0]
    h = _blend(dirs)
    y = _run(h, x, seg, sc)
    pairs, ranges, fading, blended = h.last_launch()
    plan = _plan(case)
    assert pairs == (K + 1) // 2 and fading == bm.count_fading_passes(plan) and fading > 0, h.last_launch()
    assert blended == bm.count_blended_passes(plan, K) and blended > 0, (h.last_launch(), bm.count_blended_passes(plan, K))
    _within_bar(y, _model(case), f"case {case}, CROSSFADE")


def test_ring_out_against_the_f64_model():
    case = BLEND_CASES[2]
    x, dirs, seg, sc = blend_case(*case)
    h = _blend(dirs)
    y = _run(h, x, seg, sc, crossfade=False)
    assert h.last_launch()[2] == 0 and h.last_launch()[3] == bm.count_blended_passes(_plan(case, False), case[0])
    _within_bar(y, _model(case, False), f"case {case}, RING_OUT")
    assert (rel_rms_per_stream(_model(case, False), _model(case, True)) > 1e-3).all()


def test_a_gain_in_front_of_the_call_beside_no_gain_rows():
    """gains None reads as 1.0 everywhere; prev_gains beside it is a boundary at the call's start for every object it moves off 1.0"""
    case = BLEND_CASES[2]
    x, dirs, seg, sc = blend_case(*case)
    K = case[0]
    assert (sc["prev_gains"] != 1.0).any()
    h = _blend(dirs)
    y = _run(h, x, seg, sc, gains=None)
    plan = bm.blend_plan(S, K, case[4], sc["idx"], sc["idx1"], sc["weights"], seg, None, sc["prev_idx"], sc["prev_idx1"], sc["prev_weights"],
                         sc["prev_gains"], True)
    assert h.last_launch()[2:] == (bm.count_fading_passes(plan), bm.count_blended_passes(plan, K)), h.last_launch()
    m = bm.model_blend_f64(x, dirs, sc["idx"], sc["idx1"], sc["weights"], seg, None, sc["prev_idx"], sc["prev_idx1"], sc["prev_weights"],
                           sc["prev_gains"], True, GAIN)
    _within_bar(y, m, f"case {case}, gains None, prev_gains given")
    unit = bm.model_blend_f64(x, dirs, sc["idx"], sc["idx1"], sc["weights"], seg, None, sc["prev_idx"], sc["prev_idx1"], sc["prev_weights"],
                              None, True, GAIN)
    assert (rel_rms_per_stream(unit[:, :, :BLOCK], m[:, :, :BLOCK]) > 1e-3).all()       # (prev_gains does something)


# ---- d. the same cases against the unchanged library's 2 K-object composition --------------------------------------------------
@pytest.mark.parametrize("case", BLEND_CASES, ids=_IDS)
def test_blended_trajectories_against_the_unchanged_library_on_2k_objects(case):
    x, dirs, seg, sc = blend_case(*case)
    y = _run(_blend(dirs), x, seg, sc)
    x2, idx2, gains2, pi2, pg2 = bm.as_2k_scene(x, sc["idx"], sc["idx1"], sc["weights"], sc["gains"], sc["prev_idx"], sc["prev_idx1"],
                                                sc["prev_weights"], sc["prev_gains"])
    want = _run_plain(_plain(dirs), x2, idx2, seg, gains2, pi2, pg2)
    _within_bar(y, want.astype(np.float64), f"case {case} against 2 K objects through libohs_scene.so")


# ---- e. the bits do not depend on cuts, ranges or the neighbours ---------------------------------------------------------------
def test_cuts_ranges_and_neighbours_do_not_change_the_bits():
    K, blocks, seg = 3, 24, 2
    dirs = make_layout(N_DIRS, 512)
    x3 = make_input(S, K, blocks, seed=6540)
    sc3 = bm.make_blend_scene(S, K, blocks, seg, N_DIRS, seed=41)
    x, sc = x3[1:2], {k: v[1:2] for k, v in sc3.items()}        # (stream 1 alone)
    one = _blend(dirs, 1)
    whole = _run(one, x, seg, sc)
    assert one.last_launch()[1] == 16, one.last_launch()        # 16 ranges, each but the first with a dry block in front
    m = bm.model_blend_f64(x, dirs, sc["idx"], sc["idx1"], sc["weights"], seg, sc["gains"], sc["prev_idx"], sc["prev_idx1"],
                           sc["prev_weights"], sc["prev_gains"], True, GAIN)
    _within_bar(whole, m, "one stream, 24 blocks in one call")
    rows = ("idx", "idx1", "weights", "gains")
    per_block = {k: np.repeat(sc[k], seg, axis=1) for k in rows}        # [1][blocks][K]
    h = _blend(dirs, 1)
    out, pos = [], 0
    for nb in [1, 5, 7, 11]:
        cut = {k: np.ascontiguousarray(per_block[k][:, pos:pos + nb]) for k in rows}
        for k in rows:
            cut["prev_" + k] = sc["prev_" + k] if pos == 0 else per_block[k][:, pos - 1]
        out.append(_run(h, x[:, :, pos * BLOCK:(pos + nb) * BLOCK], 1, cut))
        pos += nb
    assert pos == blocks
    _same_bits(np.concatenate(out, axis=2), whole, "calls of 1, 5, 7 and 11 blocks against one call")
    y3 = _run(_blend(dirs, S), x3, seg, sc3)
    _same_bits(y3[1:2], whole, "the same stream inside a 3-stream handle")


# ---- f. EQ and reset, guard bands, containment, flush-denormals ----------------------------------------------------------------
def test_eq_filters_the_ear_signals_and_reset_gives_a_new_handles_bits(oracle):
    case = BLEND_CASES[2]
    x, dirs, seg, sc = blend_case(*case)
    off, on = _blend(dirs), _blend(dirs, eq=True)
    dry = _run(off, x, seg, sc)
    _within_bar(dry, _model(case), "EQ off")
    ref, _ = _oracle_eq(oracle, dry)
    got = _run(on, x, seg, sc)
    assert (rel_rms_per_stream(got, dry) > 1e-3).all()          # (the EQ does something)
    _same_bits(got, ref, "EQ(gain * conv): the oracle's EQ over the ear signals")
    again = _run(on, x, seg, sc)                                # (overlap and EQ state ring into this one)
    assert (rel_rms_per_stream(again[:, :, :BLOCK], got[:, :, :BLOCK]) > 1e-3).all()
    on.reset()
    _same_bits(_run(on, x, seg, sc), got, "behind ohs_scene2_reset")


def test_guard_bands_and_surplus_channels():
    import torch
    K, blocks, seg = 3, 5, 2
    frames = blocks * BLOCK
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S, K, blocks, seed=6560)
    sc = bm.make_blend_scene(S, K, blocks, seg, N_DIRS, seed=61)
    want = _run(_blend(dirs), x, seg, sc)
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
    h = _blend(dirs)
    h.process_ptr(d_in.data_ptr() + 4 * lead, d_out.data_ptr() + 4 * 48, blocks, in_ss, in_cs, out_ss, out_cs, K, seg, sc["idx"], sc["gains"],
                  sc["prev_idx"], sc["prev_gains"], True, torch.cuda.current_stream().cuda_stream, sc["idx1"], sc["weights"],
                  sc["prev_idx1"], sc["prev_weights"])
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    gb.gaps_intact(got.view(np.uint32), mask, gb.SENT_OUT, "the blended scene call's output")
    assert d_in.cpu().numpy().tobytes() == xin.tobytes(), "the input was written"
    y = gb.take(got, S, frames, 48, out_ss, out_cs)
    assert np.isfinite(y).all(), "a surplus input channel or an input gap was read"
    _same_bits(y, want, "guard-banded strides against the contiguous run")


def test_a_nan_in_one_object_of_one_stream_stays_in_that_stream():
    case = BLEND_CASES[2]
    x, dirs, seg, sc = blend_case(*case)
    clean = _run(_blend(dirs), x, seg, sc)
    xn = x.copy()
    xn[1, 2, 3 * BLOCK + 17] = np.nan           # (the odd last object: a blended one)
    y = _run(_blend(dirs), xn, seg, sc)
    assert np.isnan(y[1]).any()
    _same_bits(y[[0, 2]], clean[[0, 2]], "the streams beside the poisoned one")
    _same_bits(y[1:2, :, :3 * BLOCK], clean[1:2, :, :3 * BLOCK], "the poisoned stream in front of the NaN")


def test_flush_denormals_changes_no_bit_of_a_loud_signal():
    case = BLEND_CASES[2]
    x, dirs, seg, sc = blend_case(*case)
    ieee, ftz = _blend(dirs), _blend(dirs)
    ftz.set_flush_denormals(1)
    _same_bits(_run(ftz, x, seg, sc), _run(ieee, x, seg, sc), "flush-denormals on against off, a loud signal")


# ---- g. every refused call leaves the handle usable ----------------------------------------------------------------------------
def test_argument_errors_leave_the_handle_usable():
    import torch
    from open_headstage_amd import _ffi, scene2
    L = scene2.scene2_lib()
    K, blocks, seg = 3, 4, 2
    frames = blocks * BLOCK
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S, K, blocks, seed=6580)
    sc = bm.make_blend_scene(S, K, blocks, seg, N_DIRS, seed=81)
    d = torch.from_numpy(x.copy()).cuda()
    out = torch.empty((S, 2, frames), dtype=torch.float32, device="cuda")
    INV, OK = _ffi.OHS_ERR_INVALID_ARG, _ffi.OHS_OK
    up, fp = C.POINTER(C.c_uint32), _ffi.fp
    f = L.ohs_scene2_process_blended

    def call(h, d_out=None, n_blocks=blocks, n_obj=K, sg=seg, stride=2, mode=1, **over):
        a = dict(sc, **over)

        def u(name):
            v = a[name]
            return None if v is None else np.ascontiguousarray(v, np.uint32).ctypes.data_as(up)

        def fl(name):
            v = a[name]
            return None if v is None else np.ascontiguousarray(v, np.float32).ctypes.data_as(fp)
        return f(h._h if h is not None else None, C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr() if d_out is None else d_out), n_blocks,
                 K * frames, frames, 2 * frames, frames, n_obj, sg, u("idx"), fl("gains"), stride, u("prev_idx"), fl("prev_gains"), mode, None,
                 u("idx1"), fl("weights"), u("prev_idx1"), fl("prev_weights"))

    def changed(name, where, value):
        v = sc[name].copy()
        v[where] = value
        return {name: v}

    h, twin = _blend(dirs), _blend(dirs)
    # the pair idx1 / weights
    assert call(h, idx1=None) == INV and b"both" in L.ohs_scene2_last_error()
    assert call(h, weights=None) == INV
    # idx1 and prev_idx1 against the table, anywhere a row is read
    for where in [(0, 0, 0), (S - 1, 1, K - 1), (1, 1, 0)]:
        assert call(h, **changed("idx1", where, N_DIRS)) == INV, where
        assert b"dir_idx1" in L.ohs_scene2_last_error()
    assert call(h, **changed("prev_idx1", (S - 1, K - 1), N_DIRS)) == INV and b"prev_idx1" in L.ohs_scene2_last_error()
    assert call(h, **changed("prev_idx1", (0, 0), 0xffffffff)) == INV
    # weights outside [0, 1], or NaN
    for bad in (-0.25, 1.5, np.nan, np.inf):
        assert call(h, **changed("weights", (1, 1, 1), bad)) == INV, bad
        assert b"weight" in L.ohs_scene2_last_error()
    assert call(h, **changed("weights", (S - 1, 1, K - 1), np.nextafter(np.float32(1), np.float32(2)))) == INV
    assert call(h, **changed("prev_weights", (1, 2), 2.0)) == INV and b"prev_weight" in L.ohs_scene2_last_error()
    assert call(h, **changed("prev_weights", (0, 0), np.nan)) == INV
    # three of the inherited refusals
    assert call(h, **changed("idx", (1, 0, 2), N_DIRS)) == INV
    assert call(h, mode=2) == INV
    assert call(h, d_out=d.data_ptr()) == INV                   # in place
    assert call(h, n_obj=65) == INV and call(h, stride=1) == INV and call(None) == INV
    assert call(_blend()) == INV                                # no table
    assert h.last_launch() == (0, 0, 0, 0)                      # none of them launched anything
    # -0.0 is a weight; under RING_OUT the entries in front of the call are not read
    assert call(_blend(dirs), **changed("weights", (0, 0, 1), -0.0)) == OK
    assert call(_blend(dirs), mode=0, **changed("prev_weights", (1, 2), 2.0)) == OK
    # ... nor touched the state: the handle serves as its twin does
    assert call(h) == OK
    torch.cuda.synchronize()
    got = out.cpu().numpy().copy()
    _same_bits(got, _run(twin, x, seg, sc), "the valid call behind the refused ones")
    _same_bits(_run(h, x, seg, sc), _run(twin, x, seg, sc), "and the call after it")

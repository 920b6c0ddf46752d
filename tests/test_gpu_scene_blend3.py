"""ohs_scene3_process_blended3 (libohs_scene3.so): every object of a scene inside a triangle of three measured directions, blended
inside the kernel (k_conv_p1_objects_blend3).

The yardstick is never the code under test: the f64 model of tests/scene_blend3_model.py (checked against a direct time-domain
evaluation and against the two older models in tests/test_cpu_scene_blend3.py), and the UNCHANGED libohs_scene.so / libohs_scene2.so on
handles of their own -- by bits where include/ohs_scene3.h promises bits, and as 3 K objects on triplicated channels
(conv(u h0 + w1 h1 + w2 h2, x) = conv(h0, u x) + conv(h1, w1 x) + conv(h2, w2 x)) elsewhere.  Bars: bit for bit, equal as numbers, or
1e-6 relative RMS -- the project's FFT bar, DESIGN section 2, the bar of the sibling tests -- per stream AND per 512-frame block.
3 streams, 6 blocks, seg_blocks 2, 7 directions, gain 0.7 unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest

from tests import busy_stream as bs
from tests import scene_blend3_model as tm
from tests import scene_blend_model as bm
from tests.test_cpu_layout import BAR, BLOCK, make_input, make_layout, rel_rms_per_stream  # noqa: F401
from tests.test_gpu_layout import _same_bits
from tests.test_gpu_scene import _within_bar

pytestmark = pytest.mark.gpu

S = 3
NB = 10
GAIN = 0.7
N_DIRS = 7
BLOCKS, SEG = 6, 2
# (K, taps, a shared row): K = 1, the object alone with three directions; K = 2, a plain object beside a three-direction one, 37 taps;
# K = 3, odd, the last object alone with three; K = 5: pairs of three directions and a last object with two -- once on a shared row
BLEND3_CASES = [(1, 512, False), (2, 37, False), (3, 512, False), (5, 37, True), (5, 512, False)]
_IDS = [f"K{c[0]}-taps{c[1]}-{'shared' if c[2] else 'rows'}" for c in BLEND3_CASES]
ROWS = tm.ROWS


def blend3_case(K, taps, shared, blocks=BLOCKS, seg=SEG):
    """-> (x, dirs, seg_blocks, scene dict) of one case (tests/test_cpu_scene_blend3.py runs the mutants on these)"""
    dirs = make_layout(N_DIRS, taps)
    x = make_input(S, K, blocks, seed=8500 + 10 * K + taps)
    return x, dirs, seg, tm.make_blend3_scene(S, K, blocks, seg, N_DIRS, seed=K, shared=shared)


def _setup(h, dirs):
    h.set_gain(GAIN)
    if dirs is not None:
        h.set_directions(dirs)
    return h


def _tri(dirs=None, streams=S):
    import open_headstage_amd as ohs
    return _setup(ohs.TriSceneProcessor(streams, num_bands=NB), dirs)


def _blend(dirs=None, streams=S):
    import open_headstage_amd as ohs
    return _setup(ohs.BlendSceneProcessor(streams, num_bands=NB), dirs)


def _plain(dirs=None, streams=S):
    import open_headstage_amd as ohs
    return _setup(ohs.SceneProcessor(streams, num_bands=NB), dirs)


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


def _run(h, x, seg_blocks, sc, crossfade=True, **over):
    """one three-direction call of a TriSceneProcessor on the scene dict (entries overridden by name)"""
    import torch
    a = dict(sc, **over)
    y = h.process(_dev(x), a["idx"], seg_blocks, a["gains"], a["prev_idx"], a["prev_gains"], crossfade, a["idx1"], a["w1"], a["prev_idx1"],
                  a["prev_w1"], a["idx2"], a["w2"], a["prev_idx2"], a["prev_w2"])
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _run_two(h, x, seg_blocks, sc, crossfade=True):
    """the two-direction call of a BlendSceneProcessor (either library) on (idx, idx1, w1) of the scene dict"""
    import torch
    y = h.process(_dev(x), sc["idx"], seg_blocks, sc["gains"], sc["prev_idx"], sc["prev_gains"], crossfade, sc["idx1"], sc["w1"],
                  sc["prev_idx1"], sc["prev_w1"])
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _run_one(h, x, idx, seg_blocks, gains=None, prev_idx=None, prev_gains=None, crossfade=True):
    import torch
    y = h.process(_dev(x), idx, seg_blocks, gains, prev_idx, prev_gains, crossfade)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _figures(x, seg, sc, fade=True, **over):
    """(fading, four-row, six-row passes) of the model's plan"""
    a = dict(sc, **over)
    plan = tm.blend3_plan(x.shape[0], int(np.shape(a["idx"])[-1]), x.shape[2] // BLOCK, *tm.args(a), seg, a["gains"], a["prev_idx"],
                          a["prev_idx1"], a["prev_idx2"], a["prev_w1"], a["prev_w2"], a["prev_gains"], fade)
    return tm.count_fading_passes(plan), tm.count_blended_passes(plan), tm.count_blended3_passes(plan)


def _model(x, dirs, seg, sc, fade=True, **over):
    a = dict(sc, **over)
    return tm.model_blend3_f64(x, dirs, *tm.args(a), seg, crossfade=fade, gain=GAIN, **tm.kw(a))


def _equal_as_numbers(y, want, what):
    ne = np.argwhere(~(y == want))
    assert ne.size == 0, f"{what}: {len(ne)} samples differ as numbers, first (stream, ear, frame) {ne[0].tolist()}: " \
                         f"{y[tuple(ne[0])]!r} against {want[tuple(ne[0])]!r}"


# ---- a. trajectories against the f64 model -------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_gains", [True, False], ids=["gains", "no_gains"])
@pytest.mark.parametrize("fade", [True, False], ids=["crossfade", "ring_out"])
@pytest.mark.parametrize("case", BLEND3_CASES, ids=_IDS)
def test_trajectories_against_the_f64_model(case, fade, with_gains):
    x, dirs, seg, sc = blend3_case(*case)
    K = case[0]
    over = {} if with_gains else dict(gains=None, prev_gains=None)
    h = _tri(dirs)
    y = _run(h, x, seg, sc, fade, **over)
    pairs, ranges, fading, blended, blended3 = h.last_launch()
    want = _figures(x, seg, sc, fade, **over)
    print(f"case {case}, crossfade {fade}, gains {with_gains}: launch {h.last_launch()}, the model's figures {want}")
    assert pairs == (K + 1) // 2 and ranges >= 1 and (fading, blended, blended3) == want, (h.last_launch(), want)
    assert blended3 > 0 and (fading > 0) == fade
    _within_bar(y, _model(x, dirs, seg, sc, fade, **over), f"case {case}, crossfade {fade}, gains {with_gains}")


# ---- b. the same cases against the unchanged library's 3 K-object composition ---------------------------------------------------
@pytest.mark.parametrize("case", BLEND3_CASES, ids=_IDS)
def test_trajectories_against_the_unchanged_library_on_3k_objects(case):
    x, dirs, seg, sc = blend3_case(*case)
    y = _run(_tri(dirs), x, seg, sc)
    x3, idx3, gains3, pi3, pg3 = tm.as_3k_scene(x, *tm.args(sc), **tm.kw(sc))
    want = _run_one(_plain(dirs), x3, idx3, seg, gains3, pi3, pg3)
    _within_bar(y, want.astype(np.float64), f"case {case} against 3 K objects through libohs_scene.so")


# ---- c. bit equalities ----------------------------------------------------------------------------------------------------------
def _moving(shape, seed):
    """an index per object and segment that moves in every segment, and one more in front of the call"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, N_DIRS, shape).astype(np.uint32)
    for k in range(1, shape[1]):
        a[:, k] = (a[:, k - 1] + 1 + rng.integers(0, N_DIRS - 1, a[:, k].shape)) % N_DIRS
    before = ((a[:, 0] + 1 + rng.integers(0, N_DIRS - 1, a[:, 0].shape)) % N_DIRS).astype(np.uint32)
    assert (a[:, 1:] != a[:, :-1]).all() and (before != a[:, 0]).all()
    return a, before


@pytest.mark.parametrize("K", [2, 3])
def test_w2_zero_has_the_bits_of_the_two_direction_calls(K):
    """w2 all +0.0, idx2 moving in every segment and in front of the call: ohs_scene2_process_blended on libohs_scene2.so, and
    ohs_scene3_process_blended on the same handle, bit for bit, with their launch figures"""
    x, dirs, seg, sc = blend3_case(K, 512, False)
    sc = dict(sc, w1=bm.make_blend_scene(S, K, BLOCKS, seg, N_DIRS, seed=K)["weights"],
              prev_w1=bm.make_blend_scene(S, K, BLOCKS, seg, N_DIRS, seed=K)["prev_weights"])
    sc["idx2"], sc["prev_idx2"] = _moving(sc["idx"].shape, 30 + K)
    sc["w2"], sc["prev_w2"] = np.zeros_like(sc["w1"]), np.zeros_like(sc["prev_w1"])
    ref = _blend(dirs)
    want = _run_two(ref, x, seg, sc)
    h = _tri(dirs)
    y = _run(h, x, seg, sc)
    assert h.last_launch() == ref.last_launch() + (0,) and ref.last_launch()[2] > 0 and ref.last_launch()[3] > 0, (h.last_launch(), ref.last_launch())
    _same_bits(y, want, f"K = {K}, w2 +0.0: ohs_scene2_process_blended on libohs_scene2.so")
    h.reset()
    y = _run_two(h, x, seg, sc)
    assert h.last_launch() == ref.last_launch() + (0,)
    _same_bits(y, want, f"K = {K}: ohs_scene3_process_blended on the same handle")
    h.reset()
    _same_bits(_run(h, x, seg, sc, prev_idx2=None, prev_w2=None), want, f"K = {K}, w2 +0.0, nothing named in front of the call")


@pytest.mark.parametrize("K", [2, 3])
def test_w1_and_w2_zero_have_the_bits_of_the_one_direction_call(K):
    x, dirs, seg, sc = blend3_case(K, 512, False)
    sc["idx1"], sc["prev_idx1"] = _moving(sc["idx"].shape, 40 + K)
    sc["idx2"], sc["prev_idx2"] = _moving(sc["idx"].shape, 50 + K)
    for k in ("w1", "w2", "prev_w1", "prev_w2"):
        sc[k] = np.zeros_like(sc[k])
    ref = _plain(dirs)
    want = _run_one(ref, x, sc["idx"], seg, sc["gains"], sc["prev_idx"], sc["prev_gains"])
    h = _tri(dirs)
    y = _run(h, x, seg, sc)
    assert h.last_launch() == ref.last_launch() + (0, 0) and ref.last_launch()[2] > 0, (h.last_launch(), ref.last_launch())
    _same_bits(y, want, f"K = {K}, w1 = w2 = +0.0: ohs_scene_process on libohs_scene.so")
    h.reset()
    _same_bits(_run_one(h, x, sc["idx"], seg, sc["gains"], sc["prev_idx"], sc["prev_gains"]), want, f"K = {K}: ohs_scene3_process on the same handle")


def mixed_scene(blocks=BLOCKS, seg=SEG):
    """K = 7: pair 0 plain (w1 = w2 = +0.0), pair 1 with two directions (w2 = +0.0), pair 2 with three, the odd last object alone with
    three.  idx1 and idx2 are held per object (so that a zero's sign changes no change); idx, the weights that are not zero and the
    gains follow make_blend3_scene."""
    K = 7
    sc = tm.make_blend3_scene(S, K, blocks, seg, N_DIRS, seed=77)
    sc["w1"], sc["w2"] = np.clip(sc["w1"], 0.1, 0.5).astype(np.float32), np.clip(sc["w2"], 0.05, 0.4).astype(np.float32)
    sc["prev_w1"], sc["prev_w2"] = np.clip(sc["prev_w1"], 0.1, 0.5).astype(np.float32), np.clip(sc["prev_w2"], 0.05, 0.4).astype(np.float32)
    for k in ("w1", "prev_w1"):
        sc[k][..., 0:2] = 0.0
    for k in ("w2", "prev_w2"):
        sc[k][..., 0:4] = 0.0
    for k in ("idx1", "idx2"):
        sc[k] = np.broadcast_to(sc[k][:, :1], sc[k].shape).copy()
        sc["prev_" + k] = sc[k][:, 0].copy()
    return K, sc


def test_a_mixed_scene_equals_the_scene_with_every_pass_on_six_rows():
    """Every +0.0 weight of the mixed scene written -0.0 sends every pass through six rows: (1 A[d0] + (-0) A[d1]) + (-0) A[d2] is
    A[d0], and (u A[d0] + w1 A[d1]) + (-0) A[d2] is the four-row pass's row, each operation rounded by itself -- the three kinds of
    pass in one block against the six-row pass alone, equal as numbers (a zero's sign may differ)."""
    K, sc = mixed_scene()
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S, K, BLOCKS, seed=8700)
    h, six = _tri(dirs), _tri(dirs)
    y = _run(h, x, SEG, sc)
    pairs, _, fading, blended, blended3 = h.last_launch()
    assert (fading, blended, blended3) == _figures(x, SEG, sc) and fading > 0, h.last_launch()
    assert blended >= S * BLOCKS and blended3 >= 2 * S * BLOCKS and blended + blended3 == S * BLOCKS * 3 + sum(_old_halves(x, sc)[1:]), h.last_launch()
    neg = {k: np.where(sc[k] == 0, np.float32(-0.0), sc[k]).astype(np.float32) for k in ("w1", "w2", "prev_w1", "prev_w2")}
    assert all(np.signbit(v).any() for v in neg.values())
    want = _run(six, x, SEG, dict(sc, **neg))
    assert six.last_launch()[:3] == (pairs, h.last_launch()[1], fading) and six.last_launch()[3] == 0, six.last_launch()
    assert six.last_launch()[4] == S * BLOCKS * 4 + fading, six.last_launch()
    _equal_as_numbers(y, want, "the mixed scene against the same scene with every pass on six rows")
    # ... and no sample of this scene is a zero, so equal as numbers is equal in bits
    assert (want != 0).all() and np.isfinite(want).all()
    _same_bits(y, want, "the mixed scene against the same scene with every pass on six rows")
    _within_bar(y, _model(x, dirs, SEG, sc), "the mixed scene against the f64 model")


def test_plain_and_two_direction_pairs_have_the_bits_of_libohs_scene2():
    """the mixed scene's first four objects -- a plain pair and a two-direction pair, every w2 +0.0 -- through the three-direction
    entry against ohs_scene2_process_blended on libohs_scene2.so: the pass rule promises its passes operation for operation"""
    _, sc = mixed_scene()
    sc = {k: np.ascontiguousarray(v[..., :4]) for k, v in sc.items()}
    assert (sc["w2"] == 0).all() and (sc["w1"][..., :2] == 0).all() and (sc["w1"][..., 2:] > 0).all()
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S, 4, BLOCKS, seed=8710)
    ref, h = _blend(dirs), _tri(dirs)
    want = _run_two(ref, x, SEG, sc)
    y = _run(h, x, SEG, sc)
    assert h.last_launch() == ref.last_launch() + (0,) and ref.last_launch()[3] >= S * BLOCKS, (h.last_launch(), ref.last_launch())
    _same_bits(y, want, "a plain pair and a two-direction pair against ohs_scene2_process_blended on libohs_scene2.so")


def _old_halves(x, sc):
    """(plain, four-row, six-row) passes through OLD entries in the model's plan of the mixed scene"""
    a = sc
    plan = tm.blend3_plan(S, 7, x.shape[2] // BLOCK, *tm.args(a), SEG, a["gains"], a["prev_idx"], a["prev_idx1"], a["prev_idx2"], a["prev_w1"],
                          a["prev_w2"], a["prev_gains"], True)
    n = [0, 0, 0]
    for row in plan:
        for passes in row:
            for (pair, old), kind in tm._pass_kinds(passes).items():
                if old:
                    n[kind] += 1
    return tuple(n)


# ---- d. the change rule -----------------------------------------------------------------------------------------------------------
def test_idx2_changes_an_object_only_beside_a_w2():
    K = 2
    x, dirs, seg, sc = blend3_case(K, 512, False)
    held = {k: np.broadcast_to(sc[k][:, :1], sc[k].shape).copy() for k in ROWS}         # nothing changes in any segment ...
    held.update({"prev_" + k: held[k][:, 0].copy() for k in ROWS})
    held["w1"][...], held["prev_w1"][...] = 0.25, 0.25
    moving, before = _moving(sc["idx"].shape, 60)                                       # ... but idx2, in every one and at the call's start
    # beside w2 = +0.0 on both sides: no bit, no figure
    zero = dict(held, w2=np.zeros_like(held["w2"]), prev_w2=np.zeros_like(held["prev_w2"]))
    a, b = _tri(dirs), _tri(dirs)
    want = _run(a, x, seg, zero)
    y = _run(b, x, seg, dict(zero, idx2=moving, prev_idx2=before))
    assert a.last_launch() == b.last_launch() == (1, a.last_launch()[1], 0, S * BLOCKS, 0), (a.last_launch(), b.last_launch())
    _same_bits(y, want, "idx2 moving beside w2 = +0.0")
    # beside a w2 that is not +0.0: every segment's first block fades, the call's first too
    some = dict(held, w2=np.full_like(held["w2"], 0.125), prev_w2=np.full_like(held["prev_w2"], 0.125), idx2=moving, prev_idx2=before)
    c = _tri(dirs)
    y = _run(c, x, seg, some)
    n_segs = BLOCKS // seg
    assert c.last_launch()[2:] == _figures(x, seg, some) == (S * n_segs, 0, S * BLOCKS + S * n_segs), (c.last_launch(), _figures(x, seg, some))
    _within_bar(y, _model(x, dirs, seg, some), "idx2 moving beside w2 = 0.125")
    # ... and beside +0.0 on ONE side (w2 itself changes there, and the old half reads the old idx2)
    edge = dict(some, w2=some["w2"].copy())
    edge["w2"][:, 1] = 0.0
    d = _tri(dirs)
    y = _run(d, x, seg, edge)
    assert d.last_launch()[2:] == _figures(x, seg, edge), (d.last_launch(), _figures(x, seg, edge))
    _within_bar(y, _model(x, dirs, seg, edge), "idx2 moving beside a w2 that is +0.0 in the middle segment only")


# ---- e. a cut ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_with_every_prev_row_handed_over_equal_one():
    K = 3
    x, dirs, seg, sc = blend3_case(K, 512, False, blocks=8)
    whole = _run(_tri(dirs), x, seg, sc)
    h = _tri(dirs)
    first = {k: np.ascontiguousarray(sc[k][:, :2]) for k in ROWS}
    first.update({"prev_" + k: sc["prev_" + k] for k in ROWS})
    second = {k: np.ascontiguousarray(sc[k][:, 2:]) for k in ROWS}
    second.update({"prev_" + k: np.ascontiguousarray(sc[k][:, 1]) for k in ROWS})
    a = _run(h, x[:, :, :4 * BLOCK], seg, first)
    b = _run(h, x[:, :, 4 * BLOCK:], seg, second)
    _same_bits(np.concatenate([a, b], axis=2), whole, "calls of 4 and 4 blocks against one call of 8")


# ---- f. rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fade", [True, False], ids=["crossfade", "ring_out"])
def test_surplus_row_entries_are_never_read(fade):
    """rows [S][n_segs + 3][K], idx_stride > n_segs: the surplus entries hold what the call refuses where it reads it"""
    x, dirs, seg, sc = blend3_case(3, 512, False)
    wide = dict(sc)
    for k, fill in (("idx", N_DIRS), ("idx1", N_DIRS), ("idx2", 0xffffffff), ("w1", np.nan), ("w2", 2.0), ("gains", np.nan)):
        wide[k] = np.concatenate([sc[k], np.full((S, 3, 3), fill, sc[k].dtype)], axis=1)
    a, b = _tri(dirs), _tri(dirs)
    want, y = _run(a, x, seg, sc, fade), _run(b, x, seg, wide, fade)
    assert np.isfinite(y).all() and a.last_launch() == b.last_launch()
    _same_bits(y, want, f"rows of 6 entries for 3 segments, crossfade {fade}")


def test_a_segment_longer_than_the_call_is_one_segment():
    x, dirs, _, _ = blend3_case(3, 512, False)
    sc = tm.make_blend3_scene(S, 3, BLOCKS, BLOCKS, N_DIRS, seed=19)
    assert sc["idx"].shape == (S, 1, 3)
    out = []
    for seg in (BLOCKS, BLOCKS + 4, 1 << 20):
        h = _tri(dirs)
        out.append(_run(h, x, seg, sc))
        assert h.last_launch()[2] > 0 and h.last_launch()[4] > 0
    _same_bits(out[1], out[0], "seg_blocks = n_blocks + 4 against seg_blocks = n_blocks")
    _same_bits(out[2], out[0], "seg_blocks = 2^20 against seg_blocks = n_blocks")
    _within_bar(out[0], _model(x, dirs, BLOCKS, sc), "one segment")


@pytest.mark.parametrize("shared", [False, True], ids=["rows", "shared"])
def test_a_gain_in_front_of_the_call_beside_no_gain_rows(shared):
    x, dirs, seg, _ = blend3_case(3, 512, False)
    sc = tm.make_blend3_scene(S, 3, BLOCKS, seg, N_DIRS, seed=20, shared=shared)
    assert (sc["prev_gains"] != 1.0).any() and (sc["idx"].ndim == 2) == shared
    h = _tri(dirs)
    y = _run(h, x, seg, sc, gains=None)
    assert h.last_launch()[2:] == _figures(x, seg, sc, gains=None), h.last_launch()
    m = _model(x, dirs, seg, sc, gains=None)
    _within_bar(y, m, f"gains None, prev_gains given, shared {shared}")
    unit = _model(x, dirs, seg, sc, gains=None, prev_gains=None)
    assert (rel_rms_per_stream(unit[:, :, :BLOCK], m[:, :, :BLOCK]) > 1e-3).all()       # (prev_gains does something)


# ---- g. every refused call writes nothing and leaves the handle usable -----------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_handle_usable():
    import torch
    from open_headstage_amd import _ffi, scene3
    L = scene3.scene3_lib()
    K, blocks, seg = 3, BLOCKS, SEG
    frames = blocks * BLOCK
    x, dirs, _, sc = blend3_case(K, 512, False)
    d = torch.from_numpy(x.copy()).cuda()
    SENT = 0x7fc0beef
    sentinel = np.full((S, 2, frames), SENT, np.uint32).view(np.float32)
    out = torch.from_numpy(sentinel.copy()).cuda()
    INV, OK = _ffi.OHS_ERR_INVALID_ARG, _ffi.OHS_OK
    up, fp = C.POINTER(C.c_uint32), _ffi.fp
    f = L.ohs_scene3_process_blended3

    def call(h, mode=1, **over):
        a = dict(sc, **over)

        def u(name):
            v = a[name]
            return None if v is None else np.ascontiguousarray(v, np.uint32).ctypes.data_as(up)

        def fl(name):
            v = a[name]
            return None if v is None else np.ascontiguousarray(v, np.float32).ctypes.data_as(fp)
        rc = f(h._h, C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr()), blocks, K * frames, frames, 2 * frames, frames, K, seg, u("idx"),
               fl("gains"), sc["idx"].shape[1], u("prev_idx"), fl("prev_gains"), mode, None, u("idx1"), fl("w1"), u("prev_idx1"), fl("prev_w1"),
               u("idx2"), fl("w2"), u("prev_idx2"), fl("prev_w2"))
        torch.cuda.synchronize()
        return rc

    def changed(name, where, value):
        v = sc[name].copy()
        v[where] = value
        return {name: v}

    def refused(what, needle, **over):
        assert call(h, **over) == INV, what
        assert needle in L.ohs_scene3_last_error(), (what, L.ohs_scene3_last_error())
        assert (out.cpu().numpy().view(np.uint32) == SENT).all(), f"{what}: the refused call wrote to the output"
        assert h.last_launch() == (0, 0, 0, 0, 0), (what, h.last_launch())

    h, twin = _tri(dirs), _tri(dirs)
    two_up = np.float32(0.5) + np.float32(2.0 ** -23)                               # 0.5 + (0.5 + 2^-23) is 1 + 2^-23 in f32: just above 1
    assert np.float32(np.float32(0.5) + two_up) == np.nextafter(np.float32(1), np.float32(2))
    refused("w1 + w2 just above 1", b"w1 + w2", **dict(changed("w1", (1, 1, 2), 0.5), **changed("w2", (1, 1, 2), two_up)))
    refused("a negative w2", b"w2 >= 0", **changed("w2", (0, 0, 0), -0.25))
    refused("a negative w1", b"w1 >= 0", **changed("w1", (S - 1, 2, K - 1), -1e-30))
    refused("a NaN w2", b"weight", **changed("w2", (1, 0, 1), np.nan))
    refused("a NaN w1", b"weight", **changed("w1", (1, 0, 1), np.nan))
    # a bad pair in the FIRST segment with nothing named in front of the call is refused under its own name, not prev_*'s
    refused("a first-segment pair above the triangle, no prev_w named", b"weight / weight2",
            prev_w1=None, prev_w2=None, **dict(changed("w1", (0, 0, 0), 0.75), **changed("w2", (0, 0, 0), 0.5)))
    assert b"prev_" not in L.ohs_scene3_last_error(), L.ohs_scene3_last_error()
    refused("the same pair beside a named prev_w2", b"weight", **dict(changed("w1", (0, 0, 0), 0.75), **changed("w2", (0, 0, 0), 0.5)))
    refused("prev_w2 above the triangle", b"prev_weight", **changed("prev_w2", (0, 1), 1.5))
    refused("a NaN prev_w2", b"prev_weight", **changed("prev_w2", (2, 0), np.nan))
    for where in [(0, 0, 0), (S - 1, 2, K - 1)]:
        refused(f"idx2 out of range at {where}", b"dir_idx2", **changed("idx2", where, N_DIRS))
    refused("prev_idx2 out of range", b"prev_idx2", **changed("prev_idx2", (1, 1), 0xffffffff))
    refused("dir_idx2 without weight2", b"both", w2=None)
    refused("weight2 without dir_idx2", b"both", idx2=None)
    refused("dir_idx2 and weight2 without dir_idx1 and weight", b"need", idx1=None, w1=None)
    refused("an idx1 out of range", b"dir_idx1", **changed("idx1", (1, 1, 0), N_DIRS))
    refused("a switch mode of 2", b"switch_mode", mode=2)
    # -0.0 is a weight; under RING_OUT the entries in front of the call are not read; a sum of exactly 1 passes
    assert call(_tri(dirs), **changed("w2", (0, 0, 1), -0.0)) == OK
    assert call(_tri(dirs), mode=0, **changed("prev_w2", (1, 2), 2.0)) == OK
    half = dict(changed("w1", (0, 0, 0), 0.5), **changed("w2", (0, 0, 0), 0.5))
    assert call(_tri(dirs), **half) == OK
    # (the sum is formed in f32: 0.5 + (0.5 + 2^-24) rounds to 1)
    assert call(_tri(dirs), **dict(half, **changed("w2", (0, 0, 0), np.nextafter(np.float32(0.5), np.float32(1))))) == OK
    out.copy_(torch.from_numpy(sentinel.copy()).cuda())
    # ... and none of them touched the state: the handle serves as its twin does
    assert call(h) == OK
    got = out.cpu().numpy().copy()
    _same_bits(got, _run(twin, x, seg, sc), "the valid call behind the refused ones")
    _same_bits(_run(h, x, seg, sc), _run(twin, x, seg, sc), "and the call after it")


# ---- h. limits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 63])
def test_64_and_63_objects_with_three_directions_in_the_last_pair(K):
    """pair 31 (K = 63: the odd last object, alone) takes the six-row pass and fades; a few objects are loud, the others silent (a silent
    pair adds exact zeros), so the figures are the small cases' and the index logic is the 64-object one"""
    S5, blocks, seg = 5, BLOCKS, SEG
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S5, K, blocks, seed=8800 + K)
    sc = tm.make_blend3_scene(S5, K, blocks, seg, N_DIRS, seed=K)
    loud = sorted({0, 1, 30, 31, 32, 33, K - 4, K - 3, K - 2, K - 1})
    for k in ("gains", "prev_gains"):
        g = np.zeros_like(sc[k])
        g[..., loud] = sc[k][..., loud]
        sc[k] = g
    last = K - 1
    sc["w2"][..., last], sc["prev_w2"][..., last] = np.float32(0.2), np.float32(0.1)           # (a change in w2 at the call's start)
    sc["w1"][..., last], sc["prev_w1"][..., last] = np.float32(0.3), np.float32(0.3)
    h = _tri(dirs, S5)
    y = _run(h, x, seg, sc)
    plan = tm.blend3_plan(S5, K, blocks, *tm.args(sc), seg, sc["gains"], sc["prev_idx"], sc["prev_idx1"], sc["prev_idx2"], sc["prev_w1"],
                          sc["prev_w2"], sc["prev_gains"], True)
    kinds = [tm._pass_kinds(p) for row in plan for p in row]
    assert all(k[(31, False)] == 2 for k in kinds) and sum((31, True) in k for k in kinds) >= S5
    assert h.last_launch()[0] == 32 and h.last_launch()[2:] == _figures(x, seg, sc), (h.last_launch(), _figures(x, seg, sc))
    _within_bar(y, tm.model_blend3_f64(x, dirs, *tm.args(sc), seg, crossfade=True, gain=GAIN, **tm.kw(sc)), f"K = {K}, three directions in pair 31")


def full_scene3():
    """tests/test_gpu_scene_wide.py's full_scene with a third direction and a second weight: -> (the scene on the table of 65 536, the
    same scene on a table of its nine rows); rows 0 and 65 535 stand in all three slots, object 1 has w2 = +0.0"""
    from tests.test_gpu_scene_wide import NINE, full_scene
    pos, pos1, w, g = full_scene()
    rng = np.random.default_rng(616)
    pos2 = (pos1 + 1 + rng.integers(0, 7, pos.shape)) % 9
    pos2 = np.where(pos2 == pos, (pos2 + 1) % 9, pos2)
    pos2 = np.where(pos2 == pos1, (pos2 + 1) % 9, pos2)
    pos2 = np.where(pos2 == pos, (pos2 + 1) % 9, pos2)
    assert (pos2 != pos).all() and (pos2 != pos1).all()
    w1 = (w * np.float32(0.5)).astype(np.float32)
    w2 = rng.uniform(0.05, 0.45, pos.shape).astype(np.float32)
    w2[:, :, 1] = 0.0
    c = np.ascontiguousarray

    def scene_of(table_idx):
        i, j, k = (table_idx[p].astype(np.uint32) for p in (pos, pos1, pos2))
        return dict(idx=c(i[:, 1:]), idx1=c(j[:, 1:]), idx2=c(k[:, 1:]), w1=c(w1[:, 1:]), w2=c(w2[:, 1:]), gains=c(g[:, 1:]),
                    prev_idx=c(i[:, 0]), prev_idx1=c(j[:, 0]), prev_idx2=c(k[:, 0]), prev_w1=c(w1[:, 0]), prev_w2=c(w2[:, 0]), prev_gains=c(g[:, 0]))
    big, small = scene_of(NINE), scene_of(np.arange(9, dtype=np.uint32))
    for k in ("idx", "idx1", "idx2"):
        assert {0, 65535} <= set(np.concatenate([big[k].ravel(), big["prev_" + k].ravel()]).tolist()), k
    return big, small


def test_full_table_of_65536_directions():
    """tests/test_gpu_scene_wide.py's table and shape; K = 3 reads the zero row behind the table.  A row's spectrum does not depend on
    where in the table it sits: the same scene on a table of the nine rows, bit for bit."""
    from tests.test_gpu_scene_wide import NINE, full_table
    table = full_table()
    big, small = full_scene3()
    x = make_input(3, 3, 6, seed=21500)
    h = _tri(table)
    y = _run(h, x, 2, big)
    assert h.last_launch()[4] > 0 and h.last_launch()[2] > 0
    _within_bar(y, _model(x, table, 2, big), "65 536 directions of 8 taps, three per object")
    _same_bits(y, _run(_tri(table[NINE]), x, 2, small), "the table of 65 536 against a table of those nine rows")


# ---- i. flush modes, silence, scaling ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_the_flush_mode_changes_no_bit_of_a_loud_signal_and_silence_gives_zeros(mode):
    x, dirs, seg, sc = blend3_case(3, 512, False)
    ieee, ftz = _tri(dirs), _tri(dirs)
    ftz.set_flush_denormals(mode)
    want = _run(ieee, x, seg, sc)
    assert float(np.abs(want).max()) > 0.01
    _same_bits(_run(ftz, x, seg, sc), want, f"flush mode {mode} against mode 0, a loud signal")
    quiet = _tri(dirs)
    quiet.set_flush_denormals(mode)
    y = _run(quiet, np.zeros_like(x), seg, sc)
    assert (y == 0).all(), f"mode {mode}: silence in, {int((y != 0).sum())} samples that are not zero out"


def test_scaling_a_stream_by_a_power_of_two_scales_its_output_exactly():
    x, dirs, seg, sc = blend3_case(3, 512, False)
    ks = np.array([0, 40, -40], np.int32)
    twin = _run(_tri(dirs), x, seg, sc)
    got = _run(_tri(dirs), np.ldexp(x, ks[:, None, None]).astype(np.float32), seg, sc)
    _same_bits(np.ldexp(got, -ks[:, None, None]).astype(np.float32), twin, f"streams times 2^{ks.tolist()}, unscaled")
    assert got[0].tobytes() == twin[0].tobytes(), "the stream that was not scaled"


# ---- j. one randomised sequence over the three processing entries of one handle --------------------------------------------------
FUZZ_SEED = 20261020


def draw_sequence(seed=FUZZ_SEED, n_ops=14):
    """-> a list of ("call", dict) and setter ops (tests/test_gpu_scene_fuzz.py's scheme): K, seg_blocks, blocks, the entry (1, 2 or
    3 directions), the switch mode, the row form, gains and every prev_* given or None are drawn per call"""
    rng = np.random.default_rng(seed)
    ops = []
    for n in range(n_ops):
        if n % 2 == 0 and n > 0:        # a setter in front of every second call, the three in turn
            which = (n // 2 - 1) % 3
            ops.append([("set_gain", float(rng.choice([0.5, 1.0, 1.3]))), ("reset",),
                        ("set_directions", int(rng.choice([8, 37, 512])), int(rng.integers(0, 1000)))][which])
        K, seg, blocks = int(rng.choice([1, 2, 3, 5, 8])), int(rng.choice([1, 2, 3])), int(rng.integers(1, 7))
        sc = tm.make_blend3_scene(S, K, blocks, seg, N_DIRS, seed=int(rng.integers(0, 1000)), shared=bool(rng.random() < 0.3))
        for name in ("gains", "prev_idx", "prev_idx1", "prev_idx2", "prev_w1", "prev_w2", "prev_gains"):
            if rng.random() < 0.3:
                sc[name] = None
        ops.append(("call", dict(K=K, seg=seg, blocks=blocks, entry=(3, 2, 1, 3, 3)[n % 5], fade=bool(rng.random() < 0.7), sc=sc,
                                 x_seed=int(rng.integers(0, 1 << 30)))))
    return ops


def test_one_randomised_sequence_over_the_three_entries_against_one_model():
    """one handle, one model: the model carries the overlap from call to call whatever entry served it"""
    from tests import scene_model as sm
    ops = draw_sequence()
    assert {op[1]["entry"] for op in ops if op[0] == "call"} == {1, 2, 3}
    assert {op[0] for op in ops} >= {"call", "set_gain", "reset", "set_directions"}
    dirs = make_layout(N_DIRS, 512)
    h = _tri(dirs)
    gain, tail = GAIN, None
    for n, op in enumerate(ops):
        if op[0] == "set_gain":         # (the overlap is kept without the gain: the model runs at gain 1, tail and all)
            gain = op[1]
            h.set_gain(gain)
        elif op[0] == "reset":
            h.reset()
            tail = None
        elif op[0] == "set_directions":
            dirs = make_layout(N_DIRS, op[1]) * np.float32(1.0 + (op[2] % 7) / 16.0)
            h.set_directions(dirs)
            tail = None
        else:
            c = op[1]
            sc, seg = c["sc"], c["seg"]
            x = make_input(S, c["K"], c["blocks"], seed=c["x_seed"] % 100000)
            if c["entry"] == 3:
                y = _run(h, x, seg, sc, c["fade"])
                m, tail = tm.model_blend3_f64(x, dirs, *tm.args(sc), seg, crossfade=c["fade"], gain=1.0, tail_in=tail, with_tail=True, **tm.kw(sc))
                want = _figures(x, seg, sc, c["fade"])
            elif c["entry"] == 2:
                y = _run_two(h, x, seg, sc, c["fade"])
                m, tail = bm.model_blend_f64(x, dirs, sc["idx"], sc["idx1"], sc["w1"], seg, sc["gains"], sc["prev_idx"], sc["prev_idx1"],
                                             sc["prev_w1"], sc["prev_gains"], c["fade"], 1.0, tail, True)
                plan = bm.blend_plan(S, c["K"], c["blocks"], sc["idx"], sc["idx1"], sc["w1"], seg, sc["gains"], sc["prev_idx"], sc["prev_idx1"],
                                     sc["prev_w1"], sc["prev_gains"], c["fade"])
                want = (bm.count_fading_passes(plan), bm.count_blended_passes(plan, c["K"]), 0)
            else:
                y = _run_one(h, x, sc["idx"], seg, sc["gains"], sc["prev_idx"], sc["prev_gains"], c["fade"])
                m, tail = sm.model_scene_f64(x, dirs, sc["idx"], seg, sc["gains"], sc["prev_idx"], sc["prev_gains"], c["fade"], 1.0, tail, True)
                plan = sm.scene_plan(S, c["K"], c["blocks"], sc["idx"], seg, sc["gains"], sc["prev_idx"], sc["prev_gains"], c["fade"])
                want = (sm.count_fading_passes(plan), 0, 0)
            assert h.last_launch()[2:] == want, (n, c["entry"], h.last_launch(), want)
            _within_bar(y, gain * m, f"op {n}: entry with {c['entry']} direction(s), K = {c['K']}, seg {seg}, {c['blocks']} blocks, crossfade {c['fade']}")


# ---- k. the call on a busy stream against its quiet twin ---------------------------------------------------------------------------
def test_the_call_on_a_busy_stream_has_its_quiet_twins_bits():
    """tests/busy_stream.py's harness: the caller's side stream is busy when the call is made, the input arrives by a copy queued behind
    that work, every host row is overwritten the moment the call returns, the output leaves by a copy queued behind the call"""
    import time

    import torch
    K = 3
    x, dirs, seg, sc = blend3_case(K, 512, False)
    frames = BLOCKS * BLOCK
    quiet = _tri(dirs)
    t0 = time.perf_counter()
    want = _run(quiet, x, seg, sc)
    enqueue_s = time.perf_counter() - t0
    h = _tri(dirs)
    busy = bs.BusyStream()
    rows = bs.row_arrays(sc)
    src = torch.from_numpy(x.copy()).pin_memory()
    nan = float("nan")
    d_in = torch.full((S, K, frames), nan, device="cuda")
    d_out = torch.full((S, 2, frames), nan, device="cuda")
    keep = torch.full((S, 2, frames), nan, device="cuda")
    torch.cuda.synchronize()
    try:
        busy.fill(bs.filler_seconds(min(enqueue_s, 0.01)))
        with torch.cuda.stream(busy.stream):
            d_in.copy_(src, non_blocking=True)
            h.process_ptr(d_in.data_ptr(), d_out.data_ptr(), BLOCKS, K * frames, frames, 2 * frames, frames, K, seg, rows["idx"], rows["gains"],
                          rows["prev_idx"], rows["prev_gains"], True, busy.handle, rows["idx1"], rows["w1"], rows["prev_idx1"], rows["prev_w1"],
                          rows["idx2"], rows["w2"], rows["prev_idx2"], rows["prev_w2"])
            busy.premise("ohs_scene3_process_blended3")
            bs.scribble(rows)
            rec = h.last_launch()
            keep.copy_(d_out, non_blocking=True)
            d_in.fill_(nan)
            d_out.fill_(nan)
    finally:
        torch.cuda.synchronize()
    assert rec == quiet.last_launch(), (rec, quiet.last_launch())
    bs.same_bits(keep.cpu().numpy(), want, "ohs_scene3_process_blended3 on a busy stream")

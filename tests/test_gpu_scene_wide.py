"""Both object-scene kernels (k_conv_p1_objects in libohs_scene.so, k_conv_p1_objects_blend in libohs_scene2.so) at the limits their
headers name: 64 objects, 65 536 directions, row arrays longer than the segments read, segments longer than the call.

The yardstick is never the call under test: the f64 models of tests/scene_model.py and tests/scene_blend_model.py (held to their
time-domain twins at K = 64, and shown to be far from a 32-bit change set, a dropped pair 31 and a rendered odd partner, in
tests/test_cpu_scene.py and tests/test_cpu_scene_blend.py), or a second handle of the same library where bits are promised.  Bars:
bit for bit, or 1e-6 relative RMS per stream AND per 512-frame block (_within_bar: the project's FFT bar).  No other
tolerance appears here.  Gain 0.7 throughout; with -s every comparison prints its worst figures."""
import numpy as np
import pytest

from tests import scene_blend_model as bm
from tests import scene_model as sm
from tests.test_cpu_layout import BLOCK, make_input, make_layout
from tests.test_gpu_layout import _same_bits
from tests.test_gpu_scene import _within_bar
from tests.test_gpu_scene_blend import GAIN, _blend, _plain, _run, _run_plain

pytestmark = pytest.mark.gpu

N_DIRS = 7
# ---- 1. wide scenes ------------------------------------------------------------------------------------------------------------------
WIDE_S, WIDE_BLOCKS, WIDE_SEG = 5, 6, 2         # five streams cross one workgroup of the layout shape; three segments
# (K, which half of wide_patterns(K)): three patterns per scene, one per segment, the first against prev_*
WIDE_CASES = [(K, half) for K in (33, 63, 64) for half in (0, 1)]
_WIDE_IDS = [f"K{K}-patterns{3 * h}to{3 * h + 2}" for K, h in WIDE_CASES]


def wide_case(K, half, all_loud, blend):
    """-> (x, dirs, seg_blocks, scene): scene is (idx, gains, prev_idx, prev_gains), or with blend make_wide_blend_scene's dict
    (tests/test_cpu_scene.py and tests/test_cpu_scene_blend.py run the wide mutants on these)"""
    changed = sm.wide_patterns(K)[3 * half:3 * half + 3]
    loud = None if all_loud else sm.wide_loud(K)
    x = make_input(WIDE_S, K, WIDE_BLOCKS, seed=20000 + 1000 * half + 7 * K)
    make = bm.make_wide_blend_scene if blend else sm.make_wide_scene
    return x, make_layout(N_DIRS, 512), WIDE_SEG, make(WIDE_S, K, WIDE_BLOCKS, WIDE_SEG, changed, loud, N_DIRS, seed=10 * K + half)


def _blend_args(sc):
    return (sc["idx"], sc["idx1"], sc["weights"])


def _blend_kw(sc):
    return dict(gains=sc["gains"], prev_idx=sc["prev_idx"], prev_idx1=sc["prev_idx1"], prev_weights=sc["prev_weights"],
                prev_gains=sc["prev_gains"])


def kinds_of_change(sc):
    """the objects that change in a wide blended scene hold some that change ONLY in their weight and some ONLY in their second
    direction, beside a weight that is not +0.0 (asserted; -> the two counts)"""
    rows = {k: np.concatenate([sc["prev_" + k][:, None], sc[k]], axis=1) for k in ("idx", "idx1", "weights", "gains")}
    d = {k: v[:, 1:].view(np.uint32) != v[:, :-1].view(np.uint32) for k, v in rows.items()}
    only_w = int((d["weights"] & ~d["idx"] & ~d["idx1"] & ~d["gains"]).sum())
    read = (rows["weights"][:, 1:].view(np.uint32) | rows["weights"][:, :-1].view(np.uint32)) != 0
    only_idx1 = int((d["idx1"] & read & ~d["idx"] & ~d["weights"] & ~d["gains"]).sum())
    assert only_w > 0 and only_idx1 > 0, (only_w, only_idx1)
    return only_w, only_idx1


def _wide_plain(K, half, all_loud):
    x, dirs, seg, (idx, gains, pi, pg) = wide_case(K, half, all_loud, False)
    h = _plain(dirs, WIDE_S)
    y = _run_plain(h, x, idx, seg, gains, pi, pg)
    plan = sm.scene_plan(WIDE_S, K, WIDE_BLOCKS, idx, seg, gains, pi, pg, True)
    want = sm.count_fading_passes(plan)
    assert want == sum(len({c // 2 for c in pat}) for pat in sm.wide_patterns(K)[3 * half:3 * half + 3]) * WIDE_S
    assert h.last_launch()[0] == (K + 1) // 2 and h.last_launch()[2] == want, (h.last_launch(), want)
    return y, sm.model_scene_f64(x, dirs, idx, seg, gains, pi, pg, True, GAIN)


def _wide_blend(K, half, all_loud):
    x, dirs, seg, sc = wide_case(K, half, all_loud, True)
    h = _blend(dirs, WIDE_S)
    y = _run(h, x, seg, sc)
    plan = bm.blend_plan(WIDE_S, K, WIDE_BLOCKS, *_blend_args(sc), seg, sc["gains"], sc["prev_idx"], sc["prev_idx1"], sc["prev_weights"],
                         sc["prev_gains"], True)
    fading, blended = bm.count_fading_passes(plan), bm.count_blended_passes(plan, K)
    assert fading == sum(len({c // 2 for c in pat}) for pat in sm.wide_patterns(K)[3 * half:3 * half + 3]) * WIDE_S and blended > 0
    assert h.last_launch()[0] == (K + 1) // 2 and h.last_launch()[2:] == (fading, blended), (h.last_launch(), fading, blended)
    kinds_of_change(sc)
    return y, bm.model_blend_f64(x, dirs, *_blend_args(sc), seg, crossfade=True, gain=GAIN, **_blend_kw(sc))


@pytest.mark.parametrize("case", WIDE_CASES, ids=_WIDE_IDS)
@pytest.mark.parametrize("kernel", ["plain", "blend"])
def test_wide_scene_few_loud_against_the_f64_model(kernel, case):
    """objects 30 .. 35 and the last six are loud, every other gain is 0.0 (a silent pair adds exact zeros): the error is the K = 8
    cases', the change set's index logic is the 64-object one"""
    y, m = (_wide_plain if kernel == "plain" else _wide_blend)(*case, False)
    _within_bar(y, m, f"{kernel} kernel, K = {case[0]}, patterns {3 * case[1]} .. {3 * case[1] + 2}, few loud")


@pytest.mark.parametrize("case", WIDE_CASES, ids=_WIDE_IDS)
@pytest.mark.parametrize("kernel", ["plain", "blend"])
def test_wide_scene_all_loud_against_the_f64_model(kernel, case):
    """the same rows with every object loud, held to the bar itself: the objects' inputs are independent noise, so the relative error
    of the sum does not grow with K, and the f32 accumulation over P = 32 pairs adds about eps sqrt(P / 2) = 1e-7"""
    y, m = (_wide_plain if kernel == "plain" else _wide_blend)(*case, True)
    _within_bar(y, m, f"{kernel} kernel, K = {case[0]}, patterns {3 * case[1]} .. {3 * case[1] + 2}, all loud")


# ---- 2. the full direction table ------------------------------------------------------------------------------------------------------
FULL_DIRS, FULL_TAPS = 65536, 8
NINE = np.array([0, 255, 256, 1023, 1024, 32767, 32768, 65534, 65535], np.uint32)      # (they cross the upload's slices of 1 024)


def full_table():
    """[65 536][2][8] float32 from a seeded generator, its rows pairwise distinct"""
    t = (np.float32(0.125) * np.random.default_rng(4242).standard_normal((FULL_DIRS, 2, FULL_TAPS))).astype(np.float32)
    assert np.unique(t.reshape(FULL_DIRS, -1).view(np.uint32), axis=0).shape[0] == FULL_DIRS
    assert len({t[d].tobytes() for d in NINE}) == len(NINE)         # the rows the scene uses are distinct
    return t


def full_scene(S=3, K=3, blocks=6, seg=2):
    """indices from NINE, every one of them in idx and in idx1; object 0 blended, 1 at w = +0.0, the odd last one blended (its partner
    is the zero row behind the table); a gain per object; rows [S][n_segs][K], prev_* given"""
    rng = np.random.default_rng(515)
    n_segs = blocks // seg
    n = S * (n_segs + 1) * K
    pos = np.concatenate([rng.permutation(9) for _ in range(-(-n // 9))])[:n].reshape(S, n_segs + 1, K)
    pos1 = (pos + 1 + rng.integers(0, 8, pos.shape)) % 9
    w = rng.uniform(0.05, 0.95, pos.shape).astype(np.float32)
    w[:, :, 1] = 0.0
    g = np.broadcast_to(rng.choice(np.array([0.5, 0.75, 1.0, 1.25], np.float32), (S, 1, K)), pos.shape).copy()
    assert set(pos.ravel()) == set(range(9)) and set(pos1.ravel()) == set(range(9)) and (pos != pos1).all()
    return pos, pos1, w, g


def _scene_of(pos, pos1, w, g, table_idx):
    i, j = table_idx[pos].astype(np.uint32), table_idx[pos1].astype(np.uint32)
    c = np.ascontiguousarray
    return dict(idx=c(i[:, 1:]), idx1=c(j[:, 1:]), weights=c(w[:, 1:]), gains=c(g[:, 1:]), prev_idx=c(i[:, 0]), prev_idx1=c(j[:, 0]),
                prev_weights=c(w[:, 0]), prev_gains=c(g[:, 0]))


@pytest.mark.parametrize("kernel", ["plain", "blend"])
def test_full_table_of_65536_directions(kernel):
    table = full_table()
    pos, pos1, w, g = full_scene()
    big, small = _scene_of(pos, pos1, w, g, NINE), _scene_of(pos, pos1, w, g, np.arange(9, dtype=np.uint32))
    x = make_input(3, 3, 6, seed=21500)
    if kernel == "plain":
        y = _run_plain(_plain(table), x, big["idx"], 2, big["gains"], big["prev_idx"], big["prev_gains"])
        m = sm.model_scene_f64(x, table, big["idx"], 2, big["gains"], big["prev_idx"], big["prev_gains"], True, GAIN)
        nine = _run_plain(_plain(table[NINE]), x, small["idx"], 2, small["gains"], small["prev_idx"], small["prev_gains"])
    else:
        h = _blend(table)
        y = _run(h, x, 2, big)
        assert h.last_launch()[3] > 0
        m = bm.model_blend_f64(x, table, *_blend_args(big), 2, crossfade=True, gain=GAIN, **_blend_kw(big))
        nine = _run(_blend(table[NINE]), x, 2, small)
    _within_bar(y, m, f"{kernel} kernel, 65 536 directions of 8 taps, indices from {NINE.tolist()}")
    # a row's spectrum does not depend on where in the table, or in which slice of the upload, it sits
    _same_bits(y, nine, f"{kernel} kernel: the table of 65 536 against a table of those nine rows")


@pytest.mark.parametrize("kernel", ["plain", "blend"])
def test_a_table_of_one_direction(kernel):
    """n_dirs = 1: the zero row is row 1; K = 3, so it is read"""
    dirs = make_layout(1, 512)
    x = make_input(3, 3, 6, seed=21600)
    sc = bm.make_blend_scene(3, 3, 6, 2, N_DIRS, seed=16)
    zero = {k: np.zeros_like(sc[k]) for k in ("idx", "idx1", "prev_idx", "prev_idx1")}
    sc = dict(sc, **zero)
    if kernel == "plain":
        h = _plain(dirs)
        y = _run_plain(h, x, sc["idx"], 2, sc["gains"], sc["prev_idx"], sc["prev_gains"])
        assert h.last_launch()[2] > 0          # (the gains change)
        m = sm.model_scene_f64(x, dirs, sc["idx"], 2, sc["gains"], sc["prev_idx"], sc["prev_gains"], True, GAIN)
    else:
        h = _blend(dirs)
        y = _run(h, x, 2, sc)
        assert h.last_launch()[2] > 0 and h.last_launch()[3] > 0
        m = bm.model_blend_f64(x, dirs, *_blend_args(sc), 2, crossfade=True, gain=GAIN, **_blend_kw(sc))
    _within_bar(y, m, f"{kernel} kernel, a table of one direction, K = 3")


@pytest.mark.parametrize("taps", [1, 511])
@pytest.mark.parametrize("kernel", ["plain", "blend"])
def test_taps_of_1_and_511(kernel, taps):
    dirs = make_layout(N_DIRS, taps)
    x = make_input(3, 3, 6, seed=21700 + taps)
    sc = bm.make_blend_scene(3, 3, 6, 2, N_DIRS, seed=17)
    if kernel == "plain":
        y = _run_plain(_plain(dirs), x, sc["idx"], 2, sc["gains"], sc["prev_idx"], sc["prev_gains"])
        m = sm.model_scene_f64(x, dirs, sc["idx"], 2, sc["gains"], sc["prev_idx"], sc["prev_gains"], True, GAIN)
    else:
        y = _run(_blend(dirs), x, 2, sc)
        m = bm.model_blend_f64(x, dirs, *_blend_args(sc), 2, crossfade=True, gain=GAIN, **_blend_kw(sc))
    _within_bar(y, m, f"{kernel} kernel, {taps} taps")


# ---- 3. row strides and segment edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fade", [True, False], ids=["crossfade", "ring_out"])
@pytest.mark.parametrize("kernel", ["plain", "blend"])
def test_surplus_row_entries_are_never_read(kernel, fade):
    """rows [S][n_segs + 3][K], idx_stride > n_segs: the three surplus entries of every row hold what the call refuses where it reads
    it -- the index n_dirs, a NaN weight, a NaN gain.  The call is served, with the bits of the call on dense rows."""
    S, K, blocks, seg = 3, 3, 7, 2
    n_segs = 4
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S, K, blocks, seed=21800)
    sc = bm.make_blend_scene(S, K, blocks, seg, N_DIRS, seed=18)
    wide = dict(sc)
    for k, fill in (("idx", N_DIRS), ("idx1", N_DIRS), ("weights", np.nan), ("gains", np.nan)):
        assert sc[k].shape == (S, n_segs, K)
        wide[k] = np.concatenate([sc[k], np.full((S, 3, K), fill, sc[k].dtype)], axis=1)
    if kernel == "plain":
        a, b = _plain(dirs), _plain(dirs)
        want = _run_plain(a, x, sc["idx"], seg, sc["gains"], sc["prev_idx"], sc["prev_gains"], fade)
        y = _run_plain(b, x, wide["idx"], seg, wide["gains"], sc["prev_idx"], sc["prev_gains"], fade)
    else:
        a, b = _blend(dirs), _blend(dirs)
        want = _run(a, x, seg, sc, fade)
        y = _run(b, x, seg, wide, fade)
    assert np.isfinite(y).all() and a.last_launch() == b.last_launch() and (a.last_launch()[2] > 0) == fade
    _same_bits(y, want, f"{kernel} kernel, rows of {n_segs + 3} entries for {n_segs} segments, crossfade {fade}")


@pytest.mark.parametrize("kernel", ["plain", "blend"])
def test_a_segment_longer_than_the_call_is_one_segment(kernel):
    S, K, blocks = 3, 3, 5
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S, K, blocks, seed=21900)
    sc = bm.make_blend_scene(S, K, blocks, blocks, N_DIRS, seed=19)
    assert sc["idx"].shape == (S, 1, K)
    out = []
    for seg in (blocks, blocks + 4, 1 << 20):
        if kernel == "plain":
            h = _plain(dirs)
            out.append(_run_plain(h, x, sc["idx"], seg, sc["gains"], sc["prev_idx"], sc["prev_gains"]))
        else:
            h = _blend(dirs)
            out.append(_run(h, x, seg, sc))
        assert h.last_launch()[2] > 0           # (prev_*: a boundary at the call's start)
    _same_bits(out[1], out[0], f"{kernel} kernel, seg_blocks = n_blocks + 4 against seg_blocks = n_blocks")
    _same_bits(out[2], out[0], f"{kernel} kernel, seg_blocks = 2^20 against seg_blocks = n_blocks")


def test_a_gain_in_front_of_a_shared_row_without_gain_rows():
    """gains None, prev_gains given, ONE row for all streams (idx_stride 0) in the blended call: the host stages the 1.0 rows itself, a
    single row of them"""
    S, K, blocks, seg = 3, 3, 6, 2
    dirs = make_layout(N_DIRS, 512)
    x = make_input(S, K, blocks, seed=22000)
    sc = bm.make_blend_scene(S, K, blocks, seg, N_DIRS, seed=20, shared=True)
    assert sc["idx"].ndim == 2 and (sc["prev_gains"] != 1.0).any()
    h = _blend(dirs)
    y = _run(h, x, seg, sc, gains=None)
    plan = bm.blend_plan(S, K, blocks, *_blend_args(sc), seg, None, sc["prev_idx"], sc["prev_idx1"], sc["prev_weights"], sc["prev_gains"], True)
    assert h.last_launch()[0] == 2 and h.last_launch()[2:] == (bm.count_fading_passes(plan), bm.count_blended_passes(plan, K)), h.last_launch()
    m = bm.model_blend_f64(x, dirs, *_blend_args(sc), seg, crossfade=True, gain=GAIN, **dict(_blend_kw(sc), gains=None))
    _within_bar(y, m, "blended call, a shared row, gains None, prev_gains given")
    unit = bm.model_blend_f64(x, dirs, *_blend_args(sc), seg, crossfade=True, gain=GAIN, **dict(_blend_kw(sc), gains=None, prev_gains=None))
    from tests.test_cpu_layout import rel_rms_per_stream
    assert (rel_rms_per_stream(unit[:, :, :BLOCK], m[:, :, :BLOCK]) > 1e-3).all()       # (prev_gains does something)

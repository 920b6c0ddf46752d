"""The object-scene kernels under the harnesses built for every kernel family: the three flush-denormals promises
(tests/flush_modes.py), exact scaling and non-finite containment (tests/special_values.py).  Checkers unchanged.

Both libraries (k_conv_p1_objects, k_conv_p1_objects_blend): 3 streams, K = 3 -- in the blended case the odd last object is
blended --, 7 directions of 512 taps, seg_blocks 2, object 0 moving in EVERY segment so that pair 0 fades in each, the other objects
on tests/scene_blend_model.py's trajectories.  Calls of 6 and 5 blocks on one handle, the second continuing the first one's overlap
with prev_* handed on.  The twin is the same configuration in mode 0 on the same input; bars: bit for bit, or equal as numbers.
The kernels form (x gain) ramp in front of the transform and the blended one u A + w B in front of the product -- places for a
subnormal to appear or survive that no other family has."""
import numpy as np
import pytest

from tests import flush_modes as fm
from tests import scene_blend_model as bm
from tests import scene_model as sm
from tests import special_values as sv
from tests.test_cpu_layout import BLOCK, make_input, make_layout
from tests.test_gpu_layout import _same_bits
from tests.test_gpu_scene_blend import _blend, _plain, _run, _run_plain

pytestmark = pytest.mark.gpu

S, K, N_DIRS, SEG = 3, 3, 7, 2
CALLS = (6, 5)
TOTAL = sum(CALLS)
CROSSING = 3            # falling_input's block: stream s passes 2^-126 in block CROSSING + 2 - s, all inside the first call
C_GAIN_POW = 5          # case C: every object gain times 2^5 (exact): the OUTPUT starts in the normal range as well, and falls through it
KERNELS = ["plain", "blend"]


def modes_scene(gain_pow=0):
    """-> one scene dict per call (rows [S][n_segs][K], prev_* what stood in front of the call); every object gain times 2^gain_pow"""
    n_segs = (TOTAL + 1) // SEG
    sc = bm.make_blend_scene(S, K, n_segs * SEG, SEG, N_DIRS, seed=55)
    moving, before = sm.make_switching_rows(S, K, n_segs, N_DIRS, seed=55)
    sc["idx"][:, :, 0], sc["prev_idx"][:, 0] = moving[:, :, 0], before[:, 0]
    assert (sc["idx"][:, 1:, 0] != sc["idx"][:, :-1, 0]).all() and (sc["idx"][:, 0, 0] != sc["prev_idx"][:, 0]).all()
    assert (sc["weights"][:, :, 2] != 0).all()          # (the odd last object is blended)
    sc["gains"], sc["prev_gains"] = np.ldexp(sc["gains"], gain_pow).astype(np.float32), np.ldexp(sc["prev_gains"], gain_pow).astype(np.float32)
    rows = ("idx", "idx1", "weights", "gains")
    calls, k0 = [], 0
    for nb in CALLS:
        k1 = k0 + (nb + SEG - 1) // SEG
        c = {k: np.ascontiguousarray(sc[k][:, k0:k1]) for k in rows}
        for k in rows:
            c["prev_" + k] = sc["prev_" + k] if k0 == 0 else np.ascontiguousarray(sc[k][:, k0 - 1])
        calls.append(c)
        k0 = k1
    return calls


def modes_dirs():
    return make_layout(N_DIRS, 512)


def modes_noise(seed=23000):
    return make_input(S, K, TOTAL, seed=seed)


def model_calls(kernel, x, gain_pow=0, gain=1.0):
    """the f64 model of the two calls, the tail carried -> [S][2][TOTAL * 512] f64 (tests/test_cpu_flush_modes.py)"""
    out, tail, pos = [], None, 0
    for nb, c in zip(CALLS, modes_scene(gain_pow)):
        xc = x[:, :, pos * BLOCK:(pos + nb) * BLOCK]
        if kernel == "plain":
            y, tail = sm.model_scene_f64(xc, modes_dirs(), c["idx"], SEG, c["gains"], c["prev_idx"], c["prev_gains"], True, gain, tail, True)
        else:
            y, tail = bm.model_blend_f64(xc, modes_dirs(), c["idx"], c["idx1"], c["weights"], SEG, c["gains"], c["prev_idx"], c["prev_idx1"],
                                         c["prev_weights"], c["prev_gains"], True, gain, tail, True)
        out.append(y)
        pos += nb
    return np.concatenate(out, axis=2)


def _handle(kernel, mode=0, streams=S):
    h = (_plain if kernel == "plain" else _blend)(modes_dirs(), streams)
    h.set_gain(1.0)
    h.set_flush_denormals(mode)
    return h


def _call(kernel, h, x, c, seg=SEG, **over):
    c = dict(c, **over)
    if kernel == "plain":
        return _run_plain(h, x, c["idx"], seg, c["gains"], c["prev_idx"], c["prev_gains"])
    return _run(h, x, seg, c)


def _both_calls(kernel, h, x, scene=None):
    """the calls of 6 and 5 blocks -> (their outputs, the launch records)"""
    out, rec, pos = [], [], 0
    for nb, c in zip(CALLS, scene or modes_scene()):
        out.append(_call(kernel, h, x[:, :, pos * BLOCK:(pos + nb) * BLOCK], c))
        rec.append(h.last_launch())
        assert rec[-1][2] > 0 and (kernel == "plain" or rec[-1][3] > 0), rec[-1]
        pos += nb
    return out, rec


# ---- flush A: the normal range ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("kernel", KERNELS)
def test_flush_a_the_mode_changes_no_bit_of_a_loud_signal(kernel, mode):
    x = modes_noise()
    want, rec0 = _both_calls(kernel, _handle(kernel, 0), x)
    got, rec = _both_calls(kernel, _handle(kernel, mode), x)
    assert rec == rec0
    first = 0
    for i, (y, t) in enumerate(zip(got, want)):
        assert float(np.abs(t).max()) > 0.01
        fm.check_same_bits(y, t, f"{kernel} kernel, mode {mode}, call {i}", first)
        first += CALLS[i]


# ---- flush B: below the range ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,mode", [("silent", 1), ("silent", 2), ("subnormal", 2)])
@pytest.mark.parametrize("kernel", KERNELS)
def test_flush_b_silence_out_and_silence_kept(kernel, which, mode):
    x = {"silent": fm.silent_input, "subnormal": fm.subnormal_input}[which](modes_noise())
    twin, rec0 = _both_calls(kernel, _handle(kernel, 0), x)
    h = _handle(kernel, mode)
    got, rec = _both_calls(kernel, h, x)
    assert rec == rec0
    first = 0
    for i, (y, t) in enumerate(zip(got, twin)):
        fm.check_silent(y, f"{kernel} kernel, {which} input, mode {mode}, call {i}", first, twin=t)
        first += CALLS[i]
    # the state silence left behind is silence: loud noise through this handle and through a fresh one in the same mode
    loud = modes_noise(23100)
    c = modes_scene()[0]
    after, fresh = _call(kernel, h, loud[:, :, :CALLS[0] * BLOCK], c), _call(kernel, _handle(kernel, mode), loud[:, :, :CALLS[0] * BLOCK], c)
    assert np.isfinite(fresh).all() and float(np.abs(fresh).max()) > 0.01
    ne = np.argwhere(~(after == fresh))
    assert ne.size == 0, f"{kernel} kernel, {which} input, mode {mode}: {len(ne)} samples behind the silent calls differ from a fresh handle's, " \
                         f"first (stream, ear, frame) {ne[0].tolist()}"


# ---- flush C: through the range --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("kernel", KERNELS)
def test_flush_c_no_subnormal_sample_leaves(kernel, mode):
    """tests/test_cpu_flush_modes.py shows on the f64 model that this input and scene leave every stream at least NEED subnormals"""
    x = fm.falling_input(modes_noise(), CROSSING)
    twin, rec0 = _both_calls(kernel, _handle(kernel, 0), x, modes_scene(C_GAIN_POW))
    got, rec = _both_calls(kernel, _handle(kernel, mode), x, modes_scene(C_GAIN_POW))
    assert rec == rec0
    normal = (np.abs(np.concatenate(got, axis=2)) >= fm.TINY).sum(axis=(1, 2))
    assert (normal >= fm.NEED).all(), f"{kernel} kernel, mode {mode}: samples per stream in the normal range: {normal}"
    counts = fm.check_no_subnormal(np.concatenate(got, axis=2), f"{kernel} kernel, mode {mode}", twin=np.concatenate(twin, axis=2), need=fm.NEED)
    print(f"{kernel} kernel, mode {mode}: subnormal samples per stream of the mode-0 twin: {counts}")
    first = 0
    for i, y in enumerate(got):
        fm.check_no_subnormal(y, f"{kernel} kernel, mode {mode}, call {i}", first)
        first += CALLS[i]


# ---- exact scaling -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_scaling_a_stream_by_a_power_of_two_scales_its_output_bit_for_bit(kernel):
    x = modes_noise()
    ks = np.array([0, 40, -40], np.int32)
    twin, _ = _both_calls(kernel, _handle(kernel), x)
    got, _ = _both_calls(kernel, _handle(kernel), sv.scaled(x, ks))
    for i, (y, t) in enumerate(zip(got, twin)):
        _same_bits(sv.unscaled(y, ks), t, f"{kernel} kernel, streams times 2^{ks.tolist()}, call {i}, unscaled")
        sv.check_scaling(y, t, ks, f"{kernel} kernel, call {i}")
        _same_bits(y[:1], t[:1], f"{kernel} kernel, call {i}: the stream that was not scaled")


@pytest.mark.parametrize("kernel", KERNELS)
def test_moving_a_power_of_two_from_an_objects_input_to_its_gain_keeps_every_bit(kernel):
    """(x 2^-k) (gain 2^k) is x gain exactly, object by object"""
    x = modes_noise()
    k = np.array([3, -5, 7], np.int32)
    xs = np.ldexp(x, -k[None, :, None]).astype(np.float32)
    scene = []
    for c in modes_scene():
        c = dict(c)
        for name in ("gains", "prev_gains"):
            c[name] = np.ldexp(c[name], k).astype(np.float32)
        scene.append(c)
    twin, rec0 = _both_calls(kernel, _handle(kernel), x)
    got, rec = _both_calls(kernel, _handle(kernel), xs, scene)
    assert rec == rec0
    for i, (y, t) in enumerate(zip(got, twin)):
        _same_bits(y, t, f"{kernel} kernel, objects' gains times 2^{k.tolist()} and inputs times 2^{(-k).tolist()}, call {i}")


# ---- containment -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [np.inf, -np.inf])
@pytest.mark.parametrize("kernel", KERNELS)
def test_an_infinity_in_one_object_stays_in_its_stream(kernel, value):
    x = modes_noise()
    c = modes_scene()[0]
    nb, at = CALLS[0], 2 * BLOCK + 31
    clean = _call(kernel, _handle(kernel), x[:, :, :nb * BLOCK], c)
    y = _call(kernel, _handle(kernel), sv.poison(x[:, :, :nb * BLOCK], 1, 2, at, value), c)       # (the odd last object of stream 1)
    assert not np.isfinite(y[1]).all()
    _same_bits(y[[0, 2]], clean[[0, 2]], f"{kernel} kernel, {value}: the streams beside the poisoned one")
    # (a block is one transform: in front of the sample means in front of its block, as for the reference's partitions)
    _same_bits(y[1:2, :, :2 * BLOCK], clean[1:2, :, :2 * BLOCK], f"{kernel} kernel, {value}: the poisoned stream in front of the sample's block")


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_nan_in_a_ranges_dry_block_stays_in_the_references_window(kernel):
    """one stream of 24 blocks runs as many ranges; every range but the first computes the block in front of it dry, for its tail.  A
    NaN in such a block -- the last block of one range, the dry block of the next -- makes that block and the one behind it NaN: one
    partition, the reference's window (special_values.reference_window).  Every other block keeps the clean run's bits."""
    blocks = 24
    sc = bm.make_blend_scene(1, K, blocks, SEG, N_DIRS, seed=56)
    x = make_input(1, K, blocks, seed=23200)
    h = _handle(kernel, 0, 1)
    clean = _call(kernel, h, x, sc)
    ranges = h.last_launch()[1]
    assert ranges > 1 and ranges <= blocks, h.last_launch()
    ck = ranges // 2
    t = ck * blocks // ranges - 1               # the last block in front of range ck's first
    assert 0 < t < blocks - 2 and (ck - 1) * blocks // ranges <= t
    h2 = _handle(kernel, 0, 1)
    y = _call(kernel, h2, sv.poison(x, 0, 0, t * BLOCK + 100, np.nan), sc)
    assert h2.last_launch() == h.last_launch()
    window = sv.reference_window(t, 1)
    assert window == (t, t + 1) and sv.nonfinite_blocks(y[0]) == [t, t + 1], (sv.nonfinite_blocks(y[0]), t)
    assert np.isnan(y[0, :, t * BLOCK + 100:(t + 2) * BLOCK]).all()
    sv.check_containment(y, clean, 0, window, t * BLOCK + 100, sv.window_mask(blocks * BLOCK, window, t * BLOCK + 100),
                         f"{kernel} kernel, NaN in block {t}, the dry block of range {ck} of {ranges}")

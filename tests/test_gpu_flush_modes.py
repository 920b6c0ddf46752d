"""Every convolution kernel under the handle's flush-denormals mode (ohs_batch_set_flush_denormals, ohs_engine_set_flush_denormals):
the three promises of tests/flush_modes.py -- A: in the normal range the mode changes no bit, B: below the range silence comes out
and silence is what stays behind, C: through the range no subnormal sample ever leaves -- in modes 1 (FTZ, what the plugin runs
under) and 2 (FTZ | DAZ), for every convolution family and call kind of the batch handle and for the single-stream engine.

The families, call kinds, call lengths, expected plans and hooks are tests/test_gpu_special_values.py's own (family(), KINDS,
run_twins): the smallest shapes at which each family is still the one that serves, and a case that fell back to another kernel
fails.  The twin of every case is the same handle in mode 0 on the same input: it is the bit-level reference of A, and in B and C
it shows that the case is not vacuous (tests/test_cpu_flush_modes.py shows on the oracle that the conditions can be met, and that
each checker can fail).  The mode must not change the plan: run_twins holds both handles to the same last_conv_plan(),
last_eq_form() and last_layout_launch() after every call.

Every call prints `special-values <case>: call k (n blocks) -> ...`: run with -s to see what served it."""
import numpy as np
import pytest

from tests import batch_model as bm
from tests import flush_modes as fm
from tests.test_gpu_special_values import (BLOCK, FAMILIES, GAIN, K_LAYOUT, KIND_CALLS, KINDS, OUT_OF_PLACE_ONLY, PLACE_IDS, SEG, S, IrScheduled, Plain,
                                           _kinds_configure, _noise, _rows, _with_places, family, run_twins)

pytestmark = pytest.mark.gpu

MODES = (1, 2)
# B: (input, mode) -- `subnormal` in mode 2 only: in mode 1 the samples are read, and sums of them may reach the normal range
B_CASES = [("silent", 1), ("silent", 2), ("subnormal", 2)]
B_IDS = [f"{i}_mode{m}" for i, m in B_CASES]
B_INPUT = {"silent": fm.silent_input, "subnormal": fm.subnormal_input}


def _family(key, exp_tuning):
    """family() plus one case of this file: block 8192 with pending tails -- 8 192 taps, path 1 re-loaded with 6 000 taps in front of
    the second call, whose pending tails are added behind the block-8192 kernel"""
    if key != "xb_pending_tails":
        return family(key, exp_tuning)
    from open_headstage_amd import synth
    f = family("xb", exp_tuning)
    f.key = key
    f.events = {1: [(1, synth.hrir_set(6000)[1])]}

    def hook(k, bp):
        for p, h in f.events.get(k, ()):
            bp.set_ir(p, h)
    f.hook = hook
    return f


_CASES = _with_places(FAMILIES + ["xb_pending_tails"], OUT_OF_PLACE_ONLY + ("xb_pending_tails",))


def _in_mode(make, mode):
    def mk():
        bp = make()
        bp.set_flush_denormals(mode)
        return bp
    return mk


def _per_call(check):
    """run_twins' after_call: the checker on every call's output, the failure naming the block within the case"""
    return lambda k, pos, y, yt, what: check(y, yt, what, pos) if check is fm.check_same_bits else check(y, what, pos)


def _silence_is_kept(name, entry, dev, fresh, k, x, in_place):
    """B's last part: normal-amplitude noise into the handle that has been fed silence and into one created fresh in the same mode
    (in the configuration the case's hooks leave): equal as numbers, finite, loud"""
    y, yf = entry.run(dev, k, x, in_place), entry.run(fresh, k, x, in_place)
    print(f"flush-modes {name}: noise behind the silence -> conv {dev.last_conv_plan()}, EQ {dev.last_eq_form()}; a fresh handle -> conv "
          f"{fresh.last_conv_plan()}, EQ {fresh.last_eq_form()}")
    assert np.isfinite(yf).all() and float(np.abs(yf).max()) > 0.01, name
    ne = ~(y == yf)
    if ne.any():
        s, c, fr = (int(v) for v in np.argwhere(ne)[np.argmin(np.argwhere(ne)[:, 2])])
        raise AssertionError(f"{name}: behind the silence {int(ne.sum())} samples differ from a fresh handle's, first at stream {s}, channel {c}, frame {fr}, "
                             f"block {fr // BLOCK}: {y[s, c, fr]!r} against {yf[s, c, fr]!r}: the state that silence left is not silence")


# ---- the convolution families, EQ off -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=[f"mode{m}" for m in MODES])
@pytest.mark.parametrize("key,in_place", _CASES[0], ids=_CASES[1])
def test_a_normal_range_convolution(exp_tuning, key, in_place, mode):
    f = _family(key, exp_tuning)
    assert in_place in f.places
    x = _noise(1800, sum(f.calls) * BLOCK, n=f.S)
    name = f"flush A, {key}, {PLACE_IDS[in_place]}, mode {mode}"
    run_twins(name, _in_mode(f.make, mode), f.calls, f.expect, x, x, in_place, hook=f.hook, make_twin=f.make,
              after_call=_per_call(fm.check_same_bits))


@pytest.mark.parametrize("which,mode", B_CASES, ids=B_IDS)
@pytest.mark.parametrize("key,in_place", _CASES[0], ids=_CASES[1])
def test_b_below_the_range_convolution(exp_tuning, key, in_place, which, mode):
    """The twin's condition (non-zero in more than half its samples, asserted last) is what found the 1/N folded into the tables of the
    block-2048 and block-8192 plans: in IEEE arithmetic products of the `silent` input with them rounded to zero on the 2^-149 grid
    (non-zero samples of the twin's stream 0 then: lb 13 473 of 32 768, lb_unequal 3 130 of 32 768, xb and xb_p2 0 of 270 336; exact
    arithmetic rounded once gives 92 %, 81 % and 73 % for 1 300, 8 192 and 16 384 taps).  The 1/N goes with the gain now."""
    f = _family(key, exp_tuning)
    assert in_place in f.places
    n0 = f.calls[0]
    u = _noise(1810, (sum(f.calls) + n0) * BLOCK, n=f.S)
    x = B_INPUT[which](u[:, :, :sum(f.calls) * BLOCK])
    name = f"flush B, {key}, {PLACE_IDS[in_place]}, {which} input, mode {mode}"
    make = _in_mode(f.make, mode)
    y, yt, dev, _ = run_twins(name, make, f.calls, f.expect, x, x, in_place, hook=f.hook, make_twin=f.make, twin_quiet=True,
                              after_call=_per_call(fm.check_silent))
    fresh = make()
    for k in sorted(f.events):
        f.hook(k, fresh)
    _silence_is_kept(name, Plain(), dev, fresh, len(f.calls), u[:, :, sum(f.calls) * BLOCK:], in_place)
    fm.check_silent(y, name, twin=yt)       # (the twin's condition last: what the handle in the mode owes has been held by then)


@pytest.mark.parametrize("mode", MODES, ids=[f"mode{m}" for m in MODES])
@pytest.mark.parametrize("key,in_place", _CASES[0], ids=_CASES[1])
def test_c_through_the_range_convolution(exp_tuning, key, in_place, mode):
    f = _family(key, exp_tuning)
    assert in_place in f.places
    x = fm.falling_input(_noise(1820, sum(f.calls) * BLOCK, n=f.S), f.calls[0] + 1)
    name = f"flush C, {key}, {PLACE_IDS[in_place]}, mode {mode}"
    y, yt, _, _ = run_twins(name, _in_mode(f.make, mode), f.calls, f.expect, x, x, in_place, hook=f.hook, make_twin=f.make, twin_quiet=True,
                            after_call=_per_call(fm.check_no_subnormal))
    counts = fm.check_no_subnormal(y, name, twin=yt)
    print(f"flush-modes {name}: subnormal samples per stream of the mode-0 twin: min {min(counts)}, max {max(counts)}")


RELOADED = [c for c in zip(*_CASES) if c[0][0] in ("tp_gated", "lb_pending_tails", "xb_pending_tails")]
LATE = 5


@pytest.mark.parametrize("mode", MODES, ids=[f"mode{m}" for m in MODES])
@pytest.mark.parametrize("key,in_place", [c[0] for c in RELOADED], ids=[c[1] for c in RELOADED])
def test_c_output_crosses_the_range_at_the_reload(exp_tuning, key, in_place, mode):
    """C again for the families whose hook re-loads a path, with the crossing LATE = 5 blocks later.  The responses are L1-normalised
    per ear (synth.hrir_set): 1 300 to 8 192 decaying taps put the output 5 to 6 octaves below the input, so under the input of the
    case above the output -- and with it everything the frames in front of the re-load still owe the frames behind it -- has left
    the normal range several blocks BEFORE the re-load: the kernels that merge and add the pending tails see zeros there.  Five
    blocks later the outputs of streams 0 .. 4 (one octave apart) cross 2^-126 in the blocks around the re-load, and the tails'
    operands are small normals whose sum with the call's own output is subnormal wherever it is not flushed."""
    f = _family(key, exp_tuning)
    assert in_place in f.places and sum(f.calls) >= f.calls[0] + 1 + LATE + 4
    x = fm.falling_input(_noise(1825, sum(f.calls) * BLOCK, n=f.S), f.calls[0] + 1 + LATE)
    name = f"flush C, crossing {LATE} blocks later, {key}, {PLACE_IDS[in_place]}, mode {mode}"
    y, yt, _, _ = run_twins(name, _in_mode(f.make, mode), f.calls, f.expect, x, x, in_place, hook=f.hook, make_twin=f.make, twin_quiet=True,
                            after_call=_per_call(fm.check_no_subnormal))
    counts = fm.check_no_subnormal(y, name, twin=yt)
    blk = yt[:, :, f.calls[0] * BLOCK:(f.calls[0] + min(4, f.calls[1])) * BLOCK]          # (the tails of 8 192 taps last several blocks)
    mixed = [(int(fm.subnormal_mask(blk[s]).sum()), int((np.abs(blk[s]) >= fm.TINY).sum())) for s in range(f.S)]
    print(f"flush-modes {name}: subnormal samples per stream of the mode-0 twin: min {min(counts)}, max {max(counts)}; (subnormal, normal) samples "
          f"of the twin's first blocks behind the re-load, per stream: {mixed}")
    assert any(min(m) >= 100 for m in mixed), f"{name}: no stream of the twin crosses 2^-126 in the first blocks behind the re-load: {mixed}"


# ---- the call kinds, EQ and gain schedules on ---------------------------------------------------------------------------------------------
class IrScheduledCut(IrScheduled):
    """KINDS' ir_scheduled rings out; this is its other switch mode: the old response is cut off (the reference's set_ir)"""
    def call(self, bp, k, xt, out):
        return bp.process_ir_scheduled(xt, SEG, _rows(k, bm.n_segments(xt.shape[2] // BLOCK, SEG)), "cut", out=out)


ALL_KINDS = dict(KINDS, ir_scheduled_cut=IrScheduledCut)
_KIND_CASES = _with_places(list(ALL_KINDS), ("layout", "layout_scheduled"))


def _kind(kind, in_place):
    import open_headstage_amd as ohs
    entry = ALL_KINDS[kind]()
    assert in_place in entry.places
    lay = getattr(entry, "layout", False)
    make = lambda: _kinds_configure(ohs.BatchProcessor(S, num_bands=bm.NB))     # noqa: E731
    return entry, K_LAYOUT if lay else 2, make, [("none" if lay else "block512_p1", None)] * 2, None if lay else ["row_ring"] * 2


@pytest.mark.parametrize("mode", MODES, ids=[f"mode{m}" for m in MODES])
@pytest.mark.parametrize("kind,in_place", _KIND_CASES[0], ids=_KIND_CASES[1])
def test_a_normal_range_call_kinds(kind, in_place, mode):
    entry, ch, make, expect, want = _kind(kind, in_place)
    x = _noise(1830, sum(KIND_CALLS) * BLOCK, ch)
    name = f"flush A, {kind}, {PLACE_IDS[in_place]}, mode {mode}"
    run_twins(name, _in_mode(make, mode), KIND_CALLS, expect, x, x, in_place, entry=entry, eq_want=want, make_twin=make,
              after_call=_per_call(fm.check_same_bits))


@pytest.mark.parametrize("which,mode", B_CASES, ids=B_IDS)
@pytest.mark.parametrize("kind,in_place", _KIND_CASES[0], ids=_KIND_CASES[1])
def test_b_below_the_range_call_kinds(kind, in_place, which, mode):
    """As above (the layout kernels' tables had the 1/1024: the twin's stream 0 was non-zero in 767 and 0 of 11 264 samples)."""
    entry, ch, make, expect, want = _kind(kind, in_place)
    n = sum(KIND_CALLS) * BLOCK
    u = _noise(1840, n + KIND_CALLS[0] * BLOCK, ch)
    x = B_INPUT[which](u[:, :, :n])
    name = f"flush B, {kind}, {PLACE_IDS[in_place]}, {which} input, mode {mode}"
    y, yt, dev, _ = run_twins(name, _in_mode(make, mode), KIND_CALLS, expect, x, x, in_place, entry=entry, eq_want=want, make_twin=make,
                              twin_quiet=True, after_call=_per_call(fm.check_silent))
    _silence_is_kept(name, entry, dev, _in_mode(make, mode)(), len(KIND_CALLS), u[:, :, n:], in_place)
    fm.check_silent(y, name, twin=yt)


@pytest.mark.parametrize("mode", MODES, ids=[f"mode{m}" for m in MODES])
@pytest.mark.parametrize("kind,in_place", _KIND_CASES[0], ids=_KIND_CASES[1])
def test_c_through_the_range_call_kinds(kind, in_place, mode):
    entry, ch, make, expect, want = _kind(kind, in_place)
    x = fm.falling_input(_noise(1850, sum(KIND_CALLS) * BLOCK, ch), KIND_CALLS[0] + 1)
    name = f"flush C, {kind}, {PLACE_IDS[in_place]}, mode {mode}"
    y, yt, _, _ = run_twins(name, _in_mode(make, mode), KIND_CALLS, expect, x, x, in_place, entry=entry, eq_want=want, make_twin=make,
                            twin_quiet=True, after_call=_per_call(fm.check_no_subnormal))
    counts = fm.check_no_subnormal(y, name, twin=yt)
    print(f"flush-modes {name}: subnormal samples per stream of the mode-0 twin: min {min(counts)}, max {max(counts)}")


# ---- the single-stream engine ---------------------------------------------------------------------------------------------------------------
ENGINE_BLOCKS = 24
HOST_BLOCKS = {"host_1024": (1024,) * 12,
               "ragged": (1024, 300, 512, 2048, 77, 1000, 1536, 35, 1024, 700, 512, 1496, 1024, 1000)}      # 24 blocks of 512 in all
assert all(sum(v) == ENGINE_BLOCKS * BLOCK for v in HOST_BLOCKS.values())
ENGINE_CROSSING = 5     # C: the input crosses 2^-124 in block 5 and reaches zero before the end
_ENGINE_CASES = [(t, h, r) for t in (512, 1300) for h in HOST_BLOCKS for r in (False, True)]
_ENGINE_IDS = [f"taps{t}-{h}-{'resident' if r else 'launch_per_call'}" for t, h, r in _ENGINE_CASES]


def _engine(taps, mode):
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    e = ohs.ConvolutionEngine.new()
    for p, h in enumerate(synth.hrir_set(taps)):
        e.set_ir(p, h)
    e.set_flush_denormals(mode)
    return e


def _engine_run(e, x1, sizes, resident):
    """x1 [2][frames] through e in host blocks of `sizes` -> [1][2][frames]; one resident kernel at a time: the mode is switched on
    for this run only"""
    assert sum(sizes) == x1.shape[1]
    e.set_realtime(resident)
    try:
        out, pos = [], 0
        for n in sizes:
            out.append(np.stack(e.process_block(x1[0, pos:pos + n].copy(), x1[1, pos:pos + n].copy())))
            pos += n
        return np.concatenate(out, axis=1)[None]
    finally:
        e.set_realtime(False)


def _engine_noise(first_id, blocks):
    from open_headstage_amd import synth
    return synth.white_noise([first_id], blocks * BLOCK)


@pytest.mark.parametrize("taps,host,resident", _ENGINE_CASES, ids=_ENGINE_IDS)
def test_engine_in_every_mode(taps, host, resident):
    """A, B and C for ohs_engine_*: responses of one and of three partitions (the latter: the sums computed ahead), host blocks of
    1 024 frames and a ragged list through the FIFO adapter, launch per call and the resident kernel.  The FIFO's fill is part of an
    engine's state, so behind the ragged list the fresh engine of B is brought to the same fill by the same calls on true zeros."""
    sizes = HOST_BLOCKS[host]
    u = _engine_noise(1860, ENGINE_BLOCKS + 4)
    ua, noise = u[:, :, :ENGINE_BLOCKS * BLOCK], u[0][:, ENGINE_BLOCKS * BLOCK:]
    inputs = {"A": ua, "silent": fm.silent_input(ua), "subnormal": fm.subnormal_input(ua), "C": fm.falling_input(ua, ENGINE_CROSSING)}
    twins = {k: _engine_run(_engine(taps, 0), v[0], sizes, resident) for k, v in inputs.items()}
    assert all(np.isfinite(t).all() for t in twins.values()) and float(np.abs(twins["A"]).max()) > 0.01
    for mode in MODES:
        name = f"flush engine, {taps} taps, {host}, {'resident' if resident else 'launch per call'}, mode {mode}"
        fm.check_same_bits(_engine_run(_engine(taps, mode), ua[0], sizes, resident), twins["A"], name + ", A")
        for which in ("silent", "subnormal") if mode == 2 else ("silent",):
            e = _engine(taps, mode)
            fm.check_silent(_engine_run(e, inputs[which][0], sizes, resident), f"{name}, B ({which} input)", twin=twins[which])
            fresh = _engine(taps, mode)
            if host == "ragged":
                _engine_run(fresh, np.zeros_like(ua[0]), sizes, resident)
            y, yf = _engine_run(e, noise, (1024, 1024), resident), _engine_run(fresh, noise, (1024, 1024), resident)
            assert np.isfinite(yf).all() and float(np.abs(yf).max()) > 0.01 and np.array_equal(y, yf), f"{name}, B ({which} input): the state that silence left is not silence"
        counts = fm.check_no_subnormal(_engine_run(_engine(taps, mode), inputs["C"][0], sizes, resident), name + ", C", twin=twins["C"])
        print(f"flush-modes {name}: subnormal samples of the mode-0 twin: {counts}")


@pytest.mark.parametrize("mode", MODES, ids=[f"mode{m}" for m in MODES])
def test_chain_process_in_every_mode(mode):
    """ohs_chain_process: the 10-band EQ in front of the engine and the output gain behind it, both handles in the mode"""
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    from open_headstage_amd.dsp import process_chain
    bands = synth.eq_table()
    sizes = HOST_BLOCKS["host_1024"]

    def run(m, x1):
        e, q = _engine(512, m), ohs.StereoParametricEQ.new(len(bands), synth.FS)
        for i, b in enumerate(bands):
            q.update_band_coeffs(i, synth.FS, b)
        q.set_flush_denormals(m)
        out, pos = [], 0
        for n in sizes:
            l, r = x1[0, pos:pos + n].copy(), x1[1, pos:pos + n].copy()
            process_chain(e, q, l, r, eq_enable=True, output_gain=GAIN)
            out.append(np.stack([l, r]))
            pos += n
        return np.concatenate(out, axis=1)[None]
    ua = _engine_noise(1870, ENGINE_BLOCKS)
    name = f"flush chain, mode {mode}"
    ta = run(0, ua[0])
    assert float(np.abs(ta).max()) > 0.01
    fm.check_same_bits(run(mode, ua[0]), ta, name + ", A")
    for which in ("silent", "subnormal") if mode == 2 else ("silent",):
        x = B_INPUT[which](ua)
        fm.check_silent(run(mode, x[0]), f"{name}, B ({which} input)", twin=run(0, x[0]))
    x = fm.falling_input(ua, ENGINE_CROSSING)
    fm.check_no_subnormal(run(mode, x[0]), name + ", C", twin=run(0, x[0]))


@pytest.mark.parametrize("mode", MODES, ids=[f"mode{m}" for m in MODES])
def test_engine_clone_inherits_the_mode(mode):
    """a clone made behind set_flush_denormals runs in the mode"""
    sizes = HOST_BLOCKS["host_1024"]
    ua = _engine_noise(1880, ENGINE_BLOCKS)
    xs = fm.silent_input(ua)
    twin = _engine_run(_engine(1300, 0), xs[0], sizes, False)
    fm.check_silent(_engine_run(_engine(1300, mode).clone(), xs[0], sizes, False), f"flush clone, mode {mode}, B", twin=twin)
    fm.check_same_bits(_engine_run(_engine(1300, mode).clone(), ua[0], sizes, False), _engine_run(_engine(1300, 0), ua[0], sizes, False),
                       f"flush clone, mode {mode}, A")


def test_set_flush_denormals_on_a_resident_engine_holds_from_the_next_call():
    """the resident kernel set its mode when it started: set_flush_denormals(1) in mid-stream must reach the very next call.  Host
    blocks of 1 024 frames leave nothing in the FIFOs, and what the mode-0 calls left in the ring and the overlaps is subnormal and
    stays so under every product and sum: every sample from that call on is a zero"""
    ua = _engine_noise(1890, ENGINE_BLOCKS)
    xs = fm.silent_input(ua)[0]
    e, twin = _engine(1300, 0), _engine(1300, 0)
    yt = _engine_run(twin, xs, HOST_BLOCKS["host_1024"], True)
    e.set_realtime(True)
    try:
        out = []
        for k in range(12):
            if k == 4:
                e.set_flush_denormals(1)
            out.append(np.stack(e.process_block(xs[0, k * 1024:(k + 1) * 1024].copy(), xs[1, k * 1024:(k + 1) * 1024].copy())))
    finally:
        e.set_realtime(False)
    y = np.concatenate(out, axis=1)[None]
    assert np.array_equal(y[:, :, :4096].view(np.uint32), yt[:, :, :4096].view(np.uint32)), "mode 0 in front of the switch"
    fm.check_silent(y[:, :, 4096:], "flush mode set on a resident engine", first_block=8, twin=yt[:, :, 4096:])

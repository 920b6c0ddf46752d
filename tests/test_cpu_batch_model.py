"""The host model of the batch handle's contract (tests/batch_model.py), the part that needs no GPU: the model is right, a check
at the bar can fail on it, and the generator reaches what tests/test_gpu_fuzz_call_kinds.py is there for.

* a single call of each kind on a fresh model IS the kind's existing model function (np.array_equal on f64), and calls of one kind in
  a row are one call on the concatenated input: tails, overlap and EQ state chain, `prev` names the set in front of the cut;
* the two f32 legs: plain calls with the EQ on against oracle.chain_process per stream, CUT against the oracle engine driven with
  set_ir, both at the project's bar;
* every rule of the contract, broken alone, moves the first block behind it by more than 1e-3 relative RMS in every stream -- three
  orders above the bar, the convention of test_modes_differ_by_far_more_than_the_bar_on_the_gpu_tests_inputs;
* over the default seeds the generator takes every ordered pair of call kinds, every setter between two different kinds, and every
  variant of the calls' arguments."""
import numpy as np
import pytest

from tests import batch_model as bm
from tests.batch_model import BLOCK, HandleModel, REFUSED
from tests.test_cpu_ir_crossfade import model_ir_crossfade
from tests.test_cpu_ir_schedule import CUT, RING_OUT, engine_cut_reference, model_ir_schedule, rel_rms_per_stream, render_f64
from tests.test_cpu_layout import BAR, make_input, make_layout, model_layout_f64
from tests.test_cpu_layout_schedule import make_table, model_layout_schedule_f64

S, GAIN = 3, float(np.float32(0.7))          # (the handle holds its gain in float32)


def _noise(seed, blocks, streams=S):
    from open_headstage_amd import synth
    return synth.white_noise(range(seed, seed + streams), blocks * BLOCK)


def _model(oracle, taps=512, eq=False, broken=None, K=3, streams=S):
    """a model as the generator sets a handle up: own responses, shared table 0, all three tables of choices, one layout"""
    m = HandleModel(oracle, streams, broken=broken)
    own = bm._sets(2, taps, 50)
    for p in range(4):
        m.set_ir(p, own[0, p])
    coeffs, en = bm.make_tables()
    for b in range(bm.NB):
        m.set_band_coeffs(b, coeffs[0, b], en[0, b])
    m.set_schedule_tables(coeffs, en)
    if taps <= BLOCK:
        m.set_schedule_irs(bm._sets(bm.N_CHOICES, taps, 11))
    m.set_layout_irs(make_layout(K, min(taps, BLOCK)))
    m.set_layout_table(make_table(bm.N_CHOICES, K, min(taps, BLOCK)))
    m.set_gain(GAIN)
    m.set_eq_enabled(eq)
    return m


def _oracle_eq(oracle, x, seg_blocks, rows, tables):
    """x through fresh oracle EQs, table rows[s][k] (of `tables`) refreshed in front of segment k -> float32"""
    from open_headstage_amd import synth
    e = np.empty_like(x)
    n = x.shape[2] // BLOCK
    for s in range(x.shape[0]):
        q = oracle.StereoParametricEQ(bm.NB, synth.FS)
        for k, b0 in enumerate(range(0, n, seg_blocks)):
            for b in range(bm.NB):
                q.set_band_coeffs(b, tables[0][rows[s][k], b], bool(tables[1][rows[s][k], b]))
            sl = slice(b0 * BLOCK, min(b0 + seg_blocks, n) * BLOCK)
            l, r = x[s, 0, sl].copy(), x[s, 1, sl].copy()
            q.process_block(l, r)
            e[s, 0, sl], e[s, 1, sl] = l, r
    return e


# ---- 1. reduction to the existing models ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", [512, 200])
def test_a_single_call_of_each_kind_is_the_existing_model(oracle, taps):
    x, xl = _noise(4000, 5), make_input(S, 3, 5, seed=4100)
    own, sets = list(bm._sets(2, taps, 50)[0]), bm._sets(bm.N_CHOICES, taps, 11)
    tables = bm.make_tables()
    idx = np.array([[0, 2, 1], [3, 3, 0], [1, 0, 2]])
    gains = np.array([0.4, 0.9, 0.55], np.float32)
    # plain, EQ off and on
    assert np.array_equal(_model(oracle, taps).process(x), GAIN * render_f64(oracle, x, lambda s, t: own)[0])
    e0 = _oracle_eq(oracle, x, 5, np.zeros((S, 1), int), tables)
    assert np.abs(e0 - x).max() > 0.01
    assert np.array_equal(_model(oracle, taps, eq=True).process(x), GAIN * render_f64(oracle, e0, lambda s, t: own)[0])
    # the EQ-scheduled kinds: the oracle EQ refreshed per segment, the render, the segments' gains
    e1 = _oracle_eq(oracle, x, 2, np.broadcast_to(idx[0], (S, 3)), tables)
    want = render_f64(oracle, e1, lambda s, t: own)[0]
    for k in range(3):
        want[:, :, k * 1024:(k + 1) * 1024] *= np.float64(gains[k])
    assert np.array_equal(_model(oracle, taps, eq=True).process_scheduled(x, 2, idx[0], gains), want)
    assert np.array_equal(_model(oracle, taps, eq=True).process_scheduled_streams(x, 2, idx[0], gains), want)
    e2 = _oracle_eq(oracle, x, 2, idx, tables)
    got = _model(oracle, taps, eq=True).process_scheduled_streams(x, 2, idx, None)
    assert np.array_equal(got, GAIN * render_f64(oracle, e2, lambda s, t: own)[0])
    assert (rel_rms_per_stream(got, want) > 1e-3).all()
    # the IR kinds
    for rows in (idx, idx[1]):
        for mode in (RING_OUT, CUT):
            assert np.array_equal(_model(oracle, taps).process_ir_scheduled(x, 2, rows, mode),
                                  GAIN * model_ir_schedule(oracle, x, sets, rows, 2, mode)[0])
        for prev in (None, np.array([1, 0, 3]) if rows.ndim == 2 else 1):
            assert np.array_equal(_model(oracle, taps).process_ir_crossfaded(x, 2, rows, prev),
                                  GAIN * model_ir_crossfade(oracle, x, sets, rows, 2, prev)[0])
    # the layout kinds: the dry signal, and the EQ behind it
    lay, table = make_layout(3, taps), make_table(bm.N_CHOICES, 3, taps)
    m = _model(oracle, taps, eq=True)
    dry = m.process_layout(xl)
    assert np.array_equal(dry, model_layout_f64(oracle, xl, lay, GAIN))
    d32 = dry.astype(np.float32)
    assert np.array_equal(m.layout_eq(d32), _oracle_eq(oracle, d32, 5, np.zeros((S, 1), int), tables))
    for rows in (idx, idx[1]):
        for fade, prev in ((True, None), (True, np.array([1, 0, 3]) if rows.ndim == 2 else 1), (False, None)):
            got = _model(oracle, taps).process_layout_scheduled(xl, rows, 2, prev, fade)
            # (the model keeps its overlap in front of the gain: the sum over the sets first, then the gain)
            assert np.array_equal(got, GAIN * model_layout_schedule_f64(oracle, xl, table, rows, 2, prev, fade, 1.0))
            assert np.allclose(got, model_layout_schedule_f64(oracle, xl, table, rows, 2, prev, fade, GAIN), rtol=0, atol=1e-15)


def test_calls_of_one_kind_in_a_row_are_one_call_on_the_concatenated_input(oracle):
    x, xl = _noise(4200, 7), make_input(S, 3, 7, seed=4300)
    a, b = slice(0, 3 * BLOCK), slice(3 * BLOCK, 7 * BLOCK)
    idx = np.array([[0, 2, 1, 3, 0, 1, 2], [3, 3, 0, 1, 1, 2, 0], [1, 0, 2, 2, 3, 0, 1]])
    gains = np.linspace(0.35, 0.95, 7).astype(np.float32)

    def both(call, xx):
        """-> (the cut sequence, the whole)"""
        m1, m2 = _model(oracle, eq=True), _model(oracle, eq=True)
        return np.concatenate([call(m1, xx[:, :, a], 0), call(m1, xx[:, :, b], 3)], axis=2), call(m2, xx, None)

    def seg(n0):        # seg_blocks 1: the rows cut where the call is
        return slice(None) if n0 is None else (slice(0, 3) if n0 == 0 else slice(3, 7))

    cases = {
        "process": lambda m, v, n0: m.process(v),
        "scheduled": lambda m, v, n0: m.process_scheduled(v, 1, idx[0, seg(n0)], gains[seg(n0)]),
        "scheduled_streams": lambda m, v, n0: m.process_scheduled_streams(v, 1, idx[:, seg(n0)], gains[seg(n0)]),
        "ir_scheduled": lambda m, v, n0: m.process_ir_scheduled(v, 1, idx[:, seg(n0)], RING_OUT),
        "ir_crossfaded": lambda m, v, n0: m.process_ir_crossfaded(v, 1, idx[:, seg(n0)], idx[:, 2] if n0 == 3 else None),
    }
    for kind, call in cases.items():
        cut, whole = both(call, x)
        assert np.allclose(cut, whole, rtol=0, atol=1e-14), kind
    # ... the adoption of a shared row carries the second call of a plain pair: scheduled, then plain, is one scheduled call
    m1, m2 = _model(oracle, eq=True), _model(oracle, eq=True)
    row = np.array([0, 2, 1, 1, 1, 1, 1])
    g = np.array([0.4, 0.9, 0.55, 0.55, 0.55, 0.55, 0.55], np.float32)
    cut = np.concatenate([m1.process_scheduled(x[:, :, a], 1, row[:3], g[:3]), m1.process(x[:, :, b])], axis=2)
    assert np.allclose(cut, m2.process_scheduled(x, 1, row, g), rtol=0, atol=1e-14)
    # the layout kinds, the EQ behind them
    for kind in bm.LAYOUT_KINDS:
        def call(m, v, n0):
            dry = m.process_layout(v) if kind == "layout" else m.process_layout_scheduled(v, idx[:, seg(n0)], 1, idx[:, 2] if n0 == 3 else None)
            return dry, m.layout_final(dry)
        m1, m2 = _model(oracle, eq=True), _model(oracle, eq=True)
        (d1, f1), (d2, f2), (dw, fw) = call(m1, xl[:, :, a], 0), call(m1, xl[:, :, b], 3), call(m2, xl, None)
        assert np.allclose(np.concatenate([d1, d2], axis=2), dw, rtol=0, atol=1e-14), kind
        assert (rel_rms_per_stream(np.concatenate([f1, f2], axis=2), fw) <= 1e-6).all(), kind     # (the f32 EQ of two roundings of one signal)


def test_long_responses_are_binaural_f64_over_everything_fed_since_the_reset(oracle):
    m = _model(oracle, taps=bm.LONG_TAPS)
    assert m.long and m.process_ir_scheduled(_noise(1, 1), 1, [0]) is REFUSED and m.process_ir_crossfaded(_noise(1, 1), 1, [0]) is REFUSED
    x = _noise(4400, 9)
    own = list(bm._sets(2, bm.LONG_TAPS, 50)[0])
    got = np.concatenate([m.process(x[:, :, :BLOCK]), m.process(x[:, :, BLOCK:4 * BLOCK]), m.process(x[:, :, 4 * BLOCK:])], axis=2)
    for s in range(S):
        l, r = oracle.binaural_f64(x[s, 0], x[s, 1], own)
        assert np.allclose(got[s], GAIN * np.stack([l, r]), rtol=0, atol=1e-13)
    m.reset()
    l, r = oracle.binaural_f64(x[0, 0, :BLOCK], x[0, 1, :BLOCK], own)
    assert np.allclose(m.process(x[:, :, :BLOCK])[0], GAIN * np.stack([l, r]), rtol=0, atol=1e-13)


# ---- 2. the two f32 legs --------------------------------------------------------------------------------------------------------
def test_plain_calls_with_the_eq_on_against_the_oracle_chain(oracle):
    from open_headstage_amd import synth
    m = _model(oracle, eq=True)
    x = _noise(4500, 11)
    got = np.concatenate([m.process(x[:, :, :4 * BLOCK]), m.process(x[:, :, 4 * BLOCK:])], axis=2)
    ref = np.empty_like(x)
    coeffs, en = bm.make_tables()
    for s in range(S):
        eng, eq = oracle.ConvolutionEngine(), oracle.StereoParametricEQ(bm.NB, synth.FS)
        for p in range(4):
            eng.set_ir(p, bm._sets(2, 512, 50)[0, p])
        for b in range(bm.NB):
            eq.set_band_coeffs(b, coeffs[0, b], bool(en[0, b]))
        l, r = x[s, 0].copy(), x[s, 1].copy()
        oracle.chain_process(eng, eq, l, r, eq_enable=True, gain=GAIN)
        ref[s, 0], ref[s, 1] = l, r
    err = rel_rms_per_stream(ref, got)
    print("oracle chain against the model, relative RMS per stream:", err)
    assert (err <= BAR).all(), err


def test_cut_against_the_oracle_engine_driven_with_set_ir(oracle):
    m = _model(oracle)
    m.set_gain(1.0)
    x = _noise(4600, 9)
    idx = np.array([[0, 2, 2, 3, 0], [3, 3, 0, 1, 1], [1, 0, 2, 2, 3]])
    got = m.process_ir_scheduled(x, 2, idx, CUT)
    err = rel_rms_per_stream(engine_cut_reference(oracle, x, bm._sets(bm.N_CHOICES, 512, 11), idx, 2), got)
    assert (err <= BAR).all(), err


# ---- 3. the checker can fail ----------------------------------------------------------------------------------------------------
def _call(kind, blocks, x_seed, **kw):
    op = {"op": "call", "kind": kind, "blocks": blocks, "x_seed": x_seed, "refused": False, "io": None, "seg": 1}
    op.update(kw)
    return op


def _scenarios(spec):
    """rule -> [ops behind the generator's own setup; the LAST call's first block is the one behind the rule]"""
    Sn, K = spec["S"], 3
    rows = np.stack([(np.arange(2) + s) % bm.N_CHOICES for s in range(Sn)])
    lay = [{"op": "set_layout_irs", "K": K, "seed": 7 * spec["seed"]}, {"op": "set_layout_table", "K": K, "seed": 7 * spec["seed"]}]
    eq_on, x0 = {"op": "set_eq_enabled", "on": True}, 900000 + 1000 * spec["seed"]
    return {
        "eq_not_shared": [lay + [eq_on, _call("process", 3, x0), _call("layout", 2, x0 + 100, K=K)]],
        "layout_overlap_shared": [lay + [_call("process", 2, x0), _call("layout", 2, x0 + 100, K=K)],
                                  lay + [_call("layout", 2, x0 + 100, K=K), _call("process", 2, x0)]],
        "no_adoption": [[_call("ir_scheduled", 2, x0, idx=np.array([0, 1]), mode=RING_OUT), _call("process", 1, x0 + 100)],
                        [_call("ir_crossfaded", 2, x0, idx=np.array([0, 1]), prev=None), _call("process", 1, x0 + 100)],
                        [eq_on, _call("scheduled", 2, x0, table_idx=np.array([1, 2]), gains=None), _call("process", 1, x0 + 100)],
                        [_call("scheduled", 2, x0, table_idx=None, gains=np.array([0.9, 0.6], np.float32)), _call("process", 1, x0 + 100)]],
        "adopt_per_stream": [[_call("ir_scheduled", 2, x0, idx=rows, mode=RING_OUT), _call("process", 1, x0 + 100)],
                             [eq_on, _call("scheduled_streams", 2, x0, table_idx=rows, gains=None), _call("process", 1, x0 + 100)],
                             [_call("scheduled_streams", 2, x0, table_idx=None, gains=np.array([0.9, 0.6], np.float32)),
                              _call("process", 1, x0 + 100)]],
        "set_ir_drops_all": [[_call("process", 2, x0), {"op": "set_ir", "path": 1, "seed": 50 + spec["seed"], "which": 1},
                              _call("process", 1, x0 + 100)]],
        "reset_keeps_layout": [lay + [_call("layout", 2, x0, K=K), {"op": "reset"}, _call("layout", 1, x0 + 100, K=K)]],
        "cut_start_no_boundary": [[_call("process", 2, x0), _call("ir_scheduled", 2, x0 + 100, idx=rows, mode=CUT)]],
        "prev_ignored": [[_call("ir_crossfaded", 2, x0, idx=rows, prev=(rows[:, 0] + 1) % bm.N_CHOICES)],
                         lay + [_call("layout_scheduled", 2, x0, K=K, idx=rows, prev=(rows[:, 0] + 1) % bm.N_CHOICES, crossfade=True)]],
        "layout_eq_in_front": [lay + [eq_on, _call("process", 3, x0), _call("layout", 2, x0 + 100, K=K)]],
    }


@pytest.mark.parametrize("rule", bm.RULES)
def test_a_broken_rule_moves_the_first_block_behind_it_by_far_more_than_the_bar(oracle, rule):
    worst = np.inf
    for seed in (0, 1, 2, 4):                   # (the generator's own streams, responses, tables and noise; one-partition seeds)
        spec = bm.sequence(seed)
        setup = spec["ops"][:next(i for i, op in enumerate(spec["ops"]) if op["op"] == "call")]
        for ops in _scenarios(spec)[rule]:
            out = []
            for broken in (None, rule):
                m = HandleModel(oracle, spec["S"], broken=broken)
                out.append(bm.run_model(m, spec, setup + [{"op": "set_gain", "gain": 1.0}] + ops))
            (op, good), (_, bad) = out[0][-1], out[1][-1]
            assert good is not REFUSED and float(np.sqrt(np.mean(good[:, :, :BLOCK] ** 2, axis=(1, 2))).min()) >= 0.01
            d = rel_rms_per_stream(bad[:, :, :BLOCK], good[:, :, :BLOCK])
            print(f"{rule}, seed {seed}, {[o.get('kind', o['op']) for o in ops]}: first block of the last call moves by "
                  f"{d.min():.3e} .. {d.max():.3e}")
            assert (d > 1e-3).all(), (rule, seed, op["kind"], d)
            for (_, g), (_, b) in zip(out[0][:-1], out[1][:-1]):        # (and nothing in front of the rule moves)
                assert np.array_equal(g, b), (rule, seed)
            worst = min(worst, float(d.min()))
    assert worst > 1e-3


# ---- 4. the generator's coverage ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def specs():
    return [bm.sequence(seed) for seed in range(bm.DEFAULT_SEEDS)]


def _calls(spec, refused=False):
    return [op for op in spec["ops"] if op["op"] == "call" and op["refused"] == refused]


def test_the_generator_is_deterministic_and_within_its_shapes(specs):
    for seed, spec in enumerate(specs):
        again = bm.sequence(seed)
        assert repr(again) == repr(spec)
        calls = _calls(spec)
        assert len(calls) in (13, 14) and 1 <= spec["S"] <= 20 and spec["taps"] in (512, 200)
        assert all(c["blocks"] in bm.BLOCK_CHOICES and c["seg"] in bm.SEG_CHOICES for c in calls)
        assert sum(c["blocks"] for c in calls) <= bm.MAX_BLOCKS, seed
        if spec["S"] > 6:           # the wide seed: short calls but the one that reaches the overlapped path
            assert sorted(c["blocks"] for c in calls)[-2] <= 5
        if spec["long"]:
            assert not any(c["kind"] in bm.IR_KINDS for c in calls)
    assert sum(spec["long"] for spec in specs) == 2 and sum(spec["S"] > 6 for spec in specs) == 1
    assert {spec["taps"] for spec in specs} == {512, 200}


def test_the_walk_takes_every_ordered_pair_of_call_kinds(specs):
    assert sorted(bm.euler_circuit(7)[:-1].count(k) for k in range(7)) == [7] * 7
    pairs = set()
    for spec in specs:
        kinds = [c["kind"] for c in _calls(spec)]
        assert kinds == bm.kind_walk(spec["seed"])
        pairs |= set(zip(kinds, kinds[1:]))
    missing = [(a, b) for a in bm.KINDS for b in bm.KINDS if (a, b) not in pairs]
    assert not missing, missing
    # the seeds whose handle holds long responses walk the pairs of the five kinds it serves
    long_pairs = set()
    for spec in specs:
        if spec["long"]:
            kinds = [c["kind"] for c in _calls(spec)]
            long_pairs |= set(zip(kinds, kinds[1:]))
    assert len(long_pairs) == len(bm.LONG_KINDS) ** 2


def test_every_setter_stands_between_two_calls_of_different_kinds(specs):
    seen = set()
    for spec in specs:
        last, between = None, []
        for op in spec["ops"]:
            if op["op"] != "call":
                between.append(op["op"])
            elif not op["refused"]:
                if last is not None and last != op["kind"]:
                    seen |= set(between)
                last, between = op["kind"], []
    assert seen >= set(bm.SETTERS), set(bm.SETTERS) - seen


def test_every_variant_of_the_calls_occurs(specs):
    seen = set()
    for spec in specs:
        eq_on, per_stream = False, False
        for op in spec["ops"]:
            if op["op"] == "set_eq_enabled":
                eq_on = op["on"]
            elif op["op"] == "set_stream_band_coeffs":
                per_stream = True
            elif op["op"] == "share_eq_table":
                per_stream = False
            if op["op"] != "call":
                continue
            k = op["kind"]
            if op["refused"]:
                assert (k == "scheduled" and per_stream) or (k in bm.IR_KINDS and spec["long"]), (spec["seed"], k)
                seen.add("refused: per-stream tables" if k == "scheduled" else "refused: long responses, " + k)
                continue
            assert not (k == "scheduled" and per_stream) and not (k == "scheduled_streams" and per_stream and op["table_idx"] is not None)
            seen.add(("eq on, " if eq_on else "eq off, ") + ("layout" if k in bm.LAYOUT_KINDS else "stereo"))
            if per_stream:
                seen.add("static per-stream tables, " + k)
            if k in ("scheduled", "scheduled_streams"):
                seen.add(k + (", gains only" if op["table_idx"] is None else ", tables only" if op["gains"] is None else ", both"))
                for name in ("table_idx", "gains"):
                    if k == "scheduled_streams" and op[name] is not None:
                        seen.add(f"{name}: " + ("shared row" if op[name].ndim == 1 else "rows per stream"))
            if k in ("ir_scheduled", "ir_crossfaded", "layout_scheduled"):
                seen.add(k + (", shared row" if op["idx"].ndim == 1 else ", rows per stream"))
                n_segs = bm.n_segments(op["blocks"], op["seg"])
                assert op["idx"].shape[-1] == n_segs and op["idx"].max() < bm.N_CHOICES
            if k == "ir_scheduled":
                seen.add("CUT" if op["mode"] == CUT else "RING_OUT")
            if k in ("ir_crossfaded", "layout_scheduled"):
                seen.add(k + (", prev NULL" if op["prev"] is None else ", prev given"))
            if k == "layout_scheduled":
                seen.add("layout table, crossfade " + ("on" if op["crossfade"] else "off"))
            if k in bm.STEREO_KINDS:
                io = op["io"]
                seen.add("tensors" if io["gaps"] is None else "guarded, tight gaps" if io["gaps"][0] == 1 else "guarded, wide gaps")
                seen.add("in place" if io["in_place"] else "out of place")
        # the overlapped EQ || convolution path with several time chunks, in every seed
        eq_on, found = False, False
        for op in spec["ops"]:
            if op["op"] == "set_eq_enabled":
                eq_on = op["on"]
            found = found or (op["op"] == "call" and not op["refused"] and op["kind"] in bm.STEREO_KINDS and op["blocks"] >= 64 and eq_on)
        assert found, spec["seed"]
    want = {"CUT", "RING_OUT", "refused: per-stream tables", "refused: long responses, ir_scheduled", "refused: long responses, ir_crossfaded",
            "eq on, stereo", "eq off, stereo", "eq on, layout", "eq off, layout", "layout table, crossfade on", "layout table, crossfade off",
            "tensors", "guarded, tight gaps", "guarded, wide gaps", "in place", "out of place",
            "table_idx: shared row", "table_idx: rows per stream", "gains: shared row", "gains: rows per stream"}
    want |= {f"{k}, {v}" for k in ("scheduled", "scheduled_streams") for v in ("gains only", "tables only", "both")}
    want |= {f"{k}, {v}" for k in ("ir_scheduled", "ir_crossfaded", "layout_scheduled") for v in ("shared row", "rows per stream")}
    want |= {f"{k}, {v}" for k in ("ir_crossfaded", "layout_scheduled") for v in ("prev NULL", "prev given")}
    assert seen >= want, sorted(want - seen)
    print(sorted(seen - want))

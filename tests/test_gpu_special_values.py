"""Exact scaling and non-finite containment for every convolution kernel family, EQ form and call kind of the batch handle.

Every case runs two handles of identical configuration through the same calls: the twin gets the clean, unscaled input.

(a) scaling: stream s of the other handle's input is multiplied by 2^ks[s], ks = (0, +40, -40, +80, -80) over the streams; after every
    call every stream, divided by its scale, equals the twin's bit for bit (tests/special_values.check_scaling) -- a leak between
    chains at ANY level, an added constant or an absolute threshold breaks it.  tests/test_cpu_special_values.py shows that the
    reference arithmetic itself has this property at these scales and shapes.  Once per family stream 1 (scale 2^40) is also held
    to the project's bar against f64 arithmetic, so that the twins are not two wrongs agreeing.
(b) flush: under set_flush_denormals(2) a stream whose every input sample is subnormal comes out as zeros and changes no other stream.
(c) containment, EQ off: one NaN / +Inf / -Inf sample in stream 1, block b.  Every other stream stays bit-identical to the twin; stream
    1 differs from it only inside allowed_window(b, Pmax, back, fwd) with the family's documented allowance (include/ohs_hip.h, beside
    ohs_batch_set_conv_plan; allowance() below), is non-finite wherever the reference (the oracle engine on the same input) is from the
    poisoned sample on, and is bit-identical again behind the window: the state has drained.
(d) containment, EQ on: the recurrence never recovers, so stream 1 is non-finite from the poisoned sample to the end; the blocks in front
    of the documented look-back (16 samples, 64 for the wave-ring forms, 0 for the conveyor) and every other stream are bit-identical.
(e) recovery: reset() and the first call's input again give the bits of a fresh handle -- behind the window, and once per family with
    the NaN in the last block of the last call, so that every piece of state still holds it when reset() comes; a per-path set_ir behind a poisoned call leaves
    the other streams alone; the single-stream engine, launch per call and resident, keeps the reference's window exactly.

After every call the library is asked what served it (last_conv_plan, last_eq_form, last_layout_launch); the case names the kernel,
and a case that fell back to another one fails.  Every call prints `special-values <case>: call k (n blocks) -> ...`: run with -s."""
import types

import numpy as np
import pytest

from tests import batch_model as bm
from tests import special_values as sv
from tests.special_values import UNEQUAL, irs_for, parts_of
from tests.test_gpu_conv_guard_bands import _handle, _ranges_ok, f64_reference
from tests.util import assert_parity

pytestmark = pytest.mark.gpu

BLOCK = sv.BLOCK
GAIN = 0.75             # (_handle's)
S = 5                   # ten EQ chains: two full waves of the row form and a ragged one
POISONED = 1

# The documented allowance per convolution family, in blocks of 512 frames (include/ohs_hip.h, beside ohs_batch_set_conv_plan): a
# family whose transform spans F blocks spreads a non-finite sample over the transforms that hold it.  (back, fwd) is added to the
# reference's [b, b + Pmax].
#   block 512 (one partition, time-parallel, sequential): F = 1, the reference's own blocking: nothing added.
#   hop 1536: F = 3.  The sample's hop is non-finite as a whole (2 blocks back when it sits in the hop's last block), and so is the
#     next hop when the sample lies in the 512 frames its window reads back: 2 blocks behind b + 1.
#   block 2048 / block 8192: F = 4 / 16.  With P = ceil(Pmax / F) partitions of F blocks, the sample's F-block and the P behind it:
#     F - 1 back, F P + F - 1 - Pmax forward (4 for 1300 taps, 3 for 2048, 15 for 8192; never more than 2 F - 2).
SPAN = {"block512_p1": 1, "block512_tp": 1, "sequential": 1, "hop1536_p1": 3, "block2048": 4, "block8192": 16}


def allowance(served, pmax):
    F = SPAN[served]
    if served in ("block2048", "block8192"):
        return F - 1, F * -(-pmax // F) + F - 1 - pmax
    return {1: (0, 0), 3: (2, 2)}[F]


for _f, _F in SPAN.items():             # the issue's caps, for every response length: no measurement
    assert all(allowance(_f, _p)[0] <= _F and allowance(_f, _p)[1] <= 2 * _F for _p in range(1, 200)), _f


def _noise(first_id, frames, channels=2, n=S):
    from open_headstage_amd import synth
    x = synth.white_noise(range(first_id, first_id + n * ((channels + 1) // 2)), frames)
    return np.ascontiguousarray(x.reshape(n, -1, frames)[:, :channels])


def _served(bp):
    return {"conv": bp.last_conv_plan(), "eq": bp.last_eq_form(), "layout": bp.last_layout_launch()}


# ---- the call kinds ------------------------------------------------------------------------------------------------------------------
class Plain:
    places = (False, True)

    def run(self, bp, k, x, in_place):
        """call k on x [S][C][frames] -> the output [S][2][frames] as numpy"""
        import torch
        xt = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        y = self.call(bp, k, xt, xt if in_place else None)
        torch.cuda.synchronize()
        return y.cpu().numpy()

    def call(self, bp, k, xt, out):
        return bp.process(xt, out=out)

    def model(self, m, k, x1):
        return m.process(x1)


SEG = 2


def _row(k, n_segs, n=bm.N_CHOICES):
    return np.asarray([(1 + k + 2 * j) % n for j in range(n_segs)], np.uint32)           # changes in every segment


def _rows(k, n_segs, n=bm.N_CHOICES):
    return np.stack([(_row(k, n_segs, n) + s) % n for s in range(S)]).astype(np.uint32)


def _gain_rows(k, n_segs):
    return (0.5 + 0.125 * ((np.arange(S)[:, None] + 3 * np.arange(n_segs)[None, :] + k) % 7)).astype(np.float32)


class Scheduled(Plain):
    def args(self, k, nb, one=None):
        n = bm.n_segments(nb, SEG)
        return SEG, _row(k, n), _gain_rows(k, n)[2]

    def call(self, bp, k, xt, out):
        return bp.process_scheduled(xt, *self.args(k, xt.shape[2] // BLOCK), out=out)

    def model(self, m, k, x1):
        return m.process_scheduled(x1, *self.args(k, x1.shape[2] // BLOCK))


class ScheduledStreams(Plain):
    def args(self, k, nb):
        n = bm.n_segments(nb, SEG)
        return SEG, _rows(k, n), _gain_rows(k, n)

    def call(self, bp, k, xt, out):
        return bp.process_scheduled_streams(xt, *self.args(k, xt.shape[2] // BLOCK), out=out)

    def model(self, m, k, x1):
        seg, t, g = self.args(k, x1.shape[2] // BLOCK)
        return m.process_scheduled_streams(x1, seg, t[POISONED:POISONED + 1], g[POISONED:POISONED + 1])


class IrScheduled(Plain):
    def call(self, bp, k, xt, out):
        return bp.process_ir_scheduled(xt, SEG, _rows(k, bm.n_segments(xt.shape[2] // BLOCK, SEG)), "ring_out", out=out)

    def model(self, m, k, x1):
        return m.process_ir_scheduled(x1, SEG, _rows(k, bm.n_segments(x1.shape[2] // BLOCK, SEG))[POISONED:POISONED + 1], "ring_out")

    def reports(self, bp):
        assert bp.last_conv_ir_scheduled() and not bp.last_conv_ir_crossfaded()


class IrCrossfaded(Plain):
    def __init__(self, calls):
        self.calls = calls

    def prev(self, k):
        return None if k == 0 else _rows(k - 1, bm.n_segments(self.calls[k - 1], SEG))[:, -1].copy()

    def call(self, bp, k, xt, out):
        return bp.process_ir_crossfaded(xt, SEG, _rows(k, bm.n_segments(xt.shape[2] // BLOCK, SEG)), self.prev(k), out=out)

    def model(self, m, k, x1):
        pv = self.prev(k)
        return m.process_ir_crossfaded(x1, SEG, _rows(k, bm.n_segments(x1.shape[2] // BLOCK, SEG))[POISONED:POISONED + 1],
                                       None if pv is None else pv[POISONED:POISONED + 1])

    def reports(self, bp):
        assert bp.last_conv_ir_crossfaded()


K_LAYOUT = 6            # 5.1


class Layout(Plain):
    places = (False,)
    layout = True

    def call(self, bp, k, xt, out):
        return bp.process_layout(xt)

    def model(self, m, k, x1):
        """the DRY signal (gain x layout, in front of the EQ); HandleModel.layout_eq is the rest"""
        return m.process_layout(x1)

    def reports(self, bp):
        assert bp.last_layout_launch()[0] == (K_LAYOUT + 1) // 2 and not bp.last_layout_scheduled(), bp.last_layout_launch()


class LayoutScheduled(IrCrossfaded):
    places = (False,)
    layout = True

    def call(self, bp, k, xt, out):
        return bp.process_layout_scheduled(xt, _rows(k, bm.n_segments(xt.shape[2] // BLOCK, SEG)), SEG, self.prev(k), True)

    def model(self, m, k, x1):
        pv = self.prev(k)
        return m.process_layout_scheduled(x1, _rows(k, bm.n_segments(x1.shape[2] // BLOCK, SEG))[POISONED:POISONED + 1], SEG,
                                          None if pv is None else pv[POISONED:POISONED + 1], True)

    def reports(self, bp):
        assert bp.last_layout_launch()[0] == (K_LAYOUT + 1) // 2 and bp.last_layout_scheduled(), bp.last_layout_launch()


# ---- two handles through the same calls ----------------------------------------------------------------------------------------------
def run_twins(name, make, calls, expect, x_dev, x_twin, in_place, entry=None, hook=None, after_call=None, eq_want=None, make_twin=None,
              twin_quiet=False):
    """make() -> a configured handle (called twice); calls: lengths in blocks; expect: per call (family, ranges) as in
    tests/test_gpu_conv_guard_bands.py; hook(k, bp): applied to both handles in front of call k >= 1; after_call(k, first block, y, twin's
    y); eq_want: per call the EQ form's name (None: the EQ is off); make_twin: the twin's own make() (tests/test_gpu_flush_modes.py: the
    same handle in another denormal mode); twin_quiet: the case feeds the twin a signal below the normal range and says itself what
    its output must hold -- only then is the twin's output not held to be loud -> (y [S][2][frames], the twin's, the two handles)"""
    entry = entry or Plain()
    assert len(calls) >= 2 and len(set(calls[:2])) == 2 and len(expect) == len(calls)
    dev, twin = make(), (make_twin or make)()
    ys, yts, pos = [], [], 0
    for k, nb in enumerate(calls):
        if hook is not None and k:
            hook(k, dev)
            hook(k, twin)
        sl = slice(pos * BLOCK, (pos + nb) * BLOCK)
        y, yt = entry.run(dev, k, x_dev[:, :, sl], in_place), entry.run(twin, k, x_twin[:, :, sl], in_place)
        sd, st = _served(dev), _served(twin)
        what = f"{name}: call {k} ({nb} blocks)"
        print(f"special-values {what} -> conv {sd['conv']}, EQ {sd['eq']}, layout {sd['layout']}")
        assert sd == st, f"{what}: served by {sd}, the twin by {st}"
        assert sd["conv"][0] == expect[k][0] and _ranges_ok(sd["conv"][1], expect[k][1]), f"{what}: served by {sd['conv']}, the case names {expect[k]}"
        if eq_want is not None:
            assert sd["eq"][0] == eq_want[k], f"{what}: the EQ was served by {sd['eq']}, the case names {eq_want[k]}"
        for bp in (dev, twin):
            getattr(entry, "reports", lambda b: None)(bp)
        assert np.isfinite(yt).all() and (twin_quiet or float(np.abs(yt).max()) > 0.01), what
        if after_call is not None:
            after_call(k, pos, y, yt, what)
        ys.append(y)
        yts.append(yt)
        pos += nb
    return np.concatenate(ys, axis=2), np.concatenate(yts, axis=2), dev, twin


# ---- the convolution families: tests/test_gpu_conv_guard_bands.py's keys, tap counts and call lengths, at S = 5 ------------------------
def family(key, exp_tuning):
    """-> make, irs (at the start), calls + expect (the scaling case), more + more_expect (further calls of the containment case), places,
    hook, events {call: [(path, response)]} (what the hook does, for the references), pmax (behind the hook)"""
    from open_headstage_amd import synth
    f = types.SimpleNamespace(key=key, S=S, hook=None, events={}, more=(), more_expect=(), places=(False, True), f64_windows=None)
    if key in ("p1_own_tails", "p1_pre_pass"):
        per_stream, taps, f.calls, ranges = {"p1_own_tails": (4, 512, (3, 17), (3, 4)), "p1_pre_pass": (3, 200, (19, 5), (3, 3))}[key]
        exp_tuning("p1_target_waves", per_stream * S)
        f.irs = synth.hrir_set(taps)
        f.make = lambda: _handle(S, f.irs, 1, lib=exp_tuning.lib)
        f.expect = [("block512_p1", r) for r in ranges]
        f.more, f.more_expect = (6,), [("block512_p1", None)]
    elif key == "hop1536":
        f.irs = synth.hrir_set(512)
        f.make = lambda: _handle(S, f.irs, 2)
        f.calls, f.expect = (5, 7), [("hop1536_p1", 2), ("hop1536_p1", 3)]
        f.more, f.more_expect = (8,), [("hop1536_p1", 3)]
    elif key in ("tp", "tp_unequal"):
        f.irs = synth.hrir_set(1300) if key == "tp" else irs_for(UNEQUAL)
        f.make = lambda: _handle(S, f.irs, 1)
        f.calls, f.expect = (7, 2), [("block512_tp", None)] * 2
        f.more, f.more_expect = (9,), [("block512_tp", None)]
    elif key == "tp_gated":
        # the product route of the guard-band cases: one-partition responses, then two paths re-loaded behind the first call
        hb = synth.hrir_set(2000)
        f.irs = [hb[0][:512], hb[1][:300], hb[2][:512], hb[3][:200]]
        f.events = {1: [(0, synth.hrir_set(400)[0]), (2, synth.hrir_set(1300)[2])]}
        f.make = lambda: _handle(S, f.irs, 1)
        f.calls, f.expect = (5, 3, 11), [("block512_p1", None), ("block512_tp", None), ("block512_tp", None)]
    elif key in ("lb", "lb_unequal"):
        f.irs = synth.hrir_set(1300) if key == "lb" else irs_for(UNEQUAL)
        f.make = lambda: _handle(S, f.irs, 0)
        f.calls, f.expect = (7, 16, 9), [("block2048", None)] * 3
        f.more, f.more_expect = (12,), [("block2048", None)]
    elif key == "lb_pending_tails":
        f.irs = synth.hrir_set(1300)
        f.events = {1: [(1, synth.hrir_set(900)[1])]}
        f.make = lambda: _handle(S, f.irs, 0)
        f.calls, f.expect = (7, 3, 18), [("block2048", None)] * 3
        f.more, f.more_expect = (8,), [("block2048", None)]
    elif key == "xb":
        f.irs = synth.hrir_set(8192)
        f.make = lambda: _handle(S, f.irs, 0)
        f.calls, f.expect, f.places = (129, 135), [("block8192", None)] * 2, (False,)
        f.more, f.more_expect = (3,), [("block2048", None)]
    elif key == "xb_p2":
        # two partitions of 8192 taps: the second one's product waits in registers for the next 8192-frame block; the library takes
        # this kernel for them from 32 streams on.  f64 direct convolution of 264 blocks with 16 384 taps takes ten seconds: stream 1
        # is held to it over the blocks around the cut between the calls and around an 8192-frame boundary of the second call.
        f.S = 34
        f.irs = synth.hrir_set(16384)
        f.make = lambda: _handle(f.S, f.irs, 0)
        f.calls, f.expect, f.places = (129, 135), [("block8192", None)] * 2, (False,)
        f.more, f.more_expect = (3,), [("block2048", None)]
        f.f64_windows = ((125, 133), (190, 198))
    else:
        raise KeyError(key)
    if f.events:
        def hook(k, bp):
            for p, h in f.events.get(k, ()):
                bp.set_ir(p, h)
        f.hook = hook
    mid = f.calls[0] + f.calls[1] // 2
    # the poisoned blocks, both in the second call: its middle and the block in front (for the large transforms: the positions in
    # the transform's span with the longest reach forward and back)
    f.bs = {"lb": (16, 15), "lb_unequal": (16, 15), "xb": (f.calls[0] + 64, f.calls[0] + 79),
            "xb_p2": (f.calls[0] + 64, f.calls[0] + 79)}.get(key, (mid, mid - 1))
    assert all(f.calls[0] <= b < f.calls[0] + f.calls[1] for b in f.bs), f.bs
    last = list(f.irs)
    for k in sorted(f.events):
        for p, h in f.events[k]:
            last[p] = h
    f.irs_last = last
    f.pmax = max(parts_of(len(h)) for h in last)
    return f


FAMILIES = ["p1_own_tails", "p1_pre_pass", "hop1536", "tp", "tp_gated", "lb", "lb_pending_tails", "xb", "xb_p2", "tp_unequal", "lb_unequal"]
PLACE_IDS = {False: "out_of_place", True: "in_place"}
OUT_OF_PLACE_ONLY = ("xb", "xb_p2")         # block 8192 serves out-of-place calls only


def _with_places(keys, only_out):
    cases = [(k, p) for k in keys for p in ((False,) if k in only_out else (False, True))]
    return cases, [f"{k}-{PLACE_IDS[p]}" for k, p in cases]


def _timeline(f, calls):
    """f64_reference's timeline: per path [(first frame, response)]"""
    tl = [[(0, f.irs[p])] for p in range(4)]
    for k in sorted(f.events):
        for p, h in f.events[k]:
            tl[p].append((sum(calls[:k]) * BLOCK, h))
    return tl


def _oracle_nonfinite(oracle, x1, f, calls):
    """what the reference engine makes non-finite for stream x1 [2][frames], the hook's set_ir calls applied where the calls begin"""
    eng = oracle.ConvolutionEngine()
    for p in range(4):
        eng.set_ir(p, f.irs[p])
    starts = {sum(calls[:k]): k for k in range(len(calls))}
    out = np.empty_like(x1)
    for t in range(x1.shape[1] // BLOCK):
        for p, h in f.events.get(starts.get(t, -1), ()):
            eng.set_ir(p, h)
        out[0, t * BLOCK:(t + 1) * BLOCK], out[1, t * BLOCK:(t + 1) * BLOCK] = eng.process_block(x1[0, t * BLOCK:(t + 1) * BLOCK],
                                                                                               x1[1, t * BLOCK:(t + 1) * BLOCK])
    return ~np.isfinite(out)


# ---- (a) scaling, denormal mode 0 ---------------------------------------------------------------------------------------------------
_FAMILY_CASES = _with_places(FAMILIES, OUT_OF_PLACE_ONLY)


@pytest.mark.parametrize("key,in_place", _FAMILY_CASES[0], ids=_FAMILY_CASES[1])
def test_scaling_convolution(exp_tuning, oracle, key, in_place):
    f = family(key, exp_tuning)
    assert in_place in f.places
    ks = sv.scales_for(f.S)
    x = _noise(1000, sum(f.calls) * BLOCK, n=f.S)
    name = f"scaling, {key}, {PLACE_IDS[in_place]}"
    y, yt, _, _ = run_twins(name, f.make, f.calls, f.expect, sv.scaled(x, ks), x, in_place, hook=f.hook,
                            after_call=lambda k, pos, y, yt, what: sv.check_scaling(y, yt, ks, what))
    if not in_place and f.f64_windows:
        u = sv.unscaled(y, ks)[POISONED]
        reach = max(len(h) for h in f.irs) - 1
        for b0, b1 in f.f64_windows:        # the input from `reach` frames in front of the window on: its last frames are the window's
            lo, hi = b0 * BLOCK, b1 * BLOCK
            yl, yr = oracle.binaural_f64(x[POISONED, 0, lo - reach:hi], x[POISONED, 1, lo - reach:hi], f.irs)
            a, r = assert_parity(u[:, lo:hi], GAIN * np.stack([yl, yr])[:, reach:], f"{name}, blocks [{b0}, {b1})")
            print(f"special-values {name}: stream {POISONED} (scale 2^{ks[POISONED]}) against f64 direct convolution over blocks [{b0}, {b1}): "
                  f"abs RMS {a:.3e}, rel RMS {r:.3e}")
    elif not in_place:      # once per family: stream 1, unscaled, against f64 direct convolution
        a, r = assert_parity(sv.unscaled(y, ks)[POISONED], f64_reference(oracle, x[POISONED], _timeline(f, f.calls)), name)
        print(f"special-values {name}: stream {POISONED} (scale 2^{ks[POISONED]}) against f64 direct convolution: abs RMS {a:.3e}, rel RMS {r:.3e}")


EQ_FORMS = {"pair_ring": (2, (3, 17), ("wave_ring", "wave_ring"), 64), "quad_ring": (3, (3, 17), ("wave_ring", "wave_ring"), 64),
            "wave_ring": (0, (17, 20), ("wave_ring", "wave_ring"), 64),      # the library's own choice from 8 192 samples on
            "row_form": (1, (3, 17), ("row_ring", "row_ring"), 16), "conveyor": (0, (3, 17), ("conveyor", "conveyor"), 0),
            "per_stream_tables": (0, (3, 17), ("row_ring", "wave_ring"), 64)}


def _eq_case(form, exp_tuning):
    """-> (make, calls, expect, the EQ form per call, look-back in samples, coefficient tables [S][nb][5]) on 512 taps, block 512"""
    from open_headstage_amd import synth
    eq_form, calls, want, back = EQ_FORMS[form]
    exp_tuning.DEFAULTS.setdefault("eq_form", "0")
    exp_tuning("eq_form", eq_form)
    irs = synth.hrir_set(512)
    tabs = bm.make_tables()[0]
    table_of = [tabs[s % len(tabs)] if form == "per_stream_tables" else tabs[0] for s in range(S)]

    def make():
        bp = _handle(S, irs, 1, lib=exp_tuning.lib, eq=True)
        for b in range(bm.NB):
            bp.set_band_coeffs(b, tabs[0][b], True)
        if form == "per_stream_tables":
            for s in range(S):
                for b in range(bm.NB):
                    bp.set_stream_band_coeffs(s, b, table_of[s][b], True)
        if form == "conveyor":
            bp.set_eq_exact_specials(True)
        return bp
    return make, irs, calls, [("block512_p1", None)] * len(calls), list(want), back, table_of


def _oracle_eq(oracle, coeffs, x1):
    from open_headstage_amd import synth
    q = oracle.StereoParametricEQ(coeffs.shape[0], synth.FS)
    for b in range(coeffs.shape[0]):
        q.set_band_coeffs(b, coeffs[b], True)
    l, r = x1[0].copy(), x1[1].copy()
    q.process_block(l, r)
    return np.stack([l, r])


@pytest.mark.parametrize("in_place", [False, True], ids=list(PLACE_IDS.values()))
@pytest.mark.parametrize("form", list(EQ_FORMS))
def test_scaling_eq_forms(exp_tuning, oracle, form, in_place):
    make, irs, calls, expect, want, _, table_of = _eq_case(form, exp_tuning)
    ks = sv.scales_for(S)
    x = _noise(1100, sum(calls) * BLOCK)
    name = f"scaling, EQ {form}, {PLACE_IDS[in_place]}"
    y, _, _, _ = run_twins(name, make, calls, expect, sv.scaled(x, ks), x, in_place, eq_want=want,
                           after_call=lambda k, pos, y, yt, what: sv.check_scaling(y, yt, ks, what))
    if not in_place:        # stream 1: the oracle's EQ (the kernels are bit-exact against it), then f64 direct convolution
        e = _oracle_eq(oracle, table_of[POISONED], x[POISONED])
        yl, yr = oracle.binaural_f64(e[0], e[1], irs)
        a, r = assert_parity(sv.unscaled(y, ks)[POISONED], GAIN * np.stack([yl, yr]), name)
        print(f"special-values {name}: stream {POISONED} against oracle EQ + f64 direct convolution: abs RMS {a:.3e}, rel RMS {r:.3e}")


KIND_CALLS = (6, 5)
KINDS = {"scheduled": Scheduled, "scheduled_streams": ScheduledStreams, "ir_scheduled": IrScheduled,
         "ir_crossfaded": lambda: IrCrossfaded(KIND_CALLS), "layout": Layout, "layout_scheduled": lambda: LayoutScheduled(KIND_CALLS)}


def _kinds_setup():
    """what every call kind chooses from: four EQ tables, four sets of 200 taps, four 5.1 layouts of 200 taps"""
    return bm.make_tables(), bm._sets(bm.N_CHOICES, 200, 3), bm._layouts(bm.N_CHOICES, K_LAYOUT, 200, 5)


def _kinds_configure(bp):
    tabs, sets, lays = _kinds_setup()
    for p in range(4):
        bp.set_ir(p, sets[0][p])
    for b in range(bm.NB):
        bp.set_band_coeffs(b, tabs[0][0][b], True)
    bp.set_gain(GAIN)
    bp.set_eq_enabled(True)
    bp.set_schedule_tables(*tabs)
    bp.set_schedule_irs(sets)
    bp.set_layout_irs(lays[0])
    bp.set_layout_table(lays)
    return bp


_KIND_CASES = _with_places(list(KINDS), ("layout", "layout_scheduled"))         # the layout calls are out of place only


@pytest.mark.parametrize("kind,in_place", _KIND_CASES[0], ids=_KIND_CASES[1])
def test_scaling_call_kinds(oracle, kind, in_place):
    """the other six call kinds, each with a schedule that changes in mid-call (segments of two blocks); EQ on"""
    import open_headstage_amd as ohs
    entry = KINDS[kind]()
    assert in_place in entry.places
    lay = getattr(entry, "layout", False)
    ks = sv.scales_for(S)
    x = _noise(1200, sum(KIND_CALLS) * BLOCK, K_LAYOUT if lay else 2)
    name = f"scaling, {kind}, {PLACE_IDS[in_place]}"
    # (a layout call is served by the layout kernel: reports() asks last_layout_launch; no stereo convolution has run on the handle)
    y, _, _, _ = run_twins(name, lambda: _kinds_configure(ohs.BatchProcessor(S, num_bands=bm.NB)), KIND_CALLS,
                           [("none" if lay else "block512_p1", None)] * 2,
                           sv.scaled(x, ks), x, in_place, entry=entry, eq_want=None if lay else ["row_ring"] * 2,
                           after_call=lambda k, pos, y, yt, what: sv.check_scaling(y, yt, ks, what))
    if in_place:
        return
    # stream 1 against the host model of the header's contract (tests/batch_model.py), one stream wide
    m = _kinds_configure(bm.HandleModel(oracle, 1))
    u = sv.unscaled(y, ks)
    if not lay:
        ref, pos = [], 0
        for k, nb in enumerate(KIND_CALLS):
            ref.append(np.asarray(entry.model(m, k, np.ascontiguousarray(x[POISONED:POISONED + 1, :, pos * BLOCK:(pos + nb) * BLOCK])), np.float64)[0])
            pos += nb
        a, r = assert_parity(u[POISONED], np.concatenate(ref, axis=1), name)
        print(f"special-values {name}: stream {POISONED} against the host model: abs RMS {a:.3e}, rel RMS {r:.3e}")
        return
    # The layout kinds run the EQ BEHIND the convolution, and the f32 recurrence answers a 2e-7 difference of its input with 2e-4 of
    # its own rounding: as in tests/test_gpu_fuzz_call_kinds.py, a third handle with the EQ off gives the dry signal d, which is held
    # to the bar against the model, and the output must be the oracle's EQ of d bit for bit.
    dry = _kinds_configure(ohs.BatchProcessor(S, num_bands=bm.NB))
    dry.set_eq_enabled(False)
    pos, worst = 0, (0.0, 0.0)
    for k, nb in enumerate(KIND_CALLS):
        sl = slice(pos * BLOCK, (pos + nb) * BLOCK)
        d = entry.run(dry, k, x[:, :, sl], False)
        ref = np.asarray(entry.model(m, k, np.ascontiguousarray(x[POISONED:POISONED + 1, :, sl])), np.float64)[0]
        worst = max(worst, assert_parity(d[POISONED], ref, f"{name}, call {k}, dry signal"))
        want = m.layout_eq(np.ascontiguousarray(d[POISONED:POISONED + 1]))[0]
        bad = np.argwhere(sv._bits_differ(u[POISONED][:, sl], want))
        assert bad.size == 0, f"{name}, call {k}: stream {POISONED} differs from the oracle EQ of the dry signal in {len(bad)} samples, first (ear, frame) {bad[0].tolist()}"
        pos += nb
    print(f"special-values {name}: stream {POISONED}: dry signal against the host model: abs RMS {worst[0]:.3e}, rel RMS {worst[1]:.3e}; "
          f"output = oracle EQ of the dry signal, bit for bit")


# ---- (b) flush modes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["eq_on", "convolution_only"])
def test_flush_mode_2_reads_a_subnormal_stream_as_silence(exp_tuning, path):
    """FTZ | DAZ on both handles; stream 2 times 2^-140: every sample is subnormal (or underflows to zero) and is read as zero -- the
    stream's output is zeros, the other streams' is the twin's bit for bit"""
    from open_headstage_amd import synth
    quiet = 2
    ks = np.zeros(S, np.int32)
    ks[quiet] = -140
    if path == "eq_on":
        make0, _, calls, expect, want, _, _ = _eq_case("row_form", exp_tuning)
    else:
        irs = synth.hrir_set(1300)
        make0, calls, expect, want = (lambda: _handle(S, irs, 0)), (7, 16, 9), [("block2048", None)] * 3, None

    def make():
        bp = make0()
        bp.set_flush_denormals(2)
        return bp
    x = _noise(1300, sum(calls) * BLOCK)
    xs = sv.scaled(x, ks)
    tiny = np.abs(xs[quiet])
    assert float(tiny.max()) < float(np.finfo(np.float32).tiny) and int((tiny > 0).sum()) > tiny.size // 2

    def check(k, pos, y, yt, what):
        for s in range(S):
            if s == quiet:
                nz = np.argwhere(y[s] != 0)
                assert nz.size == 0, f"{what}: the subnormal stream {s} is not silent in {len(nz)} samples, first (channel, frame) {nz[0].tolist()}: {y[s][tuple(nz[0])]!r}"
            else:
                bad = np.argwhere(sv._bits_differ(y[s], yt[s]))
                assert bad.size == 0, f"{what}: stream {s} differs from the twin in {len(bad)} samples, first (channel, frame) {bad[0].tolist()}"
    run_twins(f"flush mode 2, {path}", make, calls, expect, xs, x, False, eq_want=want, after_call=check)


# ---- (c) containment, EQ off, and (e) reset -------------------------------------------------------------------------------------------
VALUES = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf}
# (value, channel, frame of the block, which of the family's two blocks, in place where the family allows it): every value, both
# channels, both frames, both blocks, both places
COMBOS = [("nan", 0, 17, 0, False), ("nan", 1, 511, 1, True), ("pinf", 1, 17, 1, False), ("pinf", 0, 511, 0, True), ("ninf", 0, 17, 1, True),
          ("ninf", 1, 511, 0, False)]


def _fresh_bits_after_reset(name, f, dev, x0, in_place, entry=None):
    """(e): reset() and the first call's input again -> the bits of a fresh handle (in the hook's final configuration)"""
    entry = entry or Plain()
    fresh = f.make()
    if f.hook is not None:
        for k in sorted(f.events):
            f.hook(k, fresh)
    dev.reset()
    y, yf = entry.run(dev, 0, x0, in_place), entry.run(fresh, 0, x0, in_place)
    print(f"special-values {name}: after reset -> conv {dev.last_conv_plan()}, EQ {dev.last_eq_form()}; a fresh handle -> conv {fresh.last_conv_plan()}")
    assert dev.last_conv_plan() == fresh.last_conv_plan(), (dev.last_conv_plan(), fresh.last_conv_plan())
    assert np.isfinite(yf).all() and float(np.abs(yf).max()) > 0.01
    for s in range(y.shape[0]):
        bad = np.argwhere(sv._bits_differ(y[s], yf[s]))
        assert bad.size == 0, (f"{name}: after reset() stream {s} differs from a fresh handle in {len(bad)} samples, first (channel, frame) "
                               f"{bad[0].tolist()}: {y[s][tuple(bad[0])]!r} against {yf[s][tuple(bad[0])]!r}")
    return fresh


@pytest.mark.parametrize("value,channel,frame,which,alt", COMBOS,
                         ids=[f"{v}_{'LR'[c]}_{fr}_{'mid' if w == 0 else 'other'}_{'in_place_where_served' if p else 'out_of_place'}" for v, c, fr, w, p in COMBOS])
@pytest.mark.parametrize("key", FAMILIES)
def test_containment_convolution(exp_tuning, oracle, key, value, channel, frame, which, alt):
    f = family(key, exp_tuning)
    in_place = alt and True in f.places
    calls, expect = tuple(f.calls) + tuple(f.more), list(f.expect) + list(f.more_expect)
    b = f.bs[which]
    served = f.expect[1][0]
    back, fwd = allowance(served, f.pmax)
    window = sv.allowed_window(b, f.pmax, back, fwd, call_first=calls[0])
    assert sum(calls) > window[1] + 3, (calls, window)
    x = _noise(1400, sum(calls) * BLOCK, n=f.S)
    at = b * BLOCK + frame
    xp = sv.poison(x, POISONED, channel, at, VALUES[value])
    name = f"containment, {key}, {value} in {'LR'[channel]} at block {b} frame {frame}, {PLACE_IDS[in_place]}"
    y, yt, dev, _ = run_twins(name, f.make, calls, expect, xp, x, in_place, hook=f.hook)
    ref = _oracle_nonfinite(oracle, xp[POISONED], f, calls)
    assert sv.blocks_of(ref) == list(range(b, b + f.pmax + 1)) or key.endswith("unequal") or key == "tp_gated", sv.blocks_of(ref)
    # (`ref` includes the ear that the poisoned channel reaches through a muted path only: one partition of zeros in the reference, and
    # 0 x NaN is NaN there -- and here: include/ohs_hip.h promises "non-finite wherever the reference is")
    diff = sv._bits_differ(y[POISONED], yt[POISONED]).any(axis=0).reshape(-1, BLOCK).any(axis=1)
    seen = np.flatnonzero(diff)
    print(f"special-values {name}: reference window {sv.reference_window(b, f.pmax)} (non-finite blocks of the oracle {sv.blocks_of(ref)}), "
          f"allowed {window} ({served}: back {back}, fwd {fwd}), blocks that differ from the twin [{seen.min()}, {seen.max()}], "
          f"non-finite blocks {sv.nonfinite_blocks(y[POISONED])[:1]} .. {sv.nonfinite_blocks(y[POISONED])[-1:]}")
    sv.check_containment(y, yt, POISONED, window, at, ref, name)
    _fresh_bits_after_reset(name, f, dev, x[:, :, :calls[0] * BLOCK], in_place)


@pytest.mark.parametrize("key", FAMILIES)
def test_reset_clears_state_that_still_holds_a_nan(exp_tuning, key):
    """the NaN sits in the LAST block of the last call: ring, window ring, input history, overlaps and pending tails all hold it when
    reset() comes.  A reset that only turned counters back would leave it to be multiplied by whatever reads the slot next."""
    f = family(key, exp_tuning)
    in_place = True in f.places
    b = sum(f.calls) - 1
    x = _noise(1450, sum(f.calls) * BLOCK, n=f.S)
    xp = sv.poison(x, POISONED, 0, b * BLOCK + 17, np.nan)
    name = f"reset inside the window, {key}"
    y, _, dev, _ = run_twins(name, f.make, f.calls, f.expect, xp, x, in_place, hook=f.hook)
    assert not np.isfinite(y[POISONED][:, b * BLOCK + 17:]).any(), name
    fresh = _fresh_bits_after_reset(name, f, dev, x[:, :, :f.calls[0] * BLOCK], in_place)
    # and the call behind that one: whatever the first call after the reset did not read must be clean as well
    x1 = x[:, :, f.calls[0] * BLOCK:(f.calls[0] + f.calls[1]) * BLOCK]
    got, want = Plain().run(dev, 1, x1, in_place), Plain().run(fresh, 1, x1, in_place)
    assert np.isfinite(want).all() and dev.last_conv_plan() == fresh.last_conv_plan()
    bad = np.argwhere(sv._bits_differ(got, want))
    assert bad.size == 0, f"{name}: the second call behind the reset differs from a fresh handle's in {len(bad)} samples, first (stream, channel, frame) {bad[0].tolist()}"


# ---- (d) containment, EQ on, and (e) reset --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value,channel,late", [("nan", 0, False), ("pinf", 1, True), ("ninf", 0, True)], ids=["nan_L_near", "pinf_R_511", "ninf_L_511"])
@pytest.mark.parametrize("form", list(EQ_FORMS))
def test_containment_eq_forms(exp_tuning, form, value, channel, late):
    """`near`: the poisoned sample sits exactly one look-back (+ 1) into its block, so that the block in front must be untouched --
    one sample more of look-back and it would not be"""
    make, _, calls0, expect, want, lookback, _ = _eq_case(form, exp_tuning)
    calls = tuple(calls0) + (4,)
    expect, want = expect + [("block512_p1", None)], want + [want[0]]
    if form == "wave_ring":
        want[-1] = "row_ring"           # (a call of 4 blocks is below the library's threshold for the wave ring)
    b = calls[0] + calls[1] // 2
    frame = 511 if late else lookback + 1
    at = b * BLOCK + frame
    first = (at - lookback) // BLOCK            # the first block the look-back may touch
    assert first == b
    x = _noise(1500, sum(calls) * BLOCK)
    xp = sv.poison(x, POISONED, channel, at, VALUES[value])
    name = f"containment, EQ {form}, {value} in {'LR'[channel]} at block {b} frame {frame}"
    y, yt, dev, _ = run_twins(name, make, calls, expect, xp, x, False, eq_want=want)
    last = sum(calls) - 1
    print(f"special-values {name}: look-back {lookback} samples, stream {POISONED} non-finite in blocks {sv.nonfinite_blocks(y[POISONED])[:1]} .. {last}")
    sv.check_containment(y, yt, POISONED, (first, last), at, sv.window_mask(sum(calls) * BLOCK, (b, last)), name)
    f = types.SimpleNamespace(make=make, hook=None, events={})
    _fresh_bits_after_reset(name, f, dev, x[:, :, :calls[0] * BLOCK], False)


# ---- (e) a per-path set_ir behind a poisoned call; the single-stream engine ------------------------------------------------------------
def test_block_2048_per_path_set_ir_behind_a_poisoned_call(exp_tuning, oracle):
    """the pending tails are computed from the input history, which holds the NaN: the other streams must not see it, and the
    poisoned stream keeps the family's window (the reference: path 1 forgets the sample, the other paths do not)"""
    from open_headstage_amd import synth
    f = family("lb", exp_tuning)
    f.events = {2: [(1, synth.hrir_set(900)[1])]}

    def hook(k, bp):
        for p, h in f.events.get(k, ()):
            bp.set_ir(p, h)
    calls, b = (7, 5, 18), 9
    at = b * BLOCK + 17
    x = _noise(1600, sum(calls) * BLOCK)
    xp = sv.poison(x, POISONED, 0, at, np.nan)
    name = "block 2048, per-path set_ir behind a poisoned call"
    y, yt, _, _ = run_twins(name, f.make, calls, [("block2048", None)] * 3, xp, x, False, hook=hook)
    ref = _oracle_nonfinite(oracle, xp[POISONED], f, calls)
    window = sv.allowed_window(b, f.pmax, *allowance("block2048", f.pmax), call_first=calls[0])
    print(f"special-values {name}: stream {POISONED} non-finite in blocks {sv.nonfinite_blocks(y[POISONED])}, the oracle's {sv.blocks_of(ref)}, "
          f"allowed {window}")
    sv.check_containment(y, yt, POISONED, window, at, ref, name)


@pytest.mark.parametrize("realtime", [False, True], ids=["launch_per_call", "resident"])
def test_engine_keeps_the_reference_window(oracle, realtime):
    """ohs_engine_* on 4 x 2048 taps, host blocks of 512 frames: a NaN in block b makes blocks [b, b + P] non-finite, exactly the
    oracle engine's; every other block is bit-identical to a clean engine's; re-loading the four paths (the reference's only reset)
    gives the bits of a fresh engine"""
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    irs = synth.hrir_set(2048)
    n, b, at = 14, 5, 5 * BLOCK + 17
    x = synth.white_noise([1700], n * BLOCK)[0]
    xp = x.copy()
    xp[0, at] = np.nan

    def engines():
        eg, eo = ohs.ConvolutionEngine.new(), oracle.ConvolutionEngine()
        for p in range(4):
            eg.set_ir(p, irs[p])
            eo.set_ir(p, irs[p])
        return eg, eo

    def run(e, sig, blocks, resident):
        """one resident kernel at a time: the mode is switched on for this run only"""
        e.set_realtime(resident)
        try:
            return np.concatenate([np.stack(e.process_block(sig[0, t * BLOCK:(t + 1) * BLOCK].copy(), sig[1, t * BLOCK:(t + 1) * BLOCK].copy()))
                                   for t in blocks], axis=1)
        finally:
            e.set_realtime(False)
    (eg, eo), (clean, co), (fresh, _) = engines(), engines(), engines()
    y, yc = run(eg, xp, range(n), realtime), run(clean, x, range(n), realtime)
    yo = np.concatenate([np.stack(eo.process_block(xp[0, t * BLOCK:(t + 1) * BLOCK], xp[1, t * BLOCK:(t + 1) * BLOCK])) for t in range(n)], axis=1)
    lo, hi = sv.reference_window(b, 4)
    print(f"special-values engine ({'resident' if realtime else 'launch per call'}): non-finite blocks {sv.nonfinite_blocks(y)}, the oracle's "
          f"{sv.nonfinite_blocks(yo)}")
    assert sv.nonfinite_blocks(yo) == list(range(lo, hi + 1)) == sv.nonfinite_blocks(y)
    sv.check_containment(y[None], yc[None], 0, (lo, hi), at, ~np.isfinite(yo), "engine")
    for p in range(4):
        eg.set_ir(p, irs[p])
    y2, yf = run(eg, x, range(3), realtime), run(fresh, x, range(3), realtime)
    assert np.isfinite(yf).all() and np.array_equal(y2.view(np.uint32), yf.view(np.uint32))

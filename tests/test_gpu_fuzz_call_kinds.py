"""Randomised sequences over ALL SEVEN call kinds of one batch handle, against the host model of the header's contract
(tests/batch_model.py, checked by tests/test_cpu_batch_model.py): every ordered pair of kinds, every setter between two kinds,
refusals, guarded pointer calls and launch reports.  tests/test_gpu_fuzz.py's test_fuzz_batch issues the plain call only; each kind
has a thorough file of its own; this one is about what the kinds leave for each other on a handle.

After every call:

a. stereo kinds: the output against the model's f64 expectation, relative RMS per stream over the call AND per stream and block of
   512 frames, both at the project's bar (1e-6).  A hand-over error confined to the first block of a 70-block call is diluted
   eight-fold in the call's RMS; per block it is not.  Every reference block has an RMS of 0.01 at least (asserted: the generator
   draws its gains for it).
b. layout kinds: a second handle with the EQ off receives the layout operations alone; its output d is within the bar of the
   model's dry signal, and the main handle's output equals, BIT FOR BIT, the model's oracle EQ instances applied to d -- instances
   whose state the stereo calls of every kind have advanced in between.  The EQ state that layout and stereo calls share is checked
   against independent arithmetic here and nowhere else.
c. refused calls return OHS_ERR_INVALID_ARG, and the next call is still on the model.
d. about half of the stereo calls go through the *_ptr forms on a guarded allocation (tests/guard_bands.py): every gap intact, the
   input untouched when out of place.
e. the launch reports the header names: the kernel family and the per-block set look-up of the IR kinds, the layout kernel, the
   scheduled EQ kernel -- a sequence must not slip onto a fallback and pass there.

A failure names seed, step, kind, arguments, the two operations in front, stream and block.
Measured on an MI355X over seeds 0 .. 39, worst over all kinds: 2.46e-7 per call, 2.83e-7 per block (the f32 oracle engine sits at
2.0-2.1e-7 per block against the same model); 182 layout calls compared bit for bit, 186 guarded calls, 50 refusals.
OHS_FUZZ_SEEDS=40 python -m pytest tests/test_gpu_fuzz_call_kinds.py -m gpu   for a longer soak (OHS_FUZZ_FIRST skips seeds below it)."""
import os

import numpy as np
import pytest

from tests import batch_model as bm
from tests.batch_model import BLOCK, REFUSED
from tests.guard_bands import SENT_IN, SENT_OUT, filled, gaps_intact, layout, place, take
from tests.test_cpu_ir_schedule import rel_rms_per_stream
from tests.test_cpu_layout import BAR
from tests.util import RMS_TOL

pytestmark = pytest.mark.gpu

_EXTRA = int(os.environ.get("OHS_FUZZ_SEEDS", "0"))
_FIRST = int(os.environ.get("OHS_FUZZ_FIRST", "0"))
MIN_BLOCK_RMS = 0.01
assert BAR == RMS_TOL == 1e-6


def _short(v):
    if isinstance(v, np.ndarray):
        flat = np.round(v, 3).tolist() if v.dtype.kind == "f" else v.tolist()
        text = str(flat)
        return text if len(text) <= 160 else f"{text[:150]} ... shape {v.shape}"
    return v


def _describe(op):
    return "{" + ", ".join(f"{k}: {_short(v)}" for k, v in op.items() if k not in ("op", "x_seed")) + "}" if op["op"] == "call" \
        else f"{op['op']}({', '.join(f'{k}={_short(v)}' for k, v in op.items() if k != 'op')})"


def _per_block(a):
    """[S][2][n * 512] -> RMS per stream and block [S][n]"""
    a = np.asarray(a, np.float64)
    return np.sqrt(np.mean(a.reshape(a.shape[0], 2, -1, BLOCK) ** 2, axis=(1, 3)))


class _Sequence:
    def __init__(self, oracle, seed):
        import open_headstage_amd as ohs
        self.spec = bm.sequence(seed)
        self.S = self.spec["S"]
        self.model = bm.HandleModel(oracle, self.S)
        self.main = ohs.BatchProcessor(self.S, num_bands=bm.NB)
        self.dry = ohs.BatchProcessor(self.S, num_bands=bm.NB)        # the layout operations alone, EQ off
        self.dry.set_eq_enabled(False)
        self.plan, self.history = 0, []
        self.worst = {}             # kind -> [worst per-call figure, its step, worst per-block figure, its (step, stream, block)]
        self.counts = {"bit-compared layout calls": 0, "guarded calls": 0, "refused calls": 0, "scheduled EQ kernel": 0}
        self.families = set()

    def where(self, step, op):
        front = "; ".join(_describe(o) for o in self.history[-2:]) or "nothing"
        return (f"seed {self.spec['seed']} (S {self.S}, taps {bm.LONG_TAPS if self.spec['long'] else self.spec['taps']}), step {step}, "
                f"{op.get('kind', op['op'])} {_describe(op)}; in front of it: {front}")

    # ---- the metrics of (a) ------------------------------------------------------------------------------------------------------
    def within_bar(self, got, ref, step, op, what):
        where = self.where(step, op)
        assert np.isfinite(got).all(), f"{where}: non-finite samples in the {what}"
        ref_b = _per_block(ref)
        quiet = np.argwhere(ref_b < MIN_BLOCK_RMS)
        assert quiet.size == 0, (f"{where}: the reference's block RMS is {ref_b.min():.4f} < {MIN_BLOCK_RMS} at (stream, block) "
                                 f"{quiet[:4].tolist()}: the relative metric needs a louder input")
        err_b = _per_block(np.asarray(got, np.float64) - ref) / ref_b
        err_c = rel_rms_per_stream(got, ref)
        w = self.worst.setdefault(op["kind"], [0.0, None, 0.0, None])
        if err_c.max() > w[0]:
            w[0], w[1] = float(err_c.max()), step
        if err_b.max() > w[2]:
            s, t = np.unravel_index(np.argmax(err_b), err_b.shape)
            w[2], w[3] = float(err_b.max()), (step, int(s), int(t))
        bad = np.flatnonzero(err_c > BAR)
        assert bad.size == 0, f"{where}: {what}, relative RMS over the call {err_c[bad[0]]:.3e} in stream {bad[0]} (bar {BAR:.0e}; all {err_c})"
        bad = np.argwhere(err_b > BAR)
        assert bad.size == 0, (f"{where}: {what}, relative RMS {err_b[tuple(bad[0])]:.3e} in stream {bad[0][0]}, block {bad[0][1]} of "
                               f"{err_b.shape[1]} (bar {BAR:.0e}; over the call {err_c[bad[0][0]]:.3e}; {len(bad)} blocks above the bar: "
                               f"{bad[:8].tolist()})")

    # ---- one stereo call on the main handle ---------------------------------------------------------------------------------------
    def stereo(self, op, x, step):
        import torch
        k, n, seg, bp = op["kind"], op["blocks"], op["seg"], self.main
        extra = {"process": (), "scheduled": (seg, op.get("table_idx"), op.get("gains")),
                 "scheduled_streams": (seg, op.get("table_idx"), op.get("gains")),
                 "ir_scheduled": (seg, op.get("idx"), op.get("mode")), "ir_crossfaded": (seg, op.get("idx"), op.get("prev"))}[k]
        io = op["io"]
        if io["gaps"] is None:                  # the tensor interface
            xt = torch.from_numpy(x.copy()).cuda()
            out = xt if io["in_place"] else None
            y = (bp.process(xt, out=out) if k == "process" else getattr(bp, "process_" + k)(xt, *extra, out=out))
            torch.cuda.synchronize()
            if not io["in_place"]:
                assert np.array_equal(xt.cpu().numpy().view(np.uint32), x.view(np.uint32)), f"{self.where(step, op)}: the input changed"
            return y.cpu().numpy(), True
        # the pointer form on a guarded allocation
        lead, frames = io["gaps"][0], n * BLOCK
        ss, cs, total, mask = layout(self.S, frames, *io["gaps"])
        hin = filled(total, SENT_IN)
        place(hin, x, lead, ss, cs)
        d_in = torch.from_numpy(hin.copy()).cuda()
        d_out = d_in if io["in_place"] else torch.from_numpy(filled(total, SENT_OUT).copy()).cuda()
        st = torch.cuda.current_stream().cuda_stream
        getattr(bp, "process_ptr" if k == "process" else f"process_{k}_ptr")(d_in.data_ptr() + 4 * lead, d_out.data_ptr() + 4 * lead, n, ss,
                                                                             cs, *extra, st)
        torch.cuda.synchronize()
        out, inb = d_out.cpu().numpy(), d_in.cpu().numpy()
        where = self.where(step, op)
        gaps_intact(out.view(np.uint32), mask, SENT_IN if io["in_place"] else SENT_OUT, where + ", output buffer")
        if not io["in_place"]:
            changed = np.flatnonzero(inb.view(np.uint32) != hin.view(np.uint32))
            assert changed.size == 0, f"{where}: {changed.size} words of the input buffer changed, first at {changed[:6]}"
        self.counts["guarded calls"] += 1
        aligned = all(v % 4 == 0 for v in (lead, ss, cs))
        return take(out, self.S, frames, lead, ss, cs), aligned

    def refused(self, op, x, step):
        """(c): OHS_ERR_INVALID_ARG, nothing queued, the buffers untouched"""
        import torch
        from open_headstage_amd import _ffi
        k, seg = op["kind"], op["seg"]
        extra = (seg, op.get("table_idx"), op.get("gains")) if k == "scheduled" else \
            (seg, op["idx"], op["mode"]) if k == "ir_scheduled" else (seg, op["idx"], op["prev"])
        xt = torch.from_numpy(x.copy()).cuda()
        out = torch.full_like(xt, 7.0)
        with pytest.raises(_ffi.OhsError) as e:
            getattr(self.main, "process_" + k)(xt, *extra, out=out)
        assert e.value.status == _ffi.OHS_ERR_INVALID_ARG, f"{self.where(step, op)}: {e.value}"
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), f"{self.where(step, op)}: a refused call wrote its output"
        self.counts["refused calls"] += 1

    # ---- (e) the launch reports ---------------------------------------------------------------------------------------------------
    def stereo_reports(self, op, step, aligned):
        k, bp, where = op["kind"], self.main, self.where(step, op)
        family = bp.last_conv_plan()[0]
        self.families.add(family)
        code = 2 if bp.last_conv_ir_crossfaded() else 1 if bp.last_conv_ir_scheduled() else 0
        n_segs = bm.n_segments(op["blocks"], op["seg"])
        if k in bm.IR_KINDS:
            rows = np.broadcast_to(np.asarray(op["idx"])[..., :n_segs], (self.S, n_segs))
            shared, vary = np.ndim(op["idx"]) == 1, bool((rows != rows[:, :1]).any())
            fades = k == "ir_crossfaded" and (vary or (op["prev"] is not None and
                                                       bool((np.broadcast_to(np.asarray(op["prev"]).reshape(-1), (self.S,)) != rows[:, 0]).any())))
            want = 2 if fades else 0 if (shared and not vary) else 1
            assert family == "block512_p1" and code == want, f"{where}: served by {family}, set look-up {code}; the header names block512_p1, {want}"
        else:
            assert code == 0, f"{where}: the report of a per-block set look-up ({code}) behind a call without one"
            if not self.spec["long"]:
                ok = ("block512_p1", "hop1536_p1") if self.plan == 2 else ("block512_p1",)
                assert family in ok, f"{where}: served by {family} under plan {self.plan}"
            elif self.plan != 1 and aligned:
                assert family == "block2048", f"{where}: served by {family} under plan {self.plan}"
            else:
                assert family in ("block512_tp", "sequential", "block2048"), f"{where}: served by {family} under plan {self.plan}"
        if not (self.model.eq_enabled and self.eq_any_enabled()):
            return
        form, scheduled = bp.last_eq_form()
        assert form != "none", where
        rows = op.get("table_idx") if k in ("scheduled", "scheduled_streams") else None
        changes = rows is not None and bool((np.diff(np.asarray(rows)[..., :n_segs], axis=-1) != 0).any())
        if not changes:
            assert not scheduled, f"{where}: the scheduled EQ kernel is reported behind a call whose tables do not change"
        elif op["blocks"] < 64 and form == "wave_ring":      # (one time chunk; the schedule tables share their enabled flags)
            assert scheduled, f"{where}: the wave ring served the call, but not its scheduled kernel"
        self.counts["scheduled EQ kernel"] += int(scheduled)

    def eq_any_enabled(self):
        return any(self.model._table_of(s)[1].any() for s in range(self.S))

    # ---- the sequence -------------------------------------------------------------------------------------------------------------
    def run(self):
        import torch
        for step, op in enumerate(self.spec["ops"]):
            if op["op"] != "call":
                args = bm.setter_args(self.spec, op)
                getattr(self.main, op["op"])(*args)
                if op["op"] in ("set_layout_irs", "set_layout_table", "reset"):
                    getattr(self.dry, op["op"])(*args)
                if op["op"] == "set_conv_plan":
                    self.plan = op["plan"]
                bm.model_setter(self.model, self.spec, op)
                self.history.append(op)
                continue
            x = bm.call_input(self.spec, op)
            ref = bm.model_call(self.model, op, x)
            where = self.where(step, op)
            if op["refused"]:
                assert ref is REFUSED, f"{where}: the model serves a call the generator expects refused"
                self.refused(op, x, step)
            elif op["kind"] in bm.STEREO_KINDS:
                assert ref is not REFUSED, f"{where}: the model refuses"
                y, aligned = self.stereo(op, x, step)
                self.within_bar(y, ref, step, op, "output against the f64 model")
                self.stereo_reports(op, step, aligned)
            else:
                xt = torch.from_numpy(x).cuda()
                self.dry.set_gain(self.model.gain)
                if op["kind"] == "layout":
                    d, y = self.dry.process_layout(xt), self.main.process_layout(xt)
                else:
                    args = (op["idx"], op["seg"], op["prev"], op["crossfade"])
                    d, y = self.dry.process_layout_scheduled(xt, *args), self.main.process_layout_scheduled(xt, *args)
                torch.cuda.synchronize()
                d, y = d.cpu().numpy(), y.cpu().numpy()
                self.within_bar(d, ref, step, op, "dry output (EQ off, layout operations alone) against the f64 model")
                want = self.model.layout_eq(d)
                for s in range(self.S):
                    bad = np.argwhere(y[s].view(np.uint32) != want[s].view(np.uint32))
                    assert bad.size == 0, (f"{where}: stream {s} differs from the oracle EQ of the dry output (the state the stereo calls "
                                           f"share) in {len(bad)} samples, first (ear, frame) {bad[:4].tolist()}, last {bad[-1].tolist()}; EQ "
                                           f"{'on' if self.model.eq_enabled else 'off'}")
                self.counts["bit-compared layout calls"] += 1
                # (e)
                n_segs = bm.n_segments(op["blocks"], op["seg"])
                plain = op["kind"] == "layout"
                if not plain:
                    rows = np.asarray(op["idx"])[..., :n_segs]
                    boundary = op["crossfade"] and op["prev"] is not None and bool((np.asarray(op["prev"]).reshape(-1) != rows[..., 0]).any())
                    plain = rows.ndim == 1 and bool((rows == rows[0]).all()) and not boundary
                for bp in (self.main, self.dry):
                    assert bp.last_layout_scheduled() == (not plain), f"{where}: k_conv_p1_layout_irs reported {bp.last_layout_scheduled()}"
                    assert bp.last_layout_launch()[0] == (op["K"] + 1) // 2, f"{where}: {bp.last_layout_launch()} for {op['K']} channels"
            self.history.append(op)
        return self


@pytest.mark.parametrize("seed", range(_FIRST if _EXTRA else 0, max(bm.DEFAULT_SEEDS, _EXTRA)))
def test_fuzz_call_kinds_against_the_model(oracle, seed):
    q = _Sequence(oracle, seed).run()
    for kind, (c, c_step, b, b_at) in sorted(q.worst.items()):
        print(f"call-kinds seed {seed}: {kind}: worst relative RMS per call {c:.3e} (step {c_step}), per block {b:.3e} (step, stream, block {b_at})")
    print(f"call-kinds seed {seed}: {q.counts}; convolution families {sorted(q.families)}")
    calls = [op for op in q.spec["ops"] if op["op"] == "call"]
    assert q.counts["refused calls"] == sum(op["refused"] for op in calls)
    assert q.counts["bit-compared layout calls"] == sum(op["kind"] in bm.LAYOUT_KINDS for op in calls)
    if q.spec["long"]:
        # the handle's own 1300 taps: the block-2048 plan served calls of this sequence, and both IR kinds were refused
        assert "block2048" in q.families and q.counts["refused calls"] >= 2, (q.families, q.counts)

"""Every asynchronous entry point held to its stream contract on a BUSY stream (include/ohs_hip.h, beside ohs_batch_process).

The harness is tests/busy_stream.py.  A scenario is a script of setters and calls.  It runs three times:

  the quiet twin   a fresh handle on the default stream, inputs uploaded beforehand, a device-wide wait behind every step: how the rest
                   of the suite runs.  Its host time per call sizes the filler.
  the busy runs    fresh handles on two caller streams created one after the other (the runtime hands streams to hardware queues in
                   turn: a caller stream that shares a queue with the handle's second stream would hide a missing wait, two neighbours
                   cannot both share it).  Filler, then per call: the input copied device to device into a NaN buffer BEHIND the
                   filler, the call, its host rows scribbled the moment it returns, the output copied to a keep buffer, both buffers
                   NaN again -- all on the caller's stream, nothing waited for until the end.

Busy run and twin agree BIT FOR BIT in every output and in every launch record (a plan that depended on timing would show), and the
twin is held to independent arithmetic once per scenario: tests/batch_model.py's HandleModel and the scene models, at the suite's bar
of 1e-6 relative RMS per stream and per 512-frame block; a layout or scene call's EQ, which runs behind the renderer, is compared bit
for bit with the oracle's EQ on the output of a third, EQ-less handle, as tests/test_gpu_fuzz_call_kinds.py does.  "Both wrong alike"
is thereby excluded.

The premise -- the caller's stream is still busy when the last call that must not block has returned -- is asserted, never skipped
(busy_stream.PremiseError): it is the test of asynchrony itself.

Shapes: 5 streams; layouts of 3 channels, scenes of 3 objects over 8 directions; the ten bands of synth.eq_table; 66 blocks with the EQ
on for the stereo kinds (six time chunks, the handle's second stream; 66 is no multiple of the cuts), 6 blocks in segments of 2
elsewhere; responses of 300 taps under plan 1, and for the plain call also 1300 taps under plan 0 (block 2048) and 6700 taps, 130
blocks, out of place, EQ off -- one convolution launch of 130 blocks, which is what the block-8192 kernel asks for.

Scenarios: A late input, early reuse (every entry point); B host rows scribbled on return; C more calls than staging slots; D
by-value setters between queued calls; E device-table setters behind queued work; F one handle moved between two streams; G the
deferred pipeline; H the three sync calls; I two deliberately wrong CALLERS that the harness must report as a mismatch."""
import time

import numpy as np
import pytest

from tests import batch_model as bm
from tests import busy_stream as bs
from tests import scene_blend_model as sbm
from tests import scene_model as sm
from tests.batch_model import BLOCK
from tests.test_cpu_layout import BAR, make_input, make_layout, rel_rms_per_stream
from tests.test_cpu_scene import rel_rms_per_block

pytestmark = pytest.mark.gpu

S, K, N_DIRS, NB = 5, 3, 8, bm.NB
TAPS, BIG, SMALL, SEG = 300, 66, 6, 2
GAIN = 0.8
assert BAR == 1e-6

# entry point -> the call kind scenario A drives it through (tests/test_cpu_stream_order.py: the set is the headers')
SCENARIO_A = {
    "ohs_batch_process": "process", "ohs_batch_process_scheduled": "scheduled",
    "ohs_batch_process_scheduled_streams": "scheduled_streams", "ohs_batch_process_ir_scheduled": "ir_scheduled",
    "ohs_batch_process_ir_crossfaded": "ir_crossfaded", "ohs_batch_process_layout": "layout",
    "ohs_batch_process_layout_scheduled": "layout_scheduled", "ohs_batch_process_deferred": "deferred", "ohs_batch_join": "join",
    "ohs_batch_sync": "sync", "ohs_node_batch_process": "node", "ohs_scene_process": "scene", "ohs_scene_sync": "scene_sync",
    "ohs_scene2_process": "scene2", "ohs_scene2_process_blended": "blended", "ohs_scene2_sync": "scene2_sync",
}
IN_PLACE_KINDS = ("process", "scheduled", "scheduled_streams", "ir_scheduled", "ir_crossfaded", "deferred", "node")   # the headers' "d_in may equal d_out"
ROW_KINDS = ("scheduled", "scheduled_streams", "ir_scheduled", "ir_crossfaded", "layout_scheduled", "scene", "scene2", "blended")
STAGED_KINDS = ("scheduled_streams", "ir_crossfaded", "layout_scheduled", "scene", "blended")        # scenario C
STEREO = ("process", "deferred", "scheduled", "scheduled_streams", "ir_scheduled", "ir_crossfaded", "node")
RIG_OF = {"layout": "batch", "layout_scheduled": "batch", "scene": "scene", "scene2": "scene2", "blended": "scene2", "node": "node"}


# ---- the material: responses, tables, inputs, rows -------------------------------------------------------------------------------------
def _own_irs(taps):
    """the handle's own four responses"""
    if taps <= BLOCK:
        return bm._sets(2, taps, 5)[0]
    if taps == bm.LONG_TAPS:
        return bm.long_irs(5)[0]
    rng = np.random.default_rng(4000 + taps)          # bm.long_irs' recipe at any length: decaying noise, a direct tap, L1-normalised per ear
    k = np.arange(taps, dtype=np.float64)
    hs = [g * (0.5 * rng.standard_normal(taps) * np.exp(-k / (taps / 4.0))) for g in (1.0, 0.4, 0.4, 1.0)]
    for p, d in enumerate((30, 45, 46, 31)):
        hs[p][d] += 3.0 * (1.0, 0.4, 0.4, 1.0)[p]
    nl, nr = np.abs(hs[0]).sum() + np.abs(hs[2]).sum(), np.abs(hs[1]).sum() + np.abs(hs[3]).sum()
    return np.stack([hs[p] / n for p, n in enumerate([nl, nr, nl, nr])]).astype(np.float32)


def _dirs(seed=11):
    return make_layout(N_DIRS, TAPS, seed=seed)


def batch_setup(taps=TAPS, plan=1, eq=True):
    """a batch handle's setters, as ops for the handle and for HandleModel alike"""
    irs, (coeffs, en) = _own_irs(taps), bm.make_tables()
    ops = [("set", "set_ir", (p, irs[p])) for p in range(4)]
    ops += [("set", "set_band_coeffs", (b, coeffs[0, b], True)) for b in range(NB)]
    ops += [("set", "set_schedule_tables", (coeffs, en)), ("set", "set_layout_irs", (bm._layouts(1, K, TAPS, 3)[0],)),
            ("set", "set_layout_table", (bm._layouts(bm.N_CHOICES, K, TAPS, 4),))]
    if taps <= BLOCK:
        ops.append(("set", "set_schedule_irs", (bm._sets(bm.N_CHOICES, TAPS, 7),)))
    return ops + [("set", "set_gain", (GAIN,)), ("set", "set_eq_enabled", (eq,)), ("set", "set_conv_plan", (plan,)),
                  ("set", "set_flush_denormals", (0,)), ("set", "share_eq_table", ())]


class Call:
    def __init__(self, kind, x, rows=None, seg=SEG, in_place=False, observe=True, mode="ring_out"):
        self.kind, self.x, self.rows, self.seg, self.in_place, self.observe, self.mode = kind, x, rows or {}, seg, in_place, observe, mode
        self.blocks = x.shape[2] // BLOCK

    def __repr__(self):
        return f"{self.kind}({self.blocks} blocks{', in place' if self.in_place else ''})"


def _varying(rng, shape, n=bm.N_CHOICES):
    """indices that change at every segment"""
    a = np.zeros(shape, np.uint32)
    a[..., 0] = rng.integers(0, n, shape[:-1])
    for k in range(1, shape[-1]):
        a[..., k] = (a[..., k - 1] + rng.integers(1, n, shape[:-1])) % n
    return a


def make_call(kind, seed=0, blocks=None, in_place=False, observe=True):
    """one call of `kind` with an input and rows of its own"""
    from open_headstage_amd import synth
    rng = np.random.default_rng(77000 + seed)
    stereo = kind in STEREO
    n = blocks or (BIG if stereo else SMALL)
    n_segs = -(-n // SEG)
    x = synth.white_noise(range(500 + 10 * seed, 500 + 10 * seed + S), n * BLOCK) if stereo else make_input(S, K, n, seed=900 + 20 * seed)
    rows = {}
    if kind == "scheduled":
        rows = {"table_idx": _varying(rng, (n_segs,)), "gain": rng.uniform(0.5, 1.0, n_segs)}
    elif kind == "scheduled_streams":
        rows = {"table_idx": _varying(rng, (S, n_segs)), "gain": rng.uniform(0.5, 1.0, (S, n_segs))}
    elif kind == "ir_scheduled":
        rows = {"ir_idx": _varying(rng, (S, n_segs))}
    elif kind == "ir_crossfaded":
        rows = {"ir_idx": _varying(rng, (S, n_segs)), "prev_idx": rng.integers(0, bm.N_CHOICES, S)}
    elif kind == "layout_scheduled":
        rows = {"idx": _varying(rng, (S, n_segs)), "prev": rng.integers(0, bm.N_CHOICES, S)}
    elif kind in ("scene", "scene2"):
        idx, g, pi, pg = sm.make_scene(S, K, n, SEG, N_DIRS, seed=seed)
        rows = {"dir_idx": idx, "obj_gain": g, "prev_idx": pi, "prev_gain": pg}
    elif kind == "blended":
        r = sbm.make_blend_scene(S, K, n, SEG, N_DIRS, seed=seed)
        rows = {"dir_idx": r["idx"], "obj_gain": r["gains"], "prev_idx": r["prev_idx"], "prev_gain": r["prev_gains"],
                "dir_idx1": r["idx1"], "weight": r["weights"], "prev_idx1": r["prev_idx1"], "prev_weight": r["prev_weights"]}
    return Call(kind, np.ascontiguousarray(x, np.float32), bs.row_arrays(rows), in_place=in_place, observe=observe,
                mode="cut" if seed % 2 else "ring_out")


# ---- the rigs: handle, warm-up, one call, the launch record -----------------------------------------------------------------------------
def _apply(h, ops):
    for _, name, args in ops:
        getattr(h, name)(*args)


def scene_setup(eq=True):
    from tests.test_gpu_layout import _eq_bands
    ops = [("set", "set_gain", (GAIN,)), ("set", "set_directions", (_dirs(),))]
    ops += [("set", "set_band_coeffs", (i, c, en)) for i, (c, en) in enumerate(_eq_bands())]
    return ops + [("set", "set_eq_enabled", (eq,))]


def make_handle(rig, script):
    """a fresh handle of rig (type, setup ops), warmed: the script once on the default stream -- a first call of a kind, or of a launch
    geometry that needs more scratch than any before, may allocate and wait for its stream; a kind that stages rows is called as often
    as there are staging slots, every slot allocates at its first use --, then reset() and the setup again (a shared row leaves its
    last table and gain behind, a setter of the script its value)"""
    import open_headstage_amd as ohs
    import torch
    kind, setup = rig
    if kind == "node":
        h = ohs.NodeBatchProcessor(S, num_bands=NB, n_devices=1)
    else:
        h = {"batch": ohs.BatchProcessor, "scene": ohs.SceneProcessor, "scene2": ohs.BlendSceneProcessor}[kind](S, num_bands=NB)

    def configure():
        if kind != "node":
            return _apply(h, setup)
        st = dict((name, []) for _, name, _ in setup)
        for _, name, args in setup:
            st[name].append(args)
        h.set_tables([a[1] for a in st["set_ir"]], np.stack([a[1] for a in st["set_band_coeffs"]]), [a[2] for a in st["set_band_coeffs"]])
        for name in ("set_gain", "set_eq_enabled", "set_conv_plan"):
            getattr(h, name)(*st[name][-1])
    configure()
    seen = set()
    for op in script:                   # the script itself, setters included: a by-value setter changes the launches of the calls behind it
        if op[0] == "set":
            getattr(h, op[1])(*op[2])
        elif op[0] == "call":
            c = op[1]
            for _ in range(bs.staging_slots() if c.rows and c.kind not in seen else 1):
                x = torch.from_numpy(c.x).cuda()
                invoke(h, c, bs.row_arrays(c.rows), x, x if c.in_place else torch.empty(out_shape(c), device="cuda"), None)
            seen.add(c.kind)
    if "deferred" in seen:
        h.join()
    torch.cuda.synchronize()
    h.reset()
    configure()
    torch.cuda.synchronize()
    return h


def out_shape(c):
    return (S, 2, c.x.shape[2])


def invoke(h, c, rows, d_in, d_out, hs):
    k, r = c.kind, rows
    if k in ("process", "deferred"):
        h.process(d_in, out=d_out, hip_stream=hs, deferred=k == "deferred")
    elif k == "scheduled":
        h.process_scheduled(d_in, c.seg, r["table_idx"], r["gain"], out=d_out, hip_stream=hs)
    elif k == "scheduled_streams":
        h.process_scheduled_streams(d_in, c.seg, r["table_idx"], r["gain"], out=d_out, hip_stream=hs)
    elif k == "ir_scheduled":
        h.process_ir_scheduled(d_in, c.seg, r["ir_idx"], c.mode, out=d_out, hip_stream=hs)
    elif k == "ir_crossfaded":
        h.process_ir_crossfaded(d_in, c.seg, r["ir_idx"], r["prev_idx"], out=d_out, hip_stream=hs)
    elif k == "layout":
        h.process_layout(d_in, out=d_out, hip_stream=hs)
    elif k == "layout_scheduled":
        h.process_layout_scheduled(d_in, r["idx"], c.seg, r["prev"], True, out=d_out, hip_stream=hs)
    elif k in ("scene", "scene2"):
        h.process(d_in, r["dir_idx"], c.seg, r["obj_gain"], r["prev_idx"], r["prev_gain"], True, out=d_out, hip_stream=hs)
    elif k == "blended":
        h.process(d_in, r["dir_idx"], c.seg, r["obj_gain"], r["prev_idx"], r["prev_gain"], True, r["dir_idx1"], r["weight"],
                  r["prev_idx1"], r["prev_weight"], out=d_out, hip_stream=hs)
    else:
        assert k == "node", k
        h.process([d_in], [d_out])


def report(h, rig_kind):
    """the launch records the headers name"""
    if rig_kind in ("scene", "scene2"):
        return h.last_launch()
    if rig_kind == "node":
        h = h.device_batch(0)
    return (h.last_conv_plan(), h.last_eq_form(), h.last_conv_ir_scheduled(), h.last_conv_ir_crossfaded(), h.last_layout_launch(),
            h.last_layout_scheduled(), tuple(sorted(h.conv_plan_counts().items())))


def _sync(h, rig_kind, hs):
    if rig_kind == "node":
        h.sync()
    else:
        h.sync(hs or 0)


class _Buffers:
    """NaN device buffers, one per shape and role: calls of one geometry share them, as a host's steps do"""

    def __init__(self):
        self.pool = {}

    def get(self, role, shape):
        import torch
        key = (role, tuple(shape))
        if key not in self.pool:
            self.pool[key] = torch.full(tuple(shape), float("nan"), device="cuda")
        return self.pool[key]

    def of(self, c):
        d_out = self.get("out", out_shape(c))
        return (d_out if c.in_place else self.get("in", c.x.shape)), d_out


# ---- the quiet twin ---------------------------------------------------------------------------------------------------------------------
def run_quiet(rig, script):
    """-> (outputs per call, launch records per call, host seconds spent enqueueing)"""
    import torch
    h = make_handle(rig, script)
    bufs, outs, reps, host = _Buffers(), [], [], 0.0
    for op in script:
        if op[0] == "set":
            getattr(h, op[1])(*op[2])
        elif op[0] == "join":
            h.join()
        elif op[0] == "sync":
            _sync(h, rig[0], None)
        elif op[0] == "call":
            c = op[1]
            src, rows, (d_in, d_out) = torch.from_numpy(c.x).cuda(), bs.row_arrays(c.rows), bufs.of(c)
            keep = torch.empty(out_shape(c), device="cuda")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d_in.copy_(src)
            invoke(h, c, rows, d_in, d_out, None)
            keep.copy_(d_out)
            host += time.perf_counter() - t0
            torch.cuda.synchronize()
            outs.append(d_out.cpu().numpy())
            reps.append(report(h, rig[0]))
        torch.cuda.synchronize()
    return outs, reps, host


# ---- the busy run -----------------------------------------------------------------------------------------------------------------------
def run_busy(rig, script, streams, seconds, scribble=True, wrong=None):
    """The script on streams[0] (ops ("on", i, wait) move to streams[i]) behind a filler of `seconds` -> (outputs of the observed
    calls, launch records).  streams: BusyStreams, or a function of the handle that gives them (the node batch owns its stream).
    wrong: ("producer" | "consumer", a function that picks a second stream once the filler runs): scenario I's callers."""
    import torch
    h = make_handle(rig, script)
    if callable(streams):
        streams = streams(h)
    nan = float("nan")
    calls = [op[1] for op in script if op[0] == "call"]
    src = [torch.from_numpy(c.x).cuda() for c in calls]
    keep = [torch.full(out_shape(c), nan, device="cuda") for c in calls]
    done = [torch.cuda.Event() for _ in calls]
    bufs = _Buffers()
    for c in calls:
        bufs.of(c)
    reps, pending, cur, j, last = [], [], 0, 0, "nothing"
    busy = streams[0]
    torch.cuda.synchronize()
    try:
        busy.fill(seconds)
        side = wrong[1]() if wrong else None

        def collect(st, jj, d_out):
            if wrong and wrong[0] == "consumer":
                with torch.cuda.stream(side):                   # no event from the caller's stream to this one
                    keep[jj].copy_(d_out, non_blocking=True)
            else:
                keep[jj].copy_(d_out, non_blocking=True)
                d_out.fill_(nan)

        def flush(st):
            with torch.cuda.stream(st):
                for jj, d_out in pending:
                    collect(st, jj, d_out)
            pending.clear()

        for op in script:
            st = streams[cur].stream
            if op[0] == "set":
                getattr(h, op[1])(*op[2])
                last = op[1]
            elif op[0] == "on":
                if op[2]:
                    streams[op[1]].stream.wait_stream(st)
                cur = op[1]
            elif op[0] == "premise":
                busy.premise(last)
            elif op[0] == "drained":
                busy.drained(last)
            elif op[0] == "fired":
                assert done[op[1]].query(), f"{last} returned, but call {op[1]}, whose staging slot it took, has not completed"
            elif op[0] == "join":
                h.join(st.cuda_stream)
                last = "ohs_batch_join"
                flush(st)
            elif op[0] == "sync":
                _sync(h, rig[0], st.cuda_stream)
                last = "the sync call"
                busy.drained(last)
                assert all(e.query() for e in done[:j]), "the sync call returned, but an event recorded behind an earlier call has not fired"
                flush(st)
            else:
                c = op[1]
                rows, (d_in, d_out) = bs.row_arrays(c.rows), bufs.of(c)
                last = f"call {j}, {c!r}"
                with torch.cuda.stream(st):
                    if wrong and wrong[0] == "producer":
                        with torch.cuda.stream(side):           # behind the upstream work, a little work of its own, and no event back
                            side.wait_event(busy.busy_done)
                            for _ in range(20):
                                bs._filler_tensor().fill_(1.0)
                            d_in.copy_(src[j], non_blocking=True)
                    else:
                        d_in.copy_(src[j], non_blocking=True)
                    invoke(h, c, rows, d_in, d_out, st.cuda_stream)
                    if scribble:
                        bs.scribble(rows)
                    done[j].record(st)
                    reps.append(report(h, rig[0]))
                    if c.kind != "deferred":
                        flush(st)                               # (every other use of the handle joins by itself)
                    if not c.in_place:
                        d_in.fill_(nan)
                    if c.kind == "deferred":
                        if c.observe:
                            pending.append((j, d_out))
                    elif c.observe:
                        collect(st, j, d_out)
                j += 1
        assert not pending, "the script leaves a deferred call unjoined"
    finally:
        torch.cuda.synchronize()
    return [keep[i].cpu().numpy() if c.observe else None for i, c in enumerate(calls)], reps


# ---- the anchor: the twin against independent arithmetic ----------------------------------------------------------------------------------
def _per_block_ok(got, ref, what):
    assert np.isfinite(got).all(), f"{what}: non-finite samples"
    e, eb = rel_rms_per_stream(got, ref), rel_rms_per_block(got, ref)
    print(f"{what}: twin against the f64 model, relative RMS per stream, worst {e.max():.3e}; per block, worst {eb.max():.3e}")
    assert (e <= BAR).all(), f"{what}: relative RMS per stream {e} (bar {BAR:.0e})"
    assert (eb <= BAR).all(), f"{what}: relative RMS per block, worst {eb.max():.3e} at {np.unravel_index(eb.argmax(), eb.shape)} (bar {BAR:.0e})"


def _eqless(rig, script):
    kind, setup = rig
    off = [op for op in setup if op[1] != "set_eq_enabled"] + [("set", "set_eq_enabled", (False,))]
    return (kind, off), [op for op in script if not (op[0] == "set" and op[1] == "set_eq_enabled")]


MODEL_SKIPS = ("set_conv_plan", "set_flush_denormals")      # which kernel serves a call, and flushing on a signal in the normal range, change no arithmetic


class _LongConvOracle:
    """The oracle with direct_conv_f64 through an f64 FFT for responses beyond 2048 taps: HandleModel convolves a long handle's whole
    history with every path, and 5 streams x 4 paths x 66 560 frames x 6700 taps in the time domain are seven seconds.  A transform
    of 2^17 points in f64 is good to some 1e-15 relative, nine orders below the bar the result is used at."""

    def __init__(self, oracle):
        self._o = oracle

    def __getattr__(self, name):
        return getattr(self._o, name)

    def direct_conv_f64(self, x, h):
        if len(h) <= 2048:
            return self._o.direct_conv_f64(x, h)
        x, h = np.asarray(x, np.float32).astype(np.float64), np.asarray(h, np.float32).astype(np.float64)
        n = 1 << int(np.ceil(np.log2(len(x) + len(h))))
        return np.fft.irfft(np.fft.rfft(x, n) * np.fft.rfft(h, n), n)[:len(x)]


def anchor(oracle, rig, script, outs, what):
    from tests.test_gpu_layout import _oracle_eq
    kind, setup = rig
    renders_behind = any(op[0] == "call" and op[1].kind not in STEREO for op in script)
    dry = run_quiet(*_eqless(rig, script))[0] if renders_behind else None
    if kind in ("batch", "node"):
        m = bm.HandleModel(_LongConvOracle(oracle), S)
        step = lambda name, args: name in MODEL_SKIPS or getattr(m, name)(*args)
    else:
        state = {"dirs": None, "tail": None, "eqs": None}

        def step(name, args):
            if name == "set_directions":
                state.update(dirs=np.array(args[0]), tail=None)
            elif name == "reset":
                state.update(tail=None, eqs=None)
    for _, name, args in setup:
        step(name, args)
    j = 0
    for op in script:
        if op[0] == "set":
            step(op[1], op[2])
        if op[0] != "call":
            continue
        c, r, label = op[1], op[1].rows, f"{what}, call {j} {op[1]!r}"
        if c.kind in STEREO:
            ref = {"process": lambda: m.process(c.x), "deferred": lambda: m.process(c.x), "node": lambda: m.process(c.x),
                   "scheduled": lambda: m.process_scheduled(c.x, c.seg, r["table_idx"], r["gain"]),
                   "scheduled_streams": lambda: m.process_scheduled_streams(c.x, c.seg, r["table_idx"], r["gain"]),
                   "ir_scheduled": lambda: m.process_ir_scheduled(c.x, c.seg, r["ir_idx"], c.mode),
                   "ir_crossfaded": lambda: m.process_ir_crossfaded(c.x, c.seg, r["ir_idx"], r["prev_idx"])}[c.kind]()
            assert ref is not bm.REFUSED, label
            _per_block_ok(outs[j], ref, label)
        elif kind == "batch":
            ref = m.process_layout(c.x) if c.kind == "layout" else m.process_layout_scheduled(c.x, r["idx"], c.seg, r["prev"], True)
            _per_block_ok(dry[j], ref, label + " (EQ off)")
            bs.same_bits(outs[j], m.layout_eq(dry[j]), label + ": the oracle's EQ of the EQ-less handle's output")
        else:
            args = dict(seg_blocks=c.seg, gains=r["obj_gain"], prev_idx=r["prev_idx"], prev_gains=r["prev_gain"], crossfade=True, gain=GAIN,
                        tail_in=state["tail"], with_tail=True)
            if c.kind == "blended":
                ref, state["tail"] = sbm.model_blend_f64(c.x, state["dirs"], r["dir_idx"], r["dir_idx1"], r["weight"], prev_idx1=r["prev_idx1"],
                                                         prev_weights=r["prev_weight"], **args)
            else:
                ref, state["tail"] = sm.model_scene_f64(c.x, state["dirs"], r["dir_idx"], **args)
            _per_block_ok(dry[j], ref, label + " (EQ off)")
            want, state["eqs"] = _oracle_eq(oracle, dry[j], state["eqs"])
            bs.same_bits(outs[j], want, label + ": the oracle's EQ of the EQ-less handle's output")
        j += 1


# ---- one scenario, start to end -----------------------------------------------------------------------------------------------------------
_twins = {}


def twin_of(oracle, key, rig, script):
    """the quiet twin's outputs, records and enqueue time, anchored to the models: once per scenario, shared by the tests that run it"""
    if key not in _twins:
        outs, reps, host = run_quiet(rig, script)
        anchor(oracle, rig, script, outs, key)
        _twins[key] = (outs, reps, host)
    return _twins[key]


def compare(got, twin, what):
    (outs, reps), (t_outs, t_reps, _) = got, twin
    if reps != t_reps:
        bad = next(i for i, (a, b) in enumerate(zip(reps, t_reps)) if a != b) if len(reps) == len(t_reps) else -1
        raise bs.DataMismatch(f"{what}: the launch records differ from the twin's at call {bad}: {reps[bad]} against {t_reps[bad]}")
    for j, (y, t) in enumerate(zip(outs, t_outs)):
        if y is not None:
            bs.same_bits(y, t, f"{what}, call {j}")


def scenario(oracle, key, rig, script, scribble=True, two_streams=False):
    """the twin once, then the busy run on each of two caller streams created one after the other (two_streams: the script moves
    between them; it runs in both orders)"""
    import torch
    twin = twin_of(oracle, key, rig, script)
    seconds = bs.filler_seconds(twin[2])
    if rig[0] == "node":                    # the slot's own stream is the caller's stream here: filler and copies go onto it
        slot = []
        got = run_busy(rig, script, lambda h: slot.append(bs.BusyStream(torch.cuda.ExternalStream(h.stream(0)))) or slot, seconds, scribble)
        print(f"{key}: host enqueue on the twin {twin[2] * 1e3:.3f} ms, filler {seconds * 1e3:.1f} ms = {slot[0].units} units")
        return compare(got, twin, key)
    streams = [bs.BusyStream(), bs.BusyStream()]
    for i in range(2):
        order = [streams[i], streams[1 - i]]
        got = run_busy(rig, script, order if two_streams else order[:1], seconds, scribble)
        print(f"{key}, caller stream {i}: host enqueue on the twin {twin[2] * 1e3:.3f} ms, filler {seconds * 1e3:.1f} ms = {order[0].units} units")
        compare(got, twin, f"{key}, caller stream {i}")


def script_of(kind, in_place=False):
    """scenario A's script of one entry point"""
    if kind == "join":
        return [("call", make_call("deferred", 1)), ("premise",), ("join",), ("premise",)]
    if kind == "deferred":
        return [("call", make_call("deferred", 2, in_place=in_place)), ("join",), ("premise",)]
    if kind in ("sync", "scene_sync", "scene2_sync"):
        c = {"sync": "process", "scene_sync": "scene", "scene2_sync": "blended"}[kind]
        return [("call", make_call(c, 3)), ("premise",), ("sync",)]
    if kind == "node":                      # (its outputs are complete behind ohs_node_batch_sync, says the header)
        return [("call", make_call(kind, 4, in_place=in_place)), ("premise",), ("sync",)]
    return [("call", make_call(kind, 4, in_place=in_place)), ("premise",)]


def rig_of(kind, **kw):
    t = RIG_OF.get({"scene_sync": "scene", "scene2_sync": "blended"}.get(kind, kind), "batch")
    return (t, scene_setup() if t in ("scene", "scene2") else batch_setup(**kw))


# ---- A. late input, early reuse: every entry point ------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", sorted(SCENARIO_A))
def test_a_late_input_early_reuse(oracle, entry):
    kind = SCENARIO_A[entry]
    scenario(oracle, f"A {entry}", rig_of(kind), script_of(kind), scribble=False)


@pytest.mark.parametrize("entry", sorted(e for e, k in SCENARIO_A.items() if k in IN_PLACE_KINDS))
def test_a_in_place(oracle, entry):
    kind = SCENARIO_A[entry]
    scenario(oracle, f"A {entry} in place", rig_of(kind), script_of(kind, in_place=True), scribble=False)


@pytest.mark.parametrize("taps,plan,blocks,eq,family", [(1300, 0, BIG, True, "block2048"), (6700, 0, 130, False, "block8192")])
def test_a_long_responses(oracle, taps, plan, blocks, eq, family):
    """the block-2048 family with its tail launches under the six time chunks, and the block-8192 kernel (one launch of 130 blocks)"""
    key = f"A ohs_batch_process, {taps} taps"
    script = [("call", make_call("process", 5, blocks=blocks))]
    if taps == bm.LONG_TAPS:                # (a second call continues the first one's per-path tails)
        script.append(("call", make_call("process", 6, blocks=blocks)))
    script.append(("premise",))
    scenario(oracle, key, ("batch", batch_setup(taps, plan, eq)), script)
    assert _twins[key][1][-1][0][0] == family, _twins[key][1][-1]


# ---- B. rows are the caller's again on return ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", sorted(e for e, k in SCENARIO_A.items() if k in ROW_KINDS))
def test_b_rows_scribbled_on_return(oracle, entry):
    kind = SCENARIO_A[entry]
    scenario(oracle, f"A {entry}", rig_of(kind), script_of(kind), scribble=True)          # (A's twin: the same script)


# ---- C. more calls than staging slots ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", STAGED_KINDS)
def test_c_more_calls_than_staging_slots(oracle, kind):
    """the calls up to the slot count must not block; the next one waits on the host for the slot's last user, and then that call is done"""
    n = bs.staging_slots()
    assert n == 4, "the scenario is six calls over four slots; a new slot count wants a new look at it"
    script = []
    for i in range(n + 2):
        script.append(("call", make_call(kind, 10 + i, blocks=SMALL)))
        if i == n - 1:
            script.append(("premise",))
        if i >= n:
            script.append(("fired", i - n))
    scenario(oracle, f"C {kind}", rig_of(kind), script)


# ---- D. by-value setters between queued calls ---------------------------------------------------------------------------------------------
def test_d_by_value_setters_between_queued_calls(oracle):
    """every call leaves with the gain, bands, EQ switch, flush mode and plan in force when it was MADE"""
    band = bm.make_tables(seed=12)[0][2, 4]
    sets = [("set_gain", (0.55,)), ("set_band_coeffs", (4, band, True)), ("set_eq_enabled", (False,)), ("set_flush_denormals", (1,)),
            ("set_conv_plan", (1,))]
    script = [("call", make_call("process", 20)), ("premise",)]
    for i, (name, args) in enumerate(sets):
        script += [("set", name, args), ("call", make_call("process", 21 + i)), ("premise",)]
    key = "D by-value setters"
    scenario(oracle, key, ("batch", batch_setup(plan=2)), script)
    families = [r[0][0] for r in _twins[key][1]]
    assert families[-1] == "block512_p1" and families[-2] == "hop1536_p1", families         # the plan change is visible in the records


# ---- E. device-table setters behind queued work -------------------------------------------------------------------------------------------
E_CASES = {
    "set_ir": ("process", lambda: ("set_ir", (1, bm._sets(2, TAPS, 5)[1][1]))),
    "reset": ("process", lambda: ("reset", ())),
    "set_schedule_tables": ("scheduled_streams", lambda: ("set_schedule_tables", bm.make_tables(seed=12))),
    "set_schedule_irs": ("ir_crossfaded", lambda: ("set_schedule_irs", (bm._sets(bm.N_CHOICES, TAPS, 8),))),
    "set_layout_irs": ("layout", lambda: ("set_layout_irs", (bm._layouts(1, K, TAPS, 5)[0],))),
    "set_layout_table": ("layout_scheduled", lambda: ("set_layout_table", (bm._layouts(bm.N_CHOICES, K, TAPS, 6),))),
    "ohs_scene_set_direction_irs": ("scene", lambda: ("set_directions", (_dirs(seed=12),))),
}


@pytest.mark.parametrize("setter", sorted(E_CASES))
def test_e_device_table_setter_waits_for_queued_work(oracle, setter):
    """still busy in front of the setter, drained behind it; the queued call has the old tables' bits, the next one the new ones"""
    kind, make = E_CASES[setter]
    name, args = make()
    script = [("call", make_call(kind, 30)), ("premise",), ("set", name, args), ("drained",), ("call", make_call(kind, 31))]
    scenario(oracle, f"E {setter}", rig_of(kind), script)


def test_e_stream_band_upload_waits_in_the_next_call(oracle):
    """a per-stream EQ band is host state until the next processing call uploads it, and THAT call waits for its stream"""
    band = bm.make_tables(seed=12)[0][1, 3]
    script = [("call", make_call("process", 32)), ("set", "set_stream_band_coeffs", (2, 3, band, True)), ("premise",),
              ("call", make_call("process", 33)), ("drained",)]
    scenario(oracle, "E set_stream_band_coeffs", rig_of("process"), script)


# ---- F. two caller streams, one signal ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["process", "ir_crossfaded", "layout_scheduled", "deferred_then_plain", "deferred_join_on_b"])
def test_f_one_handle_moved_between_two_streams(oracle, case):
    """call 1 on A behind the filler, B made to wait for A, call 2 on B continues the signal; a deferred call on A is joined by the
    library in front of the next call on B, or by ohs_batch_join on B alone"""
    if case == "deferred_then_plain":
        # (a call of another geometry: with the deferred call's buffers it would overwrite the output this scenario reads behind it)
        script = [("call", make_call("deferred", 40)), ("on", 1, True), ("call", make_call("process", 41, blocks=SMALL)), ("premise",)]
    elif case == "deferred_join_on_b":
        script = [("call", make_call("deferred", 42)), ("on", 1, False), ("join",), ("premise",)]
    else:
        script = [("call", make_call(case, 43)), ("on", 1, True), ("call", make_call(case, 44)), ("premise",)]
    scenario(oracle, f"F {case}", rig_of(case if case in RIG_OF else "process"), script, two_streams=True)


# ---- G. the deferred pipeline under load --------------------------------------------------------------------------------------------------
def test_g_deferred_pipeline_under_load(oracle):
    """three deferred calls back to back on the same buffers wait chunk by chunk for one another (only the last output survives: it
    carries the EQ state and the overlaps of the first two); then a deferred call and a call of another geometry, which joins fully"""
    script = [("call", make_call("deferred", 50, observe=False)), ("call", make_call("deferred", 51, observe=False)),
              ("call", make_call("deferred", 52)), ("join",), ("call", make_call("deferred", 53)),
              ("call", make_call("process", 54, blocks=SMALL)), ("premise",)]
    scenario(oracle, "G deferred pipeline", rig_of("process"), script)


# ---- H. the sync calls ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["deferred", "node"])
def test_h_sync_waits_for_the_stream_and_a_pending_deferred_call(oracle, kind):
    """(ohs_batch_sync behind a plain call, ohs_scene_sync and ohs_scene2_sync run under A) behind the sync call the filler's event
    and the event recorded behind the call have fired, and the output is complete"""
    script = [("call", make_call(kind, 60)), ("premise",), ("sync",)]
    scenario(oracle, f"H {kind}", rig_of(kind), script)


# ---- I. the harness can fail ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrong", ["producer", "consumer"])
def test_i_a_wrong_caller_is_reported_as_a_mismatch(oracle, wrong):
    """A deliberately wrong CALLER, never a wrong library: the producer copy (or the copy-out) is queued on a second side stream with no
    event between the two.  No memory is freed or out of range: the call (or the copy) reads the NaN the buffer still holds, a wrong
    value, which must come out as DataMismatch -- not as a pass, and not as a PremiseError."""
    import torch
    rig, script = rig_of("process"), script_of("process")
    twin = twin_of(oracle, "A ohs_batch_process", rig, script)
    busy = bs.BusyStream()
    seconds = bs.filler_seconds(twin[2])

    def pick():
        """the first of up to four fresh streams on which a marker event completes while the caller's stream is still busy"""
        for _ in range(4):
            st, ev = torch.cuda.Stream(), torch.cuda.Event()
            ev.record(st)
            t0 = time.perf_counter()
            while not ev.query() and busy.still_busy() and time.perf_counter() - t0 < 0.005:
                pass
            if ev.query() and busy.still_busy():
                return st
        raise AssertionError("no second stream ran beside the busy one: a marker event completed on none of four fresh streams while "
                             "the caller's stream was still busy")

    with pytest.raises(bs.DataMismatch) as e:
        compare(run_busy(rig, script, [busy], seconds, True, (wrong, pick)), twin, f"I wrong {wrong}")
    print(f"I wrong {wrong}: reported as {e.value}")
    assert "NaN" in str(e.value)

"""The batch handle's contract (include/ohs_hip.h) as ONE host model, and the generator of the call sequences that
tests/test_gpu_fuzz_call_kinds.py drives the library through.  Pure numpy plus the CPU oracle; checked by
tests/test_cpu_batch_model.py.

The seven call kinds of a handle share state, and the header says how:

    EQ        one StereoParametricEQ per stream (the oracle's: pinned in bits).  Stereo kinds run it IN FRONT of the convolution,
              layout kinds BEHIND it, on the same per-stream state.  A table is refreshed per segment and stream with
              set_band_coeffs: five constants and the enabled flag replaced, s1 / s2 kept.
    stereo    the handle's four responses, the table of HRIR sets, per-path tails [S][4][512] in f64 (render_f64 of
              tests/test_cpu_ir_schedule.py).  set_ir(path) zeroes that path's tail of every stream and keeps the other three.
    layout    the single layout, the table of layouts, ONE overlap [S][2][512] in f64, before the gain; independent of the stereo tails.
    adoption  a shared row is adopted into the handle (the last segment's table and gain, or HRIR set); rows per stream adopt nothing.
    reset     zeroes EQ state, stereo tails and layout overlap; tables and responses stay.
    refusals  process_scheduled (and table rows of process_scheduled_streams) on static per-stream tables; either IR kind on a handle
              whose own responses exceed one partition.  A refused call changes nothing.

Every stereo method returns gain_k * render(e) in f64, e = the oracle EQ of x in f32 bits (x itself with the EQ disabled).  A layout
method returns the DRY f64 signal gain * conv(x); HandleModel.layout_eq then pushes a float32 dry signal -- the GPU's own, in the GPU
test -- through the streams' EQ instances, which is what the call's output must equal bit for bit.

Handles whose own responses are longer than one partition keep what every stream was fed since the last reset instead of tails: a
path's output is the f64 convolution of that history from the path's last set_ir on (oracle.binaural_f64 over everything, computed
over the window the call's frames can see).

`broken` names ONE rule to break (RULES): the mutants tests/test_cpu_batch_model.py uses to show that a check at the bar sees each.

sequence(seed) is the generator: 14 calls whose kinds are a window of an Euler circuit over all ordered pairs of kinds (the default
seeds' windows cover the circuit), one of the handle's setters in turn between two calls, the refusals where the handle's state asks
for them, and per call its rows, gains, switch mode, `prev`, plan and buffer form.  The GPU test's per-block metric asks every block
of the reference for an RMS of 0.01, so the generator knows how loud its responses are (first_block_level) and draws every gain
between the floor that condition sets (gain_floor; never below 0.3) and 1 -- and a channel count out of {1, 3, 6} that some gain
below 0.9 serves: six channels come with 200 taps only, make_layout's L1 normalisation leaves six times 512 taps too quiet.  For the
same reason the EQ tables are variants of synth.eq_table (gains of a few dB), not tables with shelves of up to 9 dB.
"""
import functools

import numpy as np

from tests.test_cpu_ir_crossfade import model_ir_crossfade
from tests.test_cpu_ir_schedule import BLOCK, CUT, RING_OUT, make_sets, model_ir_schedule, render_f64
from tests.test_cpu_layout import make_input
from tests.test_cpu_layout_schedule import make_table, model_layout_schedule_f64

KINDS = ("process", "scheduled", "scheduled_streams", "ir_scheduled", "ir_crossfaded", "layout", "layout_scheduled")
STEREO_KINDS, LAYOUT_KINDS, IR_KINDS = KINDS[:5], KINDS[5:], KINDS[3:5]
LONG_KINDS = ("process", "scheduled", "scheduled_streams", "layout", "layout_scheduled")      # what a handle with long responses serves
# (in the order the generator takes them between calls: static per-stream tables live for six calls, or until a call they refuse)
SETTERS = ("set_stream_band_coeffs", "set_ir", "set_band_coeffs", "set_gain", "set_eq_enabled", "set_schedule_tables",
           "share_eq_table", "set_schedule_irs", "set_layout_irs", "set_layout_table", "reset")
REFUSED = "refused"
RULES = ("eq_not_shared", "layout_overlap_shared", "no_adoption", "adopt_per_stream", "set_ir_drops_all", "reset_keeps_layout",
         "cut_start_no_boundary", "prev_ignored", "layout_eq_in_front")
NB = 10
N_CHOICES = 4           # EQ tables, HRIR sets and layouts per table
LONG_TAPS = 1300
EAR, SRC = (0, 1, 0, 1), (0, 0, 1, 1)       # path -> the ear it feeds, the speaker signal it reads


def n_segments(n_blocks, seg_blocks):
    return -(-int(n_blocks) // int(seg_blocks))


class HandleModel:
    def __init__(self, oracle, S, num_bands=NB, broken=None):
        from open_headstage_amd import synth
        assert broken is None or broken in RULES, broken
        self.oracle, self.S, self.nb, self.broken = oracle, int(S), int(num_bands), broken
        self.eqs = [oracle.StereoParametricEQ(self.nb, synth.FS) for _ in range(self.S)]
        # (the mutant whose layout calls have an EQ state of their own)
        self.eqs_layout = [oracle.StereoParametricEQ(self.nb, synth.FS) for _ in range(self.S)] if broken == "eq_not_shared" else self.eqs
        c0, e0 = zip(*[self.eqs[0].get_band_coeffs(b) for b in range(self.nb)])     # a fresh handle's table: the reference's defaults
        self.shared = (np.array(c0, np.float32), np.array(e0, bool))
        self.stream_tabs = None                 # static per-stream tables ([S][nb][5], [S][nb]) once a stream has a band of its own
        self.sched_tabs = None                  # (coeffs [n][nb][5], enabled [n][nb])
        self.gain, self.eq_enabled = 1.0, False
        self.irs = [np.zeros(1, np.float32) for _ in range(4)]      # (a fresh handle's paths are mute)
        self.sets = None
        self.tails = np.zeros((self.S, 4, BLOCK))
        self.fed = np.zeros((self.S, 2, 0), np.float32)             # long responses: the EQ'd input since the last reset ...
        self.since = [0, 0, 0, 0]                                   # ... and where each path's history begins in it
        self.layout_irs = self.layout_table = None
        self.lay_ov = np.zeros((self.S, 2, BLOCK))
        self._eq_pending = False                # a layout call's EQ has still to run (layout_eq)

    # ---- setters ----------------------------------------------------------------------------------------------------------------
    @property
    def long(self):
        return max(len(h) for h in self.irs) > BLOCK

    def set_ir(self, path, ir):
        ir = np.ascontiguousarray(ir, np.float32).ravel()
        was_long = self.long
        self.irs[path] = ir if ir.size else np.zeros(1, np.float32)
        if (was_long != self.long) and (self.fed.shape[2] or self.tails.any()):
            raise NotImplementedError("a handle that changes between one and several partitions in mid-stream is outside this model")
        self.since[path] = self.fed.shape[2]
        self.tails[:, range(4) if self.broken == "set_ir_drops_all" else path] = 0.0

    def set_band_coeffs(self, band, coeffs, enabled):
        self.shared[0][band], self.shared[1][band] = coeffs, bool(enabled)
        if self.stream_tabs is not None:        # the shared call sets the band of EVERY stream
            self.stream_tabs[0][:, band], self.stream_tabs[1][:, band] = coeffs, bool(enabled)

    def set_stream_band_coeffs(self, stream, band, coeffs, enabled):
        if self.stream_tabs is None:            # the first such call gives every stream a copy of the shared table
            self.stream_tabs = (np.stack([self.shared[0]] * self.S), np.stack([self.shared[1]] * self.S))
        self.stream_tabs[0][stream, band], self.stream_tabs[1][stream, band] = coeffs, bool(enabled)

    def share_eq_table(self):
        self.stream_tabs = None

    def set_gain(self, gain):
        self.gain = float(np.float32(gain))

    def set_eq_enabled(self, on):
        self.eq_enabled = bool(on)

    def set_schedule_tables(self, coeffs, enabled):
        self.sched_tabs = (np.array(coeffs, np.float32), np.array(enabled, bool))

    def set_schedule_irs(self, sets):
        self.sets = np.array(sets, np.float32)

    def set_layout_irs(self, irs):
        self.layout_irs = np.array(irs, np.float32)
        self.lay_ov[:] = 0.0

    def set_layout_table(self, table):
        self.layout_table = np.array(table, np.float32)
        self.lay_ov[:] = 0.0

    def reset(self):
        for q in set(self.eqs) | set(self.eqs_layout):
            q.reset_all_bands_state()
        self.tails[:] = 0.0
        self.fed = np.zeros((self.S, 2, 0), np.float32)
        self.since = [0, 0, 0, 0]
        if self.broken != "reset_keeps_layout":
            self.lay_ov[:] = 0.0

    # ---- the EQ -----------------------------------------------------------------------------------------------------------------
    def _table_of(self, s):
        """the handle's own table for stream s -> (coeffs [nb][5], enabled [nb])"""
        return (self.stream_tabs[0][s], self.stream_tabs[1][s]) if self.stream_tabs is not None else self.shared

    @staticmethod
    def _refresh(q, table):
        for b in range(table[0].shape[0]):
            q.set_band_coeffs(b, table[0][b], bool(table[1][b]))

    def _eq(self, eqs, x, seg_blocks=None, rows=None):
        """x [S][2][frames] float32 through the streams' EQ instances; rows [S][n_segs]: the schedule table per stream and segment
        (None: the handle's own table(s), refreshed once) -> float32, x's own bits where the EQ is disabled"""
        x = np.ascontiguousarray(x, np.float32)
        if not self.eq_enabled:
            return x.copy()
        n = x.shape[2] // BLOCK
        seg = n if rows is None else int(seg_blocks)
        e = np.empty_like(x)
        for s, q in enumerate(eqs):
            for k, b0 in enumerate(range(0, n, seg)):
                table = self._table_of(s) if rows is None else (self.sched_tabs[0][rows[s][k]], self.sched_tabs[1][rows[s][k]])
                self._refresh(q, table)
                sl = slice(b0 * BLOCK, min(b0 + seg, n) * BLOCK)
                l, r = x[s, 0, sl].copy(), x[s, 1, sl].copy()
                q.process_block(l, r)
                e[s, 0, sl], e[s, 1, sl] = l, r
        return e

    def layout_eq(self, d):
        """what a layout call returns for the dry signal d [S][2][frames] float32: the handle's EQ, on the state the stereo calls share"""
        assert self._eq_pending, "layout_eq follows a layout call"
        self._eq_pending = False
        if self.broken == "layout_eq_in_front":
            return np.array(d, np.float32)
        return self._eq(self.eqs_layout, d)

    # ---- the stereo kinds -------------------------------------------------------------------------------------------------------
    def _rows(self, a, n_segs, dtype):
        """a schedule's rows as [S][n_segs], and whether it was ONE row for all streams"""
        a = np.asarray(a, dtype)
        assert a.shape[-1] >= n_segs and (a.ndim == 1 or a.shape[0] == self.S), a.shape
        return np.broadcast_to(a[..., :n_segs], (self.S, n_segs)), a.ndim == 1

    def _conv_own(self, e):
        """e through the handle's four responses, continuing the stereo state -> y f64 before the gain"""
        if not self.long:
            y, self.tails = render_f64(self.oracle, e, lambda s, t: self.irs, None, self.tails)
            return y
        pos, frames = self.fed.shape[2], e.shape[2]
        self.fed = np.concatenate([self.fed, e], axis=2)
        y = np.zeros((self.S, 2, frames))
        for p, h in enumerate(self.irs):
            start = max(self.since[p], pos - (len(h) - 1))
            for s in range(self.S):
                y[s, EAR[p]] += self.oracle.direct_conv_f64(np.ascontiguousarray(self.fed[s, SRC[p], start:]), h)[pos - start:]
        return y

    def _gained(self, y, seg_blocks, gains):
        """gains [S][n_segs] (None: the handle's gain) applied per segment"""
        if gains is None:
            return self.gain * y
        out = np.empty_like(y)
        for k in range(gains.shape[1]):
            sl = slice(k * seg_blocks * BLOCK, (k + 1) * seg_blocks * BLOCK)
            out[:, :, sl] = gains[:, k, None, None].astype(np.float64) * y[:, :, sl]
        return out

    def _begin(self):
        assert not self._eq_pending, "the previous layout call's layout_eq has not run"

    def process(self, x):
        self._begin()
        return self.gain * self._conv_own(self._eq(self.eqs, x))

    def _eq_scheduled(self, x, seg_blocks, table_idx, gains, adopt):
        n_segs = n_segments(x.shape[2] // BLOCK, seg_blocks)
        rows, one_t = (None, True) if table_idx is None else self._rows(table_idx, n_segs, np.int64)
        g, one_g = (None, True) if gains is None else self._rows(gains, n_segs, np.float32)
        y = self._gained(self._conv_own(self._eq(self.eqs, x, seg_blocks, rows)), seg_blocks, g)
        if adopt:                               # the last segment's table and gain ARE the handle's now, as if the setters had been called
            if rows is not None:
                t = int(rows[0, -1])
                for b in range(self.nb):
                    self.set_band_coeffs(b, self.sched_tabs[0][t, b], self.sched_tabs[1][t, b])
            if g is not None:
                self.set_gain(g[0, -1])
        return y

    def process_scheduled(self, x, seg_blocks, table_idx=None, gains=None):
        self._begin()
        if self.stream_tabs is not None:
            return REFUSED
        assert (table_idx is None or np.ndim(table_idx) == 1) and (gains is None or np.ndim(gains) == 1)
        return self._eq_scheduled(x, seg_blocks, table_idx, gains, adopt=self.broken != "no_adoption")

    def process_scheduled_streams(self, x, seg_blocks, table_idx=None, gains=None):
        self._begin()
        if table_idx is not None and self.stream_tabs is not None:
            return REFUSED
        return self._eq_scheduled(x, seg_blocks, table_idx, gains, adopt=self.broken == "adopt_per_stream")

    def _adopt_set(self, rows, shared):
        if (shared and self.broken != "no_adoption") or (not shared and self.broken == "adopt_per_stream"):
            self.irs = [np.array(h) for h in self.sets[int(rows[0, -1])]]

    def process_ir_scheduled(self, x, seg_blocks, ir_idx, mode=RING_OUT):
        self._begin()
        if self.long:
            return REFUSED
        mode = {"ring_out": RING_OUT, "cut": CUT}.get(mode, mode)
        rows, shared = self._rows(ir_idx, n_segments(x.shape[2] // BLOCK, seg_blocks), np.int64)
        e = self._eq(self.eqs, x)
        if mode == CUT and self.broken == "cut_start_no_boundary":
            def drop(s, t):
                k = t // seg_blocks
                return range(4) if (t % seg_blocks == 0 and k > 0 and rows[s, k] != rows[s, k - 1]) else ()
            y, self.tails = render_f64(self.oracle, e, lambda s, t: self.sets[int(rows[s, t // seg_blocks])], drop, self.tails)
        else:
            y, self.tails = model_ir_schedule(self.oracle, e, self.sets, rows, seg_blocks, mode, self.tails)
        self._adopt_set(rows, shared)
        return self.gain * y

    def process_ir_crossfaded(self, x, seg_blocks, ir_idx, prev_idx=None):
        self._begin()
        if self.long:
            return REFUSED
        rows, shared = self._rows(ir_idx, n_segments(x.shape[2] // BLOCK, seg_blocks), np.int64)
        if self.broken == "prev_ignored":
            prev_idx = None
        y, self.tails = model_ir_crossfade(self.oracle, self._eq(self.eqs, x), self.sets, rows, seg_blocks, prev_idx, self.tails)
        self._adopt_set(rows, shared)
        return self.gain * y

    # ---- the layout kinds: the dry signal; layout_eq is the rest -----------------------------------------------------------------
    def _layout(self, x, table, idx, seg_blocks, prev, crossfade):
        self._begin()
        x = np.ascontiguousarray(x, np.float32)
        if self.broken == "layout_eq_in_front":         # the mutant: the stereo chain's order, the channels in pairs through the EQ
            x = x.copy()
            for c in range(0, x.shape[1], 2):
                pair = np.stack([x[:, c], x[:, min(c + 1, x.shape[1] - 1)]], axis=1)
                x[:, c:c + 2] = self._eq(self.eqs, pair)[:, :x.shape[1] - c]
        if self.broken == "layout_overlap_shared":      # the mutant: the layout calls add, and leave, the stereo calls' overlap
            tail_in = np.stack([self.tails[:, 0] + self.tails[:, 2], self.tails[:, 1] + self.tails[:, 3]], axis=1)
        else:
            tail_in = self.lay_ov
        if self.broken == "prev_ignored":
            prev = None
        y, tail = model_layout_schedule_f64(self.oracle, x, table, idx, seg_blocks, prev, crossfade, 1.0, tail_in, with_tail=True)
        if self.broken == "layout_overlap_shared":
            self.tails[:, :2], self.tails[:, 2:] = tail, 0.0
        else:
            self.lay_ov = tail
        self._eq_pending = True
        return self.gain * y

    def process_layout(self, x):
        return self._layout(x, self.layout_irs[None], np.zeros(1, np.int64), x.shape[2] // BLOCK, None, False)

    def process_layout_scheduled(self, x, idx, seg_blocks, prev=None, crossfade=True):
        idx = np.asarray(idx, np.int64)
        n_segs = n_segments(x.shape[2] // BLOCK, seg_blocks)
        return self._layout(x, self.layout_table, idx[..., :n_segs], seg_blocks, prev, crossfade)

    def layout_final(self, dry):
        """for the CPU tests: the call's output with the model's own dry signal rounded to float32"""
        return self.layout_eq(np.asarray(dry, np.float32))


# ---- the inputs: responses, tables, signals -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_tables(n_tables=N_CHOICES, nb=NB, seed=11):
    """n_tables variants of synth.eq_table (its ten bands: a low shelf, eight peaks, a high shelf), every centre frequency, Q and gain
    moved a little per table and seed so that all coefficients differ (what tests/test_gpu_schedule.py's _tables is there for), every
    band enabled; the gains stay within a few dB, so that white noise leaves the cascade at about the level it entered
    -> (coeffs [n][nb][5] float32, enabled [n][nb] bool)"""
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    rng = np.random.default_rng(seed)
    bands = synth.eq_table()
    assert len(bands) == nb
    coeffs = np.zeros((n_tables, nb, 5), np.float32)
    for t in range(n_tables):
        for b, band in enumerate(bands):
            fc = band.center_freq * 2.0 ** (0.06 * t + 0.01 * (seed % 7) - 0.1)
            coeffs[t, b] = ohs.biquad_coefficients(band.filter_type, synth.FS, fc, band.q * (1.0 + 0.08 * t),
                                                   band.gain_db + float(rng.uniform(-1.5, 1.5)))
    flat = coeffs.reshape(-1, 5)
    assert len({tuple(r) for r in flat.view(np.uint32).tolist()}) == flat.shape[0]
    coeffs.setflags(write=False)
    return coeffs, np.ones((n_tables, nb), bool)


@functools.lru_cache(maxsize=None)
def long_irs(seed, n=2):
    """n sets of four responses of LONG_TAPS taps [n][4][LONG_TAPS] for a handle's OWN paths: make_sets' recipe (decaying noise, a direct
    tap per path, L1-normalised per ear) with a decay of 300 frames, so that a block from rest is not much quieter than the others and
    the third partition still carries 3 % of the first one's amplitude"""
    rng = np.random.default_rng(1000 + seed)
    k = np.arange(LONG_TAPS, dtype=np.float64)
    out = np.zeros((n, 4, LONG_TAPS), np.float32)
    for i in range(n):
        hs = []
        for p, (d, g) in enumerate([(30, 1.0), (45, 0.4), (45, 0.4), (30, 1.0)]):
            h = 0.5 * rng.standard_normal(LONG_TAPS) * np.exp(-k / 300.0)
            h[d + 3 * i + p] += 3.0
            hs.append(g * h)
        nl, nr = np.abs(hs[0]).sum() + np.abs(hs[2]).sum(), np.abs(hs[1]).sum() + np.abs(hs[3]).sum()
        for p, nrm in enumerate([nl, nr, nl, nr]):
            out[i, p] = (hs[p] / nrm).astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _sets(n, taps, seed):
    a = make_sets(n, taps, seed)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _layouts(n, K, taps, seed):
    a = make_table(n, K, taps, seed)
    a.setflags(write=False)
    return a


def own_irs(spec, seed):
    """the two sets [2][4][taps] a handle's own paths are loaded from"""
    return long_irs(seed) if spec["long"] else _sets(2, spec["taps"], seed)


# ---- how loud the quietest block of a call's reference is ---------------------------------------------------------------------
# The per-block metric of the GPU test is relative, and it asks every block of the reference for an RMS of 0.01.  The quietest
# blocks are those that start from rest (a fresh handle, a reset, CUT, a new layout): only the head of the response has arrived.  For
# white noise of RMS 1 / sqrt(3) their expected RMS follows from the responses; the generator draws a call's gains above the floor
# that keeps it at LEVEL_TARGET, a quarter above the condition for the block-to-block spread of filtered noise.
NOISE_RMS = 3.0 ** -0.5
LEVEL_TARGET = 0.0125
EQ_FACTOR = 0.78        # the tables of make_tables on white noise: the high shelf's -3 dB over most of the band
FADE_FACTOR = 0.8       # a fading block: x f through one set and x g through another, sqrt(2 / 3) of the energy


def first_block_level(ears):
    """ears: per ear the responses that sum into it -> the expected RMS of the first block from rest, the quieter ear's"""
    def energy(h):
        h2 = np.zeros(BLOCK)
        m = min(len(h), BLOCK)
        h2[:m] = np.asarray(h[:m], np.float64) ** 2
        return float(np.mean(np.cumsum(h2)))
    return NOISE_RMS * min(np.sqrt(sum(energy(h) for h in ear)) for ear in ears)


def stereo_level(sets):
    """the quietest set of sets [...][4][taps]"""
    a = np.asarray(sets).reshape(-1, 4, np.shape(sets)[-1])
    return min(first_block_level([[h[0], h[2]], [h[1], h[3]]]) for h in a)


def layout_level(layouts):
    """the quietest layout of layouts [...][K][2][taps]"""
    a = np.asarray(layouts)
    a = a.reshape((-1,) + a.shape[-3:])
    return min(first_block_level([list(h[:, 0]), list(h[:, 1])]) for h in a)


def gain_floor(level, eq=False, fade=False):
    return LEVEL_TARGET / (level * (EQ_FACTOR if eq else 1.0) * (FADE_FACTOR if fade else 1.0))


def stereo_input(spec, op):
    from open_headstage_amd import synth
    return synth.white_noise(range(op["x_seed"], op["x_seed"] + spec["S"]), op["blocks"] * BLOCK)


def layout_input(spec, op):
    return make_input(spec["S"], op["K"], op["blocks"], seed=op["x_seed"])


def call_input(spec, op):
    return layout_input(spec, op) if op["kind"] in LAYOUT_KINDS else stereo_input(spec, op)


def setter_args(spec, op):
    """the arrays a setter op stands for -> the positional arguments of HandleModel.<op> and BatchProcessor.<op>"""
    name, taps = op["op"], spec["taps"]
    if name == "set_ir":
        return (op["path"], own_irs(spec, op["seed"])[op["which"], op["path"]])
    if name in ("set_band_coeffs", "set_stream_band_coeffs"):
        c = make_tables(seed=op["seed"])[0][op["table"], op["band"]]
        return ((op["stream"],) if name == "set_stream_band_coeffs" else ()) + (op["band"], c, op["enabled"])
    if name == "set_gain":
        return (op["gain"],)
    if name == "set_eq_enabled":
        return (op["on"],)
    if name == "set_conv_plan":
        return (op["plan"],)
    if name == "set_schedule_tables":
        return make_tables(seed=op["seed"])
    if name == "set_schedule_irs":
        return (_sets(N_CHOICES, taps, op["seed"]),)
    if name == "set_layout_irs":
        return (_layouts(1, op["K"], taps, op["seed"])[0],)
    if name == "set_layout_table":
        return (_layouts(N_CHOICES, op["K"], taps, op["seed"]),)
    assert name in ("share_eq_table", "reset"), name
    return ()


def model_setter(model, spec, op):
    if op["op"] != "set_conv_plan":             # (which kernel serves a call is no part of the contract's arithmetic)
        getattr(model, op["op"])(*setter_args(spec, op))


def model_call(model, op, x):
    """one call op on the model -> REFUSED or the f64 expectation (layout kinds: the dry signal; layout_eq has still to run)"""
    k, a = op["kind"], op
    if k == "process":
        return model.process(x)
    if k == "scheduled":
        return model.process_scheduled(x, a["seg"], a["table_idx"], a["gains"])
    if k == "scheduled_streams":
        return model.process_scheduled_streams(x, a["seg"], a["table_idx"], a["gains"])
    if k == "ir_scheduled":
        return model.process_ir_scheduled(x, a["seg"], a["idx"], a["mode"])
    if k == "ir_crossfaded":
        return model.process_ir_crossfaded(x, a["seg"], a["idx"], a["prev"])
    if k == "layout":
        return model.process_layout(x)
    assert k == "layout_scheduled", k
    return model.process_layout_scheduled(x, a["idx"], a["seg"], a["prev"], a["crossfade"])


def run_model(model, spec, ops=None):
    """the whole sequence on the model -> [(op, expectation)] per call op (layout kinds: the final output with the model's own dry
    signal, layout_final)"""
    out = []
    for op in spec["ops"] if ops is None else ops:
        if op["op"] != "call":
            model_setter(model, spec, op)
            continue
        y = model_call(model, op, call_input(spec, op))
        if y is not REFUSED and op["kind"] in LAYOUT_KINDS:
            y = model.layout_final(y)
        out.append((op, y))
    return out


# ---- the generator --------------------------------------------------------------------------------------------------------------
def euler_circuit(n):
    """a closed walk over the complete directed graph on n nodes, loops included, that takes every one of the n * n ordered pairs
    exactly once (Hierholzer) -> n * n + 1 nodes, the last one the first"""
    unused = {a: list(range(n)) for a in range(n)}
    stack, out = [0], []
    while stack:
        a = stack[-1]
        if unused[a]:
            stack.append(unused[a].pop())
        else:
            out.append(stack.pop())
    out.reverse()
    assert len(out) == n * n + 1 and out[0] == out[-1] and len(set(zip(out, out[1:]))) == n * n
    return out


DEFAULT_SEEDS = 8
CALLS_PER_SEED = 14
BLOCK_CHOICES = (1, 2, 3, 5, 9, 17, 40, 70)
SEG_CHOICES = (1, 2, 3, 5)
MAX_BLOCKS = 200


def is_long_seed(seed):
    """two of every eight seeds give the handle own responses of LONG_TAPS taps"""
    return seed % 4 == 3


def is_wide_seed(seed):
    """one of every eight seeds has 9 .. 20 streams"""
    return seed % 8 == 5


def kind_walk(seed):
    """the seed's call kinds: CALLS_PER_SEED consecutive nodes of the Euler circuit over the kinds the seed's handle serves, the
    seeds' windows staggered so that the default seeds together take every ordered pair"""
    if is_long_seed(seed):
        kinds, rank, step = LONG_KINDS, seed // 4, 12
    else:
        kinds, rank, step = KINDS, seed - (seed + 1) // 4, 9
    circuit = euler_circuit(len(kinds))[:-1]
    return [kinds[circuit[(rank * step + i) % len(circuit)]] for i in range(CALLS_PER_SEED)]


def _varying_row(rng, n_segs, n_choices=N_CHOICES):
    """a row of indices that changes at every segment but (now and then) one"""
    row = np.zeros(n_segs, np.int64)
    row[0] = rng.integers(0, n_choices)
    for k in range(1, n_segs):
        row[k] = (row[k - 1] + rng.integers(1, n_choices)) % n_choices if rng.random() < 0.85 else row[k - 1]
    return row


def _rows(rng, S, n_segs, shared):
    return _varying_row(rng, n_segs) if shared else np.stack([_varying_row(rng, n_segs) for _ in range(S)])


def sequence(seed):
    """-> spec: {seed, S, taps, long, ops}.  ops: setters {"op": <HandleModel method>, ...} (setter_args gives their arrays) and
    calls {"op": "call", "kind", "blocks", "x_seed", "io", ...the call's arguments, "refused"}.  Deterministic in `seed`."""
    rng = np.random.default_rng(31000 + seed)
    long_, wide = is_long_seed(seed), is_wide_seed(seed)
    S = int(rng.integers(9, 21)) if wide else int(rng.integers(1, 7))
    taps = int(rng.choice([512, 200]))
    spec = {"seed": seed, "S": S, "taps": taps, "long": long_, "nb": NB}
    kinds = kind_walk(seed)
    # block counts: one stereo call of 70 blocks (EQ on: the overlapped EQ || convolution path), the others short enough for the budget
    big = next(i for i, k in enumerate(kinds) if k in STEREO_KINDS and i >= 2)
    pool = (1, 2, 3, 5) if wide else BLOCK_CHOICES[:-1]
    blocks = [int(rng.choice(pool)) for _ in kinds]
    blocks[big] = 70
    while sum(blocks) > MAX_BLOCKS:
        i = max((i for i in range(len(blocks)) if i != big), key=lambda i: blocks[i])
        blocks[i] = BLOCK_CHOICES[BLOCK_CHOICES.index(blocks[i]) - 1]

    ops = []
    # what the generator has to know of the handle: whether static per-stream tables are in force, the gain (adoption included), the
    # EQ switch, and how loud the responses in force are (gain_floor)
    state = {"per_stream": False, "gain": None, "eq": False, "seeds": 0, "K1": 0, "K2": 0,
             "own": stereo_level(own_irs(spec, 50 + seed)), "sets": 0.0, "lay1": 0.0, "lay2": 0.0}

    def fresh():
        state["seeds"] += 1
        return 7 * seed + state["seeds"]

    def pick_k(n_sets, lay_seed, fade):
        """a channel count out of {1, 3, 6} whose layouts are loud enough for a gain below 0.9 (at 512 taps six channels are not)"""
        for K in rng.permutation([1, 3, 6]):
            level = layout_level(_layouts(n_sets, int(K), taps, lay_seed))
            if gain_floor(level, False, fade) <= 0.9:
                return int(K), level
        raise AssertionError("no channel count is loud enough")

    def setter(name, **kw):
        op = {"op": name}
        if name == "set_ir":
            op.update(path=int(rng.integers(0, 4)), seed=50 + seed, which=1)
        elif name in ("set_band_coeffs", "set_stream_band_coeffs"):
            op.update(band=int(rng.integers(0, NB)), table=int(rng.integers(0, N_CHOICES)), seed=23 + int(rng.integers(0, 3)),
                      enabled=bool(rng.random() < 0.8))
            if name == "set_stream_band_coeffs":
                op["stream"] = int(rng.integers(0, S))
                state["per_stream"] = True
        elif name == "share_eq_table":
            state["per_stream"] = False
        elif name == "set_gain":
            op["gain"] = state["gain"] = float(np.float32(rng.uniform(kw["lo"], 1.0)))
        elif name == "set_eq_enabled":
            op["on"] = state["eq"] = kw["on"] if "on" in kw else bool(rng.random() < 0.75)
        elif name == "set_conv_plan":
            op["plan"] = int(rng.integers(0, 3))
        elif name == "set_schedule_tables":
            op["seed"] = 11 + fresh()
        elif name == "set_schedule_irs":
            op["seed"] = 11 + fresh()
            state["sets"] = stereo_level(_sets(N_CHOICES, taps, op["seed"]))
        elif name == "set_layout_irs":
            op["seed"] = fresh()
            op["K"], state["lay1"] = pick_k(1, op["seed"], False)
            state["K1"] = op["K"]
        elif name == "set_layout_table":
            op["seed"] = fresh()
            op["K"], state["lay2"] = pick_k(N_CHOICES, op["seed"], True)
            state["K2"] = op["K"]
        ops.append(op)

    # a fresh handle's setup
    for p in range(4):
        ops.append({"op": "set_ir", "path": p, "seed": 50 + seed, "which": 0})
    for b in range(NB):
        ops.append({"op": "set_band_coeffs", "band": b, "table": 0, "seed": 11 + 7 * seed, "enabled": True})
    for name in ("set_schedule_tables", "set_schedule_irs", "set_layout_irs", "set_layout_table"):
        setter(name)

    def floor_of(kind, fade):
        level = {"layout": state["lay1"], "layout_scheduled": state["lay2"]}.get(kind, min(state["own"], state["sets"]))
        lo = gain_floor(level, state["eq"] and kind in STEREO_KINDS, fade)
        assert lo <= 0.95, (seed, kind, lo)
        return max(0.3, lo)

    def call(kind, n, j, refused=False):
        seg = int(rng.choice(SEG_CHOICES))
        n_segs = n_segments(n, seg)
        op = {"op": "call", "kind": kind, "blocks": n, "seg": seg, "x_seed": 100000 + 4000 * seed + 200 * j + (100 if refused else 0),
              "refused": refused, "io": None}
        shared = bool(rng.random() < 0.5)
        if kind == "ir_scheduled":
            op.update(idx=_rows(rng, S, n_segs, shared), mode=CUT if rng.random() < 0.5 else RING_OUT)
        elif kind == "ir_crossfaded":
            op["idx"] = _rows(rng, S, n_segs, shared)
            op["prev"] = None if rng.random() < 0.4 else (int(rng.integers(0, N_CHOICES)) if shared else rng.integers(0, N_CHOICES, S))
        elif kind == "layout":
            op["K"] = state["K1"]
        elif kind == "layout_scheduled":
            op.update(K=state["K2"], idx=_rows(rng, S, n_segs, shared), crossfade=bool(rng.random() < 0.6))
            op["prev"] = None if rng.random() < 0.4 else (int(rng.integers(0, N_CHOICES)) if shared else rng.integers(0, N_CHOICES, S))
        # the gain in force: a new one where the call's quietest block asks for more, and now and then -- not always, so that a gain a
        # shared row left behind serves the next call
        lo = 0.3 if refused else floor_of(kind, kind == "ir_crossfaded" or (kind == "layout_scheduled" and op["crossfade"]))
        if not refused and (state["gain"] is None or state["gain"] < lo or rng.random() < 0.5):
            setter("set_gain", lo=lo)
        if kind in ("scheduled", "scheduled_streams"):
            what = int(rng.integers(0, 3))          # both, tables only, gains only
            if kind == "scheduled":
                shared = True
            elif state["per_stream"] and not refused:
                what = 2                            # static per-stream tables: a gain schedule over them
            op["table_idx"] = _rows(rng, S, n_segs, shared) if what != 2 else None
            g_shared = shared if kind == "scheduled" else bool(rng.random() < 0.5)
            op["gains"] = rng.uniform(lo, 1.0, n_segs if g_shared else (S, n_segs)).astype(np.float32) if what != 1 else None
            if kind == "scheduled" and op["gains"] is not None and not refused:
                state["gain"] = float(op["gains"][-1])      # adopted
        if kind in STEREO_KINDS:
            r = rng.random()
            if r < 0.5:                             # the pointer forms on a guarded allocation: tight or wide gaps
                gaps = (1, 1, 0, 1) if rng.random() < 0.4 else (64, 32, 16 * int(rng.integers(0, 3)), 128)
                op["io"] = {"gaps": gaps, "in_place": bool(rng.random() < 0.5)}
            else:
                op["io"] = {"gaps": None, "in_place": r < 0.75}
        ops.append(op)

    for j, (kind, n) in enumerate(zip(kinds, blocks)):
        if j:                                       # between two calls: one of the handle's setters, in turn
            name = SETTERS[(5 * seed + j) % len(SETTERS)]
            if name == "set_gain":
                setter(name, lo=0.9)                # (loud enough for any call; the call may still draw its own)
            elif not (name == "share_eq_table" and not state["per_stream"]):
                setter(name)
        if j == big:
            setter("set_eq_enabled", on=True)
        else:
            setter("set_eq_enabled")
        setter("set_conv_plan")
        if kind == "scheduled" and state["per_stream"]:     # refused until the handle is back on its one shared table
            call(kind, min(n, 3), j, refused=True)
            setter("share_eq_table")
        if long_ and j == 3:                        # either IR kind on a handle whose own responses exceed one partition
            for k in IR_KINDS:
                call(k, 2, j, refused=True)
        call(kind, n, j)
    spec["ops"] = ops
    return spec

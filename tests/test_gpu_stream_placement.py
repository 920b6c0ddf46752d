"""Stream placement: hundreds of DISTINCT streams, and strides beyond 32 bits (tests/stream_placement.py is the harness,
tests/test_cpu_stream_placement.py holds it to fakes).

Every call kind that carries something per stream was tested at three to nine streams; the tests that run hundreds of streams use
the plain call on three repeated inputs and compare most streams with "the stream it repeats", which a kernel that reads the row, the
table or the input of a stream 3 k away passes.  Here:

A. a permuted twin.  Handles A and B get the same configuration; every stream has an input of its own and parameters of its own (rows,
   previous rows, gains, EQ tables, object indices, second indices, weights), and B's stream j carries everything of A's stream
   pi(j), pi a seeded derangement that moves at least a third of the streams to another residue class mod 2, 4, 8, 16 and 64.  Two
   calls per case on the same handles, 5 blocks (below the EQ wave ring's threshold of 8192 frames) and 16 blocks (at it).  After
   every call: the launch records of A and B are equal (printed: `stream-placement <case> S=<S>: call k -> ...`); out_B[j] ==
   out_A[pi(j)] bit for bit for EVERY j, compared on the device; no two streams of A have identical output; and a sample of streams
   (both ends, both sides of the multiple of 16 nearest S / 2, three seeded ones) is held to the host models at the bars they hold
   elsewhere: 1e-6 relative RMS per stream and block of 512 against tests/batch_model.py, tests/scene_model.py and
   tests/scene_blend_model.py, bit for bit against the oracle where the output is EQ only.  S = 67 (ragged last workgroups of 16 and
   of 4 waves, the XCD renumbering wraps, the EQ wave ring at 16 blocks), 257 (the EQ row ring, one wave per workgroup) and 515 (four
   waves per workgroup) on 256 CUs, derived from the device's CU count otherwise.

B. a far twin.  The same calls through the pointer entries on chains beyond 2^31 and 2^32 bytes: layout F1 (three streams 2^29 + 1028
   floats apart) and F2 (one stream, channels 2^30 + 2052 floats apart), each buffer one allocation filled with sentinels behind a
   lead of 2^29 + 4096 floats, against a compact twin on contiguous tensors, bit for bit, every stream, after every call; every gap
   word checked on the device; out of place the input allocation unchanged.  The seven batch kinds, both scene libraries and the node
   batch; the entries with separate input and output strides far on either side and on both.  F1 lies WITHIN the reach of the EQ's
   ring forms ((stream stride + channel stride + frames + 1024) * 4 < 2^32), so the launch-by-launch and conveyor paths behind that
   reach are run under F2 and under F1w, F1 with the streams 2^30 + 1028 floats apart, where the record must show them.

C. one call of 2^21 + 3 blocks on one stream: chains of 4 GiB + 6 KiB, windows at the start, at bytes 2^31 and 2^32 and at the end
   against f64 direct convolution, every slab of 2^20 frames as loud as the median one, and a short call behind it.

In the far stereo cases the EQ is also held to the oracle bit for bit, whichever form ran: the oracle EQ's output through the same
call on a handle with the EQ off must give the far handle's bits.

Measured on an MI355X (256 CUs): 149 tests in 57 s, the slowest 4.7 s (whichever far test allocates first in its process), the
worst relative RMS per stream and block of all samples 2.7e-7.  No stream differed from its twin, no gap word was damaged, no call was refused.

Each call prints the case, S and the call BEFORE it is queued: a run that ends in a fault names the call that ran last."""
import numpy as np
import pytest

from tests import batch_model as bm
from tests import scene_blend_model as sbm
from tests import scene_model as scm
from tests import stream_placement as sp
from tests.guard_bands import SENT_IN, SENT_OUT
from tests.test_cpu_ir_schedule import make_rows, make_sets
from tests.test_cpu_layout import BAR, make_input, make_layout
from tests.test_cpu_layout_schedule import make_table
from tests.test_gpu_conv_guard_bands import IrScheduled, Plain
from tests.util import RMS_TOL

pytestmark = pytest.mark.gpu

BLOCK = 512
GAIN = 0.75
CALLS = (5, 16)             # 16 * 512 = 8192 frames: the EQ wave ring's threshold (csrc/eq_plan.h); 5 blocks stay below it
PLAN_CALLS = (6, 16)        # under a forced plan: a first call the hop plan can take
SEG = 2
N_CHOICES = 4
N_DIRS = 7
LAYOUT_TAPS = 200           # (six channels of 512 taps, L1-normalised per ear, leave the first block from rest too quiet for a
                            # relative bar per block: tests/batch_model.py)
COUNTS = ("wave_ring", "row_ring_1", "row_ring_4")
assert BAR == RMS_TOL == 1e-6


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _S(which):
    return sp.stream_counts(_cus())[COUNTS.index(which)]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _shared_eq():
    """the ten bands of synth.eq_table as coefficients [10][5]"""
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    return np.stack([ohs.biquad_coefficients(b.filter_type, synth.FS, b.center_freq, b.q, b.gain_db) for b in synth.eq_table()]).astype(np.float32)


def _stereo_input(S, k, calls, first_id=5000):
    """[S][2][frames]: every stream its own noise, call k continuing call k - 1"""
    from open_headstage_amd import synth
    return synth.white_noise(range(first_id, first_id + S), calls[k] * BLOCK, offset=sum(calls[:k]) * BLOCK)


def _same_bits(got, want, what):
    """got, want [n][2][frames] numpy"""
    for i in range(len(got)):
        bad = np.argwhere(got[i].view(np.uint32) != want[i].view(np.uint32))
        assert bad.size == 0, f"{what}: entry {i} differs in {len(bad)} samples, first (channel, frame) {bad[:4].tolist()}, last {bad[-1].tolist()}"


# ---- the cases: one object configures a GPU handle and tests/batch_model.py's HandleModel alike, and issues a call on either -------
class Stereo:
    """ohs_batch_process on shared tables: only the inputs differ"""
    name, channels, ir_kind, layout_kind, nb = "process", 2, False, False, 10

    def __init__(self, taps=512, plan=0):
        self.taps, self.plan = taps, plan

    def params(self, S, calls):
        return {}

    def input(self, S, k, calls):
        return _stereo_input(S, k, calls)

    def setup(self, h, P, eq=True):
        """h: a BatchProcessor or a HandleModel (the setters carry the same names)"""
        from open_headstage_amd import synth
        for p, ir in enumerate(synth.hrir_set(self.taps)):
            h.set_ir(p, ir)
        h.set_gain(GAIN)
        for b, c in enumerate(_shared_eq()):
            h.set_band_coeffs(b, c, True)
        h.set_eq_enabled(eq)
        self.configure(h, P)

    def configure(self, h, P):
        pass

    def make(self, S, P, eq=True):
        import open_headstage_amd as ohs
        bp = ohs.BatchProcessor(S, num_bands=self.nb, library=getattr(self, "lib", None))
        bp.set_conv_plan(self.plan)
        self.setup(bp, P, eq)
        return bp

    def model(self, oracle, n, P):
        m = bm.HandleModel(oracle, n, self.nb)
        self.setup(m, P)
        return m

    def call(self, h, k, nb, x, P):
        return h.process(x)

    gpu = model_call = None

    def records(self, h):
        return {"conv": h.last_conv_plan(), "eq": h.last_eq_form(), "ir_lookup": 2 if h.last_conv_ir_crossfaded() else int(h.last_conv_ir_scheduled())}

    def check_records(self, r, S, nb, what):
        want = sp.expected_eq_form(S, nb * BLOCK, _cus())[0]
        assert r["eq"][0] == want, f"{what}: the EQ ran as {r['eq']}, csrc/eq_plan.h names {want} for {2 * S} chains of {nb * BLOCK} frames"
        if self.ir_kind:
            assert r["conv"][0] == "block512_p1" and r["ir_lookup"] == (2 if self.name == "ir_crossfaded" else 1), f"{what}: {r}"
        else:
            assert r["ir_lookup"] == 0, f"{what}: {r}"
        want = {(512, 1): "block512_p1", (512, 2): "block512_p1" if self.ir_kind else "hop1536_p1", (1300, 0): "block2048",
                (1300, 1): "block512_tp"}.get((self.taps, self.plan))
        assert want is None or r["conv"][0] == want, f"{what}: plan {self.plan} on {self.taps} taps names {want}, served by {r['conv']}"


class Deferred(Stereo):
    name = "process_deferred"

    def gpu(self, h, k, nb, x, P):
        y = h.process(x, deferred=True)
        h.join()
        return y


class Host(Stereo):
    name = "process_host"

    def gpu(self, h, k, nb, x, P):
        return _dev(h.process_host(x.cpu().numpy()))


class Scheduled(Stereo):
    """one row of tables and gains for all streams: only the inputs differ, the rows are read per stream all the same"""
    name = "process_scheduled"

    def params(self, S, calls):
        rng = np.random.default_rng(41)
        self.rows = [bm._varying_row(rng, -(-nb // SEG)) for nb in calls]
        self.gains = [rng.uniform(0.5, 1.0, -(-nb // SEG)).astype(np.float32) for nb in calls]
        return {}

    def configure(self, h, P):
        h.set_schedule_tables(*bm.make_tables())

    def call(self, h, k, nb, x, P):
        return h.process_scheduled(x, SEG, self.rows[k], self.gains[k])


class ScheduledStreams(Scheduled):
    name = "process_scheduled_streams"

    def params(self, S, calls):
        rng = np.random.default_rng(42)
        return {"rows": [np.stack([bm._varying_row(rng, -(-nb // SEG)) for _ in range(S)]) for nb in calls],
                "gains": [rng.uniform(0.5, 1.0, (S, -(-nb // SEG))).astype(np.float32) for nb in calls]}

    def call(self, h, k, nb, x, P):
        return h.process_scheduled_streams(x, SEG, P["rows"][k], P["gains"][k])


class IrSched(Stereo):
    ir_kind = True

    def __init__(self, mode, taps=512, plan=0):
        super().__init__(taps, plan)
        self.mode, self.name = mode, "ir_crossfaded" if mode == "crossfaded" else f"ir_scheduled_{mode}"

    def params(self, S, calls):
        rng = np.random.default_rng(43)
        return {"rows": [np.stack([bm._varying_row(rng, -(-nb // SEG)) for _ in range(S)]) for nb in calls],
                "prev": [rng.integers(0, N_CHOICES, S).astype(np.uint32) for _ in calls]}

    def configure(self, h, P):
        h.set_schedule_irs(make_sets(N_CHOICES, 512, seed=7))

    def call(self, h, k, nb, x, P):
        if self.mode == "crossfaded":
            return h.process_ir_crossfaded(x, SEG, P["rows"][k], P["prev"][k])
        return h.process_ir_scheduled(x, SEG, P["rows"][k], self.mode)


ENABLED_COUNTS = (0, 1, 7, 12)


def _stream_tables(S, nb=16):
    """S tables of nb bands, all coefficients different; 0, 1, 7 or 12 bands enabled by s % 4 (identity rows, one pass), and 13 .. 16
    in every eleventh stream (a second pass for everyone); which bands are enabled rotates with the stream"""
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    from open_headstage_amd.dsp import FilterType
    rng = np.random.default_rng(44)
    coeffs, en = np.zeros((S, nb, 5), np.float32), np.zeros((S, nb), bool)
    for s in range(S):
        for b in range(nb):
            ft = FilterType.LowShelf if b == 0 else FilterType.HighShelf if b == nb - 1 else FilterType.Peak
            fc = min(45.0 * 2.0 ** (b * 0.55 + 0.0009 * s), 18000.0)
            coeffs[s, b] = ohs.biquad_coefficients(ft, synth.FS, float(fc), float(0.6 + 0.2 * ((s + 2 * b) % 5)), float(rng.uniform(-3, 3)))
        n = 13 + (s // 11) % 4 if s % 11 == 5 else ENABLED_COUNTS[s % 4]
        en[s, (s + np.arange(n)) % nb] = True
        assert en[s].sum() == n
    return coeffs, en


class StreamEq(Stereo):
    """static per-stream tables (ohs_batch_set_stream_eq_band_coeffs), 16 bands of which 0, 1, 7, 12 or more than 12 are enabled"""
    name, nb = "stream_eq_tables", 16

    def params(self, S, calls):
        c, e = _stream_tables(S, self.nb)
        return {"coeffs": c, "en": e}

    def setup(self, h, P, eq=True):
        from open_headstage_amd import synth
        for p, ir in enumerate(synth.hrir_set(self.taps)):
            h.set_ir(p, ir)
        h.set_gain(GAIN)
        h.set_eq_enabled(eq)
        if eq:
            for s in range(len(P["coeffs"])):
                for b in range(self.nb):
                    h.set_stream_band_coeffs(s, b, P["coeffs"][s, b], bool(P["en"][s, b]))


class Layout(Stereo):
    layout_kind = True

    def __init__(self, K, scheduled):
        super().__init__(LAYOUT_TAPS, 0)
        self.K = self.channels = K
        self.scheduled, self.name = scheduled, f"layout{'_scheduled' if scheduled else ''}_K{K}"

    def params(self, S, calls):
        rng = np.random.default_rng(45 + self.K)
        return {"rows": [np.stack([bm._varying_row(rng, -(-nb // SEG)) for _ in range(S)]) for nb in calls],
                "prev": [rng.integers(0, N_CHOICES, S).astype(np.uint32) for _ in calls]}

    def input(self, S, k, calls):
        return make_input(S, self.K, calls[k], seed=20000 + 10000 * k + 100 * self.K)

    def configure(self, h, P):
        if self.scheduled:
            h.set_layout_table(make_table(N_CHOICES, self.K, LAYOUT_TAPS, seed=3))
        else:
            h.set_layout_irs(make_layout(self.K, LAYOUT_TAPS))

    def call(self, h, k, nb, x, P):
        if self.scheduled:
            return h.process_layout_scheduled(x, P["rows"][k], SEG, P["prev"][k], True)
        return h.process_layout(x)

    def records(self, h):
        return {"layout": h.last_layout_launch(), "layout_scheduled": h.last_layout_scheduled(), "eq": h.last_eq_form()}

    def check_records(self, r, S, nb, what):
        assert r["layout"][0] == (self.K + 1) // 2 and r["layout_scheduled"] == self.scheduled, f"{what}: {r}"
        assert r["eq"][0] in ("row_ring", "wave_ring"), f"{what}: {r}"


class NodeBatch(Stereo):
    """ohs_node_batch_process over one device slot"""
    name = "node_batch"

    def make(self, S, P, eq=True):
        import open_headstage_amd as ohs
        from open_headstage_amd import synth
        nbp = ohs.NodeBatchProcessor(S, num_bands=self.nb, n_devices=1)
        nbp.set_tables(synth.hrir_set(self.taps), _shared_eq(), np.ones(self.nb, bool))
        nbp.set_conv_plan(self.plan)
        nbp.set_gain(GAIN)
        nbp.set_eq_enabled(eq)
        return nbp

    def gpu(self, h, k, nb, x, P):
        import torch
        y = torch.empty_like(x)
        torch.cuda.synchronize()
        h.process([x], [y])
        h.sync()
        return y

    def records(self, h):
        return Stereo.records(self, h.device_batch(0))


class NodeRehearsal(StreamEq):
    """three device slots sharing the one GPU (the experiments library's rehearsal), per-stream tables addressed by the JOB's stream
    id: the per-slot unpack of the tables"""
    name, nb, SLOTS = "node_rehearsal_stream_eq", 16, 3

    def make(self, S, P, eq=True):
        import open_headstage_amd as ohs
        from open_headstage_amd import synth
        nbp = ohs.NodeBatchProcessor(S, num_bands=self.nb, devices=[0] * self.SLOTS, library=self.lib)
        nbp.set_tables(synth.hrir_set(self.taps))
        nbp.set_conv_plan(self.plan)
        nbp.set_gain(GAIN)
        nbp.set_eq_enabled(eq)
        for s in range(S):
            for b in range(self.nb):
                nbp.set_stream_band_coeffs(s, b, P["coeffs"][s, b], bool(P["en"][s, b]))
        return nbp

    def gpu(self, h, k, nb, x, P):
        import torch
        shards = [h.shard(i) for i in range(self.SLOTS)]
        xs = [x[f:f + c].contiguous() for _, f, c in shards]
        ys = [torch.empty_like(a) for a in xs]
        torch.cuda.synchronize()
        h.process(xs, ys)
        h.sync()
        return torch.cat(ys)

    def records(self, h):
        return {f"slot{i}": Stereo.records(self, h.device_batch(i)) for i in range(self.SLOTS)}

    def check_records(self, r, S, nb, what):
        assert all(v["eq"][0] in ("row_ring", "wave_ring") and v["conv"][0] != "none" for v in r.values()), f"{what}: {r}"


# ---- A: the permuted twin -----------------------------------------------------------------------------------------------------------
def run_permuted_twin(case, S, calls, oracle):
    import torch
    pi = sp.derangement(S)
    P = case.params(S, calls)
    PB = sp.permuted(P, pi)
    A, B = case.make(S, P), case.make(S, PB)
    sample = sp.sample_streams(S)
    PS = sp.taken(P, sample)
    model = case.model(oracle, len(sample), PS)
    dry = case.make(S, P, eq=False) if case.layout_kind else None      # the layout operations alone: what the EQ behind them is fed
    gpu = case.gpu or case.call
    tag = f"stream-placement {case.name} S={S}"
    worst = 0.0
    for k, nb in enumerate(calls):
        what = f"{tag}: call {k} ({nb} blocks)"
        print(f"{what} ...", flush=True)
        x = case.input(S, k, calls)
        ya = gpu(A, k, nb, _dev(x), P)
        yb = gpu(B, k, nb, _dev(x[pi]), PB)
        torch.cuda.synchronize()
        ra, rb = case.records(A), case.records(B)
        print(f"{tag}: call {k} -> {ra}", flush=True)
        # 1. launch records
        assert ra == rb, f"{what}: A {ra}, B {rb}"
        case.check_records(ra, S, nb, what)
        # 2. bits, every stream
        sp.assert_permuted_twin(yb, ya, pi, what)
        # 3. nobody repeats
        sp.assert_nobody_repeats(ya, what)
        # 4. the sample against the host model
        ref = (case.model_call or case.call)(model, k, nb, np.ascontiguousarray(x[sample]), PS)
        got = ya[torch.as_tensor(sample, device=ya.device)].cpu().numpy()
        if dry is None:
            worst = max(worst, sp.assert_sample_within_bar(got, ref, sample, BAR, what + ", against tests/batch_model.py"))
        else:
            d = gpu(dry, k, nb, _dev(x), P)[torch.as_tensor(sample, device=ya.device)].cpu().numpy()
            worst = max(worst, sp.assert_sample_within_bar(d, ref, sample, BAR, what + ", EQ off, against tests/batch_model.py"))
            _same_bits(got, model.layout_eq(d), what + f", the oracle EQ of the dry output, sample {sample}")
    print(f"{tag}: sample {sample}, worst relative RMS per stream and block {worst:.3e}")
    return A, P, sample


STEREO_CASES = {"process": Stereo, "deferred": Deferred, "host": Host, "scheduled": Scheduled, "scheduled_streams": ScheduledStreams,
                "ir_ring_out": lambda *a: IrSched("ring_out", *a), "ir_cut": lambda *a: IrSched("cut", *a),
                "ir_crossfaded": lambda *a: IrSched("crossfaded", *a), "node_batch": NodeBatch}


@pytest.mark.parametrize("which", COUNTS)
@pytest.mark.parametrize("case", list(STEREO_CASES))
def test_permuted_twin_stereo_kinds(oracle, case, which):
    run_permuted_twin(STEREO_CASES[case](), _S(which), CALLS, oracle)


@pytest.mark.parametrize("which", COUNTS)
def test_permuted_twin_per_stream_eq_tables(oracle, which):
    """... and the EQ alone, bit for bit: the sample's inputs through one oracle StereoParametricEQ each, then through a handle of S
    streams with the EQ off (the convolution is a function of the bits it is fed; the other streams are fed silence)"""
    import torch
    from open_headstage_amd import synth
    S, case = _S(which), StreamEq()
    A, P, sample = run_permuted_twin(case, S, CALLS, oracle)
    A.reset()
    conv_only = Stereo().make(S, {}, eq=False)
    eqs = []
    for s in sample:
        q = oracle.StereoParametricEQ(case.nb, synth.FS)
        for b in range(case.nb):
            q.set_band_coeffs(b, P["coeffs"][s, b], bool(P["en"][s, b]))
        eqs.append(q)
    for k, nb in enumerate(CALLS):
        x = case.input(S, k, CALLS)
        xe = np.zeros_like(x)
        for q, s in zip(eqs, sample):
            l, r = x[s, 0].copy(), x[s, 1].copy()
            q.process_block(l, r)
            xe[s, 0], xe[s, 1] = l, r
            if not P["en"][s].any():
                assert np.array_equal(xe[s].view(np.uint32), x[s].view(np.uint32))
        ya, yr = A.process(_dev(x)), conv_only.process(_dev(xe))
        torch.cuda.synchronize()
        assert A.last_conv_plan() == conv_only.last_conv_plan(), (A.last_conv_plan(), conv_only.last_conv_plan())
        idx = torch.as_tensor(sample, device=ya.device)
        _same_bits(ya[idx].cpu().numpy(), yr[idx].cpu().numpy(), f"stream-placement EQ bits S={S}: call {k}, sample {sample}")


@pytest.mark.parametrize("which", COUNTS)
@pytest.mark.parametrize("scheduled", [False, True], ids=["layout", "layout_scheduled"])
@pytest.mark.parametrize("K", [6, 3])
def test_permuted_twin_layout_kinds(oracle, K, scheduled, which):
    run_permuted_twin(Layout(K, scheduled), _S(which), CALLS, oracle)


def test_permuted_twin_three_slot_rehearsal_unpacks_per_stream_tables(oracle, exp_tuning):
    exp_tuning("node_shared_device_rehearsal", "1")
    case = NodeRehearsal()
    case.lib = exp_tuning.lib
    run_permuted_twin(case, _S("wave_ring"), CALLS, oracle)


PLAN_CASES = [(c, 512, p) for c in ("process", "deferred", "host", "scheduled", "scheduled_streams", "ir_ring_out", "ir_cut", "ir_crossfaded",
                                    "node_batch") for p in (1, 2)] + \
             [(c, 1300, p) for c in ("process", "deferred", "host", "scheduled", "scheduled_streams", "node_batch") for p in (0, 1)]


@pytest.mark.parametrize("case,taps,plan", PLAN_CASES, ids=[f"{c}-taps{t}-plan{p}" for c, t, p in PLAN_CASES])
def test_permuted_twin_under_every_plan(oracle, case, taps, plan):
    """S = 67 under every plan ohs_batch_set_conv_plan accepts and the shape allows; the record must name that plan's kernel"""
    run_permuted_twin(STEREO_CASES[case](taps, plan), _S("wave_ring"), PLAN_CALLS, oracle)


# ---- A, scenes ----------------------------------------------------------------------------------------------------------------------
class Scene:
    """ohs_scene_process (blend: ohs_scene2_process_blended): rows of directions and gains per stream, crossfaded"""

    def __init__(self, K, blend):
        self.K, self.blend, self.name = K, blend, f"{'blend_' if blend else ''}scene_K{K}"

    def params(self, S, calls):
        make = sbm.make_blend_scene if self.blend else scm.make_scene
        out = []
        for k, nb in enumerate(calls):
            sc = make(S, self.K, nb, SEG, N_DIRS, seed=10 * self.K + k)
            out.append(sc if self.blend else dict(zip(("idx", "gains", "prev_idx", "prev_gains"), sc)))
        return out

    def make(self, S, eq=True):
        import open_headstage_amd as ohs
        sc = (ohs.BlendSceneProcessor if self.blend else ohs.SceneProcessor)(S, num_bands=10)
        sc.set_gain(GAIN)
        sc.set_directions(make_layout(N_DIRS, 512))
        for b, c in enumerate(_shared_eq()):
            sc.set_band_coeffs(b, c, True)
        sc.set_eq_enabled(eq)
        return sc

    def gpu(self, sc, x, p):
        if self.blend:
            return sc.process(x, p["idx"], SEG, p["gains"], p["prev_idx"], p["prev_gains"], True, p["idx1"], p["weights"], p["prev_idx1"],
                              p["prev_weights"])
        return sc.process(x, p["idx"], SEG, p["gains"], p["prev_idx"], p["prev_gains"], True)

    def model(self, x, p, tail):
        dirs = make_layout(N_DIRS, 512)
        if self.blend:
            return sbm.model_blend_f64(x, dirs, p["idx"], p["idx1"], p["weights"], SEG, p["gains"], p["prev_idx"], p["prev_idx1"],
                                       p["prev_weights"], p["prev_gains"], True, GAIN, tail, with_tail=True)
        return scm.model_scene_f64(x, dirs, p["idx"], SEG, p["gains"], p["prev_idx"], p["prev_gains"], True, GAIN, tail, with_tail=True)


@pytest.mark.parametrize("which", COUNTS)
@pytest.mark.parametrize("blend", [False, True], ids=["scene", "blend_scene"])
@pytest.mark.parametrize("K", [3, 6])
def test_permuted_twin_object_scenes(oracle, K, blend, which):
    """the same twin on the scene libraries: idx, gains, prev (blend: idx1 and weights too, the objects 1 mod 4 at +0.0) per stream"""
    import torch
    from open_headstage_amd import synth
    S, case = _S(which), Scene(K, blend)
    if blend:
        import open_headstage_amd.scene2  # noqa: F401
    pi = sp.derangement(S)
    P = case.params(S, CALLS)
    PB = sp.permuted(P, pi)
    A, B, dry = case.make(S), case.make(S), case.make(S, eq=False)
    sample = sp.sample_streams(S)
    PS = sp.taken(P, sample)
    eqs = []
    for _ in sample:
        q = oracle.StereoParametricEQ(10, synth.FS)
        for b, c in enumerate(_shared_eq()):
            q.set_band_coeffs(b, c, True)
        eqs.append(q)
    tag, tail, worst = f"stream-placement {case.name} S={S}", None, 0.0
    for k, nb in enumerate(CALLS):
        what = f"{tag}: call {k} ({nb} blocks)"
        print(f"{what} ...", flush=True)
        x = make_input(S, K, nb, seed=40000 + 10000 * k + 100 * K)
        if blend:
            assert (P[k]["weights"][:, :, 1] == 0).all() and not np.signbit(P[k]["weights"][:, :, 1]).any()
        ya, yb, d = case.gpu(A, _dev(x), P[k]), case.gpu(B, _dev(x[pi]), PB[k]), case.gpu(dry, _dev(x), P[k])
        torch.cuda.synchronize()
        ra, rb = A.last_launch(), B.last_launch()
        print(f"{tag}: call {k} -> launch {ra}, EQ behind it on {2 * S} chains", flush=True)
        # (the passes through old directions and through four table rows are sums over the streams: a permutation keeps them)
        assert ra == rb and ra[0] == (K + 1) // 2 and ra[1] >= 1, f"{what}: A {ra}, B {rb}"
        sp.assert_permuted_twin(yb, ya, pi, what)
        sp.assert_nobody_repeats(ya, what)
        idx = torch.as_tensor(sample, device=ya.device)
        ds, got = d[idx].cpu().numpy(), ya[idx].cpu().numpy()
        ref, tail = case.model(np.ascontiguousarray(x[sample]), PS[k], tail)
        worst = max(worst, sp.assert_sample_within_bar(ds, ref, sample, BAR, what + ", EQ off, against the f64 scene model"))
        want = np.empty_like(ds)
        for i, q in enumerate(eqs):
            l, r = ds[i, 0].copy(), ds[i, 1].copy()
            q.process_block(l, r)
            want[i, 0], want[i, 1] = l, r
        _same_bits(got, want, what + f", the oracle EQ of the dry output, sample {sample}")
    print(f"{tag}: sample {sample}, worst relative RMS per stream and block {worst:.3e}")


# ---- B: the far twin ----------------------------------------------------------------------------------------------------------------
GIB = float(1 << 30)


def _need(gib):
    """skip only where the device has less free memory than the test states"""
    import torch
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0] / GIB
    if free < gib:
        pytest.skip(f"needs {gib:.1f} GiB of device memory, {free:.1f} GiB are free")


def _far_buffer(lay, sentinel):
    import torch
    buf = torch.empty(lay.total, dtype=torch.float32, device="cuda")
    buf.view(torch.int32).fill_(int(np.array(sentinel, np.uint32).view(np.int32)))
    assert buf.data_ptr() % 16 == 0
    return buf


class FarScheduled(Plain):
    """ohs_batch_process_scheduled (per_stream: _scheduled_streams) with at least three segments; `identity`: a table without an
    enabled band among them -- those segments are the launch layer's copy, whose pitch is the channel stride"""

    def __init__(self, S, per_stream, identity=False):
        self.S, self.per_stream, self.identity = S, per_stream, identity

    def rows(self, k, nb):
        n = -(-nb // SEG)
        assert n >= 3
        rng = np.random.default_rng(60 + k)
        t = np.stack([bm._varying_row(rng, n) for _ in range(self.S)])
        if self.identity:
            t[:, 1] = N_CHOICES                 # the table appended in _far_stereo_make: no band enabled
        g = rng.uniform(0.5, 1.0, (self.S, n)).astype(np.float32)
        return (t, g) if self.per_stream else (t[0], g[0])

    def ptr(self, bp, k, nb, d_in, d_out, ss, cs, st):
        fn = bp.process_scheduled_streams_ptr if self.per_stream else bp.process_scheduled_ptr
        fn(d_in, d_out, nb, ss, cs, SEG, *self.rows(k, nb), st)

    def tensor(self, bp, k, nb, x, out):
        fn = bp.process_scheduled_streams if self.per_stream else bp.process_scheduled
        return fn(x, SEG, *self.rows(k, nb), out=out)

    def model(self, m, k, nb, x):
        fn = m.process_scheduled_streams if self.per_stream else m.process_scheduled
        return fn(x, SEG, *self.rows(k, nb))


def _tables_with_identity():
    c, e = bm.make_tables()
    return np.concatenate([c, c[:1]]), np.concatenate([e, np.zeros_like(e[:1])])


def _far_stereo_setup(h, S, stream_tables=None):
    """a BatchProcessor or a HandleModel for the far cases: 512 taps, the shared table or static per-stream tables, EQ on"""
    case = Stereo()
    case.setup(h, {})
    h.set_schedule_tables(*_tables_with_identity())
    h.set_schedule_irs(make_sets(IrScheduled.N_SETS))
    if stream_tables is not None:
        for s in range(S):
            for b in range(10):
                h.set_stream_band_coeffs(s, b, stream_tables[0][s, b], bool(stream_tables[1][s, b]))


def run_far_stereo(name, entry, lay_of, in_place, oracle, calls=(7, 6), stream_tables=None, beyond_the_rings=False):
    """the far twin of a stereo entry (tests/test_gpu_conv_guard_bands.py's entry classes: .ptr on the far chains, .tensor on the
    compact twin).  lay_of(frames) -> the FarLayout; device memory: one far buffer in place, two out of place.
    That file's run_case has the same shape and is not called: it builds every buffer and its mask in numpy and downloads both
    buffers whole after every call -- 6 to 10 GiB each here, where the buffers are filled, taken apart and checked on the device --
    and it asks for the convolution family by name, which these cases leave to the library."""
    import torch
    import open_headstage_amd as ohs
    S = lay_of(BLOCK).S
    entry.blocks = list(calls)
    far, twin = ohs.BatchProcessor(S, num_bands=10), ohs.BatchProcessor(S, num_bands=10)
    model, eq_model = bm.HandleModel(oracle, S, 10), bm.HandleModel(oracle, S, 10)
    conv_only = ohs.BatchProcessor(S, num_bands=10)         # EQ off: fed what the oracle EQ makes of the input
    for h in (far, twin, model, eq_model, conv_only):
        _far_stereo_setup(h, S, None if h is conv_only else stream_tables)
    conv_only.set_eq_enabled(False)
    st = torch.cuda.current_stream().cuda_stream
    tag = f"stream-placement far {name}, {'in place' if in_place else 'out of place'}"
    for k, nb in enumerate(calls):
        frames = nb * BLOCK
        lay = lay_of(frames)
        what = f"{tag}, {lay.name}: call {k} ({nb} blocks)"
        print(f"{what} ...", flush=True)
        x = _stereo_input(S, k, calls, first_id=6000)
        xt = _dev(x)
        d_in = _far_buffer(lay, SENT_IN)
        sp.far_place(d_in, xt, lay)
        d_out = d_in if in_place else _far_buffer(lay, SENT_OUT)
        base = 4 * lay.start(0, 0)
        entry.ptr(far, k, nb, d_in.data_ptr() + base, d_out.data_ptr() + base, lay.ss, lay.cs, st)
        torch.cuda.synchronize()
        xc = xt.clone()
        ref = entry.tensor(twin, k, nb, xc, xc if in_place else None)
        torch.cuda.synchronize()
        pf, pt = far.last_conv_plan(), twin.last_conv_plan()
        print(f"{tag}, {lay.name}: call {k} -> conv {pf}, EQ far {far.last_eq_form()}, EQ twin {twin.last_eq_form()}", flush=True)
        assert pf == pt, f"{what}: far {pf}, twin {pt}"
        entry.check(far, k)
        if beyond_the_rings:                    # the case names the fallback: the record must show it, and the twin on a ring form
            assert not sp.ring_addressable(lay.ss, lay.cs, frames) and far.last_eq_form()[0] == "conveyor", f"{what}: {far.last_eq_form()}"
            want = sp.expected_eq_form(S, frames, _cus())[0]
            assert twin.last_eq_form()[0] == want, f"{what}: the twin's EQ ran as {twin.last_eq_form()}, csrc/eq_plan.h names {want}"
        sp.far_gaps_intact(d_out, lay, SENT_IN if in_place else SENT_OUT, what + ", output buffer")
        if not in_place:
            sp.far_gaps_intact(d_in, lay, SENT_IN, what + ", input buffer")
            sp.assert_same_streams(sp.far_take(d_in, lay), xt, what + ", the input chains")
        y = sp.far_take(d_out, lay)
        assert bool(torch.isfinite(y).all()), f"{what}: non-finite output: an offset landed in the sentinel"
        sp.assert_same_streams(y, ref, what)
        want = entry.model(model, k, nb, x) if hasattr(entry, "model") else _guard_entry_model(entry, model, k, nb, x)
        sp.assert_sample_within_bar(y.cpu().numpy(), want, list(range(S)), BAR, what + ", against tests/batch_model.py")
        # the EQ alone, bit for bit against the oracle, whichever form ran: the oracle EQ's output (the schedule's tables per stream
        # and segment, state carried) through the same call on a handle with the EQ off -- the convolution is a function of its bits
        seg, rows = _eq_schedule(entry, S, k, nb)
        xe = _dev(eq_model._eq(eq_model.eqs, x, seg, rows))
        yr = _conv_only_call(entry, conv_only, k, nb, xe, xe if in_place else None)
        torch.cuda.synchronize()
        assert conv_only.last_conv_plan() == pf, f"{what}: the EQ-off handle ran {conv_only.last_conv_plan()}, the far one {pf}"
        sp.assert_same_streams(y, yr, what + ", the oracle EQ's output through the convolution alone")
        del d_in, d_out, y
    torch.cuda.empty_cache()


def _eq_schedule(entry, S, k, nb):
    """(seg_blocks, table rows [S][n_segs]) of the call's EQ schedule; (None, None): the handle's own table(s) throughout"""
    if isinstance(entry, FarScheduled):
        t = np.asarray(entry.rows(k, nb)[0])
        return SEG, np.broadcast_to(t, (S, t.shape[-1]))
    return None, None


def _conv_only_call(entry, bp, k, nb, x, out):
    """the entry's call on a handle whose EQ is off: the same rows, gains and sets, no tables"""
    if isinstance(entry, FarScheduled):
        fn = bp.process_scheduled_streams if entry.per_stream else bp.process_scheduled
        return fn(x, SEG, None, entry.rows(k, nb)[1], out=out)
    return entry.tensor(bp, k, nb, x, out)


def _guard_entry_model(entry, m, k, nb, x):
    if isinstance(entry, IrScheduled):
        if entry.mode == "crossfaded":
            return m.process_ir_crossfaded(x, entry.seg, entry.rows(k, nb), entry.prev(k))
        return m.process_ir_scheduled(x, entry.seg, entry.rows(k, nb), entry.mode)
    return m.process(x)


class FarIr(IrScheduled):
    """the guard-band entry with EVERY stream changing its set in every segment (its stream 0 stays on one set, and F2 has no other)"""

    def rows(self, k, nb):
        return make_rows(self.S, -(-nb // self.seg), self.N_SETS, k)


def _far_entries():
    return {"process": lambda S: Plain(), "scheduled": lambda S: FarScheduled(S, False), "scheduled_streams": lambda S: FarScheduled(S, True),
            "ir_scheduled": lambda S: FarIr(S, SEG, "ring_out"), "ir_cut": lambda S: FarIr(S, SEG, "cut"),
            "ir_crossfaded": lambda S: FarIr(S, SEG, "crossfaded")}


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("kind", ["process", "scheduled", "scheduled_streams", "ir_scheduled", "ir_cut", "ir_crossfaded"])
def test_far_f1_stereo_entries(oracle, kind, in_place):
    """F1, S = 3: stream 1 starts beyond 2^31 bytes, stream 2 beyond 2^32.  `scheduled` and `scheduled_streams` have four and three
    segments.  F1 lies within the reach of the EQ's ring forms and the calls are shorter than 8192 frames, so the EQ runs the twin's
    kernels here (test_far_f1w_... runs the fallbacks); the convolution kernels add their 64-bit stream offsets.
    Device memory: 6.1 GiB per far buffer -- 12.2 GiB out of place, 6.1 GiB in place."""
    _need(12.5 if not in_place else 6.5)
    run_far_stereo(kind, _far_entries()[kind](3), sp.layout_f1, in_place, oracle)


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_far_f1_per_stream_eq_tables(oracle, in_place):
    """static per-stream tables under F1, which the ring forms still reach: one ring launch for all streams, as in the twin, its lane
    offsets beyond 2^31 bytes (test_far_f1w_... runs the path where every stream is a launch sequence of its own).
    Device memory: 12.2 GiB out of place, 6.1 GiB in place."""
    _need(12.5 if not in_place else 6.5)
    c, e = _stream_tables(3, 10)                    # (0, 1 and 7 bands enabled: stream 0 is copied)
    assert e.sum(axis=1).tolist() == [0, 1, 7]
    run_far_stereo("per-stream tables", Plain(), sp.layout_f1, in_place, oracle, stream_tables=(c, e))


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("kind", ["scheduled", "scheduled_streams", "per_stream_tables"])
def test_far_f1w_beyond_the_reach_of_the_eq_ring_forms(oracle, kind, in_place):
    """F1 itself lies within the reach of the EQ's ring forms ((stream stride + channel stride + frames + 1024) * 4 < 2^32,
    csrc/eq_ring2_body.hpp), so the three cases above run the same kernels as their twins.  Here the streams are 2^30 + 1028 floats
    apart and the first call has 16 blocks: the twin's schedule is served by the wave ring's scheduled kernel (its per-stream tables
    by one ring launch for all streams), the far handle's cannot be -- launch by launch on the conveyor form, every stream a launch
    sequence of its own -- and the records must say so.  Same bits.
    Device memory: 10.0 GiB per far buffer -- 20.1 GiB out of place, 10.0 GiB in place."""
    _need(20.5 if not in_place else 10.5)
    if kind == "per_stream_tables":
        run_far_stereo("per-stream tables", Plain(), sp.layout_f1w, in_place, oracle, (16, 7), _stream_tables(3, 10), beyond_the_rings=True)
    else:
        run_far_stereo(kind, _far_entries()[kind](3), sp.layout_f1w, in_place, oracle, (16, 7), beyond_the_rings=True)


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("kind", ["process", "scheduled", "scheduled_streams", "ir_scheduled", "ir_cut", "ir_crossfaded"])
def test_far_f2_stereo_entries(oracle, kind, in_place):
    """F2, S = 1: the right channel starts beyond 2^32 bytes from the left one -- the only layout whose CHANNEL stride leaves 32 bits,
    so every stereo entry (k_conv_p1, k_conv_p1_irs and k_conv_p1_irs_xf are three kernels) runs under it, both ways.  The ring
    forms do not reach it: the far handle's EQ must be on record as the conveyor form.
    Device memory: 6.0 GiB per far buffer -- 12.0 GiB out of place, 6.0 GiB in place."""
    _need(12.5 if not in_place else 6.5)
    run_far_stereo(kind, _far_entries()[kind](1), sp.layout_f2, in_place, oracle, beyond_the_rings=True)


def test_far_f2_scheduled_out_of_place_with_a_table_without_bands(oracle):
    """F2, out of place, a schedule whose second segment names a table with no enabled band: those frames are the launch layer's
    copy (eq_copy_through, hipMemcpy2DAsync) with the channel stride -- more than 2^32 bytes -- as its pitch.  The segments around
    it have bands and go launch by launch on the conveyor form (the last launch of either call is one of them: the record must say
    so), and the copied frames must be the oracle's identity, bit for bit, like all the others.
    Device memory: 12.0 GiB."""
    _need(12.5)
    run_far_stereo("scheduled + identity table", FarScheduled(1, False, identity=True), sp.layout_f2, False, oracle, beyond_the_rings=True)


# ---- B, the entries with separate input and output strides: layouts and object scenes ------------------------------------------------
class _OracleEqs:
    """one oracle StereoParametricEQ per stream on the shared table, state carried from call to call"""

    def __init__(self, oracle, n):
        from open_headstage_amd import synth
        self.eqs = []
        for _ in range(n):
            q = oracle.StereoParametricEQ(10, synth.FS)
            for b, c in enumerate(_shared_eq()):
                q.set_band_coeffs(b, c, True)
            self.eqs.append(q)

    def __call__(self, d):
        want = np.empty_like(d)
        for i, q in enumerate(self.eqs):
            l, r = d[i, 0].copy(), d[i, 1].copy()
            q.process_block(l, r)
            want[i, 0], want[i, 1] = l, r
        return want


class FarLayoutEntry:
    def __init__(self, K, scheduled, S, calls, oracle):
        self.case, self.K, self.S = Layout(K, scheduled), K, S
        self.P = self.case.params(S, calls)
        self.m = self.case.model(oracle, S, self.P)
        self.name = self.case.name

    def make(self, eq=True):
        return self.case.make(self.S, self.P, eq)

    def input(self, k, calls):
        return self.case.input(self.S, k, calls)

    def ptr(self, h, k, nb, pin, pout, li, lo, st):
        if self.case.scheduled:
            h.process_layout_scheduled_ptr(pin, pout, nb, li.ss, li.cs, lo.ss, lo.cs, SEG, self.P["rows"][k], self.P["prev"][k], True, st)
        else:
            h.process_layout_ptr(pin, pout, nb, li.ss, li.cs, lo.ss, lo.cs, st)

    def tensor(self, h, k, nb, x):
        return self.case.call(h, k, nb, x, self.P)

    def records(self, h):
        return self.case.records(h)

    def dry_model(self, k, nb, x):
        return self.case.call(self.m, k, nb, x, self.P)

    def eq_of(self, d):
        return self.m.layout_eq(d)


class FarSceneEntry:
    def __init__(self, K, blend, S, calls, oracle):
        self.case, self.K, self.S = Scene(K, blend), K, S
        self.P = self.case.params(S, calls)
        self.name, self.tail, self.eq_of = self.case.name, None, _OracleEqs(oracle, S)

    def make(self, eq=True):
        return self.case.make(self.S, eq)

    def input(self, k, calls):
        return make_input(self.S, self.K, calls[k], seed=50000 + 10000 * k + 100 * self.K)

    def ptr(self, h, k, nb, pin, pout, li, lo, st):
        p = self.P[k]
        more = (p["idx1"], p["weights"], p["prev_idx1"], p["prev_weights"]) if self.case.blend else ()
        h.process_ptr(pin, pout, nb, li.ss, li.cs, lo.ss, lo.cs, self.K, SEG, p["idx"], p["gains"], p["prev_idx"], p["prev_gains"], True, st,
                      *more)

    def tensor(self, h, k, nb, x):
        return self.case.gpu(h, x, self.P[k])

    def records(self, h):
        return {"launch": h.last_launch()}

    def dry_model(self, k, nb, x):
        y, self.tail = self.case.model(x, self.P[k], self.tail)
        return y


WAYS = ("far_in", "far_out", "both_far")


def run_far_wide(entry, lay_in_of, lay_out_of, way, calls):
    """the far twin of an entry with separate input and output strides: far input with compact output, compact input with far output,
    or both far; out of place (these entries have no other form)"""
    import torch
    far, twin, dry = entry.make(), entry.make(), entry.make(eq=False)
    st = torch.cuda.current_stream().cuda_stream
    S, K = entry.S, entry.K
    tag = f"stream-placement far {entry.name}, {way}"
    for k, nb in enumerate(calls):
        frames = nb * BLOCK
        li = lay_in_of(frames) if way != "far_out" else sp.compact_layout(S, K, frames)
        lo = lay_out_of(frames) if way != "far_in" else sp.compact_layout(S, 2, frames)
        what = f"{tag}, {lay_in_of(frames).name}: call {k} ({nb} blocks)"
        print(f"{what} ...", flush=True)
        x = entry.input(k, calls)
        xt = _dev(x)
        if li.lead:
            d_in = _far_buffer(li, SENT_IN)
            sp.far_place(d_in, xt, li)
        else:
            d_in = xt.clone().reshape(-1)
        d_out = _far_buffer(lo, SENT_OUT) if lo.lead else torch.empty(lo.total, dtype=torch.float32, device="cuda")
        entry.ptr(far, k, nb, d_in.data_ptr() + 4 * li.lead, d_out.data_ptr() + 4 * lo.lead, li, lo, st)
        torch.cuda.synchronize()
        ref, d = entry.tensor(twin, k, nb, xt.clone()), entry.tensor(dry, k, nb, xt.clone())
        torch.cuda.synchronize()
        rf, rt = entry.records(far), entry.records(twin)
        print(f"{tag}: call {k} -> far {rf}, twin {rt}", flush=True)
        assert {a: v for a, v in rf.items() if a != "eq"} == {a: v for a, v in rt.items() if a != "eq"}, f"{what}: far {rf}, twin {rt}"
        if lo.lead:
            sp.far_gaps_intact(d_out, lo, SENT_OUT, what + ", output buffer")
        if li.lead:
            sp.far_gaps_intact(d_in, li, SENT_IN, what + ", input buffer")
        sp.assert_same_streams(sp.far_take(d_in, li), xt, what + ", the input chains")
        y = sp.far_take(d_out, lo)
        assert bool(torch.isfinite(y).all()), f"{what}: non-finite output: an offset landed in the sentinel"
        sp.assert_same_streams(y, ref, what)
        dn = d.cpu().numpy()
        sp.assert_sample_within_bar(dn, entry.dry_model(k, nb, x), list(range(S)), BAR, what + ", EQ off, against the f64 model")
        _same_bits(ref.cpu().numpy(), entry.eq_of(dn), what + ", the oracle EQ of the dry output")
        del d_in, d_out, y
    torch.cuda.empty_cache()


WIDE_CALLS = (5, 4)


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("scheduled", [False, True], ids=["layout", "layout_scheduled"])
def test_far_f1_layout_entries(oracle, scheduled, way):
    """F1, S = 3, six channels: input channel stride frames + 4, output channel stride frames + 8.
    Device memory: 6.1 GiB per far buffer, 12.2 GiB with both far."""
    _need(12.5 if way == "both_far" else 6.5)
    run_far_wide(FarLayoutEntry(6, scheduled, 3, WIDE_CALLS, oracle), lambda f: sp.layout_f1(f, 6, 1), lambda f: sp.layout_f1(f, 2, 2), way,
                 WIDE_CALLS)


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("scheduled", [False, True], ids=["layout", "layout_scheduled"])
def test_far_f2_layout_entries(oracle, scheduled, way):
    """F2, S = 1, three input channels 2^30 + 2052 floats apart (the odd last channel beyond 2^33 bytes), two output channels alike.
    Device memory: input 10.0 GiB, output 6.0 GiB, 16.0 GiB with both far."""
    _need({"far_in": 10.5, "far_out": 6.5, "both_far": 16.5}[way])
    run_far_wide(FarLayoutEntry(3, scheduled, 1, WIDE_CALLS, oracle), lambda f: sp.layout_f2(f, 3), lambda f: sp.layout_f2(f, 2), way, WIDE_CALLS)


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("blend", [False, True], ids=["scene", "blend_scene"])
@pytest.mark.parametrize("lay", ["F1", "F2"])
def test_far_object_scenes(oracle, lay, blend, way):
    """ohs_scene_process and ohs_scene2_process_blended, three objects: F1 at S = 3, F2 at S = 1.
    Device memory: F1 12.2 GiB with both far; F2 input 10.0 GiB, output 6.0 GiB, 16.0 GiB with both far."""
    _need((12.5 if way == "both_far" else 6.5) if lay == "F1" else {"far_in": 10.5, "far_out": 6.5, "both_far": 16.5}[way])
    S = 3 if lay == "F1" else 1
    lin = (lambda f: sp.layout_f1(f, 3, 1)) if lay == "F1" else (lambda f: sp.layout_f2(f, 3))
    lout = (lambda f: sp.layout_f1(f, 2, 2)) if lay == "F1" else (lambda f: sp.layout_f2(f, 2))
    run_far_wide(FarSceneEntry(3, blend, S, WIDE_CALLS, oracle), lin, lout, way, WIDE_CALLS)


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("lay", ["F1", "F2"])
def test_far_node_batch(oracle, lay, in_place):
    """ohs_node_batch_process over one device slot on far chains, against the same node batch's twin on compact tensors.
    Device memory: 12.2 GiB out of place, 6.1 GiB in place."""
    import torch
    _need(12.5 if not in_place else 6.5)
    lay_of = sp.layout_f1 if lay == "F1" else sp.layout_f2
    S, case, calls = lay_of(BLOCK).S, NodeBatch(), (7, 6)
    far, twin = case.make(S, {}), case.make(S, {})
    model = case.model(oracle, S, {})
    tag = f"stream-placement far node_batch, {'in place' if in_place else 'out of place'}, {lay}"
    for k, nb in enumerate(calls):
        L = lay_of(nb * BLOCK)
        what = f"{tag}: call {k} ({nb} blocks)"
        print(f"{what} ...", flush=True)
        x = _stereo_input(S, k, calls, first_id=6500)
        xt = _dev(x)
        d_in = _far_buffer(L, SENT_IN)
        sp.far_place(d_in, xt, L)
        d_out = d_in if in_place else _far_buffer(L, SENT_OUT)
        torch.cuda.synchronize()
        base = 4 * L.lead
        far.process_ptrs([d_in.data_ptr() + base], [d_out.data_ptr() + base], nb, L.ss, L.cs)
        far.sync()
        xc = xt.clone()
        torch.cuda.synchronize()
        ref = twin.process([xc], None if in_place else [torch.empty_like(xc)])[0]
        twin.sync()
        rf, rt = case.records(far), case.records(twin)
        print(f"{tag}: call {k} -> far {rf}, twin {rt}", flush=True)
        assert rf["conv"] == rt["conv"], f"{what}: far {rf}, twin {rt}"
        sp.far_gaps_intact(d_out, L, SENT_IN if in_place else SENT_OUT, what + ", output buffer")
        if not in_place:
            sp.far_gaps_intact(d_in, L, SENT_IN, what + ", input buffer")
            sp.assert_same_streams(sp.far_take(d_in, L), xt, what + ", the input chains")
        y = sp.far_take(d_out, L)
        sp.assert_same_streams(y, ref, what)
        sp.assert_sample_within_bar(y.cpu().numpy(), model.process(x), list(range(S)), BAR, what + ", against tests/batch_model.py")
        del d_in, d_out, y
    torch.cuda.empty_cache()


# ---- C: one long call whose chains cross 2^31 and 2^32 bytes ------------------------------------------------------------------------
LONG_BLOCKS = (1 << 21) + 3
WINDOW = 2048
SLAB = 1 << 20


def _f64_window(x_at, irs, w0, n):
    """GAIN * the four-path convolution's frames [w0, w0 + n) in f64 from the input frames they can see; x_at(c, a, b) -> channel c's
    frames [a, b) float32 (a >= 0)"""
    taps = max(len(h) for h in irs)
    a = max(0, w0 - (taps - 1))
    xs = [np.asarray(x_at(c, a, w0 + n), np.float64) for c in range(2)]
    y = np.zeros((2, n))
    for p, h in enumerate(irs):
        y[bm.EAR[p]] += np.convolve(xs[bm.SRC[p]], np.asarray(h, np.float64))[w0 - a:w0 - a + n]
    return GAIN * y


@pytest.mark.parametrize("taps,plan", [(512, 1), (1300, 0), (1300, 1)], ids=["taps512-plan1", "taps1300-auto", "taps1300-plan1"])
def test_one_long_call_crosses_2_31_and_2_32_bytes(taps, plan):
    """S = 1, EQ off, gain 0.75, out of place, ONE call of 2^21 + 3 blocks: each chain is 4 GiB + 6 KiB.  Windows of 2048 output frames
    -- the first, around frame 2^29 (byte 2^31), around 2^30 (byte 2^32), the last -- against f64 direct convolution of the input
    frames they can see, at tests.util.assert_parity's 1e-6; the whole output finite; the RMS of every slab of 2^20 frames within 2 %
    of the median slab's (white noise through a fixed response: the slabs agree to a fraction of a percent, so a stretch of zeros or
    of another stretch's data cannot hide between the windows); then 7 more blocks on the same handle, whose first window sees the
    long call's last input frames.  The block-8192 family must not serve the long call (its 32-bit byte offsets: call_frames < 2^29
    in csrc/api_conv.hip).  Both buffers carry the far layouts' lead and sentinels.
    Device memory: 10.0 GiB per buffer, 20.1 GiB with the handle's state."""
    import torch
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    from tests.util import assert_parity
    _need(21.0)
    frames = LONG_BLOCKS * BLOCK
    lay = sp.FarLayout("long", 1, 2, frames, 2 * (frames + 2052), frames + 2052)
    irs = synth.hrir_set(taps)
    bp = ohs.BatchProcessor(1, num_bands=10)
    for p in range(4):
        bp.set_ir(p, irs[p])
    bp.set_conv_plan(plan)
    bp.set_gain(GAIN)
    bp.set_eq_enabled(False)
    tag = f"stream-placement long call, taps {taps}, plan {plan}"
    d_in, d_out = _far_buffer(lay, SENT_IN), _far_buffer(lay, SENT_OUT)
    step = 1 << 24
    for f0 in range(0, frames, step):
        n = min(step, frames - f0)
        piece = synth.white_noise_torch(9000, 1, n, d_in.device, offset=f0)
        for c in range(2):
            d_in[lay.start(0, c) + f0:lay.start(0, c) + f0 + n] = piece[0, c]
    del piece
    torch.cuda.synchronize()
    print(f"{tag}: call 0 ({LONG_BLOCKS} blocks) ...", flush=True)
    base = 4 * lay.lead
    bp.process_ptr(d_in.data_ptr() + base, d_out.data_ptr() + base, LONG_BLOCKS, lay.ss, lay.cs, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    served = bp.last_conv_plan()
    print(f"{tag}: call 0 -> {served}", flush=True)
    assert served[0] not in ("none", "block8192"), served
    if plan == 1:
        assert served[0] == ("block512_p1" if taps <= 512 else "block512_tp"), served
    sp.far_gaps_intact(d_out, lay, SENT_OUT, tag + ", output buffer")
    sp.far_gaps_intact(d_in, lay, SENT_IN, tag + ", input buffer")

    def x_at(c, a, b):
        return d_in[lay.start(0, c) + a:lay.start(0, c) + b].cpu().numpy()

    def y_at(a, b):
        return np.stack([d_out[lay.start(0, c) + a:lay.start(0, c) + b].cpu().numpy() for c in range(2)])
    for w0 in (0, (1 << 29) - WINDOW // 2, (1 << 30) - WINDOW // 2, frames - WINDOW):
        a, r = assert_parity(y_at(w0, w0 + WINDOW), _f64_window(x_at, irs, w0, WINDOW), f"{tag}: frames [{w0}, {w0 + WINDOW})")
        print(f"{tag}: window at frame {w0} (byte {4 * w0:#x}): abs RMS {a:.3e}, rel RMS {r:.3e}")
    # the whole output: finite, and every slab as loud as the median slab
    n_slabs = frames // SLAB
    for c in range(2):
        chain = d_out[lay.start(0, c):lay.start(0, c) + frames]
        rms = []
        for s0 in range(0, n_slabs, 64):
            part = chain[s0 * SLAB:min(s0 + 64, n_slabs) * SLAB].view(-1, SLAB)
            assert bool(torch.isfinite(part).all()), f"{tag}: non-finite output in channel {c}, slabs {s0} .. {s0 + 63}"
            rms.append(part.double().pow(2).mean(dim=1).sqrt())
        assert bool(torch.isfinite(chain[n_slabs * SLAB:]).all())
        rms = torch.cat(rms).cpu().numpy()
        med = float(np.median(rms))
        off = np.flatnonzero(np.abs(rms / med - 1.0) > 0.02)
        print(f"{tag}: channel {c}: {n_slabs} slabs, median RMS {med:.5f}, min {rms.min() / med:.4f}, max {rms.max() / med:.4f} of it")
        assert med > 0.01 and off.size == 0, f"{tag}: channel {c}: {off.size} slab(s) off the median RMS {med:.5f} by more than 2 %: {off[:8]} -> {rms[off[:8]]}"
    # seven more blocks: the state the long call left behind
    print(f"{tag}: call 1 (7 blocks) ...", flush=True)
    x2 = synth.white_noise_torch(9000, 1, 7 * BLOCK, d_in.device, offset=frames)
    y2 = bp.process(x2)
    torch.cuda.synchronize()
    print(f"{tag}: call 1 -> {bp.last_conv_plan()}", flush=True)
    hist = max(len(h) for h in irs) - 1
    tail = np.stack([x_at(c, frames - hist, frames) for c in range(2)])
    both = np.concatenate([tail, x2[0].cpu().numpy()], axis=1)
    a, r = assert_parity(y2[0, :, :WINDOW].cpu().numpy(), _f64_window(lambda c, a, b: both[c, a:b], irs, hist, WINDOW),
                         f"{tag}: the first window of the call behind the long one")
    print(f"{tag}: the call behind it: abs RMS {a:.3e}, rel RMS {r:.3e}")
    del d_in, d_out
    torch.cuda.empty_cache()

"""Every convolution family at response lengths that sit on a partition edge, on edge-loaded responses (tests/ir_edges.py: flat
noise plus taps of magnitude about 1 at index 0, at taps - 1 and at b - 1, b, b + 1 for b in 512, 2048, 8192).

White noise, EQ off, gain 1, three distinct streams (32 where the block-8192 kernel asks for them), two or more consecutive calls on
one handle, Pmax + 6 blocks in all; compared with the oracle engine AND with an f64 FFT convolution, both at 1e-6 relative RMS per
stream and per block of 512 frames (tests/util.RMS_TOL), and last_conv_plan() must name the family the case is meant to run.  The
impulse probe reads the response back tap for tap against the bar measured on the oracle (tests/ir_edges.IMPULSE_BAR)."""
import numpy as np
import pytest

from tests import ir_edges as ie
from tests.ir_edges import BLOCK, LENGTHS, partitions
from tests.util import RMS_TOL

pytestmark = pytest.mark.gpu

S = 3
PATH_ALONE = 2          # the path the one-path set_ir cases re-load


def _handle(irs, plan, streams=S, lib=None):
    import open_headstage_amd as ohs
    bp = ohs.BatchProcessor(streams, num_bands=10, library=lib)
    for p in range(4):
        bp.set_ir(p, irs[p])
    bp.set_eq_enabled(False)
    bp.set_gain(1.0)
    bp.set_conv_plan(plan)
    return bp


def _engines(oracle, irs, n=S):
    out = []
    for _ in range(n):
        e = oracle.ConvolutionEngine()
        for p in range(4):
            e.set_ir(p, irs[p])
        out.append(e)
    return out


def _noise(first_id, frames, streams=S):
    from open_headstage_amd import synth
    return synth.white_noise(range(first_id, first_id + streams), frames)


def _call(bp, x, in_place=False):
    """x [S][2][n * 512] numpy -> the call's output, numpy"""
    import torch
    xt = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    y = bp.process(xt, out=xt) if in_place else bp.process(xt)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _run(bp, x, calls, want, what, in_place=False, hook=None):
    """consecutive calls of calls[k] blocks on one handle; want: the family of every call, or a function (k, blocks in front of the
    call) -> family or tuple of families; hook(k, frame): what happens in front of call k"""
    assert sum(calls) * BLOCK == x.shape[2], (calls, x.shape)
    got, pos = [], 0
    for k, nb in enumerate(calls):
        if hook is not None:
            hook(k, pos * BLOCK)
        got.append(_call(bp, x[:, :, pos * BLOCK:(pos + nb) * BLOCK], in_place))
        fam = bp.last_conv_plan()[0]
        w = want(k, pos) if callable(want) else want
        assert fam in ((w,) if isinstance(w, str) else w), f"{what}: call {k} ({nb} blocks from block {pos}) was served by {fam}, not {w}"
        pos += nb
    return np.concatenate(got, axis=2)


def _oracle_out(engs, x):
    return np.stack([np.stack(e.process_block(xs[0], xs[1])) for e, xs in zip(engs, x)])


def _hold(oracle, y, x, irs, family, taps, streams=None):
    """y against the oracle engine and against f64, per stream and block"""
    streams = range(len(x)) if streams is None else streams
    wo = ie.check(y, _oracle_out(_engines(oracle, irs, len(x)), x), streams, family, taps, "the oracle engine")
    wf = ie.check(y, ie.reference_f64(x, irs), streams, family, taps, "f64")
    print(f"ir-edges {family}, taps {taps}: worst block against the oracle {wo:.2e}, against f64 {wf:.2e}")
    assert max(wo, wf) <= RMS_TOL


# ---- one-partition families ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("taps", LENGTHS["block512_p1"])
@pytest.mark.parametrize("plan,family", [(1, "block512_p1"), (2, "hop1536_p1")])
def test_one_partition_families(oracle, plan, family, taps, in_place):
    irs = ie.edge_loaded_irs(taps)
    x = _noise(10 + taps, 7 * BLOCK)
    y = _run(_handle(irs, plan), x, (3, 4), family, f"{family}, taps {taps}", in_place)
    _hold(oracle, y, x, irs, family, taps)


# ---- families for longer responses --------------------------------------------------------------------------------------------------
def _sequential_case(exp_tuning, irs, x, what):
    """The general kernel serves a handle that keeps no input history (the experiments library with lb_min_p out of reach) behind a
    per-path set_ir, while that path is younger than its response and the call is shorter than Pmax: a first call of 3 blocks, path 1
    re-loaded with the SAME response, then calls of 1 .. 3 blocks.  -> (y, timeline for the references: path 1 forgets at frame 1536)"""
    exp_tuning("lb_min_p", 99)
    P = max(partitions(len(h)) for h in irs)
    bp = _handle(irs, 1, lib=exp_tuning.lib)
    blocks = x.shape[2] // BLOCK
    calls, left, k = [3], blocks - 3, 0
    while left:
        n = min((1, 2, 3)[k % 3], P - 1, left)
        calls.append(n)
        left, k = left - n, k + 1

    def hook(k, frame):
        if k == 1:
            bp.set_ir(1, irs[1])

    def want(k, pos):
        return "block512_tp" if k == 0 or pos - 3 >= P - 1 else "sequential"
    y = _run(bp, x, calls, want, what, hook=hook)
    assert bp.conv_plan_counts().get("sequential", 0) >= 1
    return y, [irs[0], [(0, irs[1]), (3 * BLOCK, irs[1])], irs[2], irs[3]]


def _hold_timeline(oracle, y, x, timeline, family, taps):
    """as _hold, for responses that change in mid-stream: the oracle engines get the same edits at the same frames"""
    tl = ie.timeline_of(timeline)
    edits = sorted({t for path in tl for t, _ in path})
    engs = [oracle.ConvolutionEngine() for _ in x]
    ref = []
    for a, b in zip(edits, edits[1:] + [x.shape[2]]):
        for p, path in enumerate(tl):
            for t, h in path:
                if t == a:
                    for e in engs:
                        e.set_ir(p, h)
        ref.append(_oracle_out(engs, x[:, :, a:b]))
    wo = ie.check(y, np.concatenate(ref, axis=2), range(len(x)), family, taps, "oracle engines given the same edits")
    wf = ie.check(y, ie.reference_f64(x, timeline), range(len(x)), family, taps, "f64")
    print(f"ir-edges {family}, taps {taps}: worst block against the oracle {wo:.2e}, against f64 {wf:.2e}")
    assert max(wo, wf) <= RMS_TOL


@pytest.mark.parametrize("taps", LENGTHS["sequential"])
def test_sequential_kernel(exp_tuning, oracle, taps):
    irs = ie.edge_loaded_irs(taps)
    x = _noise(20 + taps, (partitions(taps) + 6) * BLOCK)
    y, timeline = _sequential_case(exp_tuning, irs, x, f"sequential, taps {taps}")
    _hold_timeline(oracle, y, x, timeline, "sequential", taps)


@pytest.mark.parametrize("taps", LENGTHS["block512_tp"])
def test_time_parallel_block_512(oracle, taps):
    irs = ie.edge_loaded_irs(taps)
    blocks = partitions(taps) + 6
    x = _noise(30 + taps, blocks * BLOCK)
    y = _run(_handle(irs, 1), x, (4, blocks - 4), "block512_tp", f"block512_tp, taps {taps}")
    _hold(oracle, y, x, irs, "block512_tp", taps)


@pytest.mark.parametrize("taps", LENGTHS["block2048"])
@pytest.mark.parametrize("plan", [2, 0])
def test_block_2048(oracle, plan, taps):
    """(5 blocks, the rest): the second call starts inside a 2048-frame block of the stream's grid"""
    irs = ie.edge_loaded_irs(taps)
    blocks = partitions(taps) + 6
    x = _noise(40 + taps, blocks * BLOCK)
    y = _run(_handle(irs, plan), x, (5, blocks - 5), "block2048", f"block2048 under plan {plan}, taps {taps}")
    _hold(oracle, y, x, irs, f"block2048 (plan {plan})", taps)


# ---- block 8192 ---------------------------------------------------------------------------------------------------------------------
XB_BLOCKS = 128         # the shortest call the product library gives the kernel


def _xb_streams(taps):
    return 32 if taps > 8192 else S     # (two partitions of 8192 taps: from 32 streams on)


def _xb_sample(streams, taps):
    return [0, 1, 2] if streams == 3 else [0, int(np.random.default_rng(taps).integers(1, streams - 1)), streams - 1]


def _xb_run(irs, taps, x_of, want):
    """two out-of-place calls of 128 blocks on `streams` streams; x_of(device) -> [streams][2][2 * 128 * 512] on the device"""
    import torch
    streams = _xb_streams(taps)
    bp = _handle(irs, 0, streams)
    x = x_of(torch.device("cuda:0"), streams)
    ys = []
    for c in range(2):
        ys.append(bp.process(x[:, :, c * XB_BLOCKS * BLOCK:(c + 1) * XB_BLOCKS * BLOCK].contiguous()))
        torch.cuda.synchronize()
        assert bp.last_conv_plan()[0] == want, (taps, streams, c, bp.last_conv_plan())
    sample = _xb_sample(streams, taps)
    idx = torch.as_tensor(sample, device=x.device)
    return torch.cat(ys, dim=2)[idx].cpu().numpy(), x[idx].cpu().numpy(), sample


@pytest.mark.parametrize("taps", LENGTHS["block8192"] + (16385,))
def test_block_8192(oracle, taps):
    """at 16385 taps P2x would be 3: the record must say block2048"""
    from open_headstage_amd import synth
    irs = ie.edge_loaded_irs(taps)
    want = "block2048" if taps == 16385 else "block8192"
    y, x, sample = _xb_run(irs, taps, lambda dev, n: synth.white_noise_torch(50 + taps, n, 2 * XB_BLOCKS * BLOCK, dev), want)
    _hold(oracle, y, x, irs, want if taps != 16385 else "block2048 (P2x = 3)", taps, streams=sample)


# ---- mixed paths on both sides of an edge in one handle -----------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", ie.MIXED, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("plan,family,first", [(1, "block512_tp", 4), (2, "block2048", 5)])
def test_mixed_paths_on_both_sides_of_an_edge(oracle, plan, family, first, lengths):
    irs = ie.mixed_irs(lengths)
    blocks = max(partitions(t) for t in lengths) + 6
    x = _noise(60 + lengths[0], blocks * BLOCK)
    y = _run(_handle(irs, plan), x, (first, blocks - first), family, f"{family}, paths of {lengths} taps")
    _hold(oracle, y, x, irs, family, lengths)


# ---- set_ir across an edge in mid-stream --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", [0, 1])
@pytest.mark.parametrize("paths", ["all_paths", "one_path"])
@pytest.mark.parametrize("start", ["up_first", "down_first"])
@pytest.mark.parametrize("edge", ie.TRANSITIONS, ids=lambda v: f"{v[0]}-{v[1]}")
def test_set_ir_across_an_edge_in_mid_stream(oracle, edge, start, paths, plan):
    """a -> b -> a (up, then down) and b -> a -> b: three phases of P(b) + 3 blocks, each in calls of 2 blocks and the rest -- the
    two blocks behind every edit are a call of their own, and the per-block metric holds each of them on its own.  512 <-> 513 hands
    the state from a one-partition family to block 2048 (plan 0) or the time-parallel kernels (plan 1) and back."""
    a, b = edge if start == "up_first" else edge[::-1]
    n = partitions(max(edge)) + 3
    which = range(4) if paths == "all_paths" else (PATH_ALONE,)
    sets = [ie.edge_loaded_irs(t, seed=k) for k, t in enumerate((a, b, a))]
    x = _noise(70 + a, 3 * n * BLOCK)
    bp = _handle(sets[0], plan)
    now = [len(h) for h in sets[0]]
    timeline = [[(0, h)] for h in sets[0]]

    def hook(k, frame):
        if k and k % 2 == 0:
            for p in which:
                bp.set_ir(p, sets[k // 2][p])
                timeline[p].append((frame, sets[k // 2][p]))
                now[p] = len(sets[k // 2][p])

    def want(k, pos):
        if max(partitions(t) for t in now) == 1:
            return "block512_p1" if plan == 1 else ("block512_p1", "hop1536_p1")
        return "block2048" if plan == 0 else ("block512_tp", "sequential")
    what = f"set_ir {a} -> {b} -> {a}, {paths}, plan {plan}"
    y = _run(bp, x, (2, n - 2) * 3, want, what, hook=hook)
    _hold_timeline(oracle, y, x, timeline, what, (a, b, a))


# ---- the impulse probe --------------------------------------------------------------------------------------------------------------
def _probe_report(fig, family, taps):
    print(f"ir-edges impulse probe, {family}, taps {taps}: max |error| / max |h| = {fig:.2e} (bar {ie.IMPULSE_BAR:.1e})")


@pytest.mark.parametrize("plan,family", [(1, "block512_p1"), (2, "hop1536_p1")])
def test_impulse_probe_one_partition(plan, family):
    irs = ie.edge_loaded_irs(512)
    y = _run(_handle(irs, plan), ie.probe_input(S, 7 * BLOCK), (3, 4), family, f"probe, {family}")
    _probe_report(ie.assert_probe(y, irs, family, 512), family, 512)


@pytest.mark.parametrize("taps", [t for t in LENGTHS["probe"] if t > 512])
@pytest.mark.parametrize("family", ["sequential", "block512_tp", "block2048"])
def test_impulse_probe_longer_responses(exp_tuning, family, taps):
    irs = ie.edge_loaded_irs(taps)
    blocks = partitions(taps) + 6
    x = ie.probe_input(S, blocks * BLOCK)
    want = None
    if family == "sequential":      # (path 1 is re-loaded behind block 2 and forgets stream 0's impulse: the expectation follows the edit)
        y, timeline = _sequential_case(exp_tuning, irs, x, f"probe, sequential, taps {taps}")
        want = ie.reference_f64(x, timeline)
    elif family == "block512_tp":
        y = _run(_handle(irs, 1), x, (4, blocks - 4), family, f"probe, {family}, taps {taps}")
    else:
        y = _run(_handle(irs, 2), x, (5, blocks - 5), family, f"probe, {family}, taps {taps}")
    _probe_report(ie.assert_probe(y, irs, family, taps, want=want), family, taps)


@pytest.mark.parametrize("taps", [t for t in LENGTHS["probe"] if t > 512])
def test_impulse_probe_block_8192(taps):
    import torch
    irs = ie.edge_loaded_irs(taps)
    y, _, sample = _xb_run(irs, taps, lambda dev, n: torch.from_numpy(ie.probe_input(n, 2 * XB_BLOCKS * BLOCK)).to(dev), "block8192")
    _probe_report(ie.assert_probe(y, irs, "block8192", taps, streams=sample), "block8192", taps)


# ---- the engine ---------------------------------------------------------------------------------------------------------------------
def _engine_sizes(frames):
    sizes, k = [], 0
    while frames:
        n = min((1024, 512, 2048)[k % 3], frames)
        sizes.append(n)
        frames, k = frames - n, k + 1
    return sizes


def _engine_run(form, ge, x, sizes):
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    eq = ohs.StereoParametricEQ.new(10, synth.FS) if form == "chain" else None
    out, o = [], 0
    for n in sizes:
        l, r = x[0, o:o + n].copy(), x[1, o:o + n].copy()
        if form == "chain":
            ohs.process_chain(ge, eq, l, r, master_bypass=False, eq_enable=False, output_gain=1.0)
            out.append(np.stack([l, r]))
        else:
            out.append(np.stack(ge.process_block(l, r)))
        o += n
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("taps", LENGTHS["engine"])
@pytest.mark.parametrize("form", ["launch_per_call", "chain"])
def test_engine(oracle, form, taps):
    """host blocks of 1024, 512 and 2048 frames in turn: calls of 1 and 2 blocks take the general kernel, calls of 4 the
    time-parallel ones"""
    irs = ie.edge_loaded_irs(taps)
    ge = _fresh_engine(irs)
    assert [ge.num_partitions(p) for p in range(4)] == [partitions(taps)] * 4
    x = _noise(80 + taps, (partitions(taps) + 6) * BLOCK, 1)
    y = _engine_run(form, ge, x[0], _engine_sizes(x.shape[2]))[None]
    _hold(oracle, y, x, irs, f"engine ({form})", taps)
    probe = _engine_run(form, _fresh_engine(irs), ie.probe_input(1, x.shape[2])[0], _engine_sizes(x.shape[2]))[None]
    fig = ie.assert_probe(probe, irs, f"engine ({form})", taps)
    _probe_report(fig, f"engine ({form})", taps)


def _fresh_engine(irs):
    import open_headstage_amd as ohs
    ge = ohs.ConvolutionEngine.new()
    for p in range(4):
        ge.set_ir(p, irs[p])
    return ge


def test_engine_partition_counts(oracle):
    """num_partitions(path) == ceil(len / 512), and 1 for an empty response (the batch handle reports no partition count)"""
    import open_headstage_amd as ohs
    ge, eo = ohs.ConvolutionEngine.new(), oracle.ConvolutionEngine()
    lengths = (0,) + tuple(ie.all_lengths())
    for i in range(0, len(lengths), 4):
        group = (lengths[i:i + 4] + lengths[:4])[:4]
        for p, t in enumerate(group):
            h = ie.edge_loaded_irs(t, seed=p)[p]
            ge.set_ir(p, h)
            eo.set_ir(p, h)
        want = [partitions(t) for t in group]
        assert [ge.num_partitions(p) for p in range(4)] == want == [eo.num_partitions(p) for p in range(4)], group


# ---- the table families: exactly one partition --------------------------------------------------------------------------------------
N_SETS, K_LAYOUT, N_DIRS, K_OBJECTS = 4, 3, 7, 3
TABLE_CALLS = (5, 4)


def _sets(taps, seed=0):
    return np.stack([np.stack(ie.edge_loaded_irs(taps, seed=seed + i)) for i in range(N_SETS)])


def _layout_table(taps, seed=0):
    return np.stack([ie.edge_loaded_table(K_LAYOUT, taps, seed=seed + i) for i in range(N_SETS)])


def _rows(seed, n_segs):
    """[S][n_segs]: every stream changes its set at every segment"""
    rng = np.random.default_rng(seed)
    first = rng.integers(0, N_SETS, (S, 1))
    return ((first + np.cumsum(rng.integers(1, N_SETS, (S, n_segs)), axis=1)) % N_SETS).astype(np.int64)


def _model(oracle, irs):
    from tests import batch_model as bm
    m = bm.HandleModel(oracle, S)
    for p in range(4):
        m.set_ir(p, irs[p])
    return m


def _table_check(y, ref, family, taps):
    w = ie.check(y, ref, range(S), family, taps, "the f64 model")
    print(f"ir-edges {family}, taps {taps}: worst block against the f64 model {w:.2e}")
    assert w <= RMS_TOL


def _ir_schedule_calls(bp, model, taps, seed):
    """a ring-out call, a cut call, a crossfaded call on one handle -> [(what, y, model's f64)]"""
    import torch
    out = []
    for k, (kind, nb) in enumerate((("ring_out", 5), ("cut", 4), ("crossfaded", 5))):
        x = _noise(1000 * seed + 10 * k, nb * BLOCK)
        rows = _rows(seed + k, -(-nb // 2))
        xt = torch.from_numpy(x).cuda()
        if kind == "crossfaded":
            prev = (rows[:, 0] + 1) % N_SETS
            y, ref = bp.process_ir_crossfaded(xt, 2, rows, prev), model.process_ir_crossfaded(x, 2, rows, prev)
        else:
            y, ref = bp.process_ir_scheduled(xt, 2, rows, kind), model.process_ir_scheduled(x, 2, rows, kind)
        torch.cuda.synchronize()
        assert bp.last_conv_plan()[0] == "block512_p1" and bp.last_conv_ir_scheduled(), (kind, bp.last_conv_plan())
        out.append((f"IR schedule ({kind})", y.cpu().numpy(), ref))
    return out


@pytest.mark.parametrize("taps", LENGTHS["tables"])
def test_ir_schedules_plain_and_crossfaded(oracle, taps):
    own, sets = ie.edge_loaded_irs(taps, seed=9), _sets(taps)
    bp, model = _handle(own, 1), _model(oracle, own)
    bp.set_schedule_irs(sets)
    model.set_schedule_irs(sets)
    for what, y, ref in _ir_schedule_calls(bp, model, taps, 3):
        _table_check(y, ref, what, taps)


def _layout_calls(bp, model, seed):
    """two plain layout calls, then a crossfaded and a ring-out call on the table -> [(what, y, model's f64)]"""
    import torch
    from tests.test_cpu_layout import make_input
    out = []
    for k, nb in enumerate(TABLE_CALLS):
        x = make_input(S, K_LAYOUT, nb, seed=2000 + 100 * seed + 10 * k)
        y = bp.process_layout(torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        out.append(("layout", y.cpu().numpy(), _dry(model, model.process_layout(x))))
    for k, (fade, nb) in enumerate(((True, 5), (False, 4))):
        x = make_input(S, K_LAYOUT, nb, seed=3000 + 100 * seed + 10 * k)
        rows = _rows(seed + 7 + k, -(-nb // 2))
        prev = (rows[:, 0] + 1) % N_SETS
        y = bp.process_layout_scheduled(torch.from_numpy(x).cuda(), rows, 2, prev, fade)
        torch.cuda.synchronize()
        assert bp.last_layout_scheduled()
        out.append((f"layout table ({'crossfaded' if fade else 'ring-out'})", y.cpu().numpy(),
                    _dry(model, model.process_layout_scheduled(x, rows, 2, prev, fade))))
    return out


def _dry(model, y):
    """the model's layout kinds return the dry signal and expect their EQ to follow; the EQ is off here"""
    model._eq_pending = False
    return y


@pytest.mark.parametrize("taps", LENGTHS["tables"])
def test_layouts_and_layout_tables(oracle, taps):
    own = ie.edge_loaded_irs(taps, seed=9)
    bp, model = _handle(own, 1), _model(oracle, own)
    lay, table = ie.edge_loaded_table(K_LAYOUT, taps, seed=5), _layout_table(taps, seed=6)
    bp.set_layout_irs(lay)
    model.set_layout_irs(lay)
    bp.set_layout_table(table)
    model.set_layout_table(table)
    for what, y, ref in _layout_calls(bp, model, 1):
        _table_check(y, ref, what, taps)


def _scene_calls(blend, sc, dirs):
    """two consecutive calls (the overlap carries over), crossfaded and ring-out -> [(what, y, model's f64)]"""
    import torch
    from tests import scene_blend_model as sbm
    from tests import scene_model as sm
    from tests.test_cpu_layout import make_input
    out, tail = [], None
    for k, (fade, nb) in enumerate(((True, 5), (False, 4))):
        x = make_input(S, K_OBJECTS, nb, seed=4000 + 10 * k + (500 if blend else 0))
        xt = torch.from_numpy(x).cuda()
        if blend:
            a = sbm.make_blend_scene(S, K_OBJECTS, nb, 2, n_dirs=N_DIRS, seed=k)
            y = sc.process(xt, a["idx"], 2, a["gains"], a["prev_idx"], a["prev_gains"], fade, a["idx1"], a["weights"], a["prev_idx1"],
                           a["prev_weights"])
            ref, tail = sbm.model_blend_f64(x, dirs, a["idx"], a["idx1"], a["weights"], 2, a["gains"], a["prev_idx"], a["prev_idx1"],
                                            a["prev_weights"], a["prev_gains"], fade, 1.0, tail, with_tail=True)
        else:
            idx, gains, pi, pg = sm.make_scene(S, K_OBJECTS, nb, 2, n_dirs=N_DIRS, seed=k)
            y = sc.process(xt, idx, 2, gains, pi, pg, fade)
            ref, tail = sm.model_scene_f64(x, dirs, idx, 2, gains, pi, pg, fade, 1.0, tail, with_tail=True)
        torch.cuda.synchronize()
        out.append((f"{'blended ' if blend else ''}object scene ({'crossfaded' if fade else 'ring-out'})", y.cpu().numpy(), ref))
    return out


def _scene(blend):
    import open_headstage_amd as ohs
    sc = (ohs.BlendSceneProcessor if blend else ohs.SceneProcessor)(S, num_bands=10)
    sc.set_gain(1.0)
    sc.set_eq_enabled(False)
    return sc


@pytest.mark.parametrize("taps", LENGTHS["tables"])
@pytest.mark.parametrize("blend", [False, True], ids=["scene", "blend_scene"])
def test_object_directions(blend, taps):
    dirs = ie.edge_loaded_table(N_DIRS, taps, seed=8)
    sc = _scene(blend)
    sc.set_directions(dirs)
    for what, y, ref in _scene_calls(blend, sc, dirs):
        _table_check(y, ref, what, taps)


# ---- a table of 513 taps: the headers refuse it, and the handle keeps the table it had ---------------------------------------------
def _bits_equal(a, b, what):
    for (wa, ya, _), (_, yb, _) in zip(a, b):
        assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32)), f"{what}: {wa} differs after the refused upload"


def test_a_513_tap_table_is_refused_and_the_batch_handle_keeps_its_tables(oracle):
    """include/ohs_hip.h: ohs_batch_set_schedule_irs, ohs_batch_set_layout_irs and ohs_batch_set_layout_schedule_irs return
    OHS_ERR_INVALID_ARG for len > 512 before anything is queued, and the handle stays usable: after a reset it renders the tables
    it had, bit for bit"""
    from open_headstage_amd import _ffi
    own = ie.edge_loaded_irs(512, seed=9)
    bp, model = _handle(own, 1), _model(oracle, own)
    sets, lay, table = _sets(512), ie.edge_loaded_table(K_LAYOUT, 512, seed=5), _layout_table(512, seed=6)
    bp.set_schedule_irs(sets)
    bp.set_layout_irs(lay)
    bp.set_layout_table(table)
    model.set_schedule_irs(sets)
    model.set_layout_irs(lay)
    model.set_layout_table(table)
    before = _ir_schedule_calls(bp, model, 512, 3) + _layout_calls(bp, model, 1)
    for setter, arg in ((bp.set_schedule_irs, np.stack([np.stack(ie.edge_loaded_irs(513, seed=i)) for i in range(N_SETS)])),
                        (bp.set_layout_irs, ie.edge_loaded_table(K_LAYOUT, 513)),
                        (bp.set_layout_table, np.stack([ie.edge_loaded_table(K_LAYOUT, 513, seed=i) for i in range(N_SETS)]))):
        with pytest.raises(_ffi.OhsError) as e:
            setter(arg)
        assert e.value.status == _ffi.OHS_ERR_INVALID_ARG, e.value
    bp.reset()
    model.reset()
    after = _ir_schedule_calls(bp, model, 512, 3) + _layout_calls(bp, model, 1)
    _bits_equal(before, after, "batch handle")


@pytest.mark.parametrize("blend", [False, True], ids=["scene", "blend_scene"])
def test_a_513_tap_direction_table_is_refused_and_the_scene_keeps_its_table(blend):
    """include/ohs_scene.h (and ohs_scene2.h by reference): len > 512 is refused, "the handle keeps the table and the overlap it
    had\""""
    from open_headstage_amd.scene import SceneError
    dirs = ie.edge_loaded_table(N_DIRS, 512, seed=8)
    sc = _scene(blend)
    sc.set_directions(dirs)
    before = _scene_calls(blend, sc, dirs)
    with pytest.raises(SceneError) as e:
        sc.set_directions(ie.edge_loaded_table(N_DIRS, 513, seed=8))
    assert e.value.status == 1, e.value         # OHS_SCENE_ERR_INVALID_ARG / OHS_SCENE2_ERR_INVALID_ARG
    sc.reset()
    _bits_equal(before, _scene_calls(blend, sc, dirs), "scene handle")

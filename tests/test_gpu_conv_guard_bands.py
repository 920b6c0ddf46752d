"""Guard bands around every chain for every convolution kernel family: where the kernels load and store.

Nearly every other convolution test hands the library compact [S][2][frames] tensors: a store a few frames behind the end of a
chain lands in the next chain (and is overwritten there) or in the allocator's slack, and the test stays green.  Here every call
goes through the *_ptr entry on a fresh allocation laid out by tests/guard_bands.py -- a gap in front of the first chain, between
every two chains and behind the last one, NaN bits (SENT_IN) in the gaps of whatever is read, 0xDEADBEEF (SENT_OUT) in the gaps of
an output buffer of its own -- while a twin handle of identical configuration gets the same calls on compact tensors.  After EVERY
call:

* family and ranges: both handles report the same last_conv_plan(), and it is the family (for the chunked plans: the range count)
  the case names -- the library is asked, its rule is not restated; a case that fell back to another kernel fails;
* gaps: every gap word of the output buffer is still its sentinel (the failure names chain, offset and length);
* input: out of place the input allocation is bit-identical to what was uploaded;
* bits: the chains equal the twin's output bit for bit, every stream (the plan is chosen from S, the block count, in-place-ness,
  the alignment class and the handle's state, all of which the twin shares: a difference means a load reached a NaN gap, or the
  addressing depends on the stride).

Every case makes at least two calls of different lengths on the same handles: state polluted by a read behind the first call's end
(overlap, tails, input history) shows in the second.  Two layouts per case: `tight` -- every gap the smallest the family's
precondition allows (4 floats for block 2048 / 8192, 2 for hop 1536, 1 for the block-512 families) -- and `wide` -- every gap one
whole block of the family plus a remainder that keeps the alignment and is no multiple of 512, so that a whole extra block stored
behind or in front of a chain lies entirely in sentinel and its extent is reported.

Once per family stream 0 of the guarded output is also held to the project's bar against f64 direct convolution
(tests.util.assert_parity, oracle.binaural_f64): the twin comparison must not be two wrongs agreeing.  (The block-8192 kernel with
two partitions of 8192 taps is carried to the oracle by tests/test_gpu_conv_xb.py.)

Every call prints `guard-bands <case>: call k (n blocks) -> (family, ranges)`: run with -s to see what served it."""
import numpy as np
import pytest

from tests.guard_bands import SENT_IN, SENT_OUT, filled, gaps_intact, layout, place, take
from tests.test_cpu_ir_schedule import make_rows, make_sets
from tests.util import assert_parity

pytestmark = pytest.mark.gpu

BLOCK = 512
GAIN = 0.75
S3 = 3
POW2 = (2, 4, 8, 16)        # chunk counts of k_conv_p1 / k_conv_p1_irs whose chunks compute their own boundary tails


def _gaps(kind, align, block):
    """(lead, channel gap, stream gap, tail) in floats.  tight: every gap is `align`; wide: `block` + a remainder that keeps the
    alignment and is no multiple of 512 (all four different)"""
    if kind == "tight":
        return (align, align, 0, align)
    g = (block + 9 * align, block + 15 * align, 5 * align, block + 21 * align)
    assert all(v % align == 0 for v in g) and all((v - block) % 512 for v in (g[0], g[1], g[3]))
    return g


def _signal(S, first_id, frames):
    """[S][2][frames]: three different streams, repeated"""
    from open_headstage_amd import synth
    base = synth.white_noise(range(first_id, first_id + min(S, 3)), frames)
    return np.ascontiguousarray(base[np.arange(S) % base.shape[0]])


def _handle(S, irs, plan, lib=None, eq=False):
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    bands = synth.eq_table()
    bp = ohs.BatchProcessor(S, num_bands=len(bands), library=lib)
    for p in range(4):
        bp.set_ir(p, irs[p])
    bp.set_conv_plan(plan)
    bp.set_gain(GAIN)
    for i, b in enumerate(bands):
        bp.update_band_coeffs(i, synth.FS, b)
    bp.set_eq_enabled(eq)
    return bp


class Plain:
    """ohs_batch_process: through the pointer entry on the guarded buffers, through the tensor wrapper on the twin's"""
    def ptr(self, bp, k, nb, d_in, d_out, ss, cs, st):
        bp.process_ptr(d_in, d_out, nb, ss, cs, st)

    def tensor(self, bp, k, nb, x, out):
        return bp.process(x, out=out)

    def check(self, bp, k):
        pass


class IrScheduled(Plain):
    """ohs_batch_process_ir_scheduled / _crossfaded with rows per stream: stream 0 stays on set 1 (so that it is the plain
    convolution with that set, whatever the others do), every other stream changes its set in every segment"""
    N_SETS = 3

    def __init__(self, S, seg_blocks, mode):
        self.S, self.seg, self.mode, self.last = S, seg_blocks, mode, {}

    def rows(self, k, nb):
        idx = make_rows(self.S, -(-nb // self.seg), self.N_SETS, k)
        idx[0, :] = 1
        return idx

    def prev(self, k):
        return None if k == 0 else self.rows(k - 1, self.blocks[k - 1])[:, -1].copy()

    def ptr(self, bp, k, nb, d_in, d_out, ss, cs, st):
        if self.mode == "crossfaded":
            bp.process_ir_crossfaded_ptr(d_in, d_out, nb, ss, cs, self.seg, self.rows(k, nb), self.prev(k), st)
        else:
            bp.process_ir_scheduled_ptr(d_in, d_out, nb, ss, cs, self.seg, self.rows(k, nb), self.mode, st)

    def tensor(self, bp, k, nb, x, out):
        if self.mode == "crossfaded":
            return bp.process_ir_crossfaded(x, self.seg, self.rows(k, nb), self.prev(k), out=out)
        return bp.process_ir_scheduled(x, self.seg, self.rows(k, nb), self.mode, out=out)

    def check(self, bp, k):
        assert bp.last_conv_ir_scheduled(), "the plain kernel served a scheduled call"
        assert bp.last_conv_ir_crossfaded() == (self.mode == "crossfaded")


def _ranges_ok(got, want):
    if want is None:
        return True
    return got in want if isinstance(want, (tuple, set, frozenset, list)) else got == want


def run_case(name, make, S, calls, gaps, in_place, expect, entry=None, hook=None, first_id=900):
    """make() -> a configured handle (called twice: the guarded handle and its twin); calls: lengths in blocks; gaps: (lead, channel
    gap, stream gap, tail); expect: per call (family, ranges) -- ranges an int, a collection of admissible counts, or None where the
    family has no chunk count to name; hook(k, bp): applied to both handles in front of call k >= 1.
    -> (the guarded output of all calls [S][2][frames], the input [S][2][frames], the plans that served the calls)"""
    import torch
    entry = entry or Plain()
    entry.blocks = list(calls)
    assert len(calls) >= 2 and len(set(calls)) == len(calls) and len(expect) == len(calls)
    guarded, twin = make(), make()
    x = _signal(S, first_id, sum(calls) * BLOCK)
    lead = gaps[0]
    st = torch.cuda.current_stream().cuda_stream
    outs, plans, pos = [], [], 0
    for k, nb in enumerate(calls):
        if hook is not None and k:
            hook(k, guarded)
            hook(k, twin)
        frames = nb * BLOCK
        what = f"{name}: call {k} ({nb} blocks)"
        xc = np.ascontiguousarray(x[:, :, pos:pos + frames])
        ss, cs, total, mask = layout(S, frames, *gaps)
        hin = filled(total, SENT_IN)
        place(hin, xc, lead, ss, cs)
        d_in = torch.from_numpy(hin.copy()).cuda()
        d_out = d_in if in_place else torch.from_numpy(filled(total, SENT_OUT).copy()).cuda()
        assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
        entry.ptr(guarded, k, nb, d_in.data_ptr() + 4 * lead, d_out.data_ptr() + 4 * lead, ss, cs, st)
        torch.cuda.synchronize()
        out, inb = d_out.cpu().numpy(), d_in.cpu().numpy()
        xt = torch.from_numpy(xc.copy()).cuda()
        ref = entry.tensor(twin, k, nb, xt, xt if in_place else None)
        torch.cuda.synchronize()
        ref = ref.cpu().numpy()

        # family and ranges: ask the library
        pg, pt = guarded.last_conv_plan(), twin.last_conv_plan()
        print(f"guard-bands {what} -> {pg}")
        plans.append(pg)
        assert pg == pt, f"{what}: guarded {pg}, twin {pt}"
        assert pg[0] == expect[k][0] and _ranges_ok(pg[1], expect[k][1]), f"{what}: served by {pg}, the case names {expect[k]}"
        entry.check(guarded, k)
        entry.check(twin, k)
        # gaps
        gaps_intact(out.view(np.uint32), mask, SENT_IN if in_place else SENT_OUT, what + ", output buffer")
        # input
        if not in_place:
            changed = np.flatnonzero(inb.view(np.uint32) != hin.view(np.uint32))
            assert changed.size == 0, f"{what}: {changed.size} words of the input buffer changed, first at {changed[:6]}"
        # bits
        y = take(out, S, frames, lead, ss, cs)
        nan = np.argwhere(~np.isfinite(y))
        assert nan.size == 0, f"{what}: {len(nan)} non-finite output samples, first (stream, channel, frame) {nan[:4].tolist()}"
        assert float(np.abs(ref).max()) > 0.01, what
        for s in range(S):
            bad = np.argwhere(y[s].view(np.uint32) != ref[s].view(np.uint32))
            assert bad.size == 0, (f"{what}: stream {s} differs from the twin in {len(bad)} samples, first (channel, frame) "
                                   f"{bad[:4].tolist()}, last {bad[-1].tolist()}")
        outs.append(y)
        pos += frames
    return np.concatenate(outs, axis=2), x, plans


def _only(p, h):
    """four responses, all silent but path p"""
    z = np.zeros(1, np.float32)
    return [h if q == p else z for q in range(4)]


def f64_reference(oracle, x0, timeline):
    """Stream x0 [2][frames] through four paths whose responses change in mid-stream the reference's way: timeline[p] =
    [(first frame, response), ...]; from its first frame on a response sees nothing of the frames in front of it, and the tail
    of the response it replaces is dropped (set_ir resets that path only).  Built from oracle.binaural_f64, one path at a time.
    -> [2][frames] f64, gain applied"""
    frames = x0.shape[1]
    y = np.zeros((2, frames), np.float64)
    for p in range(4):
        for i, (t0, h) in enumerate(timeline[p]):
            t1 = timeline[p][i + 1][0] if i + 1 < len(timeline[p]) else frames
            if len(h) == 0 or t1 <= t0:
                continue
            l, r = oracle.binaural_f64(x0[0, t0:t1], x0[1, t0:t1], _only(p, np.asarray(h, np.float32)))
            y[0, t0:t1] += l
            y[1, t0:t1] += r
    return GAIN * y


def _against_f64(oracle, y, x, irs, what):
    yl, yr = oracle.binaural_f64(x[0, 0], x[0, 1], irs)
    a, r = assert_parity(y[0], GAIN * np.stack([yl, yr]), what)
    print(f"guard-bands {what}: stream 0 against f64 direct convolution: abs RMS {a:.3e}, rel RMS {r:.3e}")


LAYOUTS = ["tight", "wide"]
PLACES = [False, True]
PLACE_IDS = ["out_of_place", "in_place"]


# ---- the checker sees what a kernel stores: a call's last block, looked at through the mask of a call one block shorter ------------
def test_the_checker_names_every_chains_last_block_under_a_mask_one_block_short():
    """End to end on the device: sentinel upload, a call of 3 blocks, read-back.  The mask of a 2-block call on the same chain
    starts calls the third block of every chain a run of 512 samples directly behind that chain -- gaps_intact must say so, chain
    by chain, and pass under the right mask."""
    import torch
    from open_headstage_amd import synth
    from tests.guard_bands import GapDamage
    irs = synth.hrir_set(512)
    bp = _handle(S3, irs, 1)
    lead, cgap, sgap, tail = _gaps("wide", 1, 512)
    frames = 3 * BLOCK
    ss, cs, total, mask = layout(S3, frames, lead, cgap, sgap, tail)
    ss2, cs2, total2, short = layout(S3, frames - BLOCK, lead, cgap + BLOCK, sgap, tail + BLOCK)
    assert (ss2, cs2, total2) == (ss, cs, total) and int((mask & ~short).sum()) == S3 * 2 * BLOCK and not (short & ~mask).any()
    hin = filled(total, SENT_IN)
    place(hin, _signal(S3, 880, frames), lead, ss, cs)
    d_in = torch.from_numpy(hin.copy()).cuda()
    d_out = torch.from_numpy(filled(total, SENT_OUT).copy()).cuda()
    bp.process_ptr(d_in.data_ptr() + 4 * lead, d_out.data_ptr() + 4 * lead, 3, ss, cs, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    gaps_intact(out, mask, SENT_OUT)
    with pytest.raises(GapDamage) as e:
        gaps_intact(out, short, SENT_OUT, "a mask one block short")
    assert e.value.runs == [(s, c, "behind", 0, BLOCK) for s in range(S3) for c in range(2)] and e.value.n_runs == 2 * S3


# ---- block 512, one partition (k_conv_p1): 1 range; 4 (chunks that compute their own boundary tails); 3 (the pre-pass) -----------
# (target waves per stream, calls, the range counts the calls are served with: min(chunks, blocks) -- named, not computed)
P1_CASES = {"one_range": (1, (1, 2), (1, 1)), "own_tails": (4, (3, 17), (3, 4)), "pre_pass": (3, (19, 5), (3, 3))}


def _p1_make(exp_tuning, taps, per_stream):
    from open_headstage_amd import synth
    exp_tuning("p1_target_waves", per_stream * S3)
    irs = synth.hrir_set(taps)
    return lambda: _handle(S3, irs, 1, lib=exp_tuning.lib), irs


@pytest.mark.parametrize("in_place", PLACES, ids=PLACE_IDS)
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("case", list(P1_CASES))
@pytest.mark.parametrize("taps", [512, 200])
def test_block_512_one_partition(exp_tuning, taps, case, kind, in_place):
    per_stream, calls, ranges = P1_CASES[case]
    make, _ = _p1_make(exp_tuning, taps, per_stream)
    run_case(f"block 512 p1, taps {taps}, {case}, {kind}", make, S3, calls, _gaps(kind, 1, 512), in_place,
             [("block512_p1", r) for r in ranges])


def test_block_512_one_partition_against_f64(exp_tuning, oracle):
    make, irs = _p1_make(exp_tuning, 512, 4)
    y, x, _ = run_case("block 512 p1 vs f64", make, S3, (3, 17), _gaps("tight", 1, 512), False, [("block512_p1", 3), ("block512_p1", 4)])
    _against_f64(oracle, y, x, irs, "block 512, one partition")


# ---- hop 1536 (k_conv_p1_os), product library, S = 5: a single hop; last windows of 512, 1024 and 1536 new frames; several hop
#      ranges per stream.  Ranges per stream: a stream's hops (3 blocks each, the last one ragged) -- out of place any count, in
#      place a divisor of 12 --------------------------------------------------------------------------------------------------------
S_OS = 5
OS_CASES = {(3, 4): {False: (1, 2), True: (1, 2)}, (5, 7): {False: (2, 3), True: (2, 3)}, (8, 66): {False: (3, 22), True: (3, 12)}}


def _os_make(eq=False):
    from open_headstage_amd import synth
    irs = synth.hrir_set(512)
    return lambda: _handle(S_OS, irs, 2, eq=eq), irs


@pytest.mark.parametrize("in_place", PLACES, ids=PLACE_IDS)
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("calls", list(OS_CASES), ids=lambda c: "x".join(map(str, c)))
def test_hop_1536(calls, kind, in_place):
    make, _ = _os_make()
    run_case(f"hop 1536, {calls}, {kind}", make, S_OS, calls, _gaps(kind, 2, 1536), in_place,
             [("hop1536_p1", r) for r in OS_CASES[calls][in_place]])


@pytest.mark.parametrize("kind", LAYOUTS)
def test_hop_1536_behind_the_eq_out_of_place(kind):
    """the EQ writes the output buffer and the convolution runs on it in place (a divisor of 12 ranges); the input stays untouched"""
    make, _ = _os_make(eq=True)
    run_case(f"hop 1536 behind the EQ, {kind}", make, S_OS, (5, 7, 8), _gaps(kind, 2, 1536), False,
             [("hop1536_p1", 2), ("hop1536_p1", 3), ("hop1536_p1", 3)])


def test_hop_1536_against_f64(oracle):
    make, irs = _os_make()
    y, x, _ = run_case("hop 1536 vs f64", make, S_OS, (8, 66), _gaps("tight", 2, 1536), False, [("hop1536_p1", 3), ("hop1536_p1", 22)])
    _against_f64(oracle, y, x, irs, "hop 1536")


# ---- block 2048 (k_conv_lb_*), plan 0: calls that end 512, 1024 and 1536 frames into a 2048-frame tile and start off the grid ------
def _lb_make(taps):
    from open_headstage_amd import synth
    irs = synth.hrir_set(taps)
    return lambda: _handle(S3, irs, 0), irs


@pytest.mark.parametrize("in_place", PLACES, ids=PLACE_IDS)
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("calls", [(1, 2), (3, 5), (7, 16, 9)], ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("taps", [1300, 4097])
def test_block_2048(taps, calls, kind, in_place):
    make, _ = _lb_make(taps)
    run_case(f"block 2048, taps {taps}, {calls}, {kind}", make, S3, calls, _gaps(kind, 4, 2048), in_place, [("block2048", None)] * len(calls))


def test_block_2048_against_f64(oracle):
    make, irs = _lb_make(1300)
    y, x, _ = run_case("block 2048 vs f64", make, S3, (7, 16, 9), _gaps("tight", 4, 2048), True, [("block2048", None)] * 3)
    _against_f64(oracle, y, x, irs, "block 2048")


# A per-path set_ir in mid-stream on such a handle is "every path forgets" + pending tails: k_conv_lb_tails_add adds
# count = min(n_frames, len - pos) frames of them to the output of the calls that follow -- a short call inside the tails' length, then
# one that runs past their end.
def _lb_reset_setup():
    from open_headstage_amd import synth
    irs = synth.hrir_set(1300)
    new1 = synth.hrir_set(900)[1]

    def hook(k, bp):
        if k == 1:
            bp.set_ir(1, new1)

    def timeline(t):
        return [[(0, irs[0])], [(0, irs[1]), (t, new1)], [(0, irs[2])], [(0, irs[3])]]
    return (lambda: _handle(S3, irs, 0)), hook, timeline


@pytest.mark.parametrize("in_place", PLACES, ids=PLACE_IDS)
@pytest.mark.parametrize("kind", LAYOUTS)
def test_block_2048_pending_tails_behind_a_per_path_set_ir(kind, in_place):
    make, hook, _ = _lb_reset_setup()
    run_case(f"block 2048 + pending tails, {kind}", make, S3, (7, 3, 18), _gaps(kind, 4, 2048), in_place, [("block2048", None)] * 3, hook=hook)


def test_block_2048_pending_tails_against_f64(oracle):
    make, hook, timeline = _lb_reset_setup()
    y, x, _ = run_case("block 2048 + pending tails vs f64", make, S3, (7, 3, 18), _gaps("tight", 4, 2048), False, [("block2048", None)] * 3,
                       hook=hook)
    a, r = assert_parity(y[0], f64_reference(oracle, x[0], timeline(7 * BLOCK)), "block 2048 + pending tails")
    print(f"guard-bands block 2048 + pending tails: stream 0 against f64 direct convolution: abs RMS {a:.3e}, rel RMS {r:.3e}")


# ---- block 8192 (k_conv_xb), plan 0, out of place only: calls that end inside an 8192-frame block, a block-2048 call in between
#      (what tests/test_gpu_conv_xb.py::test_block_8192_kernel_matches_the_oracle_and_f64 calls "nothing stored there") -------------
def _xb_expect(calls):
    return [("block8192" if nb >= 128 else "block2048", None) for nb in calls]


def _xb_make(taps, S):
    from open_headstage_amd import synth
    irs = synth.hrir_set(taps)
    return lambda: _handle(S, irs, 0), irs


@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("calls", [(129, 135), (128, 3, 131)], ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("taps,S", [(8192, 3), (16384, 34)], ids=["one_partition", "two_partitions"])
def test_block_8192(taps, S, calls, kind):
    make, _ = _xb_make(taps, S)
    run_case(f"block 8192, taps {taps}, S {S}, {calls}, {kind}", make, S, calls, _gaps(kind, 4, 8192), False, _xb_expect(calls))


def test_block_8192_against_f64(oracle):
    make, irs = _xb_make(1024, S3)
    y, x, _ = run_case("block 8192 vs f64", make, S3, (129, 135), _gaps("tight", 4, 8192), False, _xb_expect((129, 135)))
    _against_f64(oracle, y, x, irs, "block 8192, taps 1024")


# ---- time-parallel block 512 (k_conv_tp_*), plan 1, gate-free -----------------------------------------------------------------------
def _tp_make():
    from open_headstage_amd import synth
    irs = synth.hrir_set(1300)
    return lambda: _handle(S3, irs, 1), irs


@pytest.mark.parametrize("in_place", PLACES, ids=PLACE_IDS)
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("calls", [(1, 3), (7, 2)], ids=lambda c: "x".join(map(str, c)))
def test_time_parallel_block_512(calls, kind, in_place):
    make, _ = _tp_make()
    run_case(f"time-parallel block 512, {calls}, {kind}", make, S3, calls, _gaps(kind, 1, 512), in_place, [("block512_tp", None)] * 2)


def test_time_parallel_block_512_against_f64(oracle):
    make, irs = _tp_make()
    y, x, _ = run_case("time-parallel block 512 vs f64", make, S3, (7, 2), _gaps("tight", 1, 512), False, [("block512_tp", None)] * 2)
    _against_f64(oracle, y, x, irs, "time-parallel block 512")


# ---- gated time-parallel (k_conv_tp_old) and sequential: a per-path set_ir in mid-stream --------------------------------------------
# A handle that keeps the input history of the block-2048 plan carries a per-path set_ir out as "every path forgets" + pending tails
# and never needs a per-path gate.  The gates serve where the history cannot vouch for every path's reach.  Two routes there:
#  * `no_history`: the issue's shape -- taps (1300, 700, 2000, 513) -- on the experiments library with lb_min_p out of reach: no
#    history is kept at all, the per-path set_ir leaves path 1 younger than its response;
#  * `product`: the product library as shipped -- the handle starts with one-partition responses (no history either), and after the
#    first call path 0 gets another short response and path 2 one of three partitions with nothing processed in between: path 0 is
#    younger than the history that begins now.
# Behind the set_ir a call of exactly Pmax blocks is the shortest the time-parallel kernels take (gated: k_conv_tp_old adds what
# each path may still see of the old blocks); one of Pmax - 1 blocks is served by the sequential kernel under the SAME state, which
# is what proves that the state was not gate-free.  Then one long call.
def _gated_setup(route, exp_tuning):
    """-> (make, hook, timeline(first call's frames) for f64_reference, Pmax behind the set_ir)"""
    from open_headstage_amd import synth
    hb = synth.hrir_set(2000)
    if route == "no_history":
        exp_tuning("lb_min_p", 99)
        irs = [hb[0][:1300], hb[1][:700], hb[2][:2000], hb[3][:513]]
        new1 = synth.hrir_set(700)[1]

        def hook(k, bp):
            if k == 1:
                bp.set_ir(1, new1)

        def timeline(t):
            return [[(0, irs[0])], [(0, irs[1]), (t, new1)], [(0, irs[2])], [(0, irs[3])]]
        return (lambda: _handle(S3, irs, 1, lib=exp_tuning.lib)), hook, timeline, 4
    irs = [hb[0][:512], hb[1][:300], hb[2][:512], hb[3][:200]]
    new0, new2 = synth.hrir_set(400)[0], synth.hrir_set(1300)[2]

    def hook(k, bp):
        if k == 1:
            bp.set_ir(0, new0)
            bp.set_ir(2, new2)

    def timeline(t):
        return [[(0, irs[0]), (t, new0)], [(0, irs[1])], [(0, irs[2]), (t, new2)], [(0, irs[3])]]
    return (lambda: _handle(S3, irs, 1)), hook, timeline, 3


def _gated_calls(route, which, pmax):
    """-> (calls, expect): a first call, the call behind the set_ir (Pmax blocks: gated time-parallel; Pmax - 1: sequential), a long one"""
    first = ("block512_tp", None) if route == "no_history" else ("block512_p1", None)
    if which == "gated":
        return (5, pmax, 11), [first, ("block512_tp", None), ("block512_tp", None)]
    return (5, pmax - 1, 11), [first, ("sequential", 1), ("block512_tp", None)]


@pytest.mark.parametrize("in_place", PLACES, ids=PLACE_IDS)
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("which", ["gated", "sequential"])
@pytest.mark.parametrize("route", ["no_history", "product"])
def test_gated_time_parallel_and_sequential(exp_tuning, route, which, kind, in_place):
    make, hook, _, pmax = _gated_setup(route, exp_tuning)
    calls, expect = _gated_calls(route, which, pmax)
    run_case(f"{which} behind a per-path set_ir ({route}), {kind}", make, S3, calls, _gaps(kind, 1, 512), in_place, expect, hook=hook)


@pytest.mark.parametrize("which", ["gated", "sequential"])
@pytest.mark.parametrize("route", ["no_history", "product"])
def test_gated_time_parallel_and_sequential_against_f64(exp_tuning, oracle, route, which):
    make, hook, timeline, pmax = _gated_setup(route, exp_tuning)
    calls, expect = _gated_calls(route, which, pmax)
    what = f"{which} behind a per-path set_ir ({route})"
    y, x, _ = run_case(what + " vs f64", make, S3, calls, _gaps("tight", 1, 512), False, expect, hook=hook)
    a, r = assert_parity(y[0], f64_reference(oracle, x[0], timeline(calls[0] * BLOCK)), what)
    print(f"guard-bands {what}: stream 0 against f64 direct convolution: abs RMS {a:.3e}, rel RMS {r:.3e}")


# ---- IR-scheduled and crossfaded calls (k_conv_p1_irs, k_conv_p1_irs_xf): 1 chunk, and 2 / 4 / 8 / 16 chunks that compute their own
#      boundary tails.  At S = 3 the library's own rule never yields one chunk for calls of 5 blocks or more, so the experiments
#      library serves: p1_target_waves = S is one chunk per stream, 0 is the library's own rule ------------------------------------------
IRS_CALLS = {(6, 5): 2, (32, 7): 3}         # calls -> seg_blocks


def _irs_make(exp_tuning, chunks):
    sets = make_sets(IrScheduled.N_SETS)
    if chunks == "one_chunk":
        exp_tuning("p1_target_waves", S3)

    def make():
        bp = _handle(S3, list(sets[0]), 1, lib=exp_tuning.lib)
        bp.set_schedule_irs(sets)
        return bp
    return make, sets


@pytest.mark.parametrize("in_place", PLACES, ids=PLACE_IDS)
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("chunks", ["one_chunk", "own_tails"])
@pytest.mark.parametrize("calls", list(IRS_CALLS), ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("mode", ["ring_out", "cut", "crossfaded"])
def test_ir_scheduled_and_crossfaded(exp_tuning, mode, calls, chunks, kind, in_place):
    make, _ = _irs_make(exp_tuning, chunks)
    want = 1 if chunks == "one_chunk" else POW2
    run_case(f"IR-{mode}, {calls}, seg_blocks {IRS_CALLS[calls]}, {chunks}, {kind}", make, S3, calls, _gaps(kind, 1, 512), in_place,
             [("block512_p1", want)] * 2, entry=IrScheduled(S3, IRS_CALLS[calls], mode))


@pytest.mark.parametrize("chunks", ["one_chunk", "own_tails"])
@pytest.mark.parametrize("mode", ["ring_out", "crossfaded"])
def test_ir_scheduled_and_crossfaded_against_f64(exp_tuning, oracle, mode, chunks):
    """stream 0 never leaves set 1 (and fades from set 1 to set 1 nowhere): the plain convolution with that set, while the scheduled
    kernel looks every block's set up for every stream"""
    make, sets = _irs_make(exp_tuning, chunks)
    want = 1 if chunks == "one_chunk" else POW2
    y, x, _ = run_case(f"IR-{mode} vs f64, {chunks}", make, S3, (32, 7), _gaps("tight", 1, 512), False, [("block512_p1", want)] * 2,
                       entry=IrScheduled(S3, 3, mode))
    _against_f64(oracle, y, x, list(sets[1]), f"IR-{mode}, {chunks}")

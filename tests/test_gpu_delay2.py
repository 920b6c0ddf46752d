"""ohs_delay2_process and ohs_delay2_process_filtered (libohs_delay2.so, include/ohs_delay2.h) on the device, bit for bit against
tests/delay2_model.py, the header's arithmetic in numpy, and -- unfiltered -- against libohs_delay.so on the same device.  A NaN
matches a NaN at the same position; nothing else has a tolerance.  The cases are delay2_model's, the ones tests/test_cpu_delay2.py
runs through the host build of csrc/delay2_body.hpp and through the mutants.

Not run here: the refusal of a handle that failed in the middle of an earlier call -- the build has no way to make a HIP call fail,
and none is provoked.  The filtered pass's clamp of the delay at 5 is reached by no call (tests/test_cpu_delay2.py says why and holds
it on the host)."""
import time

import numpy as np
import pytest

from tests import busy_stream as bs
from tests import delay2_model as m2
from tests import delay_model as dm

pytestmark = pytest.mark.gpu

BLOCK = m2.BLOCK


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


def _same_carry(got, want, what):
    assert got is not None and len(got) == 3, what
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == np.ascontiguousarray(w).tobytes(), what


def _hold_to_the_model(case, name):
    """-> (outputs per call, (tiles staged, gathered, filtered) per call, the handle); carried() is compared after every call"""
    import open_headstage_amd as ohs
    trace, carried = [], []
    want = m2.run_model(case, trace=trace, carried=carried)
    dl = ohs.FilteredObjectDelay(case["S"], case["Kmax"], case["max_delay"])
    outs, forms = [], []
    for n, c in enumerate(case["calls"]):
        y = dl.process(_dev(c["x"]), c["delay"], case["seg_blocks"], c["gains"], c["fir"], carry=c["carry"])
        rec = dl.last_launch()
        assert rec[:2] == (m2.TILE, m2.LDS_WINDOW)
        outs.append(y.cpu().numpy())
        forms.append(rec[2:])
        m2.check_bits(outs[n], want[n], f"{name}, call {n}")
        assert forms[n] == trace[n]["forms"], (name, n, forms[n], trace[n]["forms"])
        _same_carry(dl.carried(), carried[n], f"{name}: carried() behind call {n}")
    return outs, forms, dl


@pytest.fixture(scope="module")
def cases():
    return m2.all_cases()


# ---- a. the base case -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_blocks", [1, 2, 8])
def test_base_case(cases, seg_blocks):
    case = cases[f"base, seg_blocks {seg_blocks}"]
    c = case["calls"][0]
    assert case["S"] == 3 and case["Kmax"] == 3 and c["x"].shape[2] == 4 * BLOCK
    assert (c["delay"] != np.floor(c["delay"])).any() and not m2.is_identity(c["fir"]).any()
    if seg_blocks < 8:
        assert (c["fir"][:, 1:] != c["fir"][:, :-1]).any()                                   # the taps ramp between segments
    _, forms, _ = _hold_to_the_model(case, f"base, seg_blocks {seg_blocks}")
    assert forms[0] == (3 * 3 * 4 * BLOCK // m2.TILE, 0, 3 * 3 * 4 * BLOCK // m2.TILE)


# ---- b. the pass is the row's -------------------------------------------------------------------------------------------------------------
def test_identity_rows_in_front_of_and_behind_filtered_ones(cases):
    case = cases["mixed passes"]
    h = case["calls"][0]["fir"]
    assert m2.is_identity(h[:, 1, 0]).all() and not m2.is_identity(h[:, 2, 0]).any() and m2.is_identity(h[:, 3, 0]).all()
    _, forms, _ = _hold_to_the_model(case, "mixed passes")
    assert [f[2] for f in forms] == [20, 4] and [f[0] for f in forms] == [48, 24]


# ---- c. no taps and identity taps: libohs_delay.so's bits ------------------------------------------------------------------------------
def test_no_taps_and_identity_taps_against_object_delay_on_the_device():
    import open_headstage_amd as ohs
    case = dm.special_case()                    # NaN, infinities and subnormals in the input; every delay is at least 5
    old = ohs.ObjectDelay(case["S"], case["Kmax"], case["max_delay"])
    none, ident = (ohs.FilteredObjectDelay(case["S"], case["Kmax"], case["max_delay"]) for _ in range(2))
    nonfinite = 0
    for n, c in enumerate(case["calls"]):
        assert (c["delay"] >= m2.MIN_FILTERED).all()
        x = _dev(c["x"])
        want = old.process(x, c["delay"], 1, c["gains"], carry=c["carry"]).cpu().numpy()
        want_rec = old.last_launch()
        for dl, fir, what in ((none, None, "fir=None"), (ident, np.broadcast_to(m2.IDENTITY, c["delay"].shape + (5,)), "identity taps")):
            got = dl.process(x, c["delay"], 1, c["gains"], fir, carry=c["carry"]).cpu().numpy()
            m2.check_bits(got, want, f"{what}, call {n}, against ObjectDelay.process")
            assert (np.isnan(got) == np.isnan(want)).all()
            assert dl.last_launch() == want_rec + (0,), (what, dl.last_launch(), want_rec)
            d, g, h = dl.carried()
            assert np.array_equal(d, old.carried()[0]) and np.array_equal(g, old.carried()[1]) and m2.is_identity(h).all()
        nonfinite += int((~np.isfinite(want)).sum())
    assert nonfinite >= 8
    sub = want[0, 2]
    assert (np.abs(sub) < np.finfo(np.float32).tiny).all() and (sub != 0).sum() > BLOCK // 2
    # the whole of delay_model's cases through the unfiltered call, delays below 5 among them
    for name in ("base, seg_blocks 2", "both forms", "chained, max_delay 4096"):
        case = dm.all_cases()[name]
        old, new = ohs.ObjectDelay(case["S"], case["Kmax"], case["max_delay"]), ohs.FilteredObjectDelay(case["S"], case["Kmax"], case["max_delay"])
        for n, c in enumerate(case["calls"]):
            x = _dev(c["x"])
            m2.check_bits(new.process(x, c["delay"], case["seg_blocks"], c["gains"], carry=c["carry"]).cpu().numpy(),
                          old.process(x, c["delay"], case["seg_blocks"], c["gains"], carry=c["carry"]).cpu().numpy(), f"{name}, call {n}")
            assert new.last_launch() == old.last_launch() + (0,)


# ---- d. the ring's two ends ------------------------------------------------------------------------------------------------------------------
def test_a_delay_of_5_reads_x_n_and_max_delay_reads_the_rings_far_end(cases):
    case = cases["ring of 13"]
    assert case["max_delay"] == 7 and case["max_delay"] + 2 + m2.R == 13
    got, _, _ = _hold_to_the_model(case, "ring of 13")
    # the infinity 13 frames in front of the second call is read by its first frame's oldest input at weight 0: a NaN, and only there
    assert np.isnan(got[1][0, 1, 0]) and np.isfinite(got[1][0, 1, 1:]).all()
    # a delay of exactly 5: the node m is frame n - 4, whose newest input is x[n]; f = 0 gives it the weight 0 and y[n] = v(n - 5)
    x, h = case["calls"][0]["x"][0, 0], case["calls"][0]["fir"][0, 0, 0]
    n = 100
    v = h[0] * x[n - 5]
    for r in range(1, 5):
        v = v + h[r] * (x[n - 5 - r] + x[n - 5 + r])
    assert got[0][0, 0, n] == np.float32(v) and h[4] != 0


# ---- e. chained calls -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_delay", [600, 4090])
def test_calls_of_1_2_and_1_blocks_under_carry_are_the_one_call(cases, max_delay):
    """max_delay 4090: the history (4 096 frames) is longer than every call, and the first call's frames are still read in the last"""
    whole, _, _ = _hold_to_the_model(cases[f"one call, max_delay {max_delay}"], "one call")
    cut, _, _ = _hold_to_the_model(cases[f"chained, max_delay {max_delay}"], "chained")
    assert [c.shape[2] // BLOCK for c in cut] == [1, 2, 1]
    m2.check_bits(np.concatenate(cut, axis=2), whole[0], f"chained against one call, max_delay {max_delay}")


# ---- f. the window's edge ------------------------------------------------------------------------------------------------------------------
def test_a_window_of_2048_frames_is_staged_and_one_of_2049_gathered(cases):
    case = cases["window edge"]
    d = case["calls"][0]["delay"]
    spread = m2.LDS_WINDOW - (m2.TILE + 3 + 2 * m2.R)
    assert m2.tile_spread(5.0, d[0, 1, 0]) == spread and m2.tile_spread(5.0, d[0, 1, 1]) == spread + 1
    _, forms, _ = _hold_to_the_model(case, "window edge")
    lds, gather, filtered = forms[0]
    assert lds + gather == filtered == 8 and 1 <= gather <= 2
    # object 0 alone: its widest window is exactly 2 048 frames, and every tile is staged
    c = case["calls"][0]
    one = dict(case, Kmax=1, calls=[dict(c, x=c["x"][:, :1], delay=c["delay"][..., :1], fir=c["fir"][:, :, :1])])
    _, forms, _ = _hold_to_the_model(one, "window edge, object 0")
    assert forms[0] == (4, 0, 4)


# ---- g. shapes and strides -----------------------------------------------------------------------------------------------------------------
def test_64_objects_on_67_streams_and_one_row_for_all_streams():
    import open_headstage_amd as ohs
    S, K, max_delay = 67, 64, 600
    rng = np.random.default_rng(6764)
    x = m2.noise((S, K, BLOCK), 67)
    d = rng.uniform(5.0, max_delay, (S, 1, K))
    g = rng.uniform(-1.0, 1.0, (S, 1, K)).astype(np.float32)
    h = m2.random_taps((S, 1, K), 68)
    h[::3, :, ::5] = m2.IDENTITY                # some rows take the plain pass
    m, dl = m2.Delay2Model(S, K, max_delay), ohs.FilteredObjectDelay(S, K, max_delay)
    m2.check_bits(dl.process(_dev(x), d, 1, g, h).cpu().numpy(), m.process(x, d, 1, g, h), "per-stream rows")
    assert dl.last_launch()[2:] == m.last_launch and 0 < m.last_launch[2] < S * K * 2
    # [segs][K]: row_stream_stride 0, one row for all streams, ramping from the per-stream carry
    want = m.process(x, d[5], 1, g[5], h[6], carry=True)
    m2.check_bits(dl.process(_dev(x), d[5], 1, g[5], h[6], carry=True).cpu().numpy(), want, "shared rows")
    assert dl.last_launch()[2:] == m.last_launch
    _same_carry(dl.carried(), m.carried, "shared rows")
    # [K]: one row held over the call, no gains; the taps per stream: the three are brought to one layout
    m2.check_bits(dl.process(_dev(x), d[7, 0], 1, fir=h, carry=True).cpu().numpy(), m.process(x, d[7], 1, None, h, carry=True), "mixed layouts")
    assert dl.last_launch()[2:] == m.last_launch


def test_wide_strides_leave_the_gaps_as_they_were():
    import torch
    import open_headstage_amd as ohs
    S, K, nb, max_delay, sentinel = 2, 3, 2, 600, -123.5
    frames = nb * BLOCK
    in_cs, in_ss, out_cs, out_ss = frames + 7, 3 * (frames + 7) + 11, frames + 64, 3 * (frames + 64) + 5
    x = m2.noise((S, K, frames), 21)
    d, g = dm.base_rows(S, K, nb, max_delay)
    d = np.maximum(d, m2.MIN_FILTERED)
    h = m2.random_taps((S, nb, K), 22)
    buf_in = np.full(S * in_ss, sentinel, np.float32)
    for s in range(S):
        for c in range(K):
            buf_in[s * in_ss + c * in_cs:s * in_ss + c * in_cs + frames] = x[s, c]
    d_in, d_out = _dev(buf_in), torch.full((S * out_ss,), sentinel, device="cuda")
    dl = ohs.FilteredObjectDelay(S, K, max_delay)
    dl.process_ptr(d_in.data_ptr(), d_out.data_ptr(), nb, in_ss, in_cs, out_ss, out_cs, K, 1, d, g, nb, False,
                   torch.cuda.current_stream().cuda_stream, fir=h)
    torch.cuda.synchronize()
    out, want = d_out.cpu().numpy(), m2.Delay2Model(S, K, max_delay).process(x, d, 1, g, h)
    written = np.zeros(S * out_ss, bool)
    for s in range(S):
        for c in range(K):
            at = s * out_ss + c * out_cs
            m2.check_bits(out[at:at + frames], want[s, c], f"stream {s}, object {c}")
            written[at:at + frames] = True
    assert (out[~written] == np.float32(sentinel)).all() and (~written).sum() > 100
    assert np.array_equal(d_in.cpu().numpy(), buf_in)


# ---- h. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_every_new_refusal_leaves_the_output_the_ring_and_the_carry_as_they_were(cases):
    import torch
    import open_headstage_amd as ohs
    case = cases["chained, max_delay 600"]
    S, K, max_delay = case["S"], case["Kmax"], 600
    c0, c1 = case["calls"][0], case["calls"][1]
    want = m2.run_model(case)
    dl = ohs.FilteredObjectDelay(S, K, max_delay)
    dl.process(_dev(c0["x"]), c0["delay"], 1, c0["gains"], c0["fir"], carry=False)
    before = dl.carried()
    nb = c1["x"].shape[2] // BLOCK
    frames = nb * BLOCK
    d_in, d_out = _dev(c1["x"]), torch.full((S, K, frames), 7.25, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(delay=c1["delay"], gains=c1["gains"], fir=c1["fir"], carry=True, k=K):
        dl.process_ptr(d_in.data_ptr(), d_out.data_ptr(), nb, K * frames, frames, K * frames, frames, k, 1, delay, gains, nb, carry, stream, fir=fir)

    def bad(a, at, v):
        a = np.array(a, copy=True)
        a.reshape(-1)[at] = v
        return a

    d, g, h = c1["delay"], c1["gains"], c1["fir"]
    refused = {
        "a NaN tap": dict(fir=bad(h, 7, np.nan)), "an infinite tap": dict(fir=bad(h, 0, np.inf)), "the last tap infinite": dict(fir=bad(h, h.size - 1, -np.inf)),
        "a delay below 5": dict(delay=bad(d, 4, 4.999999)), "a delay of 1": dict(delay=bad(d, d.size - 1, 1.0)),
        # ... and what the unfiltered call refuses is refused with taps as well
        "a NaN delay": dict(delay=bad(d, 3, np.nan)), "a delay above max_delay": dict(delay=bad(d, 5, max_delay + 1e-9)),
        "a NaN gain": dict(gains=bad(g, 2, np.nan)), "another n_objects under carry": dict(k=K - 1),
    }
    for what, kw in refused.items():
        with pytest.raises(ohs.FilteredObjectDelayError) as e:
            call(**kw)
        assert e.value.status == 1, (what, e.value)
    with pytest.raises(ohs.FilteredObjectDelayError, match="below 1 \\+ OHS_DELAY2_FIR_RADIUS"):
        call(delay=bad(d, 4, 4.5))
    with pytest.raises(ohs.FilteredObjectDelayError, match="fir\\[7\\] is not finite"):
        call(fir=bad(h, 7, np.nan))
    # the unfiltered call takes a delay below 5 and leaves it as the carried one: a filtered call under carry is then refused,
    # whatever its own rows are
    low = ohs.FilteredObjectDelay(S, K, max_delay)
    low.process(_dev(c0["x"]), bad(c0["delay"], 1, 2.0), 1, c0["gains"], None, carry=False)
    low_before = low.carried()
    with pytest.raises(ohs.FilteredObjectDelayError, match="the carried delay of stream 0, object 1"):
        low.process_ptr(d_in.data_ptr(), d_out.data_ptr(), nb, K * frames, frames, K * frames, frames, K, 1, d, g, nb, True, stream, fir=h)
    _same_carry(low.carried(), low_before, "the handle behind the refused carry")
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == np.float32(7.25)).all()                  # nothing was written
    _same_carry(dl.carried(), before, "carried() behind the refusals")
    call()                                                                    # the ring and the carry are as they were: the model's second call
    torch.cuda.synchronize()
    m2.check_bits(d_out.cpu().numpy(), want[1], "the call behind the refusals")


# ---- i. asynchrony ----------------------------------------------------------------------------------------------------------------------------
def test_three_filtered_calls_queued_on_a_busy_stream_have_the_quiet_runs_bits():
    """tests/busy_stream.py's harness, as tests/test_gpu_delay.py uses it: the caller's side stream is busy when the calls are made,
    the input arrives by copies queued behind that work, delay, gains and taps are overwritten the moment each call returns, the three
    calls follow each other without a sync, and the outputs leave by copies queued behind each call"""
    import torch
    import open_headstage_amd as ohs
    S, K, nb, max_delay, calls = 3, 4, 4, 3000, 3
    frames = nb * BLOCK
    rng = np.random.default_rng(809)
    xs = [m2.noise((S, K, frames), 810 + n) for n in range(calls)]
    ds = [rng.uniform(5.0, max_delay, (S, nb, K)) for _ in range(calls)]
    gs = [rng.uniform(-1.0, 1.0, (S, nb, K)).astype(np.float32) for _ in range(calls)]
    hs = [m2.random_taps((S, nb, K), 820 + n) for n in range(calls)]
    quiet = ohs.FilteredObjectDelay(S, K, max_delay)
    model = m2.Delay2Model(S, K, max_delay)
    t0 = time.perf_counter()
    want = [quiet.process(_dev(xs[n]), ds[n], 1, gs[n], hs[n]) for n in range(calls)]
    enqueue_s = time.perf_counter() - t0
    torch.cuda.synchronize()
    want_rec = quiet.last_launch()
    for n in range(calls):
        m2.check_bits(want[n].cpu().numpy(), model.process(xs[n], ds[n], 1, gs[n], hs[n]), f"the quiet twin, call {n}")
    dl = ohs.FilteredObjectDelay(S, K, max_delay)
    busy = bs.BusyStream()
    nan = float("nan")
    pinned = [torch.from_numpy(x.copy()).pin_memory() for x in xs]
    d_in = torch.full((S, K, frames), nan, device="cuda")
    d_out = torch.full((S, K, frames), nan, device="cuda")
    keep = [torch.full((S, K, frames), nan, device="cuda") for _ in range(calls)]
    torch.cuda.synchronize()
    try:
        busy.fill(bs.filler_seconds(min(enqueue_s, 0.01)))
        with torch.cuda.stream(busy.stream):
            for n in range(calls):
                d, rows = ds[n].copy(), bs.row_arrays({"gains": gs[n], "fir": hs[n]})
                d_in.copy_(pinned[n], non_blocking=True)
                dl.process_ptr(d_in.data_ptr(), d_out.data_ptr(), nb, K * frames, frames, K * frames, frames, K, 1, d, rows["gains"], nb, n > 0,
                               busy.handle, fir=rows["fir"])
                busy.premise("ohs_delay2_process_filtered")
                d[...] = np.nan             # (the harness's scribble knows uint32 and float32 rows; the delays are f64)
                bs.scribble(rows)
                keep[n].copy_(d_out, non_blocking=True)
                d_in.fill_(nan)
                d_out.fill_(nan)
            rec = dl.last_launch()
    finally:
        torch.cuda.synchronize()
    assert rec == want_rec, (rec, want_rec)
    for n in range(calls):
        bs.same_bits(keep[n].cpu().numpy(), want[n].cpu().numpy(), f"ohs_delay2_process_filtered on a busy stream, call {n}")


# ---- j. composition with the tracked call --------------------------------------------------------------------------------------------------------
def test_render_with_distance_air_is_the_stage_then_the_tracked_call():
    """one stream, no sync in between, against: the stage with air_absorption_taps of the same distances; a sync and a host round
    trip; TrackedSceneProcessor.process_xyz.  Two calls, the second under both handles' carry"""
    import torch
    import open_headstage_amd as ohs
    from tests.test_cpu_layout import make_input, make_layout
    from tests.test_gpu_tracked import _mesh, _poses, _sources, _tracked
    S, K, blocks, seg, max_delay = 3, 5, 6, 2, 8192
    n_segs = blocks // seg
    pos, tri, T = _mesh(2)
    dirs = make_layout(len(pos), 512)
    tr_a, tr_b = _tracked(pos, tri, dirs, streams=S), _tracked(pos, tri, dirs, streams=S)
    dl_a, dl_b = ohs.FilteredObjectDelay(S, K, max_delay), ohs.FilteredObjectDelay(S, K, max_delay)
    model = m2.Delay2Model(S, K, max_delay)
    listener = np.array([0.25, -0.5, 0.125])
    side = torch.cuda.Stream()
    for n in range(2):
        x = make_input(S, K, blocks, seed=900 + n)
        radius = np.random.default_rng(910 + n).uniform(0.3, 50.0, (S, n_segs, K, 1))
        src = _sources(T, tri, S, n_segs, K, seed=90 + n) * radius + listener
        rot = _poses(S, n_segs, seed=95 + n)
        xd = _dev(x)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = ohs.render_with_distance_air(tr_a, dl_a, xd, src, rot, seg, listener=listener)
        side.synchronize()
        delay, gain = ohs.distance_rows(src, listener=listener)
        v = src - listener
        taps = ohs.air_absorption_taps(np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]))    # distance_rows' r
        assert delay.shape == (S, n_segs, K) and 5.0 < delay.min() and delay.max() < max_delay and not m2.is_identity(taps).any()
        between = dl_b.process(xd, delay, seg, gains=gain, fir=taps)
        assert dl_b.last_launch()[4] == S * K * blocks * 2
        torch.cuda.synchronize()
        host = between.cpu().numpy()
        m2.check_bits(host, model.process(x, delay, seg, gain, taps), f"the stage, call {n}")
        want = tr_b.process_xyz(_dev(host), src - listener, rot, seg)
        torch.cuda.synchronize()
        bs.same_bits(got.cpu().numpy(), want.cpu().numpy(), f"render_with_distance_air, call {n}")
        assert np.isfinite(got.cpu().numpy()).all() and np.abs(got.cpu().numpy()).max() > 0

"""ohs_delay_process (libohs_delay.so, include/ohs_delay.h) on the device, bit for bit against tests/delay_model.py, the header's arithmetic
in numpy.  A NaN matches a NaN at the same position; nothing else has a tolerance.  The cases are delay_model's, the ones
tests/test_cpu_delay.py runs through the host build of csrc/delay_body.hpp and through the mutants.

Not run here: the refusal of a handle that failed in the middle of an earlier call -- the build has no way to make a HIP call fail,
and none is provoked."""
import time

import numpy as np
import pytest

from tests import busy_stream as bs
from tests import delay_model as dm

pytestmark = pytest.mark.gpu

BLOCK = dm.BLOCK


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


def _run_device(case, dl=None):
    """-> (outputs per call, (tiles staged, tiles gathered) per call, the handle)"""
    import open_headstage_amd as ohs
    dl = dl or ohs.ObjectDelay(case["S"], case["Kmax"], case["max_delay"])
    outs, forms = [], []
    for c in case["calls"]:
        y = dl.process(_dev(c["x"]), c["delay"], case["seg_blocks"], c["gains"], carry=c["carry"])
        rec = dl.last_launch()
        assert rec[:2] == (dm.TILE, dm.LDS_WINDOW)
        outs.append(y.cpu().numpy())
        forms.append(rec[2:])
    return outs, forms, dl


def _hold_to_the_model(case, name):
    trace = []
    want = dm.run_model(case, trace=trace)
    got, forms, dl = _run_device(case)
    for n, (g, w) in enumerate(zip(got, want)):
        dm.check_bits(g, w, f"{name}, call {n}")
        assert forms[n] == trace[n]["forms"], (name, n, forms[n], trace[n]["forms"])
    return got, forms, dl


@pytest.fixture(scope="module")
def cases():
    return dm.all_cases()


# ---- a. the base case -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_blocks", [1, 2, 8])
def test_base_case(cases, seg_blocks):
    case = cases[f"base, seg_blocks {seg_blocks}"]
    assert case["S"] == 3 and case["Kmax"] == 3 and case["max_delay"] == 600 and case["calls"][0]["x"].shape[2] == 4 * BLOCK
    got, forms, _ = _hold_to_the_model(case, f"base, seg_blocks {seg_blocks}")
    x, y = case["calls"][0]["x"], got[0]
    assert np.array_equal(y[0, 0, 1:], x[0, 0, :-1]) and y[0, 0, 0] == 0.0       # a delay of exactly 1 at gain 1: the input one frame late
    assert forms[0] == (3 * 3 * 4 * BLOCK // dm.TILE, 0)


# ---- b. both kernel forms ---------------------------------------------------------------------------------------------------------------
def test_a_jump_across_the_whole_range_gathers_and_a_steady_segment_stages(cases):
    case = cases["both forms"]
    assert case["max_delay"] == 65536 and case["S"] == case["Kmax"] == 1
    _, forms, _ = _hold_to_the_model(case, "both forms")
    for lds, gather in forms:
        assert lds > 0 and gather > 0 and lds + gather == 4 * BLOCK // dm.TILE, (lds, gather)


# ---- c. chained calls -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_delay", [600, 4096])
def test_calls_of_1_2_and_1_blocks_under_carry_are_the_one_call(cases, max_delay):
    """max_delay 4096: the history (4 098 frames) is longer than every call, and the first call's frames are still read in the last"""
    whole, _, _ = _hold_to_the_model(cases[f"one call, max_delay {max_delay}"], "one call")
    cut, _, dl = _hold_to_the_model(cases[f"chained, max_delay {max_delay}"], "chained")
    assert [c.shape[2] // BLOCK for c in cut] == [1, 2, 1]
    dm.check_bits(np.concatenate(cut, axis=2), whole[0], f"chained against one call, max_delay {max_delay}")
    # what the handle carries is the last row as given
    last = cases[f"chained, max_delay {max_delay}"]["calls"][-1]
    d, g = dl.carried()
    assert np.array_equal(d, last["delay"][:, -1]) and np.array_equal(g, last["gains"][:, -1])


# ---- d. carry = 0 and reset ---------------------------------------------------------------------------------------------------------------
def test_carry_0_and_reset_start_from_silence(cases):
    case = cases["base, seg_blocks 1"]
    c = case["calls"][0]
    want = dm.run_model(case)[0]
    _, _, dl = _run_device(case)
    loud = dl.process(_dev(dm.noise(c["x"].shape, 99) * np.float32(50.0)), c["delay"][:, ::-1].copy(), 1, c["gains"], carry=True)
    assert np.abs(loud.cpu().numpy()).max() > 10.0
    dm.check_bits(dl.process(_dev(c["x"]), c["delay"], 1, c["gains"], carry=False).cpu().numpy(), want, "carry = 0 behind two calls")
    dl.process(_dev(dm.noise(c["x"].shape, 98)), c["delay"], 1, c["gains"], carry=True)
    dl.reset()
    assert dl.carried() is None
    with pytest.raises(Exception, match="carries nothing"):
        dl.process(_dev(c["x"]), c["delay"], 1, c["gains"], carry=True)
    # behind reset the ring itself is silent: a carried second call reads zeros in front of the first
    half = c["x"].shape[2] // 2
    a = dl.process(_dev(c["x"][:, :, :half]), c["delay"][:, :2], 1, c["gains"][:, :2]).cpu().numpy()
    b = dl.process(_dev(c["x"][:, :, half:]), c["delay"][:, 2:], 1, c["gains"][:, 2:], carry=True).cpu().numpy()
    dm.check_bits(np.concatenate([a, b], axis=2), want, "reset, then two calls")


# ---- e. shapes and strides -----------------------------------------------------------------------------------------------------------------
def test_64_objects_on_67_streams_and_one_row_for_all_streams():
    import open_headstage_amd as ohs
    S, K, max_delay = 67, 64, 600
    rng = np.random.default_rng(6764)
    x = dm.noise((S, K, BLOCK), 67)
    d = rng.uniform(1.0, max_delay, (S, 1, K))
    g = rng.uniform(-1.0, 1.0, (S, 1, K)).astype(np.float32)
    m, dl = dm.DelayModel(S, K, max_delay), ohs.ObjectDelay(S, K, max_delay)
    dm.check_bits(dl.process(_dev(x), d, 1, g).cpu().numpy(), m.process(x, d, 1, g), "per-stream rows")
    # [segs][K]: row_stream_stride 0, one row for all streams, ramping from the per-stream carry
    want = m.process(x, d[5], 1, g[5], carry=True)
    dm.check_bits(dl.process(_dev(x), d[5], 1, g[5], carry=True).cpu().numpy(), want, "shared rows")
    assert dl.last_launch()[2:] == m.last_launch
    # [K]: one row held over the call, no gains
    dm.check_bits(dl.process(_dev(x), d[7, 0], 1, carry=True).cpu().numpy(), m.process(x, d[7], 1, carry=True), "one row, no gains")


def test_wide_strides_leave_the_gaps_as_they_were():
    import torch
    import open_headstage_amd as ohs
    S, K, nb, max_delay, sentinel = 2, 3, 2, 600, -123.5
    frames = nb * BLOCK
    in_cs, in_ss, out_cs, out_ss = frames + 7, 3 * (frames + 7) + 11, frames + 64, 3 * (frames + 64) + 5
    x = dm.noise((S, K, frames), 21)
    d, g = dm.base_rows(S, K, nb, max_delay)
    buf_in = np.full(S * in_ss, sentinel, np.float32)
    for s in range(S):
        for c in range(K):
            buf_in[s * in_ss + c * in_cs:s * in_ss + c * in_cs + frames] = x[s, c]
    d_in, d_out = _dev(buf_in), torch.full((S * out_ss,), sentinel, device="cuda")
    dl = ohs.ObjectDelay(S, K, max_delay)
    dl.process_ptr(d_in.data_ptr(), d_out.data_ptr(), nb, in_ss, in_cs, out_ss, out_cs, K, 1, d, g, nb, False,
                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out, want = d_out.cpu().numpy(), dm.DelayModel(S, K, max_delay).process(x, d, 1, g)
    written = np.zeros(S * out_ss, bool)
    for s in range(S):
        for c in range(K):
            at = s * out_ss + c * out_cs
            dm.check_bits(out[at:at + frames], want[s, c], f"stream {s}, object {c}")
            written[at:at + frames] = True
    assert (out[~written] == np.float32(sentinel)).all() and (~written).sum() > 100
    assert np.array_equal(d_in.cpu().numpy(), buf_in)


# ---- f. special values ----------------------------------------------------------------------------------------------------------------------
def test_nan_inf_and_subnormal_input(cases):
    case = cases["special values"]
    got, _, _ = _hold_to_the_model(case, "special values")
    # the infinity max_delay + 2 frames in front of the second call is read by its first frame's oldest tap at weight 0: a NaN
    assert np.isnan(got[1][0, 0, 0]) and np.isfinite(got[1][0, 0, 1:4]).all()
    assert np.isnan(got[0][0, 1]).sum() >= 4 and (~np.isfinite(got[1][0, 1])).sum() >= 4
    sub = got[0][0, 2]
    assert (np.abs(sub) < np.finfo(np.float32).tiny).all() and (sub != 0).sum() > BLOCK      # subnormals in, subnormals out: no flush


# ---- g. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_output_and_the_handle_as_they_were(cases):
    import torch
    import open_headstage_amd as ohs
    case = cases["chained, max_delay 600"]
    S, K, max_delay = case["S"], case["Kmax"], 600
    c0, c1 = case["calls"][0], case["calls"][1]
    want = dm.run_model(case)
    dl = ohs.ObjectDelay(S, K, max_delay)
    dl.process(_dev(c0["x"]), c0["delay"], 1, c0["gains"], carry=False)
    before = dl.carried()
    nb = c1["x"].shape[2] // BLOCK
    frames = nb * BLOCK
    d_in, d_out = _dev(c1["x"]), torch.full((S, K, frames), 7.25, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(d_in_ptr=d_in.data_ptr(), d_out_ptr=d_out.data_ptr(), n_blocks=nb, in_ss=K * frames, in_cs=frames, out_ss=K * frames,
             out_cs=frames, k=K, seg=1, delay=c1["delay"], gains=c1["gains"], rss=nb, carry=True):
        dl.process_ptr(d_in_ptr, d_out_ptr, n_blocks, in_ss, in_cs, out_ss, out_cs, k, seg, delay, gains, rss, carry, stream)

    def bad(a, at, v):
        a = np.array(a, copy=True)
        a.reshape(-1)[at] = v
        return a

    d, g = c1["delay"], c1["gains"]
    refused = {
        "a NaN delay": dict(delay=bad(d, 3, np.nan)), "an infinite delay": dict(delay=bad(d, 0, np.inf)),
        "a delay below 1": dict(delay=bad(d, d.size - 1, 0.999999)), "a delay above max_delay": dict(delay=bad(d, 5, max_delay + 1e-9)),
        "a NaN gain": dict(gains=bad(g, 2, np.nan)), "an infinite gain": dict(gains=bad(g, g.size - 1, -np.inf)),
        "n_objects 0": dict(k=0), "n_objects above max_objects": dict(k=K + 1, delay=np.ones(S * nb * (K + 1)), gains=None),
        "another n_objects under carry": dict(k=K - 1), "d_out == d_in": dict(d_out_ptr=d_in.data_ptr()),
        "overlapping regions": dict(d_out_ptr=d_in.data_ptr() + 4 * frames), "d_in NULL": dict(d_in_ptr=0), "d_out NULL": dict(d_out_ptr=0),
        "a short channel stride": dict(in_cs=frames - 1), "a short stream stride": dict(out_ss=K * frames - 1),
        "seg_blocks 0": dict(seg=0), "a short row stride": dict(rss=nb - 1),
    }
    for what, kw in refused.items():
        with pytest.raises(ohs.ObjectDelayError) as e:
            call(**kw)
        assert e.value.status == 1, (what, e.value)
    # what the wrapper itself would stop or map: the C entry
    import ctypes as C
    from open_headstage_amd import delay as dmod

    def raw(n_blocks=nb, delay=d.ctypes.data_as(dmod.dp), carry=1):
        return dmod.delay_lib().ohs_delay_process(dl._h, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()), n_blocks, K * frames, frames,
                                                  K * frames, frames, K, 1, delay, g.ctypes.data_as(dmod.fp), nb, carry, C.c_void_p(stream))
    assert raw(carry=2) == 1 and b"neither 0 nor 1" in dmod.delay_lib().ohs_delay_last_error()
    assert raw(n_blocks=(1 << 24) + 1) == 1 and b"2^24" in dmod.delay_lib().ohs_delay_last_error()
    assert raw(delay=None) == 1 and b"delay is NULL" in dmod.delay_lib().ohs_delay_last_error()
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == np.float32(7.25)).all()                  # nothing was written
    after = dl.carried()
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    call()                                                                    # and the stream goes on as if nothing had been asked
    torch.cuda.synchronize()
    dm.check_bits(d_out.cpu().numpy(), want[1], "the call behind the refusals")
    # n_blocks == 0 is a call of nothing
    call(n_blocks=0)
    assert np.array_equal(dl.carried()[0], c1["delay"][:, -1])


# ---- h. asynchrony ----------------------------------------------------------------------------------------------------------------------------
def test_three_calls_queued_on_a_busy_stream_have_the_quiet_runs_bits():
    """tests/busy_stream.py's harness: the caller's side stream is busy when the calls are made, the input arrives by copies queued
    behind that work, delay and gains are overwritten the moment each call returns, the stream is still busy then, the three calls
    follow each other without a sync, and the outputs leave by copies queued behind each call"""
    import torch
    import open_headstage_amd as ohs
    S, K, nb, max_delay, calls = 3, 4, 4, 3000, 3
    frames = nb * BLOCK
    rng = np.random.default_rng(808)
    xs = [dm.noise((S, K, frames), 800 + n) for n in range(calls)]
    ds = [rng.uniform(1.0, max_delay, (S, nb, K)) for _ in range(calls)]
    gs = [rng.uniform(-1.0, 1.0, (S, nb, K)).astype(np.float32) for _ in range(calls)]
    quiet = ohs.ObjectDelay(S, K, max_delay)
    model = dm.DelayModel(S, K, max_delay)
    t0 = time.perf_counter()
    want = [quiet.process(_dev(xs[n]), ds[n], 1, gs[n]) for n in range(calls)]
    enqueue_s = time.perf_counter() - t0
    torch.cuda.synchronize()
    want_rec = quiet.last_launch()
    for n in range(calls):
        dm.check_bits(want[n].cpu().numpy(), model.process(xs[n], ds[n], 1, gs[n]), f"the quiet twin, call {n}")
    dl = ohs.ObjectDelay(S, K, max_delay)
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
                d, g = ds[n].copy(), bs.row_arrays({"gains": gs[n]})
                d_in.copy_(pinned[n], non_blocking=True)
                dl.process_ptr(d_in.data_ptr(), d_out.data_ptr(), nb, K * frames, frames, K * frames, frames, K, 1, d, g["gains"], nb, n > 0,
                               busy.handle)
                busy.premise("ohs_delay_process")
                d[...] = np.nan             # (the harness's scribble knows uint32 and float32 rows; the delays are f64)
                bs.scribble(g)
                keep[n].copy_(d_out, non_blocking=True)
                d_in.fill_(nan)
                d_out.fill_(nan)
            rec = dl.last_launch()
    finally:
        torch.cuda.synchronize()
    assert rec == want_rec, (rec, want_rec)
    for n in range(calls):
        bs.same_bits(keep[n].cpu().numpy(), want[n].cpu().numpy(), f"ohs_delay_process on a busy stream, call {n}")


# ---- i. composition with the tracked call --------------------------------------------------------------------------------------------------------
def test_render_with_distance_is_the_stage_then_the_tracked_call():
    """one stream, no sync in between, against: the stage; a sync and a host round trip; TrackedSceneProcessor.process_xyz.  Two calls,
    the second under both handles' carry"""
    import torch
    import open_headstage_amd as ohs
    from tests.test_cpu_layout import make_input, make_layout
    from tests.test_gpu_tracked import _mesh, _poses, _sources, _tracked
    S, K, blocks, seg, max_delay = 3, 5, 6, 2, 600
    n_segs = blocks // seg
    pos, tri, T = _mesh(2)
    dirs = make_layout(len(pos), 512)
    tr_a, tr_b = _tracked(pos, tri, dirs, streams=S), _tracked(pos, tri, dirs, streams=S)
    dl_a, dl_b = ohs.ObjectDelay(S, K, max_delay), ohs.ObjectDelay(S, K, max_delay)
    model = dm.DelayModel(S, K, max_delay)
    listener = np.array([0.25, -0.5, 0.125])
    side = torch.cuda.Stream()
    for n in range(2):
        x = make_input(S, K, blocks, seed=900 + n)
        radius = np.random.default_rng(910 + n).uniform(0.3, 4.0, (S, n_segs, K, 1))
        src = _sources(T, tri, S, n_segs, K, seed=90 + n) * radius + listener
        rot = _poses(S, n_segs, seed=95 + n)
        xd = _dev(x)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = ohs.render_with_distance(tr_a, dl_a, xd, src, rot, seg, listener=listener)
        side.synchronize()
        delay, gain = ohs.distance_rows(src, listener=listener)
        assert delay.shape == (S, n_segs, K) and 1.0 < delay.min() and delay.max() < max_delay
        between = dl_b.process(xd, delay, seg, gains=gain)
        torch.cuda.synchronize()
        host = between.cpu().numpy()
        dm.check_bits(host, model.process(x, delay, seg, gain), f"the stage, call {n}")
        want = tr_b.process_xyz(_dev(host), src - listener, rot, seg)
        torch.cuda.synchronize()
        bs.same_bits(got.cpu().numpy(), want.cpu().numpy(), f"render_with_distance, call {n}")
        assert np.isfinite(got.cpu().numpy()).all() and np.abs(got.cpu().numpy()).max() > 0

"""ohs_tracked_process (libohs_tracked.so, include/ohs_tracked.h): sources and poses in, two ears out, the rows on the device.

The yardstick is the COMPOSITION the header defines the result by, on the unchanged libraries and handles of their own:
ohs_lookup3p_rows (PrunedTriangleLookup's handle) -> ohs_scene3_process_blended3 (TriSceneProcessor), prev_* handed over by hand.
Everything is bit for bit: the output, the five row planes, the launch record.  No tolerance appears in this file.
3 streams, 6 blocks, seg_blocks 2, gain 0.7 unless a test says otherwise.

Not run here: the refusal of a handle that failed in the middle of an earlier call -- the product build has no way to make a HIP call
fail, and none is provoked."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import busy_stream as bs
from tests.test_cpu_layout import BLOCK, make_input, make_layout

pytestmark = pytest.mark.gpu

S = 3
NB = 10
GAIN = 0.7
BLOCKS, SEG = 6, 2


# ---- the two paths -----------------------------------------------------------------------------------------------------------------
def _mesh(level):
    from open_headstage_amd import lookup, lookup3
    pos, tri = lookup3.octahedron_mesh(level)
    return pos, np.ascontiguousarray(tri, np.uint32), lookup.table_xyz(pos).astype(np.float64)


def _tracked(pos, tri, dirs, streams=S, grid=0):
    import open_headstage_amd as ohs
    h = ohs.TrackedSceneProcessor(streams, pos, tri, grid=grid, num_bands=NB)
    h.set_gain(GAIN)
    if dirs is not None:
        h.set_directions(dirs)
    return h


class Composed:
    """PrunedTriangleLookup.rows' C entry on Cartesian input, then TriSceneProcessor.process; what stood in front of a call is kept by hand"""

    def __init__(self, pos, tri, dirs, streams=S, grid=0):
        import open_headstage_amd as ohs
        self.lk = ohs.PrunedTriangleLookup(pos, tri, grid=grid)
        self.sc = ohs.TriSceneProcessor(streams, num_bands=NB)
        self.sc.set_gain(GAIN)
        self.sc.set_directions(dirs)
        self.S = streams
        self.prev = None
        self.rows = None

    def lookup(self, n_segs, K, src, sss, sks, rot, rss):
        from open_headstage_amd import lookup3p
        from open_headstage_amd.lookup import dp
        n = self.S * n_segs * K
        arrays, ptrs = self.lk._outputs(n, False)
        lookup3p.lookup3p_check(lookup3p.lookup3p_lib().ohs_lookup3p_rows(
            self.lk._h, self.S, n_segs, K, src.ctypes.data_as(dp), sss, sks, None if rot is None else rot.ctypes.data_as(dp), rss, *ptrs))
        return tuple(a.reshape(self.S, n_segs, K) for a in arrays)

    def process(self, x, seg, src, sss, sks, rot=None, rss=0, gains=None, carry=False, crossfade=True):
        K, n_segs = src.shape[-2], -(-(x.shape[2] // BLOCK) // seg)
        i0, i1, i2, w1, w2 = self.rows = self.lookup(n_segs, K, np.ascontiguousarray(src, np.float64), sss, sks, rot, rss)
        p = self.prev if carry else None
        pg = None if p is None else p[5]
        if p is not None and pg is None and gains is not None:      # (the previous call's last segment had no gains: they read 1.0)
            pg = np.ones((self.S, K), np.float32)
        y = self.sc.process(x, i0, seg, gains, None if p is None else p[0], pg, crossfade, i1, w1, None if p is None else p[1],
                            None if p is None else p[3], i2, w2, None if p is None else p[2], None if p is None else p[4])
        self.prev = [a[:, -1, :].copy() for a in (i0, i1, i2, w1, w2)] + [None if gains is None else np.asarray(gains, np.float32)[:, -1, :].copy()]
        return y


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


def _sources(T, tri, streams, n_segs, K, seed):
    """[streams][n_segs][K][3] f64 in the table's frame: strictly inside a triangle, exactly on an edge's midpoint, exactly on a
    measurement, in turn -- every object somewhere else in every segment"""
    rng = np.random.default_rng(seed)
    src = np.empty((streams, n_segs, K, 3), np.float64)
    for n, (s, k, c) in enumerate(np.ndindex(streams, n_segs, K)):
        a, b, d = T[tri[rng.integers(len(tri))]]
        kind = (n + seed) % 3
        if kind == 0:
            w = 0.1 + rng.random(3)
            src[s, k, c] = (w[0] * a + w[1] * b + w[2] * d) / w.sum()
        elif kind == 1:
            src[s, k, c] = 0.5 * (a + b)
        else:
            src[s, k, c] = a
    return src


def _poses(streams, n_segs, seed):
    from open_headstage_amd import lookup
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(lookup.pose_matrices(rng.uniform(-180, 180, (streams, n_segs)), rng.uniform(-40, 40, (streams, n_segs)),
                                                     rng.uniform(-30, 30, (streams, n_segs))))


def _gains(streams, n_segs, K, seed):
    return np.random.default_rng(seed).choice(np.array([1.0, 0.5, 0.8, 1.0], np.float32), (streams, n_segs, K))


def _eq_on(*handles):
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    for h in handles:
        for i, b in enumerate(synth.eq_table()[:NB]):
            h.set_band_coeffs(i, ohs.biquad_coefficients(b.filter_type, synth.FS, b.center_freq, b.q, b.gain_db), b.enabled)
        h.set_eq_enabled(True)


def _same(got, want, what):
    import torch
    torch.cuda.synchronize()
    bs.same_bits(got.cpu().numpy(), want.cpu().numpy(), what)


def _same_rows(tr, co, what):
    for name, a, b in zip(("idx0", "idx1", "idx2", "w1", "w2"), tr.rows(), co.rows):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, name)


def _same_record(tr, co, what):
    assert tr.last_launch() == co.sc.last_launch() + (co.lk.last_launch()[2],), (what, tr.last_launch(), co.sc.last_launch(), co.lk.last_launch())


# ---- a. small scenes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("K", [1, 2, 5])
def test_small_scenes_have_the_composed_paths_bits(level, K):
    pos, tri, T = _mesh(level)
    assert len(tri) == (8, None, 128)[level]
    dirs = make_layout(len(pos), 37 if K == 2 else 512)
    tr, co = _tracked(pos, tri, dirs), Composed(pos, tri, dirs)
    x = _dev(make_input(S, K, BLOCKS, seed=9100 + 10 * K + level))
    n_segs = BLOCKS // SEG
    src = _sources(T, tri, S, n_segs, K, seed=K + level)
    rot, gains = _poses(S, n_segs, seed=level), _gains(S, n_segs, K, seed=K)
    seen = np.zeros(3, np.int64)
    for what, use_gains, use_rot, eq in (("plain", False, False, False), ("gains", True, False, False), ("rot", False, True, False),
                                         ("gains, rot and the EQ", True, True, True)):
        tr.reset()
        co.sc.reset()
        if eq:
            _eq_on(tr, co.sc)
        g, r = gains if use_gains else None, rot if use_rot else None
        want = co.process(x, SEG, src, n_segs, 1, r, n_segs if use_rot else 0, g)
        got = tr.process_xyz(x, src, r, SEG, g, carry=False)
        _same(got, want, f"level {level}, K = {K}, {what}")
        _same_rows(tr, co, what)
        _same_record(tr, co, what)
        rec = tr.last_launch()
        seen += (rec[3] > 0, rec[4] > 0, rec[5] > 0)
    # the four- and the six-row passes and the lookup's pass 2 all took part (the two-row passes: K = 1 on a measurement)
    assert seen.all(), seen


def test_angles_in_are_pruned_triangle_lookup_rows_conventions():
    """process(x, src_az, src_el, yaw, pitch, roll, ...) against PrunedTriangleLookup.rows on the same angles"""
    import open_headstage_amd as ohs
    pos, tri, _ = _mesh(2)
    K, n_segs = 5, BLOCKS // SEG
    dirs = make_layout(len(pos), 512)
    tr = _tracked(pos, tri, dirs)
    lk, sc = ohs.PrunedTriangleLookup(pos, tri), ohs.TriSceneProcessor(S, num_bands=NB)
    sc.set_gain(GAIN)
    sc.set_directions(dirs)
    rng = np.random.default_rng(5)
    az, el = rng.uniform(-180, 180, (S, n_segs, K)).astype(np.float32), rng.uniform(-80, 80, (S, n_segs, K)).astype(np.float32)
    az[0, 0, 0], el[0, 0, 0] = -pos[3, 0], pos[3, 1]           # (a source on a measurement: plugin azimuths are SOFA's negated)
    yaw, pitch, roll = (rng.uniform(-60, 60, (S, n_segs)).astype(np.float32) for _ in range(3))
    x = _dev(make_input(S, K, BLOCKS, seed=77))
    i0, i1, i2, w1, w2 = lk.rows(az, el, yaw, pitch, roll)
    want = sc.process(x, i0, SEG, None, None, None, True, i1, w1, None, None, i2, w2)
    got = tr.process(x, az, el, yaw, pitch, roll, SEG)
    _same(got, want, "angles in")
    for a, b in zip(tr.rows(), (i0, i1, i2, w1, w2)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert tr.last_launch() == sc.last_launch() + (lk.last_launch()[2],)


# ---- b. chaining ------------------------------------------------------------------------------------------------------------------------
def test_one_call_equals_three_under_carry_and_the_composed_path_with_prev_by_hand():
    import torch
    pos, tri, T = _mesh(2)
    K, blocks = 5, 12
    n_segs = blocks // SEG
    dirs = make_layout(len(pos), 512)
    x = make_input(S, K, blocks, seed=31)
    src, gains = _sources(T, tri, S, n_segs, K, seed=3), _gains(S, n_segs, K, seed=4)
    whole = _tracked(pos, tri, dirs).process_xyz(_dev(x), src, None, SEG, gains)
    tr, co = _tracked(pos, tri, dirs), Composed(pos, tri, dirs)
    parts, want, b0 = [], [], 0
    for n, nb in enumerate((2, 4, 6)):
        k0, k1 = b0 // SEG, (b0 + nb) // SEG
        xs = _dev(x[:, :, b0 * BLOCK:(b0 + nb) * BLOCK])
        s, g = np.ascontiguousarray(src[:, k0:k1]), np.ascontiguousarray(gains[:, k0:k1])
        parts.append(tr.process_xyz(xs, s, None, SEG, g))          # (carry=None: carried from the second call on)
        want.append(co.process(xs, SEG, s, k1 - k0, 1, gains=g, carry=n > 0))
        _same_record(tr, co, f"call {n}")
        b0 += nb
    _same(torch.cat(parts, 2), whole, "2 + 4 + 6 blocks under carry against one call of 12")
    _same(torch.cat(want, 2), whole, "the composed path with prev_* by hand against one call of 12")


def test_reset_then_fresh_equals_a_new_handle():
    pos, tri, T = _mesh(0)
    K, n_segs = 2, BLOCKS // SEG
    dirs = make_layout(len(pos), 512)
    x = _dev(make_input(S, K, BLOCKS, seed=41))
    src = _sources(T, tri, S, n_segs, K, seed=6)
    tr = _tracked(pos, tri, dirs)
    tr.process_xyz(x, _sources(T, tri, S, n_segs, K, seed=7), None, SEG)
    tr.reset()
    with pytest.raises(Exception, match="carries no rows"):
        tr.process_xyz(x, src, None, SEG, carry=True)
    got = tr.process_xyz(x, src, None, SEG)         # (carry=None behind a reset: FRESH)
    _same(got, _tracked(pos, tri, dirs).process_xyz(x, src, None, SEG, carry=False), "reset, then FRESH")


# ---- c. the header's limits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 63])
def test_sixty_four_and_sixty_three_objects(K):
    streams, pos, tri, T = 5, *_mesh(2)
    n_segs = BLOCKS // SEG
    dirs = make_layout(len(pos), 37)
    x = _dev(make_input(streams, K, BLOCKS, seed=K))
    src, rot = _sources(T, tri, streams, n_segs, K, seed=K), _poses(streams, n_segs, seed=K)
    tr, co = _tracked(pos, tri, dirs, streams), Composed(pos, tri, dirs, streams)
    for n in range(2):          # (the second call carried)
        want = co.process(x, SEG, src, n_segs, 1, rot, n_segs, carry=n > 0)
        _same(tr.process_xyz(x, src, rot, SEG), want, f"K = {K}, call {n}")
        _same_rows(tr, co, K)
        _same_record(tr, co, K)


def test_a_table_of_65536_rows_with_a_mesh_over_its_first_rows():
    pos, tri, T = _mesh(2)
    K, n_segs = 5, BLOCKS // SEG
    dirs = (0.02 * np.random.default_rng(65536).standard_normal((65536, 2, 8))).astype(np.float32)
    x = _dev(make_input(S, K, BLOCKS, seed=65))
    src = _sources(T, tri, S, n_segs, K, seed=65)
    tr, co = _tracked(pos, tri, dirs), Composed(pos, tri, dirs)
    assert tr.n_directions == 65536 and tr.n_mesh_directions == len(pos) == 66
    _same(tr.process_xyz(x, src, None, SEG), co.process(x, SEG, src, n_segs, 1), "65 536 rows")
    _same_record(tr, co, "65 536 rows")


def test_a_call_that_crosses_a_lookup_chunk_cut_inside_a_group_of_objects():
    """66 streams x 64 segments x 63 objects = 266 112 queries: the cut at query 262 144 = 63 * 4161 + 1 falls behind the first object of
    a group.  The audio is generated on the device."""
    import torch
    streams, K, blocks = 66, 63, 64
    pos, tri, T = _mesh(2)
    assert streams * blocks * K == 266112 and (1 << 18) == 63 * 4161 + 1
    dirs = make_layout(len(pos), 37)
    x = torch.randn((streams, K, blocks * BLOCK), device="cuda", generator=torch.Generator(device="cuda").manual_seed(66)) * 0.05
    rng = np.random.default_rng(66)
    w = 0.05 + rng.random((streams, blocks, K, 3))
    corners = T[tri[rng.integers(len(tri), size=(streams, blocks, K))]]           # [..][3 corners][3]
    src = np.ascontiguousarray((w[..., None] * corners).sum(-2) / w.sum(-1, keepdims=True))
    src[:, ::7, ::5] = T[rng.integers(len(T), size=src[:, ::7, ::5].shape[:-1])]    # (some on measurements: pass 2 on both sides of the cut)
    tr, co = _tracked(pos, tri, dirs, streams), Composed(pos, tri, dirs, streams)
    want = co.process(x, 1, src, blocks, 1)
    got = tr.process_xyz(x, src, None, 1)
    assert co.lk.last_launch()[1] == 2 and co.lk.last_launch()[2] > 0
    _same(got, want, "across the chunk cut")
    _same_rows(tr, co, "across the chunk cut")
    _same_record(tr, co, "across the chunk cut")


# ---- d. asynchrony ------------------------------------------------------------------------------------------------------------------------
def test_three_calls_queued_on_a_busy_stream_have_the_quiet_runs_bits():
    """tests/busy_stream.py's harness: the caller's side stream is busy when the calls are made, the input arrives by copies queued
    behind that work, src, rot and gains are overwritten the moment each call returns, the stream is still busy then, the three calls
    follow each other without a sync, and the outputs leave by copies queued behind each call"""
    import torch
    pos, tri, T = _mesh(2)
    K, n_segs, frames, calls = 5, BLOCKS // SEG, BLOCKS * BLOCK, 3
    dirs = make_layout(len(pos), 512)
    xs = [make_input(S, K, BLOCKS, seed=500 + n) for n in range(calls)]
    srcs = [_sources(T, tri, S, n_segs, K, seed=50 + n) for n in range(calls)]
    rots = [_poses(S, n_segs, seed=60 + n) for n in range(calls)]
    gains = [_gains(S, n_segs, K, seed=70 + n) for n in range(calls)]
    quiet = _tracked(pos, tri, dirs)
    t0 = time.perf_counter()
    want = [quiet.process_xyz(_dev(xs[n]), srcs[n], rots[n], SEG, gains[n]) for n in range(calls)]
    enqueue_s = time.perf_counter() - t0
    torch.cuda.synchronize()
    want_rec = quiet.last_launch()
    h = _tracked(pos, tri, dirs)
    busy = bs.BusyStream()
    nan = float("nan")
    pinned = [torch.from_numpy(x.copy()).pin_memory() for x in xs]
    d_in = torch.full((S, K, frames), nan, device="cuda")
    d_out = torch.full((S, 2, frames), nan, device="cuda")
    keep = [torch.full((S, 2, frames), nan, device="cuda") for _ in range(calls)]
    torch.cuda.synchronize()
    try:
        busy.fill(bs.filler_seconds(min(enqueue_s, 0.01)))
        with torch.cuda.stream(busy.stream):
            for n in range(calls):
                src, rot, g = srcs[n].copy(), rots[n].copy(), bs.row_arrays({"gains": gains[n]})
                d_in.copy_(pinned[n], non_blocking=True)
                h.process_ptr(d_in.data_ptr(), d_out.data_ptr(), BLOCKS, K * frames, frames, 2 * frames, frames, K, SEG, src, n_segs, 1, rot,
                              n_segs, g["gains"], True, None, busy.handle)
                busy.premise("ohs_tracked_process")
                src[...] = np.nan           # (the harness's scribble knows uint32 and float32 rows; these two are f64)
                rot[...] = np.nan
                bs.scribble(g)
                keep[n].copy_(d_out, non_blocking=True)
                d_in.fill_(nan)
                d_out.fill_(nan)
            rec = h.last_launch()
    finally:
        torch.cuda.synchronize()
    assert rec == want_rec, (rec, want_rec)
    for n in range(calls):
        bs.same_bits(keep[n].cpu().numpy(), want[n].cpu().numpy(), f"ohs_tracked_process on a busy stream, call {n}")


# ---- e. refusals --------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_output_and_the_handle_as_they_were():
    import torch
    from open_headstage_amd import SceneError
    from open_headstage_amd.lookup import dp
    pos, tri, T = _mesh(2)
    K, n_segs, frames = 5, BLOCKS // SEG, BLOCKS * BLOCK
    dirs = make_layout(len(pos), 512)
    x = _dev(make_input(S, K, BLOCKS, seed=90))
    src = _sources(T, tri, S, n_segs, K, seed=9)
    rot = _poses(S, n_segs, seed=9)
    nan = float("nan")
    d_out = torch.full((S, 2, frames), nan, device="cuda")
    tr = _tracked(pos, tri, dirs)
    first = tr.process_xyz(x, src, rot, SEG).clone()
    tr.reset()
    ok = dict(d_in=x.data_ptr(), d_out=d_out.data_ptr(), n_blocks=BLOCKS, in_ss=K * frames, in_cs=frames, out_ss=2 * frames, out_cs=frames,
              K=K, seg=SEG, src=src, sss=n_segs, sks=1, rot=rot, rss=n_segs, gains=None, mode=1, carry=0)

    def call(h=tr, **over):
        a = dict(ok, **over)
        status = h._fn("process")(h._h, C.c_void_p(a["d_in"]), C.c_void_p(a["d_out"]), a["n_blocks"], a["in_ss"], a["in_cs"], a["out_ss"], a["out_cs"],
                                  a["K"], a["seg"], None if a["src"] is None else a["src"].ctypes.data_as(dp), a["sss"], a["sks"],
                                  None if a["rot"] is None else a["rot"].ctypes.data_as(dp), a["rss"], None, a["mode"], a["carry"], None)
        h._check(status)

    def bad(a, at, v):
        a = a.copy()
        a.reshape(-1)[at] = v
        return a
    refused = [
        (dict(d_in=0), "NULL"), (dict(d_out=0), "NULL"), (dict(src=None), "src is NULL"),
        (dict(K=0), "outside 1 .. 64"), (dict(K=65), "outside 1 .. 64"), (dict(seg=0), "seg_blocks is 0"), (dict(mode=2), "switch_mode"),
        (dict(carry=2), "carry must be"), (dict(n_blocks=(1 << 24) + 1), "n_blocks too large"),
        (dict(n_blocks=1 << 23, seg=1, K=64), "schedule too large"),
        (dict(in_cs=frames - 1), "strides smaller"), (dict(out_cs=frames - 1), "strides smaller"), (dict(in_ss=frames), "strides smaller"),
        (dict(d_out=x.data_ptr()), "overlap"),
        (dict(src=bad(src, 7, np.nan)), "source coordinate"), (dict(src=bad(src, 8, np.inf)), "source coordinate"),
        (dict(src=bad(src, 9, 1.0000001e15)), "source coordinate"), (dict(rot=bad(rot, 10, np.nan)), "matrix element"),
        (dict(rot=bad(rot, 11, -2e15)), "matrix element"),
        (dict(sss=1, sks=1), "src_stream_stride"), (dict(rss=n_segs - 1), "rot_stream_stride"),
        (dict(carry=1), "carries no rows"),
    ]
    for over, text in refused:
        with pytest.raises(SceneError, match=text) as e:
            call(**over)
        assert e.value.status == 1, (over, e.value)
    # no table, and a table with fewer rows than the mesh names
    bare = _tracked(pos, tri, None)
    with pytest.raises(SceneError, match="no direction table"):
        call(bare)
    bare.set_directions(dirs[:len(pos) - 1])
    with pytest.raises(SceneError, match="65 rows, the mesh names 66"):
        call(bare)
    torch.cuda.synchronize()
    assert bool(torch.isnan(d_out).all()), "a refused call wrote to d_out"
    # a source of magnitude 1e15 exactly is accepted; then CARRY with another K is refused, and the handle is as it was
    call(src=bad(src, 9, 1e15))
    tr.reset()
    tr.process_xyz(x, src, rot, SEG)
    with pytest.raises(SceneError, match="carried rows hold 5 objects"):
        tr.process_xyz(x[:, :4].contiguous(), np.ascontiguousarray(src[:, :, :4]), rot, SEG, carry=True)
    tr.reset()
    _same(tr.process_xyz(x, src, rot, SEG), first, "the handle behind the refusals")


# ---- f. flush modes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_flush_modes_on_a_loud_signal(mode):
    pos, tri, T = _mesh(2)
    K, n_segs = 5, BLOCKS // SEG
    dirs = make_layout(len(pos), 512)
    x = _dev(make_input(S, K, BLOCKS, seed=110 + mode) * np.float32(8.0))
    src, gains = _sources(T, tri, S, n_segs, K, seed=11), _gains(S, n_segs, K, seed=11)
    tr, co = _tracked(pos, tri, dirs), Composed(pos, tri, dirs)
    tr.set_flush_denormals(mode)
    co.sc.set_flush_denormals(mode)
    _same(tr.process_xyz(x, src, None, SEG, gains), co.process(x, SEG, src, n_segs, 1, gains=gains), f"flush mode {mode}")
    _same_record(tr, co, f"flush mode {mode}")

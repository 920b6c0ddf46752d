"""The session renderer (open_headstage_amd/session.py), the part that needs no GPU: head tracks to table rows, the chunk planner,
PCM and WAV I/O, the package surface.  Every yardstick is brute force, written out here: a loop over the grid, a walk over the
blocks, Python integers."""
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 512


# ---- nearest_set --------------------------------------------------------------------------------------------------------------
def _nearest_brute(y, grid):
    best, best_d = 0, None
    for i, g in enumerate(grid):
        d = abs(((y - g + 180.0) % 360.0) - 180.0)
        if best_d is None or d < best_d:        # (strictly: the lowest index wins a tie)
            best, best_d = i, d
    return best


@pytest.mark.parametrize("grid", [np.arange(-180.0, 180.0, 5.0), np.array([170.0, -175.0, 0.0, 3.0, 90.0, -90.5, 44.0])],
                         ids=["5deg", "irregular"])
def test_nearest_set_against_a_brute_force_loop(grid):
    from open_headstage_amd.session import nearest_set
    rng = np.random.default_rng(1)
    yaws = np.concatenate([rng.uniform(-180, 180, 200), rng.uniform(-1000, 1000, 100),
                           [180.0, -180.0, 179.9, -179.9, 177.5, -177.5, 2.5, -2.5, 1.5, 360.0, 540.0, -540.0, 722.5, 0.0]])
    got = nearest_set(yaws, grid)
    assert got.dtype == np.uint32 and got.shape == yaws.shape
    want = [_nearest_brute(float(y), grid) for y in yaws]
    assert got.tolist() == want


def test_nearest_set_wraps_breaks_ties_low_and_keeps_shapes():
    from open_headstage_amd.session import nearest_set
    grid = np.arange(-180.0, 180.0, 5.0)                        # 72 sets, -180 is index 0, 175 index 71
    assert nearest_set(179.0, grid) == 0                        # across the wrap: -180 is 1 degree away, 175 is 4
    assert nearest_set(-181.0, grid) == 0 and nearest_set(180.0, grid) == 0
    assert nearest_set(177.5, grid) == 0                        # a tie between index 71 (175) and index 0 (-180): the lowest
    assert nearest_set(2.5, grid) == 36 and nearest_set(-2.5, grid) == 35      # ties between 35 (-5), 36 (0), 37 (5)
    assert nearest_set(365.0, grid) == 37 and nearest_set(-715.0, grid) == 37  # outside (-180, 180]
    a = nearest_set(np.zeros((3, 4)), grid)
    assert a.shape == (3, 4) and (a == 36).all()
    with pytest.raises(ValueError):
        nearest_set(0.0, [])


# ---- HeadTrack ----------------------------------------------------------------------------------------------------------------
def test_head_track_interpolates_through_180_and_holds_outside_the_log():
    from open_headstage_amd.session import HeadTrack
    tr = HeadTrack([1.0, 2.0, 4.0], [170.0, -170.0, -150.0])
    assert tr.at(1.5) == pytest.approx(180.0)                   # through 180, not through 0
    assert tr.at(1.25) == pytest.approx(175.0)
    assert ((tr.at(1.75) + 180.0) % 360.0) - 180.0 == pytest.approx(-175.0)
    assert ((tr.at(3.0) + 180.0) % 360.0) - 180.0 == pytest.approx(-160.0)
    assert tr.at(0.0) == pytest.approx(170.0) and tr.at(-5.0) == pytest.approx(170.0)
    assert ((tr.at(9.0) + 180.0) % 360.0) - 180.0 == pytest.approx(-150.0)
    v = tr.at(np.array([1.0, 1.5, 2.0]))
    assert v.shape == (3,) and np.allclose(v, [170.0, 180.0, 190.0])
    assert HeadTrack([0.0], [33.0]).at(7.0) == pytest.approx(33.0)


@pytest.mark.parametrize("times", [[0.0, 1.0, 1.0], [0.0, 2.0, 1.0], []])
def test_head_track_refuses_times_that_do_not_increase(times):
    from open_headstage_amd.session import HeadTrack
    with pytest.raises(ValueError):
        HeadTrack(times, [0.0] * len(times))
    with pytest.raises(ValueError):
        HeadTrack([0.0, 1.0], [0.0])


# ---- yaw_rows -----------------------------------------------------------------------------------------------------------------
def test_yaw_rows_against_sampling_the_tracks_by_hand():
    from open_headstage_amd.session import HeadTrack, nearest_set, yaw_rows
    fs, seg = 48000.0, 3
    grid = np.arange(-180.0, 180.0, 5.0)
    tracks = [HeadTrack([0.0, 0.5, 1.0], [0.0, 170.0, 200.0]), HeadTrack([0.1, 0.9], [-30.0, 30.0]), HeadTrack([0.0], [12.4])]
    for first_block, n_blocks in [(0, 10), (6, 12), (7, 12), (9, 1), (8, 1)]:
        k0, k1 = first_block // seg, -(-(first_block + n_blocks) // seg)
        want = [[_nearest_brute(float(tr.at(k * seg * BLOCK / fs)), grid) for k in range(k0, k1)] for tr in tracks]
        got = yaw_rows(tracks, first_block, n_blocks, seg, fs, grid)
        assert got.dtype == np.uint32 and got.tolist() == want, (first_block, n_blocks)
        one = yaw_rows(tracks[0], first_block, n_blocks, seg, fs, grid)
        assert one.ndim == 1 and one.tolist() == want[0]
    assert len(set(yaw_rows(tracks[0], 6, 60, seg, fs, grid).tolist())) > 5          # (the track moves: the rows change)
    # plain degrees per segment in place of tracks
    deg = np.array([[0.0, 2.6, 177.6, -181.0], [5.0, 5.0, 5.0, 5.0]])
    assert yaw_rows(deg, 6, 12, seg, fs, grid).tolist() == nearest_set(deg, grid).tolist()
    assert yaw_rows(deg[0], 6, 12, seg, fs, grid).tolist() == nearest_set(deg[0], grid).tolist()
    with pytest.raises(ValueError):
        yaw_rows(deg[:, :3], 6, 12, seg, fs, grid)


# ---- plan_calls ---------------------------------------------------------------------------------------------------------------
def test_plan_calls_over_an_exhaustive_box():
    """every call's rows, expanded block by block, give the session's set per block -- so the fades (a block whose set differs from
    the block in front of it) stay where the session puts them"""
    from open_headstage_amd.session import call_rows, plan_calls
    n_cases = 0
    for seg in (1, 2, 3, 4, 6):
        for first, n_blocks, chunk in itertools.product(range(0, 13), range(0, 13), range(1, 13)):
            first_seg, end_seg = first // seg, -(-(first + n_blocks) // seg)
            rows = (np.arange(first_seg, max(end_seg, first_seg + 1)) * 7 + 3) % 11           # the session's set per segment
            rows2 = np.stack([rows, rows[::-1]])
            per_block = [int(rows[b // seg - first_seg]) for b in range(first, first + n_blocks)]
            calls = list(plan_calls(first, n_blocks, seg, chunk))
            pos, got, got2 = first, [], []
            for i, (start, n, g, rep) in enumerate(calls):
                assert start == pos and 1 <= n <= chunk, (first, n_blocks, seg, chunk, calls)
                assert seg % g == 0 and rep == seg // g and start % g == 0
                if i + 1 < len(calls):
                    assert n % g == 0                   # only the last call may end in a short segment
                assert g == math.gcd(math.gcd(seg, start), n if i + 1 < len(calls) else 0)
                idx = call_rows(rows, first_seg, start, n, g, seg)
                assert idx.dtype == np.uint32 and idx.shape == (-(-n // g),)
                got += [int(idx[t // g]) for t in range(n)]            # the C call's rule: segment t // g of the call
                idx2 = call_rows(rows2, first_seg, start, n, g, seg)
                assert idx2.shape == (2, -(-n // g)) and idx2[0].tolist() == idx.tolist()
                got2 += [int(idx2[1, t // g]) for t in range(n)]
                pos += n
            assert pos == first + n_blocks and got == per_block
            assert got2 == [int(rows2[1, b // seg - first_seg]) for b in range(first, first + n_blocks)]
            n_cases += 1
    assert n_cases == 5 * 13 * 13 * 12
    assert list(plan_calls(0, 11, 2, 4)) == [(0, 4, 2, 1), (4, 4, 2, 1), (8, 3, 2, 1)]
    assert list(plan_calls(0, 11, 2, 3)) == [(0, 3, 1, 2), (3, 3, 1, 2), (6, 3, 1, 2), (9, 2, 1, 2)]
    assert list(plan_calls(5, 0, 2, 4)) == []
    for bad in [(0, 4, 0, 4), (0, 4, 2, 0), (-1, 4, 2, 4)]:
        with pytest.raises(ValueError):
            list(plan_calls(*bad))


# ---- PCM ----------------------------------------------------------------------------------------------------------------------
def _ints(bits, channels=3, frames=257, seed=0):
    rng = np.random.default_rng(seed + bits)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    v = rng.integers(lo, hi + 1, (channels, frames), dtype=np.int64)
    if bits == 32:
        v &= ~np.int64(0xFF)                    # float32 holds 24 bits: the values a float32 sample can represent
    v[0, :4] = [lo, hi if bits < 32 else hi - 0xFF, 0, -1 if bits < 32 else -256]
    return v


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_pcm_decode_of_encode_is_the_identity_on_representable_values(bits):
    from open_headstage_amd.session import pcm_decode, pcm_encode
    v = _ints(bits)
    raw = b"".join(int(s).to_bytes(bits // 8, "little", signed=True) for s in v.T.reshape(-1))       # (interleaved frames)
    x = pcm_decode(raw, bits, v.shape[0])
    assert x.dtype == np.float32 and x.shape == v.shape
    assert (x.astype(np.float64) * float(1 << (bits - 1)) == v).all()          # decode is int / 2^(bits - 1), exactly
    assert pcm_encode(x, bits) == raw
    assert (pcm_decode(pcm_encode(x, bits), bits, v.shape[0]) == x).all()


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_pcm_encode_clips_and_rounds_half_to_even(bits):
    from open_headstage_amd.session import pcm_encode
    full = float(1 << (bits - 1))
    x = np.array([[1.0, 2.5, -1.0, -3.0, 0.5 / full, 1.5 / full, 2.5 / full, -0.5 / full, -1.5 / full, 0.4 / full, -0.6 / full]],
                 np.float64)
    want = [(1 << (bits - 1)) - 1, (1 << (bits - 1)) - 1, -(1 << (bits - 1)), -(1 << (bits - 1)), 0, 2, 2, 0, -2, 0, -1]
    raw = pcm_encode(x, bits)
    w = bits // 8
    got = [int.from_bytes(raw[i * w:(i + 1) * w], "little", signed=True) for i in range(x.shape[1])]
    assert got == want
    for bad in (8, 12, 64):
        with pytest.raises(ValueError):
            pcm_encode(x, bad)


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_wav_round_trip(tmp_path, bits):
    from open_headstage_amd.session import pcm_decode, read_wav, write_wav
    v = _ints(bits, channels=6, frames=1000, seed=9)
    x = (v.astype(np.float64) / float(1 << (bits - 1))).astype(np.float32)
    p = tmp_path / f"a{bits}.wav"
    write_wav(p, x, 44100, bits)
    y, rate, b = read_wav(p)
    assert rate == 44100 and b == bits and y.shape == x.shape and (y == x).all()
    import wave
    with wave.open(str(p), "rb") as w:              # ... and chunk by chunk, as render_files reads
        assert (w.getnchannels(), w.getsampwidth(), w.getnframes()) == (6, bits // 8, 1000)
        parts = [pcm_decode(w.readframes(n), bits, 6) for n in (300, 300, 400)]
    assert (np.concatenate(parts, axis=1) == x).all()


def test_tracker_csv(tmp_path):
    from open_headstage_amd.session import read_track_csv
    p = tmp_path / "t.csv"
    p.write_text("time_s,yaw_deg\n# a comment\n0.0,10\n\n0.5, 20.5\n1.0,-170\n")
    tr = read_track_csv(p)
    assert tr.times_s.tolist() == [0.0, 0.5, 1.0] and tr.at(0.25) == pytest.approx(15.25)
    p.write_text("0.0,10\n0.0,11\n")
    with pytest.raises(ValueError):
        read_track_csv(p)
    p.write_text("0.0,10\nx,y\n")
    with pytest.raises(ValueError):
        read_track_csv(p)


# ---- the package surface ------------------------------------------------------------------------------------------------------
def test_package_exports_the_session_names():
    import open_headstage_amd as ohs
    for name in ("SessionRenderer", "HeadTrack", "yaw_rows", "nearest_set", "plan_calls", "render_files"):
        assert hasattr(ohs, name) and name in ohs.__all__, name
    for m in ("layout", "stereo", "layout_from_sofa", "stereo_from_sofa", "render", "reset"):
        assert callable(getattr(ohs.SessionRenderer, m)), m


def test_render_command_line_prints_its_help():
    r = subprocess.run([sys.executable, "-m", "open_headstage_amd.render", "--help"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for word in ("--sofa", "--layout", "--yaw-step", "--track", "--late", "--outdir"):
        assert word in r.stdout, word



def test_layout_constructors_refuse_a_late_part_before_anything_is_created():
    import open_headstage_amd as ohs
    late = np.zeros((4, 100), np.float32)
    with pytest.raises(ValueError):
        ohs.SessionRenderer.layout(2, np.zeros((3, 6, 2, 8), np.float32), [-10.0, 0.0, 10.0], late_irs=late)
    with pytest.raises(ValueError):
        ohs.SessionRenderer.layout_from_sofa(2, None, ohs.LAYOUT_5_1, [-10.0, 0.0, 10.0], late_irs=late)
    with pytest.raises(TypeError):
        ohs.SessionRenderer.stereo_from_sofa(2, None, [0.0], no_such_option=1)

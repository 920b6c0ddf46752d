"""Object distance with air absorption (libohs_delay2.so, include/ohs_delay2.h), the part that needs no GPU.

* tests/delay2_model.py, the header's arithmetic in numpy, against mathematics: a static filtered call on a sine leaves at H(w) computed
  from the taps, inside the cubic-Lagrange bound and a derived f32 allowance; with identity taps, and with none, it has
  tests/delay_model.py's bits;
* csrc/delay2_body.hpp compiled for the host (tests/delay2_host_check.cpp), plain and as a stand-alone program under the address and
  undefined-behaviour sanitizers, has the model's bits on every case tests/test_gpu_delay2.py compares, chooses the model's pass and
  form for every tile and finds every input inside the window it promises;
* four mutants of the model are each caught by the checker the GPU test uses;
* air_absorption_taps: the identity at r = 0, a DC sum of 1 within a derived bound, monotone in r, the f^2 law, the saturation;
* the header's names, csrc/delay2_exports.map, DELAY2_PROTOTYPES and the library's dynamic symbols are one list of ten; every entry
  refuses NULL; k_object_delay2 was built without scratch at k_object_delay's occupancy; DELAY2_UNITS shares no unit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import delay2_model as m2
from tests import delay_model as dm
from tests.test_cpu_delay import _cxx
from tests.test_cpu_scene import _dynamic_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "open_headstage_amd")
U = 2.0 ** -24          # the unit roundoff of f32


# ---- 1. the model against mathematics -------------------------------------------------------------------------------------------------
# The f32 side of a filtered sample, to first order in U, for |x| <= A and T = |h_0| + 2 sum |h_r| (the rows are static, so h_r is H_r
# exactly).  A node v: the input is A sin() rounded to f32, 1 U; a pair x[t-r] + x[t+r] rounds, 1 U of at most 2 A; its product with
# h_r rounds, 1 U -- three roundings of terms that T A bounds in sum, 3 T A U; the four additions each round a partial sum that T A
# bounds, 4 T A U: 7 T A U per node.  The interpolation is tests/test_cpu_delay.py's count with T A in A's place -- twelve roundings
# of terms bounded by T A sum|c_k|, sum|c_k| <= 5/4: 15 T A U, there taken as 16 -- and carries the four nodes' own errors under the
# weights, 5/4 * 7 T A U = 8.75 T A U.  16 + 8.75, taken as 25.
def _f32_allowance(A, T):
    return 25.0 * T * A * U


@pytest.mark.parametrize("A", [1.0, 0.01, 250.0])
def test_a_static_filtered_call_leaves_a_sine_at_the_taps_response(A):
    import open_headstage_amd as ohs
    N, max_delay = 4 * m2.BLOCK, 600
    delays = np.array([5.0, 37.0, 37.5, 100.9375, 599.5, 12.0625])
    taps = np.concatenate([ohs.air_absorption_taps(np.array([3.0, 30.0, 200.0])), m2.random_taps((3,), 5)])
    n = np.arange(N, dtype=np.float64)
    worst_rel = 0.0
    for w in (2.0 * np.pi / 32.0, 2.0 * np.pi / 7.0):
        x = np.broadcast_to((A * np.sin(w * n)).astype(np.float32), (1, len(delays), N))
        y = m2.Delay2Model(1, len(delays), max_delay).process(x, delays[None, :], 4, fir=taps[None], carry=False)
        for c, d in enumerate(delays):
            h = taps[c].astype(np.float64)
            Hw = h[0] + 2.0 * sum(h[r] * np.cos(r * w) for r in range(1, m2.TAPS))       # real: the filter is symmetric
            assert abs(Hw) == m2.response(taps[c], w)
            T = abs(h[0]) + 2.0 * np.abs(h[1:]).sum()
            live = n >= d + 2 + m2.R                                                      # every input lies inside the signal
            err = np.abs(y[0, c].astype(np.float64) - Hw * A * np.sin(w * (n - d)))[live].max()
            bound = abs(Hw) * A * w ** 4 * (9.0 / 16.0) / 24.0 if d != np.floor(d) else 0.0     # the cubic's, on the filtered sine
            print(f"A = {A}, w = {w:.3f}, delay {d}, H = {Hw:+.4f}: worst error {err:.3e}, bound {bound:.3e} + {_f32_allowance(A, T):.1e}")
            assert err <= bound + _f32_allowance(A, T), (w, d, err, bound)
            worst_rel = max(worst_rel, abs(1.0 - abs(Hw)))
    assert worst_rel > 0.5          # the filters are not the identity: leaving the taps out would miss by half the amplitude


def test_identity_taps_and_no_taps_have_delay_models_bits():
    # no taps: every case of delay_model, its form counts too (the history is longer, nothing else differs)
    for name, case in dm.all_cases().items():
        want_trace = []
        want = dm.run_model(case, trace=want_trace)
        m = m2.Delay2Model(case["S"], case["Kmax"], case["max_delay"])
        for n, c in enumerate(case["calls"]):
            dm.check_bits(m.process(c["x"], c["delay"], case["seg_blocks"], c["gains"], None, c["carry"]), want[n], f"{name}, call {n}")
            assert m.last_launch == want_trace[n]["forms"] + (0,)
            assert m2.is_identity(m.carried[2]).all() and np.array_equal(m.carried[0], c["delay"].reshape(case["S"], -1, c["x"].shape[1])[:, -1])
    # identity taps: the cases whose delays a filtered call takes -- NaN, infinities and subnormals among them
    case = dm.special_case()
    want = dm.run_model(case)
    m = m2.Delay2Model(case["S"], case["Kmax"], case["max_delay"])
    for n, c in enumerate(case["calls"]):
        assert (c["delay"] >= m2.MIN_FILTERED).all()
        fir = np.broadcast_to(m2.IDENTITY, c["delay"].shape + (m2.TAPS,))
        dm.check_bits(m.process(c["x"], c["delay"], case["seg_blocks"], c["gains"], fir, c["carry"]), want[n], f"call {n}, identity taps")
        assert m.last_launch[2] == 0
    # -0 among the taps is not the identity
    h = m2.IDENTITY.copy()
    h[3] = -0.0
    assert not m2.is_identity(h) and m2.is_identity(m2.IDENTITY)


# ---- 2. delay2_body.hpp on the host ----------------------------------------------------------------------------------------------------
def _compile(exe, extra=()):
    return subprocess.run([_cxx(), "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-I", os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tests", "delay2_host_check.cpp"), "-o", exe], capture_output=True, text=True)


@pytest.fixture(scope="module")
def traced_calls():
    """every call of every case the GPU test compares, as the model ran it; an unfiltered call; the clamp probe no call reaches"""
    out = []
    for name, case in m2.all_cases().items():
        trace = []
        m2.run_model(case, trace=trace)
        out += [(f"{name}, call {i}", t) for i, t in enumerate(trace)]
    trace = []
    special = dm.special_case()
    m = m2.Delay2Model(special["S"], special["Kmax"], special["max_delay"])
    m.trace = trace
    for c in special["calls"]:
        m.process(c["x"], c["delay"], special["seg_blocks"], c["gains"], None, c["carry"])
    out += [(f"no taps, call {i}", t) for i, t in enumerate(trace)]
    probe = m2.clamp_probe()
    probe["y"], probe["forms"] = m2.run_core(probe)
    return out + [("clamp probe", probe)]


def _run(exe, calls, tmp_path, env=None):
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.uint64(len(calls)).tobytes())
        for _, t in calls:
            S, K, total = t["ext"].shape
            H = int(t["max_delay"]) + 2 + m2.R
            filtered = t["row_h"] is not None
            f.write(np.array([S, K, total - H, H, t["seg_frames"], t["row_d"].shape[1], int(filtered)], np.uint64).tobytes())
            f.write(np.float64(t["max_delay"]).tobytes())
            arrays = [(t["front_d"], np.float64), (t["row_d"], np.float64), (t["front_g"], np.float32), (t["row_g"], np.float32)]
            if filtered:
                arrays += [(t["front_h"], np.float32), (t["row_h"], np.float32)]
            for a, dt in arrays + [(t["ext"], np.float32)]:
                f.write(np.ascontiguousarray(a, dt).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(tmp_path / "out.bin", "rb").read()
    at = 0
    for name, t in calls:
        y = np.frombuffer(raw, np.float32, t["y"].size, at).reshape(t["y"].shape)
        at += 4 * t["y"].size
        lds, gather, filtered, outside = (int(v) for v in np.frombuffer(raw, np.uint64, 4, at))
        at += 32
        m2.check_bits(y, t["y"], name)
        assert (lds, gather, filtered) == t["forms"] and outside == 0, (name, lds, gather, filtered, outside, t["forms"])
    assert at == len(raw)


def test_delay2_body_on_the_host(tmp_path, traced_calls):
    exe = str(tmp_path / "delay2_host_check")
    r = _compile(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    _run(exe, traced_calls, tmp_path)
    assert len(traced_calls) == 3 + 2 + 2 + 2 * (1 + 3) + 1 + 2 + 1
    forms = np.array([t["forms"] for _, t in traced_calls])
    assert forms[:, 0].sum() > 0 and forms[:, 1].sum() > 0 and 0 < forms[:, 2].sum() < forms[:, :2].sum()       # both forms, both passes


def test_the_host_program_under_the_sanitizers(tmp_path, traced_calls):
    """the same program built with -fsanitize=address,undefined.  A stand-alone program: nothing is preloaded and Python loads none of
    it.  Skips where the sanitizers' runtime is not installed."""
    exe = str(tmp_path / "delay2_host_check_san")
    r = _compile(exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))
    if r.returncode != 0:
        pytest.skip("the address / undefined-behaviour sanitizers' runtime is not installed: " + r.stderr.strip()[-200:])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    _run(exe, traced_calls, tmp_path, env=env)


# ---- 3. mutants --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_outputs():
    cases = m2.all_cases()
    return cases, {name: m2.run_model(case) for name, case in cases.items()}


@pytest.mark.parametrize("mutant,caught_by", [("taps_asymmetric", "base, seg_blocks 1"), ("h_at_j_over_L", "base, seg_blocks 2"),
                                              ("ring_one_short", "ring of 13")])
def test_the_checker_catches_a_mutant(model_outputs, mutant, caught_by):
    """the GPU test's checker (delay_model.check_bits) on the GPU test's cases, a wrong model in the device's place"""
    cases, want = model_outputs
    got = m2.run_model(cases[caught_by], mutant)
    with pytest.raises(AssertionError, match="differ from the model's bits"):
        for g, w in zip(got, want[caught_by]):
            m2.check_bits(g, w, caught_by)
    caught = [name for name, case in cases.items() if any(len(m2.mismatches(g, w)) for g, w in zip(m2.run_model(case, mutant), want[name]))]
    print(f"{mutant}: caught by {caught}")
    assert caught_by in caught


def test_the_clamp_left_at_1_is_caught_where_it_can_be():
    """Between two delays of at least 5 the rounded ramp never falls below 5 (rounding is monotone: D' + (D - D') a >= D' + (5 - D') = 5
    going down, >= D' going up), and a filtered call refuses every other row and carry: no call reaches the clamp.  It is held at core()
    -- and through the probe's trace at the host build of delay2_body.hpp -- on rows the call would refuse."""
    probe = m2.clamp_probe()
    want, forms = m2.run_core(probe)
    with pytest.raises(AssertionError, match="differ from the model's bits"):
        m2.check_bits(m2.run_core(probe, "clamp_at_1")[0], want, "clamp probe")
    cases = m2.all_cases()
    for name, case in cases.items():        # ... and on the cases a call takes the mutant is the model
        for g, w in zip(m2.run_model(case, "clamp_at_1"), m2.run_model(case)):
            m2.check_bits(g, w, name)


def test_the_chained_calls_are_the_one_call_in_the_model(model_outputs):
    cases, want = model_outputs
    for max_delay in (600, 4090):
        whole, cut = want[f"one call, max_delay {max_delay}"], want[f"chained, max_delay {max_delay}"]
        m2.check_bits(np.concatenate(cut, axis=2), whole[0], f"max_delay {max_delay}")
    # the window edge: object 0's widest window is LDS_WINDOW frames and staged, object 1's one frame wider and gathered
    d = cases["window edge"]["calls"][0]["delay"]
    spread = m2.LDS_WINDOW - (m2.TILE + 3 + 2 * m2.R)
    assert m2.tile_spread(5.0, d[0, 1, 0]) == spread and m2.tile_spread(5.0, d[0, 1, 1]) == spread + 1
    trace = []
    m2.run_model(cases["window edge"], trace=trace)
    lds, gather, filtered = trace[0]["forms"]
    assert lds + gather == filtered == 8 and 1 <= gather <= 2
    one = dict(cases["window edge"], Kmax=1, calls=[{k: (v[:, :1] if k == "x" else v[..., :1] if k == "delay" else v[:, :, :1] if k == "fir" else v)
                                                     for k, v in cases["window edge"]["calls"][0].items()}])
    trace = []
    m2.run_model(one, trace=trace)
    assert trace[0]["forms"] == (4, 0, 4)
    # the ring of 13: the infinity at the far end under a weight of 0
    edge = want["ring of 13"]
    assert np.isnan(edge[1][0, 1, 0]) and np.isfinite(edge[1][0, 1, 1:]).all() and np.isfinite(edge[1][0, 0]).all()
    # mixed passes: 2 streams x (object 0: segments 2, 3; object 1: segments 0, 1, 3) x 2 tiles; then object 1's first segment by the carry
    trace = []
    m2.run_model(cases["mixed passes"], trace=trace)
    assert [t["forms"][2] for t in trace] == [2 * 5 * 2, 2 * 1 * 2]


# ---- 4. air_absorption_taps ------------------------------------------------------------------------------------------------------------
def test_air_absorption_taps():
    import open_headstage_amd as ohs
    fs, k = 48000.0, 1.6e-9
    r = np.array([0.0, 0.5, 1.0, 3.0, 10.0, 30.0, 60.0, 92.0, 93.5, 150.0, 1000.0])
    h = ohs.air_absorption_taps(r)
    assert h.dtype == np.float32 and h.shape == (len(r), 5)
    assert h[0].tobytes() == m2.IDENTITY.tobytes() and m2.is_identity(h[0]) and not m2.is_identity(h[1:]).any()
    assert ohs.air_absorption_taps(np.zeros((2, 3, 4))).shape == (2, 3, 4, 5) and m2.is_identity(ohs.air_absorption_taps(np.zeros((2, 3)))).all()
    # symmetry: the nine taps are the five mirrored, which is what the kernel applies; they agree with the four-fold convolution in
    # either order of its two sides
    for i, ri in enumerate(r):
        b = min(0.25, ri * k * (np.log(10.0) / 20.0) * fs ** 2 / (16.0 * np.pi ** 2))
        full = np.array([1.0])
        for _ in range(4):
            full = np.convolve(full, [b, 1.0 - 2.0 * b, b])
        assert np.allclose(full, full[::-1], rtol=0, atol=2.0 ** -50)
        assert np.abs(h[i].astype(np.float64) - full[4:]).max() <= U * full[4] + 2.0 ** -50, (ri, h[i], full[4:])
        # DC: the exact taps sum to 1 (each factor does: b + (1 - 2b) + b); every tap is rounded to f32 once, at most U of itself, and
        # they are positive, so the nine rounded taps sum to 1 within U * 1, beside the f64 sums' own 2^-50
        assert abs((h[i, 0].astype(np.float64) + 2.0 * h[i, 1:].astype(np.float64).sum()) - 1.0) <= U + 2.0 ** -50, ri
        assert (h[i] >= 0).all()
    # monotone in r at every frequency, up to the saturation at b = 1/4 near 93 m, constant behind it
    for f in (1000.0, 5000.0, 10000.0, 20000.0, 24000.0):
        mag = np.array([m2.response(hi, 2.0 * np.pi * f / fs) for hi in h])
        assert (np.diff(mag) <= 4.0 * U).all(), (f, mag)
        assert mag[0] == 1.0 and mag[7] < mag[1]
    assert np.array_equal(h[8], h[9]) and np.array_equal(h[9], h[10]) and not np.array_equal(h[7], h[8])
    assert np.array_equal(h[10], (np.array([70.0, 56.0, 28.0, 8.0, 1.0]) / 256.0).astype(np.float32))
    sat = 0.25 * 16.0 * np.pi ** 2 / (k * (np.log(10.0) / 20.0) * fs ** 2)
    assert 92.5 < sat < 93.5
    # the law: -k f^2 r dB, within 0.2 dB at 10 kHz for 10 m; about 0.16 dB/m there
    db = 20.0 * np.log10(m2.response(h[4], 2.0 * np.pi * 10000.0 / fs))
    assert abs(db - (-k * 1e8 * 10.0)) <= 0.2 and abs(k * 1e8 - 0.16) < 1e-12, db
    for bad in (np.array([-1.0]), np.array([np.nan]), np.array([np.inf])):
        with pytest.raises(ValueError):
            ohs.air_absorption_taps(bad)


# ---- 5. the surface ----------------------------------------------------------------------------------------------------------------
ENTRIES = ["ohs_delay2_carried", "ohs_delay2_create", "ohs_delay2_destroy", "ohs_delay2_last_error", "ohs_delay2_last_launch",
           "ohs_delay2_process", "ohs_delay2_process_filtered", "ohs_delay2_reset", "ohs_delay2_status_string", "ohs_delay2_sync"]


def test_header_map_prototypes_and_library_are_one_list_of_ten():
    import open_headstage_amd as ohs
    from open_headstage_amd import delay2
    hdr = open(os.path.join(ROOT, "include", "ohs_delay2.h")).read()
    declared = sorted(set(re.findall(r"\b(ohs_delay2_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == ENTRIES == sorted(delay2.DELAY2_PROTOTYPES) and len(declared) == 10
    lib = os.path.join(PKG, "libohs_delay2.so")
    assert declared == _dynamic_symbols(lib)
    emap = open(os.path.join(PKG, "csrc", "delay2_exports.map")).read()
    assert "global: ohs_delay2_*;" in emap and "local: *;" in emap
    undefined = subprocess.run(["nm", "-D", "--undefined-only", lib], check=True, capture_output=True, text=True).stdout
    assert "ohs" not in undefined
    doc = open(os.path.join(ROOT, "SCENES.md")).read()
    for name in declared:
        assert re.search(r"\bfn " + name + r"\(", doc), f"{name} is not listed in SCENES.md"
    for name in ("FilteredObjectDelay", "FilteredObjectDelayError", "air_absorption_taps", "render_with_distance_air"):
        assert hasattr(ohs, name) and hasattr(delay2, name), name
    for name in ("process", "process_ptr", "reset", "last_launch", "carried", "sync"):
        assert callable(getattr(ohs.FilteredObjectDelay, name)) and callable(getattr(ohs.ObjectDelay, name)), name
    # the model's constants are the library's
    internal = open(os.path.join(PKG, "csrc", "delay2_internal.h")).read()
    body = open(os.path.join(PKG, "csrc", "delay2_body.hpp")).read()
    assert re.search(r"DELAY2_TILE = (\d+);", internal).group(1) == str(m2.TILE)
    assert re.search(r"DELAY2_LDS_WINDOW = (\d+);", internal).group(1) == str(m2.LDS_WINDOW)
    assert re.search(r"DELAY2_RADIUS = (\d+);", body).group(1) == re.search(r"OHS_DELAY2_FIR_RADIUS\s+(\d+)", hdr).group(1) == str(m2.R)
    assert delay2.FIR_RADIUS == m2.R and np.array_equal(delay2.IDENTITY_TAPS, m2.IDENTITY)
    assert '#include "delay_body.hpp"' in body


def test_every_entry_refuses_null():
    from open_headstage_amd import _ffi, delay2
    L = delay2.delay2_lib()
    INV = _ffi.OHS_ERR_INVALID_ARG
    assert L.ohs_delay2_create(0, 1, 1, 1, None) == INV and b"out is NULL" in L.ohs_delay2_last_error()
    h = C.c_void_p()
    for args, text in (((0, 0, 1, 1), b"n_streams 0"), ((0, 65536, 1, 1), b"n_streams 65536"), ((0, 1, 0, 1), b"max_objects 0"),
                       ((0, 1, 65, 1), b"max_objects 65"), ((0, 1, 1, 0), b"max_delay 0"), ((0, 1, 1, 65537), b"max_delay 65537")):
        assert L.ohs_delay2_create(*args, C.byref(h)) == INV and not h.value and text in L.ohs_delay2_last_error(), args
    L.ohs_delay2_destroy(None)
    assert L.ohs_delay2_process(None, None, None, 1, 0, 0, 0, 0, 1, 1, None, None, 0, 0, None) == INV and b"NULL" in L.ohs_delay2_last_error()
    assert L.ohs_delay2_process_filtered(None, None, None, 1, 0, 0, 0, 0, 1, 1, None, None, None, 0, 0, None) == INV
    assert b"NULL" in L.ohs_delay2_last_error()
    assert L.ohs_delay2_reset(None) == INV and b"NULL" in L.ohs_delay2_last_error()
    assert L.ohs_delay2_sync(None, None) == INV
    assert L.ohs_delay2_last_launch(None, None, None, None, None, None) == INV
    assert L.ohs_delay2_carried(None, None, None, None, None) == INV
    for s in (0, 1, 2, 3, 6, 99):
        assert L.ohs_delay2_status_string(s) == _ffi.lib().ohs_status_string(s), s


def test_kernel_resources_and_the_build():
    from open_headstage_amd import build
    res = build.resources()
    for name in ("k_object_delay2", "k_delay2_history"):
        assert res[name]["scratch_bytes_per_lane"] == 0 and res[name]["agprs"] == 0, (name, res[name])
    # the window of 2 048 frames is the kernel's only LDS; no fewer waves per SIMD than the unfiltered stage's kernel
    assert res["k_object_delay2"]["lds_bytes"] == 4 * m2.LDS_WINDOW
    assert res["k_object_delay2"]["occupancy_waves_per_simd"] >= res["k_object_delay"]["occupancy_waves_per_simd"] == 8
    assert res["k_object_delay2"]["vgprs"] <= 64
    assert res["k_delay2_history"]["lds_bytes"] == 0 and res["k_delay2_history"]["occupancy_waves_per_simd"] == 8
    for f in ("delay2_kernels.hip", "api_delay2.hip", "delay2_body.hpp", "delay2_internal.h"):
        assert "asm" not in open(os.path.join(PKG, "csrc", f)).read(), f
    assert build.is_current() and os.path.exists(build.DELAY2_LIB)
    assert os.path.basename(build.DELAY2_LIB) == "libohs_delay2.so" and len(build.DELAY2_UNITS) == 2
    assert all("-ffp-contract=off" in flags for _, flags in build.DELAY2_UNITS)
    others = (build.LOOKUP_UNITS + build.LOOKUP3_UNITS + build.LOOKUP3P_UNITS + build.TRACKED_UNITS + build.DELAY_UNITS + build._units() +
              [build.SCENE_UNIT, build.SCENE2_UNIT, build.SCENE3_UNIT])
    assert not {u for u, _ in build.DELAY2_UNITS} & {u for u, _ in others}
    assert len(build._all_units()) == len(others) + 2
    deps = {os.path.basename(d) for d in build._deps("delay2_kernels.hip")}
    assert {"delay2_body.hpp", "delay2_internal.h", "delay_body.hpp", "ohs_delay2.h", "delay2_exports.map"} <= deps
    assert not {"delay_internal.h", "ohs_delay.h"} & deps
    for unit in ("api_core.hip", "api_tracked.hip", "delay_kernels.hip", "api_delay.hip"):      # the older units depend on none of the new files
        assert not {"delay2_body.hpp", "delay2_internal.h", "ohs_delay2.h"} & {os.path.basename(d) for d in build._deps(unit)}
    # ten libraries beside each other
    libs = [build.LIB, build.SCENE_LIB, build.SCENE2_LIB, build.SCENE3_LIB, build.LOOKUP_LIB, build.LOOKUP3_LIB, build.LOOKUP3P_LIB,
            build.TRACKED_LIB, build.DELAY_LIB, build.DELAY2_LIB]
    assert len(set(libs)) == 10 and all(os.path.exists(p) for p in libs)

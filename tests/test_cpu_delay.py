"""Object distance (libohs_delay.so, include/ohs_delay.h), the part that needs no GPU.

* tests/delay_model.py, the header's arithmetic in numpy, against mathematics: the cubic-Lagrange bound on a sine, and Doppler;
* csrc/delay_body.hpp compiled for the host (tests/delay_host_check.cpp), plain and under the address and undefined-behaviour
  sanitizers, has the model's bits on every case tests/test_gpu_delay.py compares, chooses the model's form for every tile and finds
  every tap inside the window it promises;
* the header's names, csrc/delay_exports.map, DELAY_PROTOTYPES and the library's dynamic symbols are one list of nine; every entry
  refuses NULL; k_object_delay was built without scratch;
* distance_rows' shapes and clamps;
* four mutants of the model are each caught by the checker the GPU test uses, on the GPU test's cases."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import delay_model as dm
from tests.test_cpu_scene import _dynamic_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "open_headstage_amd")
U = 2.0 ** -24          # the unit roundoff of f32


# ---- 1. the model against mathematics -------------------------------------------------------------------------------------------------
def _sine(A, w, n):
    return (A * np.sin(w * n)).astype(np.float32)


# The f32 side of a sample, to first order in U, for |x| <= A: a weight is three differences of f (one rounding each; f itself is
# exact here and f - 1, f - 2, f + 1 of a multiple of 2^-4 are too, but the allowance does not lean on that) and three products, at
# most 6 U relative; the input sample is A sin() rounded to f32, 1 U; each of the four products rounds, 1 U; the three sums round,
# at most 3 U of a partial sum that the sum of |c_k| |x| bounds; the gain's product, 1 U.  Twelve roundings of terms bounded by
# A * sum|c_k|, and sum|c_k| <= 5/4 on [0, 1] (its value at f = 1/2: 1/16 + 9/16 + 9/16 + 1/16): 12 * 5/4 = 15, taken as 16.
def _f32_allowance(A):
    return 16.0 * A * U


@pytest.mark.parametrize("A", [1.0, 0.01, 250.0])
def test_the_interpolation_stays_inside_the_cubic_lagrange_bound(A):
    w, N, max_delay = 2.0 * np.pi / 32.0, 4 * dm.BLOCK, 600
    fracs = np.array([1.0, 7.5, 7.25, 33.125, 100.9375, 12.0625, 599.5, 3.5])
    x = np.broadcast_to(_sine(A, w, np.arange(N, dtype=np.float64)), (1, len(fracs), N))
    m = dm.DelayModel(1, len(fracs), max_delay)
    y = m.process(x, fracs[None, :], 4, carry=False)
    n = np.arange(N, dtype=np.float64)
    bound = A * w ** 4 * (9.0 / 16.0) / 24.0        # |f''''| / 4! * max over [0, 1] of |(t + 1) t (t - 1) (t - 2)| = 9/16 at t = 1/2
    worst = 0.0
    for c, d in enumerate(fracs):
        live = n >= d + 2                           # every tap lies inside the signal
        err = np.abs(y[0, c].astype(np.float64) - A * np.sin(w * (n - d)))[live].max()
        print(f"A = {A}, delay {d}: worst error {err:.3e}, bound {bound:.3e} + {_f32_allowance(A):.1e}")
        assert err <= bound + _f32_allowance(A), (d, err, bound)
        worst = max(worst, err)
        if d == np.floor(d):
            assert err <= _f32_allowance(A)         # a whole delay interpolates nothing
    assert worst >= 0.9 * bound                     # the bound is the interpolator's own: the half-sample delays come close to it


def _phase_fit(y, w, n):
    """least squares of y on sin(w n), cos(w n) -> (amplitude, phase, worst residual)"""
    B = np.stack([np.sin(w * n), np.cos(w * n)], 1)
    (p, q), *_ = np.linalg.lstsq(B, y, rcond=None)
    return np.hypot(p, q), np.arctan2(q, p), np.abs(B @ np.array([p, q]) - y).max()


def test_a_ramp_shifts_the_sine_to_w_times_one_minus_delta_over_L():
    A, w, L, max_delay = 1.0, 2.0 * np.pi / 32.0, 8 * dm.BLOCK, 600
    bound = A * w ** 4 * (9.0 / 16.0) / 24.0 + _f32_allowance(A)
    n = np.arange(L, dtype=np.float64)
    x = _sine(A, w, n)[None, None]
    for D0, D1 in ((50.0, 250.0), (420.0, 60.5)):
        delta = D1 - D0
        m = dm.DelayModel(1, 1, max_delay)
        m.process(np.zeros((1, 1, dm.BLOCK), np.float32), np.array([[D0]]), 1, carry=False)       # (D0 stands in front of the ramp)
        y = m.process(x, np.array([[D1]]), 8, carry=True)[0, 0].astype(np.float64)
        live = n >= max(D0, D1) + 2
        w_out = w * (1.0 - delta / L)
        # one sine at w (1 - delta / L) over the whole segment, up to the interpolator's error ...
        amp, ph, res = _phase_fit(y[live], w_out, n[live])
        assert res <= 2.0 * bound and abs(amp - A) <= 2.0 * bound, (res, amp)
        # ... with the phase the ramp's start gives it: d(n) = D0 + delta (n + 1) / L
        want = -w * (D0 + delta / L)
        assert abs(np.angle(np.exp(1j * (ph - want)))) <= 2.0 * bound / A, (ph, want)
        # the two halves fitted apart agree in phase: a frequency off by 1e-7 rad per frame would part them by 2e-4
        half = len(n) // 2
        first, second = live & (n < half), live & (n >= half)
        p1, p2 = _phase_fit(y[first], w_out, n[first])[1], _phase_fit(y[second], w_out, n[second])[1]
        assert abs(np.angle(np.exp(1j * (p1 - p2)))) <= 4.0 * bound / A, (p1, p2)
        # and the input's own frequency does not fit
        assert _phase_fit(y[live], w, n[live])[2] > 0.5 * A
        print(f"ramp {D0} -> {D1} over {L}: w_out / w = {w_out / w:.6f}, residual {res:.2e}, phase error {abs(np.angle(np.exp(1j * (ph - want)))):.2e}")


# ---- 2. delay_body.hpp on the host -----------------------------------------------------------------------------------------------------
def _cxx():
    from open_headstage_amd import build
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc()))), "llvm", "bin", "clang++")
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx, "no host C++ compiler"
    return cxx


def _compile(exe, extra=()):
    return subprocess.run([_cxx(), "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-I", os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tests", "delay_host_check.cpp"), "-o", exe], capture_output=True, text=True)


@pytest.fixture(scope="module")
def traced_calls():
    """every call of every case the GPU test compares, as the model ran it: (name, what core() was given and gave)"""
    out = []
    for name, case in dm.all_cases().items():
        trace = []
        dm.run_model(case, trace=trace)
        out += [(f"{name}, call {i}", case["max_delay"], t) for i, t in enumerate(trace)]
    return out


def _run(exe, calls, tmp_path, env=None):
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.uint64(len(calls)).tobytes())
        for _, max_delay, t in calls:
            S, K, total = t["ext"].shape
            H = max_delay + 2
            f.write(np.array([S, K, total - H, H, t["seg_frames"], t["row_d"].shape[1]], np.uint64).tobytes() + np.float64(max_delay).tobytes())
            for a, dt in ((t["front_d"], np.float64), (t["row_d"], np.float64), (t["front_g"], np.float32), (t["row_g"], np.float32),
                          (t["ext"], np.float32)):
                f.write(np.ascontiguousarray(a, dt).tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(tmp_path / "out.bin", "rb").read()
    at = 0
    for name, _, t in calls:
        y = np.frombuffer(raw, np.float32, t["y"].size, at).reshape(t["y"].shape)
        at += 4 * t["y"].size
        lds, gather, outside = (int(v) for v in np.frombuffer(raw, np.uint64, 3, at))
        at += 24
        dm.check_bits(y, t["y"], name)
        assert (lds, gather) == t["forms"] and outside == 0, (name, lds, gather, outside, t["forms"])
    assert at == len(raw)


def test_delay_body_on_the_host(tmp_path, traced_calls):
    exe = str(tmp_path / "delay_host_check")
    r = _compile(exe)
    assert r.returncode == 0, r.stderr[-2000:]
    _run(exe, traced_calls, tmp_path)
    assert len(traced_calls) == 3 + 2 + 2 * (1 + 3) + 2
    forms = np.array([t["forms"] for _, _, t in traced_calls])
    assert forms[:, 0].sum() > 0 and forms[:, 1].sum() > 0          # both forms are among the cases


def test_the_host_program_under_the_sanitizers(tmp_path, traced_calls):
    """the same program built with -fsanitize=address,undefined.  A stand-alone program: nothing is preloaded and Python loads none of
    it.  Skips where the sanitizers' runtime is not installed."""
    exe = str(tmp_path / "delay_host_check_san")
    r = _compile(exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))
    if r.returncode != 0:
        pytest.skip("the address / undefined-behaviour sanitizers' runtime is not installed: " + r.stderr.strip()[-200:])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    _run(exe, traced_calls, tmp_path, env=env)


# ---- 3. the surface ----------------------------------------------------------------------------------------------------------------
ENTRIES = ["ohs_delay_carried", "ohs_delay_create", "ohs_delay_destroy", "ohs_delay_last_error", "ohs_delay_last_launch", "ohs_delay_process",
           "ohs_delay_reset", "ohs_delay_status_string", "ohs_delay_sync"]


def test_header_map_prototypes_and_library_are_one_list_of_nine():
    import open_headstage_amd as ohs
    from open_headstage_amd import delay
    hdr = open(os.path.join(ROOT, "include", "ohs_delay.h")).read()
    declared = sorted(set(re.findall(r"\b(ohs_delay_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == ENTRIES == sorted(delay.DELAY_PROTOTYPES) and len(declared) == 9
    lib = os.path.join(PKG, "libohs_delay.so")
    assert declared == _dynamic_symbols(lib)
    emap = open(os.path.join(PKG, "csrc", "delay_exports.map")).read()
    assert "global: ohs_delay_*;" in emap and "local: *;" in emap
    undefined = subprocess.run(["nm", "-D", "--undefined-only", lib], check=True, capture_output=True, text=True).stdout
    assert "ohs" not in undefined
    doc = open(os.path.join(ROOT, "SCENES.md")).read()
    for name in declared:
        assert re.search(r"\bfn " + name + r"\(", doc), f"{name} is not listed in SCENES.md"
    for name in ("ObjectDelay", "ObjectDelayError", "distance_rows", "render_with_distance"):
        assert name in ohs.__all__ and hasattr(ohs, name), name
    for name in ("process", "process_ptr", "reset", "last_launch", "carried", "sync"):
        assert callable(getattr(ohs.ObjectDelay, name)), name
    # the model's constants are the library's
    internal = open(os.path.join(PKG, "csrc", "delay_internal.h")).read()
    assert re.search(r"DELAY_TILE = (\d+);", internal).group(1) == str(dm.TILE)
    assert re.search(r"DELAY_LDS_WINDOW = (\d+);", internal).group(1) == str(dm.LDS_WINDOW)


def test_every_entry_refuses_null():
    from open_headstage_amd import _ffi, delay
    L = delay.delay_lib()
    INV = _ffi.OHS_ERR_INVALID_ARG
    assert L.ohs_delay_create(0, 1, 1, 1, None) == INV and b"out is NULL" in L.ohs_delay_last_error()
    h = C.c_void_p()
    for args, text in (((0, 0, 1, 1), b"n_streams 0"), ((0, 65536, 1, 1), b"n_streams 65536"), ((0, 1, 0, 1), b"max_objects 0"),
                       ((0, 1, 65, 1), b"max_objects 65"), ((0, 1, 1, 0), b"max_delay 0"), ((0, 1, 1, 65537), b"max_delay 65537")):
        assert L.ohs_delay_create(*args, C.byref(h)) == INV and not h.value and text in L.ohs_delay_last_error(), args
    L.ohs_delay_destroy(None)
    assert L.ohs_delay_process(None, None, None, 1, 0, 0, 0, 0, 1, 1, None, None, 0, 0, None) == INV and b"NULL" in L.ohs_delay_last_error()
    assert L.ohs_delay_reset(None) == INV and b"NULL" in L.ohs_delay_last_error()
    assert L.ohs_delay_sync(None, None) == INV
    assert L.ohs_delay_last_launch(None, None, None, None, None) == INV
    assert L.ohs_delay_carried(None, None, None, None) == INV
    for s in (0, 1, 2, 3, 6, 99):
        assert L.ohs_delay_status_string(s) == _ffi.lib().ohs_status_string(s), s


def test_kernel_resources():
    from open_headstage_amd import build
    res = build.resources()
    fields = ("vgprs", "agprs", "sgprs", "scratch_bytes_per_lane", "lds_bytes", "occupancy_waves_per_simd")
    for name in ("k_object_delay", "k_delay_history"):
        assert res[name]["scratch_bytes_per_lane"] == 0 and res[name]["agprs"] == 0, (name, res[name])
    # as built: the window of 2 048 frames is the kernel's only LDS, and eight waves per SIMD fit
    assert {f: res["k_object_delay"][f] for f in fields} == \
        {"vgprs": 30, "agprs": 0, "sgprs": 61, "scratch_bytes_per_lane": 0, "lds_bytes": 4 * dm.LDS_WINDOW, "occupancy_waves_per_simd": 8}
    assert res["k_delay_history"]["lds_bytes"] == 0 and res["k_delay_history"]["occupancy_waves_per_simd"] == 8
    for f in ("delay_kernels.hip", "api_delay.hip", "delay_body.hpp", "delay_internal.h"):
        assert "asm" not in open(os.path.join(PKG, "csrc", f)).read(), f
    assert build.is_current() and os.path.exists(build.DELAY_LIB)
    assert os.path.basename(build.DELAY_LIB) == "libohs_delay.so" and len(build.DELAY_UNITS) == 2
    assert all("-ffp-contract=off" in flags for _, flags in build.DELAY_UNITS)
    others = build.LOOKUP_UNITS + build.LOOKUP3_UNITS + build.LOOKUP3P_UNITS + build.TRACKED_UNITS + build._units()
    assert not {u for u, _ in build.DELAY_UNITS} & {u for u, _ in others}
    deps = {os.path.basename(d) for d in build._deps("delay_kernels.hip")}
    assert {"delay_body.hpp", "delay_internal.h", "ohs_delay.h", "delay_exports.map"} <= deps
    for unit in ("api_core.hip", "api_tracked.hip"):            # the older units depend on none of the new headers
        assert not {"delay_body.hpp", "delay_internal.h", "ohs_delay.h"} & {os.path.basename(d) for d in build._deps(unit)}


# ---- 4. distance_rows ------------------------------------------------------------------------------------------------------------
def test_distance_rows_shapes_and_clamps():
    import open_headstage_amd as ohs
    src = np.array([[3.0, 4.0, 0.0], [0.0, 0.0, 0.001], [0.0, 0.0, 0.003], [0.0, -343.0, 0.0]])
    d, g = ohs.distance_rows(src)
    assert d.dtype == np.float64 and g.dtype == np.float32 and d.shape == g.shape == (4,)
    assert d[0] == 5.0 * (48000.0 / 343.0) and g[0] == np.float32(1.0 / 5.0)
    assert d[1] == d[2] == 0.1 * (48000.0 / 343.0) and g[1] == g[2] == np.float32(1.0 / 0.1)        # r floored at min_m
    assert d[3] == 48000.0 and g[3] == np.float32(1.0 / 343.0)
    # the delay's own floor of one frame: min_m = 1 mm at 48 kHz is 0.14 frames
    d, g = ohs.distance_rows(src[1:3], min_m=0.001)
    assert d[0] == 1.0 and g[0] == np.float32(1.0 / 0.001) and d[1] == 1.0 and g[1] == np.float32(1.0 / 0.003)
    # r = sqrt((x^2 + y^2) + z^2) in f64, in that order
    v = np.random.default_rng(3).uniform(-30.0, 30.0, (5, 7, 3))
    d, g = ohs.distance_rows(v, fs=44100.0, c=340.0, ref_m=2.0)
    r = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    assert d.shape == g.shape == (5, 7) and np.array_equal(d, np.maximum(1.0, r * (44100.0 / 340.0))) and np.array_equal(g, (2.0 / r).astype(np.float32))
    # the listener moves the origin; every shape process_xyz takes
    d2, g2 = ohs.distance_rows(v + np.array([1.0, -2.0, 0.5]), fs=44100.0, c=340.0, ref_m=2.0, listener=[1.0, -2.0, 0.5])
    assert np.allclose(d2, d, rtol=1e-12) and np.allclose(g2, g, rtol=1e-6)
    assert ohs.distance_rows(np.zeros((2, 5, 7, 3)))[0].shape == (2, 5, 7)
    for bad in (np.zeros(3), np.zeros((4, 2)), np.zeros((1, 2, 3, 4, 3))):
        with pytest.raises(ValueError):
            ohs.distance_rows(bad)
    with pytest.raises(ValueError):
        ohs.distance_rows(src, min_m=0.0)


# ---- 5. mutants ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_outputs():
    cases = dm.all_cases()
    return cases, {name: dm.run_model(case) for name, case in cases.items()}


@pytest.mark.parametrize("mutant,caught_by", [("taps_reversed", "base, seg_blocks 1"), ("ramp_at_j_over_L", "base, seg_blocks 2"),
                                              ("history_one_short", "special values"), ("carry_from_last_d", "chained, max_delay 4096")])
def test_the_checker_catches_a_mutant(model_outputs, mutant, caught_by):
    """the GPU test's checker (delay_model.check_bits) on the GPU test's cases, a wrong model in the device's place"""
    cases, want = model_outputs
    got = dm.run_model(cases[caught_by], mutant)
    with pytest.raises(AssertionError, match="differ from the model's bits"):
        for g, w in zip(got, want[caught_by]):
            dm.check_bits(g, w, caught_by)
    caught = [name for name, case in cases.items() if any(len(dm.mismatches(g, w)) for g, w in zip(dm.run_model(case, mutant), want[name]))]
    print(f"{mutant}: caught by {caught}")
    assert caught_by in caught


def test_the_chained_calls_are_the_one_call_in_the_model(model_outputs):
    cases, want = model_outputs
    for max_delay in (600, 4096):
        whole, cut = want[f"one call, max_delay {max_delay}"], want[f"chained, max_delay {max_delay}"]
        dm.check_bits(np.concatenate(cut, axis=2), whole[0], f"max_delay {max_delay}")
    x, y = cases["base, seg_blocks 1"]["calls"][0]["x"], want["base, seg_blocks 1"][0]
    assert np.array_equal(y[0, 0, 1:], x[0, 0, :-1]) and y[0, 0, 0] == 0.0          # a delay of exactly 1 at gain 1: one frame late

"""Scheduled batch calls (ohs_batch_process_scheduled), the part that needs no GPU:

* the three entry points exist in the header, in the ctypes prototypes and in the library, and refuse a NULL handle;
* the boundary rule of the wave ring (csrc/eq_ring64_body.hpp, header comment), checked on the lane-level model
  tools/model_eq_wave_ring.py: 64 lanes, the six operations O T A P N M per step in float32, each product and sum rounded by
  itself.  In step t lane t - B - 1 takes its new (pb0, pb1, a1, a2) in front of A and lane t - B its new b2 in front of M,
  for a boundary at sample B.  The model's output bits must equal the oracle EQ's, refreshed with set_band_coeffs in front of
  every segment -- for 1 .. 12 bands, boundaries at multiples of 512 with B mod 48 = 0, 16 and 32, four tables, two launches
  (the state carried from one to the next)."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ohs_batch_set_schedule_tables", "ohs_batch_process_scheduled", "ohs_batch_last_eq_form")


def _model():
    spec = importlib.util.spec_from_file_location("model_eq_wave_ring", os.path.join(ROOT, "tools", "model_eq_wave_ring.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_entry_points_exist_and_refuse_a_null_handle():
    from open_headstage_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "ohs_hip.h")).read()
    declared = set(re.findall(r"\b(ohs_[a-z0-9_]+)\s*\(", hdr))
    L = _ffi.lib()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/ohs_hip.h"
        assert name in _ffi.PROTOTYPES, f"{name} has no ctypes prototype"
        assert hasattr(L, name), f"{name} is not exported"
    one = (C.c_float * 5)()
    flag = (C.c_uint8 * 1)()
    f, s = C.c_int(), C.c_int()
    assert L.ohs_batch_set_schedule_tables(None, 1, one, flag) == _ffi.OHS_ERR_INVALID_ARG
    assert L.ohs_batch_process_scheduled(None, None, None, 1, 1024, 512, 1, None, None, None) == _ffi.OHS_ERR_INVALID_ARG
    assert L.ohs_batch_last_eq_form(None, C.byref(f), C.byref(s)) == _ffi.OHS_ERR_INVALID_ARG


# boundaries of one launch of 3 072 samples; mod 48: 512 -> 32, 1024 -> 16, 1536 -> 0, 2560 -> 16
@pytest.mark.parametrize("boundaries", [[512, 1024, 1536, 2560], [1536], [512, 2048]], ids=lambda b: "B" + "_".join(map(str, b)))
@pytest.mark.parametrize("nb", list(range(1, 13)))
def test_model_boundary_rule_matches_the_oracle_refreshed_per_segment(oracle, nb, boundaries):
    m = _model()
    assert {b % 48 for b in [512, 1024, 1536]} == {0, 16, 32}
    assert m.check(nb, boundaries, 3072, n_tables=4, seed=len(boundaries))


def test_model_tells_a_boundary_that_is_one_step_off(oracle):
    """the check has teeth: the same tables switched one sample late are not what the oracle computes"""
    m = _model()
    rng = np.random.default_rng(3)
    tabs = m.random_tables(rng, 2, 10)
    x = rng.standard_normal(2048).astype(np.float32)
    y, _ = m.ring_eq(x, tabs, [(0, 0), (1024, 1)])
    right = m.oracle_eq(x, tabs, [(0, 0), (1024, 1)])
    late = m.oracle_eq(x, tabs, [(0, 0), (1025, 1)])
    assert np.array_equal(y.view(np.uint32), right.view(np.uint32))
    assert not np.array_equal(y.view(np.uint32), late.view(np.uint32))


def test_model_lane_constants_are_the_library_s_compaction():
    """lane l: (pb0, pb1) of the enabled band it is pre lane of, (b2, a1, a2) of the one it is post lane of, else (1, 0, 0, 0, 0)"""
    m = _model()
    t = np.arange(15, dtype=np.float32).reshape(3, 5) + 1
    pb0, pb1, b2, a1, a2 = m.lane_constants(t)
    assert list(pb0[:4]) == [1, 6, 11, 1] and list(pb1[:4]) == [2, 7, 12, 0]
    assert list(b2[:5]) == [0, 3, 8, 13, 0] and list(a1[:5]) == [0, 4, 9, 14, 0] and list(a2[:5]) == [0, 5, 10, 15, 0]

"""Per-stream scheduled batch calls (ohs_batch_process_scheduled_streams), the part that needs no GPU:

* the entry point exists in the header, in the ctypes prototypes and in the library, and refuses a NULL handle;
* the lane-level model (tools/model_eq_wave_ring.py) driven per chain: three chains with 10, 7 and 12 bands follow three
  different index rows, so their boundaries lie at different multiples of 512 (B mod 48 = 0, 16 and 32 all present); two
  launches with the state carried.  The bits must equal the oracle EQ's, refreshed in front of every segment per chain -- and
  a row shifted by one segment for one chain is told apart;
* the build's resource figures: k_eq_ring_sched_streams has no scratch and fits beside four k_conv_p1 waves on a SIMD."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ohs_batch_process_scheduled_streams"

ROWS1 = [[0, 1, 1, 2, 2, 2], [3, 3, 0, 0, 1, 2], [1, 2, 3, 0, 1, 2]]
ROWS2 = [[2, 2, 3, 3, 0, 0], [0, 1, 1, 1, 1, 3], [3, 2, 1, 0, 3, 2]]
BANDS = [10, 7, 12]


def _model():
    spec = importlib.util.spec_from_file_location("model_eq_wave_ring", os.path.join(ROOT, "tools", "model_eq_wave_ring.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_entry_point_exists_and_refuses_a_null_handle():
    from open_headstage_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "ohs_hip.h")).read()
    declared = set(re.findall(r"\b(ohs_[a-z0-9_]+)\s*\(", hdr))
    L = _ffi.lib()
    assert NAME in declared, f"{NAME} is not declared in include/ohs_hip.h"
    assert NAME in _ffi.PROTOTYPES, f"{NAME} has no ctypes prototype"
    assert hasattr(L, NAME), f"{NAME} is not exported"
    assert L.ohs_batch_process_scheduled_streams(None, None, None, 1, 1024, 512, 1, None, 0, None, 0, None) == _ffi.OHS_ERR_INVALID_ARG
    from open_headstage_amd.batch import BatchProcessor
    assert hasattr(BatchProcessor, "process_scheduled_streams") and hasattr(BatchProcessor, "process_scheduled_streams_ptr")


def test_rows_put_the_chains_boundaries_at_different_places():
    m = _model()
    bounds = [[b for b, _ in m.row_schedule(r, 512, 3072)[1:]] for r in ROWS1]
    assert bounds == [[512, 1536], [1024, 2048, 2560], [512, 1024, 1536, 2048, 2560]]      # consecutive equal indices: one run
    assert {b % 48 for bs in bounds for b in bs} == {0, 16, 32}
    assert len({tuple(b) for b in bounds}) == 3
    # a launch that starts inside a segment (the overlap's time chunks): 512 samples into segment 1 of 1 024-sample segments
    assert m.row_schedule([0, 1, 1, 2], 1024, 2048, seg0=1, off0=512) == [(0, 1), (1536, 2)]


def test_model_chains_on_their_own_rows_match_the_oracle_refreshed_per_segment(oracle):
    m = _model()
    assert m.check_streams(BANDS, ROWS1, ROWS2, seed=5)


def test_model_tells_a_row_shifted_by_one_segment_for_one_chain(oracle):
    """the check has teeth: chain 1 following its row one segment late is not what the oracle computes for it; the other
    chains, on their own rows, are untouched by it"""
    m = _model()
    rng = np.random.default_rng(9)
    pools = [m.random_tables(rng, 4, nb) for nb in BANDS]
    xs = [rng.standard_normal(3072).astype(np.float32) for _ in BANDS]
    late = [ROWS1[0], [ROWS1[1][0]] + ROWS1[1][:-1], ROWS1[2]]
    ys, _ = m.ring_eq_streams(xs, pools, late, 512)
    for c in range(3):
        ref = m.oracle_eq(xs[c], pools[c], [(512 * k, t) for k, t in enumerate(ROWS1[c])])
        same = np.array_equal(ys[c].view(np.uint32), ref.view(np.uint32))
        assert same == (c != 1), f"chain {c}"


def test_scheduled_streams_kernel_register_budget():
    """Figures hipcc reported when the library was built: no scratch, and the kernel fits beside four k_conv_p1 waves on a SIMD
    (4 x alloc(k_conv_p1) + alloc(k_eq_ring_sched_streams) <= 512 registers per lane at the granule of 8)."""
    from open_headstage_amd import _ffi, build
    _ffi.lib()
    res = build.resources()
    assert "k_eq_ring_sched_streams" in res, sorted(res)

    def alloc(k):
        return -(-(res[k]["vgprs"] + res[k]["agprs"]) // 8) * 8

    k = res["k_eq_ring_sched_streams"]
    assert k["scratch_bytes_per_lane"] == 0, k
    assert 4 * alloc("k_conv_p1") + alloc("k_eq_ring_sched_streams") <= 512, (res["k_conv_p1"], k)

"""The host-only parts of the busy-stream scenarios (tests/busy_stream.py, tests/test_gpu_stream_order.py): the list of asynchronous
entry points is the headers', the scribbler leaves nothing a call would accept, the sizing rule holds, and the wrappers hand the
caller's rows to the library without a copy of their own -- or scribbling them would prove nothing."""
import numpy as np
import pytest

from tests import busy_stream as bs
from tests import test_gpu_stream_order as so


def test_every_asynchronous_entry_point_has_a_scenario():
    """a new prototype with a `void *hip_stream` cannot arrive without a scenario A"""
    found = bs.async_entry_points()
    assert len(found) == 16, found
    assert set(found) == set(so.SCENARIO_A), (sorted(set(found) ^ set(so.SCENARIO_A)))
    assert {k for k in so.SCENARIO_A.values()} >= set(so.IN_PLACE_KINDS) | set(so.ROW_KINDS) | set(so.STAGED_KINDS)
    # every script builds, premise included, and a sync entry really ends in its sync
    for entry, kind in so.SCENARIO_A.items():
        ops = [op[0] for op in so.script_of(kind)]
        assert "premise" in ops and ops[0] == "call", (entry, ops)
        assert ("sync" in ops) == (entry.endswith("_sync") or kind == "node") and ("join" in ops) == (kind in ("join", "deferred")), (entry, ops)


def test_the_header_scan_sees_a_new_prototype(tmp_path):
    import os
    import shutil
    inc = tmp_path / "include"
    shutil.copytree(os.path.join(bs.ROOT, "include"), inc)
    with open(inc / "ohs_scene.h", "a") as f:
        f.write("\n/* a comment naming void *hip_stream is no prototype */\nint ohs_scene_process_later(ohs_scene *sc,\n    void * hip_stream);\n")
    found = bs.async_entry_points(str(inc))
    assert set(found) - set(so.SCENARIO_A) == {"ohs_scene_process_later"}


def test_staging_slot_count_is_read_from_the_source():
    assert bs.staging_slots() == 4


@pytest.mark.parametrize("kind", so.ROW_KINDS)
def test_scribbled_rows_hold_nothing_a_call_accepts(kind):
    c = so.make_call(kind, 4)
    assert c.rows and all(v is not None for v in c.rows.values())
    rows = bs.row_arrays(c.rows)
    for name, a in rows.items():
        assert a is not c.rows[name] and not np.shares_memory(a, c.rows[name]) and np.array_equal(a, c.rows[name]), name
        assert a.dtype in (np.uint32, np.float32) and a.flags.c_contiguous
    bs.scribble(rows)
    for name, a in rows.items():
        if a.dtype == np.uint32:
            # above every count the headers allow: 2^24 tables, 65536 sets and directions
            assert (a == 0xFFFFFFFF).all() and int(a.min()) >= 1 << 24, name
        else:
            assert np.isnan(a).all(), name       # no gain that leaves a finite sample, no weight in [0, 1]
    for name, a in c.rows.items():                 # the pristine rows the twin and the models read are untouched
        assert (a < so.N_DIRS).all() if a.dtype == np.uint32 else np.isfinite(a).all(), name


def test_scribble_refuses_what_it_cannot_poison():
    with pytest.raises(TypeError):
        bs.scribble({"idx": np.zeros(3, np.int64)})
    bs.scribble({"absent": None})


def test_the_wrappers_pass_the_callers_rows_on_without_a_copy():
    """np.ascontiguousarray(a, dtype) IS a for a contiguous array of that dtype: what the wrappers' row helpers return is the caller's
    memory, so scribbling it after the call reaches what the library was handed"""
    from open_headstage_amd.batch import _index_rows, _prev_rows
    from open_headstage_amd.scene import _object_rows
    S, n = 5, 3
    a = np.zeros((S, n), np.uint32)
    assert _index_rows(a, S, n, "idx", np.uint32)[0] is a
    g = np.zeros(n, np.float32)
    assert _index_rows(g, S, n, "gain", np.float32)[0] is g
    p = np.zeros(S, np.uint32)
    assert np.shares_memory(_prev_rows(p, S, n, "prev"), p)
    o = np.zeros((S, n, 3), np.uint32)
    assert _object_rows(o, S, n, 3, "idx", np.uint32)[0] is o
    assert np.shares_memory(np.ascontiguousarray(p, dtype=np.uint32).reshape(-1), p) and np.shares_memory(np.ascontiguousarray(g).ravel(), g)


def test_sizing_rule():
    assert bs.JITTER == 10.0 and bs.CAP_S == 0.5 and bs.FLOOR_S < bs.CAP_S
    assert bs.filler_seconds(0.0) == bs.FLOOR_S
    assert bs.filler_seconds(0.02) == pytest.approx(0.2)                # ten times the enqueue time
    assert bs.filler_seconds(3.0) == bs.CAP_S                           # never half a second or more per scenario
    for e in (0.0, 1e-4, 0.01, 0.049, 0.05, 1.0):
        s = bs.filler_seconds(e)
        assert bs.FLOOR_S <= s <= bs.CAP_S and (s >= 10.0 * e or s == bs.CAP_S)
    assert bs.filler_units(0.25, 0.125) == 2 and bs.filler_units(0.02, 0.03) == 1 and bs.filler_units(0.5, 0.3) == 2
    assert bs.filler_units(0.05, 1e-4) * 1e-4 >= 0.05                   # never shorter than asked for
    with pytest.raises(AssertionError):
        bs.filler_units(0.6, 1e-4)


def test_the_two_failures_are_told_apart():
    assert issubclass(bs.PremiseError, AssertionError) and issubclass(bs.DataMismatch, AssertionError)
    assert not issubclass(bs.PremiseError, bs.DataMismatch) and not issubclass(bs.DataMismatch, bs.PremiseError)
    a = np.arange(6, dtype=np.float32).reshape(1, 2, 3)
    bs.same_bits(a, a.copy(), "equal")
    b = a.copy()
    b[0, 1, 2] = np.nan
    with pytest.raises(bs.DataMismatch, match="1 of 6 samples differ.*1 of them NaN"):
        bs.same_bits(b, a, "one NaN")
    with pytest.raises(bs.DataMismatch):
        bs.same_bits(-np.zeros(3, np.float32), np.zeros(3, np.float32), "the sign of zero is a bit")

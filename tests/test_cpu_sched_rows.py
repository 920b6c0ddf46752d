"""CPU suite: what the scheduled batch calls decide about a caller's rows before anything is queued.

open_headstage_amd/csrc/sched_rows.h is host-only C++ (the one pass over rows of set indices that ohs_batch_process_ir_scheduled,
ohs_batch_process_ir_crossfaded and ohs_batch_process_layout_scheduled share, the constant-row / equal-rows tests and the segment
count of the EQ-scheduled calls).  tools/check_sched_rows.cpp includes that header alone; it is built here with AddressSanitizer +
UBSan (g++, CPU only), run as a child process over an exhaustive set of small cases, and every field it prints is compared with
a numpy restatement of the field's DEFINITION (the header's comments, include/ohs_hip.h), not of the C++.

The Python side of the same calls -- batch.py's _index_rows / _prev_rows, which turn a caller's arrays into (array, row stride) --
is checked as a table of accepted and refused shapes."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 0xFFFFFFFF
LIMIT = 2
CALLS = [(1, 1), (2, 1), (3, 2), (4, 2), (5, 2)]        # (n_blocks, seg_blocks)
FIELDS = ["ok", "idx_bad", "prev_bad", "vary", "rows_differ", "prev_differ", "prev_boundary", "faded_end"]


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("sched_rows") / "check_sched_rows")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
           "-I" + os.path.join(ROOT, "open_headstage_amd", "csrc"), "-o", out, os.path.join(ROOT, "tools", "check_sched_rows.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan not installed")
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def _run(binary, words):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([binary], input=np.ascontiguousarray(words, np.uint32).tobytes(), capture_output=True, env=env, timeout=120)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in err and "runtime error" not in err, (r.returncode, err[-3000:])
    return r.stdout.decode().split("\n")[:-1]


# ---- the row scan ------------------------------------------------------------------------------------------------------------
def _all(shape):
    """every array of `shape` with entries in {0, 1}: [2 ** size, *shape]"""
    n = int(np.prod(shape))
    return np.array(list(itertools.product((0, 1), repeat=n)), np.uint32).reshape((-1,) + tuple(shape))


def _with_one_bad(a):
    """a [N, ...] -> a, then a with one entry set to LIMIT, for every position of that entry"""
    out = [a]
    for pos in itertools.product(*[range(d) for d in a.shape[1:]]):
        b = a.copy()
        b[(slice(None),) + pos] = LIMIT
        out.append(b)
    return np.concatenate(out)


def _cross(a, p):
    """all pairs of a row of a and a row of p"""
    return np.repeat(a, len(p), axis=0), np.tile(p, (len(a),) + (1,) * (p.ndim - 1))


def _cases(rows, n_segs, has_prev):
    """idx [N, rows, n_segs] (and prev [N, rows]): every {0, 1} array, plus each single out-of-range entry in idx or in prev"""
    idx = _all((rows, n_segs))
    if not has_prev:
        return _with_one_bad(idx), None
    prev = _all((rows,))
    a1, p1 = _cross(_with_one_bad(idx), prev)
    a2, p2 = _cross(idx, _with_one_bad(prev)[len(prev):])
    return np.concatenate([a1, a2]), np.concatenate([p1, p2])


def _expected(idx, prev, n_blocks, seg_blocks):
    """The fields by their definitions.  idx [N, rows, n_segs], prev [N, rows] or None -> [N, 8] of 0 / 1"""
    n_segs = idx.shape[2]
    none = np.zeros(len(idx), bool)
    idx_bad = (idx >= LIMIT).any(axis=(1, 2))
    prev_bad = (prev >= LIMIT).any(axis=1) if prev is not None else none
    vary = (idx != idx[:, :, :1]).any(axis=(1, 2))                  # some row changes along itself
    rows_differ = (idx != idx[:, :1, :]).any(axis=(1, 2))           # some row is not the first
    prev_differ = (prev != prev[:, :1]).any(axis=1) if prev is not None else none
    prev_boundary = (prev != idx[:, :, 0]).any(axis=1) if prev is not None else none
    # faded_end: the call's last block opens its segment, and in some row that segment's set is not the one in front of it --
    # the segment before, or prev where the call has one segment only
    last_opens_its_segment = (n_blocks - 1) % seg_blocks == 0
    if n_segs > 1:
        changes = (idx[:, :, -1] != idx[:, :, -2]).any(axis=1)
    else:
        changes = prev_boundary
    faded_end = changes & last_opens_its_segment
    fields = [~(idx_bad | prev_bad), idx_bad, prev_bad, vary, rows_differ, prev_differ, prev_boundary, faded_end]
    return np.stack(fields, axis=1).astype(np.uint8)


def _records(idx, prev, stride, n_blocks, seg_blocks):
    """the tool's input, one record per case: header, rows * stride entries (the padding holds PAD), prev"""
    N, rows, n_segs = idx.shape
    padded = np.full((N, rows, stride), PAD, np.uint32)
    padded[:, :, :n_segs] = idx
    head = np.tile(np.array([0, rows, n_segs, stride, LIMIT, prev is not None, n_blocks, seg_blocks], np.uint32), (N, 1))
    parts = [head, padded.reshape(N, -1)] + ([prev] if prev is not None else [])
    return np.concatenate(parts, axis=1).ravel()


@pytest.mark.parametrize("has_prev", [False, True], ids=["no_prev", "prev"])
@pytest.mark.parametrize("n_segs", [1, 2, 3])
@pytest.mark.parametrize("rows", [1, 2, 3])
def test_row_scan_against_the_definitions(check_bin, rows, n_segs, has_prev):
    idx, prev = _cases(rows, n_segs, has_prev)
    words, want = [], []
    for stride in (n_segs, n_segs + 1):
        for n_blocks, seg_blocks in CALLS:
            words.append(_records(idx, prev, stride, n_blocks, seg_blocks))
            want.append(_expected(idx, prev, n_blocks, seg_blocks))
    lines = _run(check_bin, np.concatenate(words))
    want = np.concatenate(want)
    assert len(lines) == len(want)
    got = np.frombuffer("".join(lines).encode(), np.uint8).reshape(-1, len(FIELDS)) - ord("0")
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        i = int(bad[0])
        j = i % len(idx)
        call = CALLS[(i // len(idx)) % len(CALLS)]
        pytest.fail(f"{bad.size} of {len(want)} cases differ; first: idx {idx[j].tolist()}, "
                    f"prev {None if prev is None else prev[j].tolist()}, "
                    f"(n_blocks, seg_blocks) {call}, padded {i // len(idx) >= len(CALLS)}: "
                    f"got {dict(zip(FIELDS, got[i].tolist()))}, want {dict(zip(FIELDS, want[i].tolist()))}")


def test_the_cases_hold_what_they_should():
    """the generator itself: counts, and that faults come one at a time"""
    idx, prev = _cases(3, 3, True)
    assert len(idx) == 512 * (1 + 9) * 8 + 512 * 8 * 3
    assert (((idx == LIMIT).sum(axis=(1, 2)) + (prev == LIMIT).sum(axis=1)) <= 1).all()
    assert ((idx == LIMIT).sum(axis=(1, 2)) == 1).sum() == 512 * 9 * 8 and ((prev == LIMIT).sum(axis=1) == 1).sum() == 512 * 8 * 3
    idx, prev = _cases(2, 1, False)
    assert prev is None and len(idx) == 4 * (1 + 2)


# ---- the helpers of the EQ-scheduled calls -------------------------------------------------------------------------------------
def test_segment_count(check_bin):
    calls = [(n, s) for n in range(0, 9) for s in range(1, 11)] + [(1 << 24, 1), (1 << 24, 7), ((1 << 24) - 1, 1 << 24)]
    lines = _run(check_bin, np.array([[1, n, s] for n, s in calls], np.uint32).ravel())
    for (n, s), line in zip(calls, lines):
        clamped = min(s, max(n, 1))                 # a segment is never longer than the call
        assert line == f"{clamped} {-(-n // clamped)}", (n, s, line)


def test_constant_row_and_equal_rows_compare_bits(check_bin):
    cases = []
    for rows in (1, 2, 3):
        for n in (1, 2, 3):
            for a in _all((rows, n)):
                cases.append(a)
    # gains travel as their bits: 0.0 and -0.0 differ, a NaN equals itself
    f = lambda *v: np.array(v, np.float32).view(np.uint32)      # noqa: E731
    cases += [np.stack([f(0.0, -0.0)]), np.stack([f(np.nan, np.nan)]), np.stack([f(0.5, 0.5), f(0.5, 0.5)]),
              np.stack([f(0.0, 0.0), f(-0.0, 0.0)])]
    words, want = [], []
    for a in cases:
        rows, n = a.shape
        for stride in (n, n + 1):
            padded = np.full((rows, stride), PAD, np.uint32)
            padded[:, :n] = a
            words.append(np.concatenate([np.array([2, rows, n, stride], np.uint32), padded.ravel()]))
            want.append(f"{int((a[0] == a[0, 0]).all())}{int((a == a[:1]).all())}")
    assert _run(check_bin, np.concatenate(words)) == want


# ---- batch.py: a caller's arrays -> (array, row stride) ----------------------------------------------------------------------
S, N_SEGS = 3, 4


@pytest.mark.parametrize("shape,stride", [
    ((N_SEGS,), 0),                 # one row for all streams
    ((N_SEGS + 3,), 0),             # longer: the surplus is never read
    ((S, N_SEGS), N_SEGS),          # a row per stream
    ((S, N_SEGS + 2), N_SEGS + 2),  # padded rows: the stride is the row length
])
@pytest.mark.parametrize("dtype", [np.uint32, np.float32])
def test_index_rows_accepts(shape, stride, dtype):
    from open_headstage_amd.batch import _index_rows
    src = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    a, got = _index_rows(src.tolist(), S, N_SEGS, "idx", dtype)
    assert got == stride and a.dtype == dtype and a.flags.c_contiguous and a.shape == shape and (a == src).all()
    # a view that is not contiguous is copied, not passed with a wrong stride
    wide = np.arange(int(np.prod(shape)) * 2, dtype=dtype).reshape(shape[:-1] + (shape[-1] * 2,))
    a, got = _index_rows(wide[..., ::2], S, N_SEGS, "idx", dtype)
    assert got == stride and a.flags.c_contiguous and (a == wide[..., ::2]).all()


@pytest.mark.parametrize("shape,text", [
    ((N_SEGS - 1,), f"idx needs {N_SEGS} entries"),                                                 # 1-D, too short
    ((S + 1, N_SEGS), f"idx: expected [{S}][>= {N_SEGS}] or [>= {N_SEGS}], got ({S + 1}, {N_SEGS})"),       # wrong stream count
    ((S - 1, N_SEGS), f"idx: expected [{S}][>= {N_SEGS}] or [>= {N_SEGS}], got ({S - 1}, {N_SEGS})"),
    ((S, N_SEGS - 1), f"idx: expected [{S}][>= {N_SEGS}] or [>= {N_SEGS}], got ({S}, {N_SEGS - 1})"),       # too few columns
    ((1, S, N_SEGS), f"idx: expected [{S}][>= {N_SEGS}] or [>= {N_SEGS}], got (1, {S}, {N_SEGS})"),         # 3-D
    ((), f"idx needs {N_SEGS} entries"),                                                            # a scalar is a row of one entry
])
def test_index_rows_refuses(shape, text):
    from open_headstage_amd.batch import _index_rows
    with pytest.raises(ValueError) as e:
        _index_rows(np.zeros(shape, np.uint32), S, N_SEGS, "idx", np.uint32)
    assert str(e.value) == text


def test_prev_rows():
    from open_headstage_amd.batch import _prev_rows
    # one row for all streams (stride 0): one entry, a scalar or [1]
    for prev in (2, [2], np.uint32(2), np.array([[2]])):
        pv = _prev_rows(prev, S, 0, "prev")
        assert pv.dtype == np.uint32 and pv.shape == (1,) and pv[0] == 2
    # rows per stream (any stride > 0): an entry per stream
    for stride in (N_SEGS, N_SEGS + 2):
        pv = _prev_rows([2, 0, 1], S, stride, "prev_idx")
        assert pv.dtype == np.uint32 and pv.flags.c_contiguous and pv.tolist() == [2, 0, 1]
    for prev, stride, text in [(2, N_SEGS, f"prev: expected {S} entries, got 1"),            # a scalar beside rows per stream
                               ([2, 0], N_SEGS, f"prev: expected {S} entries, got 2"),
                               ([2, 0, 1, 1], N_SEGS, f"prev: expected {S} entries, got 4"),
                               ([2, 0, 1], 0, "prev: expected 1 entries, got 3"),             # rows' worth beside one shared row
                               ([], 0, "prev: expected 1 entries, got 0")]:
        with pytest.raises(ValueError) as e:
            _prev_rows(prev, S, stride, "prev")
        assert str(e.value) == text

"""tests/stream_placement.py must be able to fail: its comparison and its reporting held to fake "libraries" written in numpy, each
of which places one stream wrongly the way a kernel could.  Every fake models a stream's output as f(input, row); each must be
reported with the streams named.  Also: a correct fake passes, the derangement has the properties the GPU tests rely on, the sample
of streams holds what it must, and the far layouts F1 and F2 put the chains where their names say, behind a lead that keeps a
truncated offset inside the allocation."""
import numpy as np
import pytest

from tests import stream_placement as sp
from tests.guard_bands import SENT_IN, SENT_OUT, GapDamage, filled

FRAMES = 1024


def _f(x, row):
    """a stream's output from its input [2][frames] and its row (a scalar): nothing of any other stream enters"""
    return (x * np.float32(1.0 + 0.125 * row) + np.float32(0.25) * np.roll(x, 1 + int(row) % 5, axis=1)).astype(np.float32)


def _inputs(S, seed=5):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (S, 2, FRAMES)).astype(np.float32)
    rows = rng.permutation(S).astype(np.int64) + 1          # every stream a row of its own
    return x, rows


def correct(x, rows):
    return np.stack([_f(x[j], rows[j]) for j in range(len(x))])


def swaps_two_outputs(x, rows, a=5, b=9):
    y = correct(x, rows)
    y[[a, b]] = y[[b, a]]
    return y


def row_of_three_back(x, rows):
    """stream j = 3 (mod 4) is served with the row of stream j - 3: a row of four chains that reads its first lane's row"""
    return np.stack([_f(x[j], rows[j - 3] if j % 4 == 3 else rows[j]) for j in range(len(x))])


def input_wraps_at_64(x, rows):
    """streams at or above 64 are served with stream j - 64's input: a stream index kept in six bits"""
    return np.stack([_f(x[j - 64] if j >= 64 else x[j], rows[j]) for j in range(len(x))])


def _twin(lib, S, seed=0):
    """the permuted twin on a numpy library -> (out_B, out_A, pi)"""
    x, rows = _inputs(S)
    pi = sp.derangement(S, seed)
    return lib(sp.permuted(x, pi), sp.permuted(rows, pi)), lib(x, rows), pi


# ---- the permutation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", sp.stream_counts(256))
def test_the_derangement_has_no_fixed_point_and_changes_a_third_of_every_residue_class(S):
    pi = sp.derangement(S)
    assert sp.is_derangement(pi) and len(pi) == S
    assert np.array_equal(pi, sp.derangement(S)), "seeded: the same permutation every time"
    for m in sp.MODULI:
        assert sp.class_change(pi, m) >= 1.0 / 3.0, (S, m, sp.class_change(pi, m))
    assert not sp.is_derangement(np.arange(S)) and not sp.is_derangement(np.r_[pi[:-1], pi[0]])


def test_the_stream_counts_are_the_three_rules_of_the_eq_plan():
    assert sp.stream_counts(256) == (67, 257, 515)
    for cus in (104, 256, 304):
        a, b, c = sp.stream_counts(cus)
        assert sp.expected_eq_form(a, 16 * 512, cus) == ("wave_ring", 1) and sp.expected_eq_form(a, 5 * 512, cus) == ("row_ring", 1)
        assert sp.expected_eq_form(b, 16 * 512, cus) == ("row_ring", 1) and sp.expected_eq_form(b - 1, 16 * 512, cus)[0] == "wave_ring"
        assert sp.expected_eq_form(c, 16 * 512, cus) == ("row_ring", 4) and sp.expected_eq_form(c - 8, 16 * 512, cus) == ("row_ring", 1)
        assert a % 16 and a % 4 and -(-a // 16) > 4 and -(-2 * a // 16) > 8


def test_permuted_carries_every_parameter():
    pi = sp.derangement(9)
    p = {"rows": np.arange(18).reshape(9, 2), "calls": [np.arange(9.0), None], "prev": (np.arange(9) * 3,)}
    q = sp.permuted(p, pi)
    assert np.array_equal(q["rows"], p["rows"][pi]) and np.array_equal(q["calls"][0], pi.astype(float)) and q["calls"][1] is None
    assert np.array_equal(q["prev"][0], 3 * pi)
    with pytest.raises(AssertionError):
        sp.permuted(np.arange(8), pi)


@pytest.mark.parametrize("S", sp.stream_counts(256))
def test_the_sample_holds_both_ends_both_sides_of_the_16_boundary_and_three_random_streams(S):
    sm = sp.sample_streams(S)
    b = 16 * int(round(S / 2 / 16))
    assert len(sm) == len(set(sm)) == 9 and all(0 <= s < S for s in sm)
    assert {0, 1, S - 2, S - 1, b - 1, b} <= set(sm) and b % 16 == 0 and abs(b - S / 2) <= 8
    assert set(sp.sample_streams(S, at_most=4)) == {0, S - 1, b - 1, b}
    with pytest.raises(AssertionError):
        sp.sample_streams(S, at_most=3)


# ---- the fakes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", sp.stream_counts(256))
def test_a_correct_library_passes(S):
    out_b, out_a, pi = _twin(correct, S)
    sp.assert_permuted_twin(out_b, out_a, pi, "correct")
    sp.assert_nobody_repeats(out_a, "correct")


def test_two_swapped_outputs_are_reported_with_the_streams_named():
    out_b, out_a, pi = _twin(swaps_two_outputs, 67)
    with pytest.raises(sp.PlacementMismatch) as e:
        sp.assert_permuted_twin(out_b, out_a, pi, "swap")
    inv = np.argsort(pi)
    # the twin's own streams 5 and 9, and the streams that carry A's 5 and 9
    assert set(e.value.streams) == {5, 9, int(inv[5]), int(inv[9])}
    text = str(e.value)
    assert "of 67 streams differ" in text and f"stream {e.value.streams[0]} (" in text and "mod 16" in text and "first (channel, frame) (0, 0)" in text
    assert e.value.pairs[0] == (e.value.streams[0], int(pi[e.value.streams[0]]))


@pytest.mark.parametrize("S", [67, 257])
def test_a_row_taken_three_streams_back_is_reported_for_every_fourth_stream(S):
    out_b, out_a, pi = _twin(row_of_three_back, S)
    with pytest.raises(sp.PlacementMismatch) as e:
        sp.assert_permuted_twin(out_b, out_a, pi, "row j - 3")
    # wrong in the twin at j = 3 (mod 4), wrong in A where pi(j) = 3 (mod 4); right in both, or wrong in both the SAME way, nowhere
    # else (both wrong: another row each, since the rows are all different)
    want = {j for j in range(S) if j % 4 == 3 or pi[j] % 4 == 3}
    assert set(e.value.streams) == want and len(want) > S // 4
    assert f"{len(want)} of {S} streams differ" in str(e.value) and "3 mod 4" in str(e.value)


def test_an_input_that_wraps_at_64_streams_is_reported():
    out_b, out_a, pi = _twin(input_wraps_at_64, 67)
    with pytest.raises(sp.PlacementMismatch) as e:
        sp.assert_permuted_twin(out_b, out_a, pi, "input j - 64")
    assert set(e.value.streams) == {64, 65, 66} | {j for j in range(67) if pi[j] >= 64}
    # ... while a row taken three streams back is invisible where every stream repeats one of three (stream s = base[s % 3], what the
    # full-size tests feed, rows alike): the comparison with "the stream it repeats" passes
    x, rows = _inputs(67)
    x3, rows3 = x[np.arange(67) % 3], rows[np.arange(67) % 3]
    assert np.array_equal(row_of_three_back(x3, rows3), correct(x3, rows3))


def test_nobody_repeats_names_the_pair():
    x, rows = _inputs(67)
    y = correct(x, rows)
    sp.assert_nobody_repeats(y)
    y[40] = y[7]
    assert sp.repeated_streams(y) == [(7, 40)]
    with pytest.raises(AssertionError, match=r"\(7, 40\)"):
        sp.assert_nobody_repeats(y, "repeat")


def test_the_sample_check_holds_the_bar_per_block():
    ref = np.random.default_rng(1).uniform(-1, 1, (4, 2, 4 * 512))
    got = ref.astype(np.float32)
    assert sp.assert_sample_within_bar(got, ref, [0, 3, 31, 66], 1e-6) < 1e-7
    got[2, 1, 512 + 17] += 1e-3            # one sample of one block: 3e-6 of the call's RMS would pass a per-call bar of 1e-5, not this one
    with pytest.raises(AssertionError, match="stream 31, block 1 of 4"):
        sp.assert_sample_within_bar(got, ref, [0, 3, 31, 66], 1e-6, "sample")
    got[0, 0, 5] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        sp.assert_sample_within_bar(got, ref, [0, 3, 31, 66], 1e-6, "sample")


# ---- far layouts ------------------------------------------------------------------------------------------------------------------
def test_f1_and_f2_put_the_chains_beyond_2_31_and_2_32_bytes_behind_a_lead_that_holds_a_truncated_offset():
    frames = 16 * 512
    f1 = sp.layout_f1(frames)
    base = f1.start(0, 0)
    assert f1.S == 3 and f1.ss == 2 ** 29 + 1028 and f1.cs == frames + 4 and f1.lead >= 2 ** 29 + 4096
    assert 2 ** 31 < 4 * (f1.start(1, 0) - base) < 2 ** 32 < 4 * (f1.start(2, 0) - base)
    f2 = sp.layout_f2(frames)
    assert f2.S == 1 and f2.cs == 2 ** 30 + 2052 and 4 * (f2.start(0, 1) - f2.start(0, 0)) > 2 ** 32 and f2.lead >= 2 ** 29 + 4096
    f2k = sp.layout_f2(frames, channels=3)
    assert 4 * (f2k.start(0, 2) - f2k.start(0, 0)) > 2 ** 33
    # what the EQ's ring forms reach (csrc/eq_ring2_body.hpp): F1 lies within it, F2 and the wider F1w do not
    f1w = sp.layout_f1w(frames)
    assert sp.ring_addressable(f1.ss, f1.cs, frames) and not sp.ring_addressable(f2.ss, f2.cs, frames)
    assert not sp.ring_addressable(f1w.ss, f1w.cs, frames) and 4 * (f1w.start(1, 0) - f1w.start(0, 0)) > 2 ** 32
    for lay in (f1, f2, f2k, f1w, sp.layout_f1(5 * 512, channels=6, k=3)):
        assert all(v % 4 == 0 for v in (lay.ss, lay.cs, lay.lead)) and 4 * lay.total <= 24 * 2 ** 30 // 2       # in + out within 24 GiB
        starts = [o for _, _, o in lay.chains()]
        assert starts == sorted(starts) and all(b - a >= lay.frames + 4 for a, b in zip(starts, starts[1:]))
        assert starts[-1] + lay.frames < lay.total
        # an element offset whose byte offset was kept in 32 bits, signed or unsigned, still lands inside the allocation
        for _, _, o in lay.chains():
            off = o - lay.start(0, 0)
            for wrong in (sp.truncated_32(off), (4 * off & 0xFFFFFFFF) // 4):
                assert 0 <= lay.start(0, 0) + wrong and lay.start(0, 0) + wrong + lay.frames <= lay.total
    assert sp.truncated_32(2 ** 29 + 1028) == 1028 - 2 ** 29 and sp.truncated_32(2 ** 30 + 2056) == 2056 and sp.truncated_32(100) == 100


class _SparseMemory:
    """an allocation of lay.total words of which only the chains are stored; every other word reads as the sentinel"""

    def __init__(self, lay, x, sentinel):
        self.lay, self.sent = lay, np.array(sentinel, np.uint32).view(np.float32)
        self.data = {o: np.array(x[s, c], np.float32) for s, c, o in lay.chains()}

    def read(self, off, n):
        assert 0 <= off and off + n <= self.lay.total, "an access outside the allocation: the lead is there to prevent it"
        out = np.full(n, self.sent, np.float32)
        for o, v in self.data.items():
            a, b = max(o, off), min(o + len(v), off + n)
            if a < b:
                out[a - off:b - off] = v[a - o:b - o]
        return out


def _far_library(mem, lay, rows, offset_of):
    """the fake through the pointer entry: stream s's channels are read at base + offset_of(s * ss) + c * cs"""
    base = lay.start(0, 0)
    return np.stack([_f(np.stack([mem.read(base + offset_of(s * lay.ss) + c * lay.cs, lay.frames) for c in range(2)]), rows[s])
                     for s in range(lay.S)])


def test_a_stream_offset_truncated_to_32_bits_under_f1_is_reported():
    lay = sp.layout_f1(FRAMES)
    x, rows = _inputs(3)
    mem = _SparseMemory(lay, x, SENT_IN)
    twin = correct(x, rows)
    sp.assert_same_streams(_far_library(mem, lay, rows, lambda o: o), twin, "64-bit offsets")
    with np.errstate(invalid="ignore"):
        got = _far_library(mem, lay, rows, sp.truncated_32)
    with pytest.raises(sp.PlacementMismatch) as e:
        sp.assert_same_streams(got, twin, "truncated")
    assert e.value.streams == [1, 2] and "2 of 3 streams differ" in str(e.value)
    assert np.isnan(got[1]).all()               # stream 1 read the lead's NaN sentinel; stream 2 read inside stream 0's chains


def test_the_far_gap_check_names_chain_and_offset_from_a_window():
    lay = sp.FarLayout("small", 3, 2, 512, 3000, 520, lead=40000, tail=4096)
    buf = filled(lay.total, SENT_OUT)
    y = np.random.default_rng(2).uniform(-1, 1, (3, 2, 512)).astype(np.float32)
    sp.far_place(buf, y, lay)
    assert np.array_equal(sp.far_take(buf, lay), y)
    sp.far_gaps_intact(buf, lay, SENT_OUT, "intact", chunk=1000)
    buf[lay.start(1, 1) + 512 + 3:lay.start(1, 1) + 512 + 5] = 1.0
    with pytest.raises(GapDamage) as e:
        sp.far_gaps_intact(buf, lay, SENT_OUT, "two words behind a chain", chunk=1000)
    assert e.value.runs[0] == (1, 1, "behind", 3, 2)
    buf = filled(lay.total, SENT_OUT)
    buf[5124] = 2.0                             # where a sign-extended offset lands: deep in the lead
    with pytest.raises(GapDamage, match="element 5124"):
        sp.far_gaps_intact(buf, lay, SENT_OUT, "lead")


# ---- the workgroup shape is derived, not recorded: the derivation is held to the C++ rule itself ------------------------------------
from tests.test_cpu_eq_plan import IN, OUT, ROW_RING, WAVE_RING, _run, checker  # noqa: E402, F401  (checker: the fixture that builds tools/check_eq_plan.cpp)


def test_expected_eq_form_is_what_eq_plan_h_decides(checker):
    """ohs_batch_last_eq_form reports the form, not the waves per workgroup; that S = 257 runs the row ring at one wave per workgroup
    and S = 515 at four rests on stream_placement.expected_eq_form.  tools/check_eq_plan.cpp -- csrc/eq_plan.h itself, compiled for
    the host -- is asked for the same launches: a shared table and per-stream tables, 5 and 16 blocks, three CU counts."""
    binary, _ = checker
    cases, want = [], []
    for cus in (104, 256, 304):
        for S in sp.stream_counts(cus) + (cus, cus + 2, 2 * cus - 1):
            for frames in (5 * 512, 16 * 512):
                for one_table in (1, 0):
                    row = dict.fromkeys(IN, 0)
                    row.update(one_table=one_table, addressable=1, n=frames, n_chains=2 * S, n_bands=10, xcd_lo=0, xcd_n=8, cus=cus)
                    cases.append([row[k] for k in IN])
                    want.append(sp.expected_eq_form(S, frames, cus))
    got = _run(binary, np.array(cases, np.int32))
    names = {ROW_RING: "row_ring", WAVE_RING: "wave_ring"}
    for c, w, g in zip(cases, want, got):
        g = dict(zip(OUT, g.tolist()))
        assert g["valid"] == 1 and (names.get(g["form"]), g["wg_waves"]) == w, (dict(zip(IN, c)), w, g)
    assert {w for w in want} == {("wave_ring", 1), ("row_ring", 1), ("row_ring", 4)}

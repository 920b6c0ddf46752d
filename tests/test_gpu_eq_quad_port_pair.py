"""k_eq_ring's quad body with ONE store per group (csrc/eq_quad_ring_mg_asm.inc): the loop the library
runs.  Step 8's outputs wait in a holding register, move to lanes b, c, merge with step 15's, and one store carries the
group's 16 outputs; store and load issue behind the group's wait in the next group's step-1 slot, in an iteration's last group
in its own step 16.  Ring, lanes, addresses and bits are those of round 15's loop, which the experiments build keeps behind
Tuning::eq_quad_cluster_port.

With the body forced (experiments build, Tuning::eq_form = 3), 2 streams (4 chains), 1 / 10 / 12 bands, the three denormal
modes, in place (ohs_eq_process_block runs the launch on one device array) and out of place (the experiments build's
ohs_debug_eq_process_block_out_of_place: the same launch from one allocation into another that starts from sentinel bits):
bit for bit against the oracle on the launch lengths at which the asm loop runs one, two and three iterations, each with
-1, 0, +1, +15, +16, +17 samples -- the ends of a group and of a pair of groups --, the state handed over from call to call;
one signal cut into three such calls with odd group counts against one call; and the same bits as round 15's loop."""
import ctypes as C

import numpy as np
import pytest

from tests import test_gpu_eq_ring_port as port
from tests.test_gpu_eq_quad_ring import _force, quad_ring       # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

FS = 48000.0
G, K = 16, 8        # csrc/eq_quad_ring_body.hpp: kQuadGroup, kQuadK (EQ_QUAD_RING_K)


def _iterations(n):
    """eq_quad_ring_wave's entry condition: with eq_form = 3 eq_plan() gives every launch of 1 .. 12 bands to the quad body,
    whatever its length, and the body runs (g_hi - 5) / K whole iterations of its asm loop where g_hi = (n + 1) / 16 leaves
    at least K groups behind the head's five"""
    g_hi = (n + 1) // G
    return (g_hi - 5) // K if g_hi - 5 >= K else 0


FIRST = [min(n for n in range(1, 2000) if _iterations(n) == k) for k in (1, 2, 3)]
LENGTHS = [n0 + d for n0 in FIRST for d in (-1, 0, 1, 15, 16, 17)]


def test_the_lengths_are_where_the_loop_starts_to_run():
    assert FIRST == [207, 335, 463]
    assert [_iterations(n - 1) for n in FIRST] == [0, 1, 2] and [_iterations(n) for n in FIRST] == [1, 2, 3]
    # both parities of the launch's group count ((n + 62 + 15) / 16 groups behind group -1) are among them
    assert {((n + 62 + G - 1) // G) % 2 for n in LENGTHS} == {0, 1}


def _bands(nb):
    from open_headstage_amd import BandConfig, FilterType, synth
    if nb == 10:
        return synth.eq_table()
    return [BandConfig(FilterType(i % 8), 90.0 * (i + 1) ** 1.7, 0.6 + 0.15 * i, (-1.0) ** i * (1.5 + 0.5 * i), True) for i in range(nb)]


def _signal(seed, n):
    """noise; the second half 1e-30 of it and the last quarter zeros, so that the state decays through the subnormal range"""
    from open_headstage_amd import synth
    x = synth.white_noise([seed], n)[0]
    x[:, n // 2:] *= np.float32(1e-30)
    x[:, 3 * n // 4:] = 0.0
    return x


_REF = {}


def _reference(oracle, nb, mode):
    """[stream][channel][sum(LENGTHS)]: the oracle's output, one process_block per launch length; computed once per (nb, mode)"""
    if (nb, mode) not in _REF:
        out = []
        for s in range(2):
            x = _signal(170 + s, sum(LENGTHS))
            _, eo = port._pair(oracle, _bands(nb))
            o = 0
            for n in LENGTHS:
                l, r = x[0, o:o + n].copy(), x[1, o:o + n].copy()
                with oracle.flush_denormals(mode):
                    eo.process_block(l, r)
                x[0, o:o + n], x[1, o:o + n] = l, r
                o += n
            out.append(x)
        _REF[(nb, mode)] = np.stack(out)
        _REF[(nb, mode)].setflags(write=False)
    return _REF[(nb, mode)]


def _process(eg, l, r, in_place):
    """one launch of n = l.size samples; -> (left, right) outputs"""
    if in_place:
        eg.process_block(l, r)
        return l, r
    from open_headstage_amd import _ffi
    lib = _ffi.experiments_lib()
    f = lib.ohs_debug_eq_process_block_out_of_place
    f.restype, f.argtypes = C.c_int, [C.c_void_p] * 5 + [C.c_size_t]
    ol, orr = np.empty_like(l), np.empty_like(r)
    keep = l.copy(), r.copy()
    assert f(eg._h, l.ctypes.data, r.ctypes.data, ol.ctypes.data, orr.ctypes.data, l.size) == 0
    assert np.array_equal(l.view(np.uint32), keep[0].view(np.uint32)) and np.array_equal(r.view(np.uint32), keep[1].view(np.uint32))
    return ol, orr


def _assert_same(got, ref, mode, what):
    if mode == 0:
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), what
    else:       # under a flush the two zeros may differ (include/ohs_hip.h)
        assert np.array_equal(got, ref), what
        d = got.view(np.uint32) != ref.view(np.uint32)
        assert np.all(got[d] == 0.0) and np.all(ref[d] == 0.0), what


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("nb", [1, 10, 12])
def test_bit_exact_at_the_first_iterations(oracle, quad_ring, nb, mode, in_place):
    ref = _reference(oracle, nb, mode)
    for s in range(2):
        eg, _ = port._pair(oracle, _bands(nb))
        eg.set_flush_denormals(mode)
        x = _signal(170 + s, sum(LENGTHS))
        o = 0
        for n in LENGTHS:
            l, r = _process(eg, x[0, o:o + n].copy(), x[1, o:o + n].copy(), in_place)
            _assert_same(l, ref[s, 0, o:o + n], mode, (s, "L", n))
            _assert_same(r, ref[s, 1, o:o + n], mode, (s, "R", n))
            o += n


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("cuts", [[223, 351, 479], [224, 480, 350]], ids=lambda c: "_".join(map(str, c)))
def test_one_signal_in_three_calls_against_one_call(oracle, quad_ring, cuts, in_place):
    """the launches' group counts are odd: a loop that pairs groups hands its state over in the middle of a pair"""
    assert all(n in LENGTHS and ((n + 62 + G - 1) // G + 1) % 2 == 1 and _iterations(n) >= 1 for n in cuts)     # (groups -1 .. g_total - 1)
    from open_headstage_amd import synth
    x = synth.white_noise([175], sum(cuts))[0]
    one, eo = port._pair(oracle, synth.eq_table())
    three, _ = port._pair(oracle, synth.eq_table())
    whole = np.stack(_process(one, x[0].copy(), x[1].copy(), in_place))
    parts, o = [], 0
    for n in cuts:
        parts.append(np.stack(_process(three, x[0, o:o + n].copy(), x[1, o:o + n].copy(), in_place)))
        o += n
    parts = np.concatenate(parts, axis=1)
    assert np.array_equal(parts.view(np.uint32), whole.view(np.uint32))
    l, r = x[0].copy(), x[1].copy()
    eo.process_block(l, r)
    assert np.array_equal(whole.view(np.uint32), np.stack([l, r]).view(np.uint32))


@pytest.mark.parametrize("sizes", [[10240], [8192, 333, 20000]], ids=lambda s: "_".join(map(str, s)))
def test_same_bits_as_the_loop_with_one_cluster_of_three(exp_tuning, monkeypatch, sizes):
    """the merged loop against round 15's (Tuning::eq_quad_cluster_port = 1) on the same input and tables: equal bits, call by call"""
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    x = synth.white_noise([176], sum(sizes))[0]
    exp_tuning.DEFAULTS.setdefault("eq_quad_cluster_port", "0")
    outs = []
    for cluster in (0, 1):
        _force(exp_tuning, monkeypatch, 3)
        exp_tuning("eq_quad_cluster_port", cluster)
        eg = ohs.StereoParametricEQ.new(10, FS)
        for i, b in enumerate(synth.eq_table()):
            eg.update_band_coeffs(i, FS, b)
        o, got = 0, []
        for n in sizes:
            l, r = x[0, o:o + n].copy(), x[1, o:o + n].copy()
            eg.process_block(l, r)
            got += [l, r]
            o += n
        outs.append(np.concatenate(got))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert not np.array_equal(outs[0][:sizes[0]], x[0, :sizes[0]])        # (an output, not the input left where it was)

"""k_eq_ring's third body (csrc/eq_quad_ring_body.hpp): the wave ring with one band per quad of lanes, four VOP2+DPP
instructions per sample.  A group is 16 steps, an asm loop iteration 8 groups = 128 samples; the first groups of a launch
(at least -1 .. 4), the remainder of the iterations and the last groups run in the C++ form of the same step.

Bit for bit against the oracle with the body forced (experiments build, Tuning::eq_form = 3): 1 .. 12 bands with disabled ones
in between, call lengths around the group, the ring of 64 steps and the loop iteration with each of its eight remainders, a
headline-length call split unevenly (the state handed over), the three denormal modes, the documented corners, the same
bits as the body with one band per pair of lanes (eq_form = 2), and -- through the batch, in place and out of place -- guard
bands of sentinel bits around every chain."""
import numpy as np
import pytest

from tests import test_gpu_eq_ring_port as port

pytestmark = pytest.mark.gpu

FS = 48000.0


def _force(exp_tuning, monkeypatch, form):
    from open_headstage_amd import _ffi, dsp
    monkeypatch.setattr(dsp, "lib", _ffi.experiments_lib)
    exp_tuning.DEFAULTS.setdefault("eq_form", "0")
    exp_tuning("eq_form", form)


@pytest.fixture()
def quad_ring(exp_tuning, monkeypatch):
    """StereoParametricEQ objects of the experiments library, k_eq_ring's quad body forced"""
    _force(exp_tuning, monkeypatch, 3)
    return exp_tuning


# a launch of n samples runs (n + 1) // 16 - 5 groups in asm, in whole iterations of 8: every remainder 0 .. 7, one sample to
# either side of every group edge, from no iteration at all (n < 207) to many
_EDGES = sorted({128 * k + 16 * t + e for k in (1, 2, 3, 9, 65) for t in range(8) for e in (-1, 0, 1)})


@pytest.mark.parametrize("n", [1, 2, 3, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97] + _EDGES + [8191, 8192, 8193])
def test_call_lengths_around_group_ring_and_iteration(oracle, quad_ring, n):
    from open_headstage_amd import synth
    eg, eo = port._pair(oracle, synth.eq_table())
    x = synth.white_noise([51], 3 * n + 5)[0]
    port._same_bits(eg, eo, x, [n, 5, n, n])        # the state carries from call to call


@pytest.mark.parametrize("enabled", [list(range(k)) for k in range(1, 13)] + [[3], [1, 4, 5, 9], [0, 2, 4, 6, 8, 10, 11, 13], [2, 3, 5, 7, 11, 12, 13]],
                         ids=lambda e: "bands_" + "_".join(map(str, e)))
def test_band_counts_and_disabled_bands(oracle, quad_ring, enabled):
    from open_headstage_amd import BandConfig, FilterType, synth
    bands = [BandConfig(FilterType(i % 8), 90.0 * (i + 1) ** 1.7, 0.6 + 0.15 * i, (-1.0) ** i * (1.5 + 0.5 * i), i in enabled)
             for i in range(max(enabled) + 2)]
    eg, eo = port._pair(oracle, bands)
    x = synth.white_noise([52], 9000)[0]
    port._same_bits(eg, eo, x, [1000, 50, 2950, 5000])


def test_headline_length_split_unevenly(oracle, quad_ring):
    from open_headstage_amd import synth
    eg, eo = port._pair(oracle, synth.eq_table())
    sizes = [200017, 97, 8192, 271950]          # 480 256 samples, the headline's call length
    x = synth.white_noise([53], sum(sizes))[0]
    port._same_bits(eg, eo, x, sizes)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_denormal_modes(oracle, quad_ring, mode):
    """the state decays through the subnormal range behind the signal's end (IEEE) or drops to zero there (FTZ, FTZ | DAZ):
    the same values in every mode; under a flush the two zeros may differ (include/ohs_hip.h)"""
    from open_headstage_amd import synth
    eg, eo = port._pair(oracle, synth.eq_table())
    eg.set_flush_denormals(mode)
    x = synth.white_noise([54], 64000)[0]
    x[:, 1500:] = 0.0
    o = 0
    for n in [1000, 20000, 43000]:
        gl, gr = x[0, o:o + n].copy(), x[1, o:o + n].copy()
        ol, orr = gl.copy(), gr.copy()
        eg.process_block(gl, gr)
        with oracle.flush_denormals(mode):
            eo.process_block(ol, orr)
        g, r = np.stack([gl, gr]), np.stack([ol, orr])
        if mode == 0:
            assert np.array_equal(g.view(np.uint32), r.view(np.uint32)), (mode, n)
        else:
            assert np.array_equal(g, r), (mode, n)
            d = g.view(np.uint32) != r.view(np.uint32)
            assert np.all(g[d] == 0.0) and np.all(r[d] == 0.0), (mode, n)
        o += n


def test_documented_corners(oracle, quad_ring):
    """include/ohs_hip.h: a -0.0 sample may come out as +0.0 (equal as numbers, every other sample bit-exact); a non-finite
    input sample makes the output non-finite from up to 64 samples before it -- everything earlier is bit-exact, and from that
    sample on the reference's output is non-finite as well"""
    from open_headstage_amd import synth
    eg, eo = port._pair(oracle, synth.eq_table())
    n = 12000
    x = synth.white_noise([55], n)[0]
    x[:, 1000:1100] = -0.0
    x[1, 5000:] = -0.0
    gl, gr = x[0].copy(), x[1].copy(); ol, orr = x[0].copy(), x[1].copy()
    eg.process_block(gl, gr); eo.process_block(ol, orr)
    assert np.array_equal(gl, ol) and np.array_equal(gr, orr)
    for g, o in ((gl, ol), (gr, orr)):
        nz = o != 0
        assert np.array_equal(g[nz].view(np.uint32), o[nz].view(np.uint32))
        d = g.view(np.uint32) != o.view(np.uint32)
        assert np.all(np.signbit(o[d])) and not np.any(np.signbit(g[d]))      # only -0.0 -> +0.0
    for k in (7013, 7014, 7015, 7016, 9000):
        eg, eo = port._pair(oracle, synth.eq_table())
        x = synth.white_noise([56], n)[0]
        x[0, k] = np.nan
        gl, gr = x[0].copy(), x[1].copy(); ol, orr = x[0].copy(), x[1].copy()
        eg.process_block(gl, gr); eo.process_block(ol, orr)
        assert np.array_equal(gr.view(np.uint32), orr.view(np.uint32))
        assert np.array_equal(gl[:k - 64].view(np.uint32), ol[:k - 64].view(np.uint32))
        assert np.isnan(ol[k:]).all() and np.isnan(gl[k:]).all()


@pytest.mark.parametrize("sizes", [[10240], [8192, 333, 20000], [100, 9999, 1]], ids=lambda s: "_".join(map(str, s)))
def test_same_bits_as_the_pair_body(exp_tuning, monkeypatch, sizes):
    """form 3 against form 2 on the same input and the same tables: equal bits, call by call"""
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    x = synth.white_noise([57], sum(sizes))[0]
    outs = []
    for form in (3, 2):
        _force(exp_tuning, monkeypatch, form)
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


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("layout", list(port._LAYOUTS))
@pytest.mark.parametrize("blocks", [17, 19, 70])
def test_guard_bands(oracle, exp_tuning, in_place, layout, blocks):
    """the port's stores and loads stay inside [0, n) of their chain: gaps of sentinel bits (NaN in the input) before, between
    and behind the chains keep their bits, every sample is bit-exact.  17 blocks = 8 704 samples: 67 iterations and 3 groups,
    19 blocks: 75 iterations and 3 groups, 70 blocks: the EQ || convolution overlap splits the call into six EQ launches"""
    import open_headstage_amd as ohs
    from open_headstage_amd import _ffi, synth
    exp_tuning.DEFAULTS.setdefault("eq_form", "0")
    exp_tuning("eq_form", 3)
    lib = _ffi.experiments_lib()
    S = port.S
    frames = blocks * 512
    lead, cgap, sgap, tail = port._LAYOUTS[layout]
    ss, cs, total, mask = port._layout(frames, lead, cgap, sgap, tail)
    irs = synth.hrir_set(512)
    coeffs, en = port._tables(ohs, False)
    x = synth.white_noise(range(80, 80 + S), frames)
    xe = np.stack([port._oracle_eq(oracle, coeffs[s], en[s], x[s]) for s in range(S)])

    bp = port._batch(ohs, lib, irs, coeffs, en, True, False)
    out, inb, hin = port._run(bp, x, lead, ss, cs, total, frames, in_place)
    ref = port._batch(ohs, lib, irs, coeffs, en, False, False)
    rout, _, _ = port._run(ref, xe, lead, ss, cs, total, frames, False)

    gap = ~mask
    sent = port.SENT_IN if in_place else port.SENT_OUT
    assert np.all(out.view(np.uint32)[gap] == sent), np.flatnonzero(out.view(np.uint32)[gap] != sent)[:8]
    if not in_place:
        assert np.array_equal(inb.view(np.uint32), hin.view(np.uint32))        # the input is only read
    y, yr = port._take(out, lead, ss, cs, frames), port._take(rout, lead, ss, cs, frames)
    for s in range(S):
        assert np.array_equal(y[s].view(np.uint32), yr[s].view(np.uint32)), f"stream {s}"

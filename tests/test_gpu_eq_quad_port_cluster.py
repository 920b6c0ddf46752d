"""k_eq_ring's quad body with the port's memory instructions in one cluster per group (csrc/eq_quad_ring_cl_asm.inc, DESIGN.md
4.5, round 15): the loop the library runs.  Step 8's value waits in a holding register, step 15's slot issues store, store,
load back to back; ring, lanes, addresses and bits are those of round 12's loop, which the experiments build keeps behind
Tuning::eq_quad_lone_port.

With the body forced (experiments build, Tuning::eq_form = 3): bit for bit against the oracle on call lengths without an asm
run, with exactly one and two iterations, with every remainder of the iteration count and around 8 192, the state handed over
from call to call; 1 and 12 bands; the three denormal modes; the same bits as round 12's loop in one process; and -- through
the batch, in place and out of place -- guard bands of sentinel bits around every chain."""
import numpy as np
import pytest

from tests import test_gpu_eq_ring_port as port
from tests.test_gpu_eq_quad_ring import _force, quad_ring       # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

FS = 48000.0
SIZE_LISTS = ([206, 207, 208, 222, 223, 224, 335, 336, 337],
              [1000 + 16 * t + e for t in range(8) for e in (-1, 0, 1)],
              [8191, 8193])


@pytest.mark.parametrize("sizes", SIZE_LISTS, ids=["first_iterations", "every_remainder", "around_8192"])
def test_bit_exact_over_consecutive_calls(oracle, quad_ring, sizes):
    """2 streams (4 chains), 10 bands"""
    from open_headstage_amd import synth
    x = synth.white_noise([61, 62], sum(sizes))
    for s in range(2):
        eg, eo = port._pair(oracle, synth.eq_table())
        port._same_bits(eg, eo, x[s], sizes)


@pytest.mark.parametrize("nb", [1, 12])
def test_one_and_twelve_bands(oracle, quad_ring, nb):
    from open_headstage_amd import BandConfig, FilterType, synth
    bands = [BandConfig(FilterType(i % 8), 90.0 * (i + 1) ** 1.7, 0.6 + 0.15 * i, (-1.0) ** i * (1.5 + 0.5 * i), True) for i in range(nb)]
    eg, eo = port._pair(oracle, bands)
    sizes = [207, 336, 8193]
    x = synth.white_noise([63 + nb], sum(sizes))[0]
    port._same_bits(eg, eo, x, sizes)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_denormal_modes(oracle, quad_ring, mode):
    """the state decays through the subnormal range behind the signal's end (IEEE) or drops to zero there (FTZ, FTZ | DAZ):
    the same values in every mode; under a flush the two zeros may differ (include/ohs_hip.h)"""
    from open_headstage_amd import synth
    eg, eo = port._pair(oracle, synth.eq_table())
    eg.set_flush_denormals(mode)
    sizes = [1000, 9000]
    x = synth.white_noise([64], sum(sizes))[0]
    x *= np.float32(1e-30)      # (small, so that the decaying state reaches the subnormal range within these call lengths)
    x[:, 600:] = 0.0
    o = 0
    for n in sizes:
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


@pytest.mark.parametrize("sizes", [[10240], [8192, 333, 20000]], ids=lambda s: "_".join(map(str, s)))
def test_same_bits_as_the_loop_with_lone_memory_instructions(exp_tuning, monkeypatch, sizes):
    """the cluster loop against round 12's (Tuning::eq_quad_lone_port = 1) on the same input and tables: equal bits, call by call"""
    import open_headstage_amd as ohs
    from open_headstage_amd import synth
    x = synth.white_noise([65], sum(sizes))[0]
    exp_tuning.DEFAULTS.setdefault("eq_quad_lone_port", "0")
    outs = []
    for lone in (0, 1):
        _force(exp_tuning, monkeypatch, 3)
        exp_tuning("eq_quad_lone_port", lone)
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


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("blocks", [17, 19])
def test_guard_bands(oracle, exp_tuning, in_place, blocks):
    """the port's stores and loads stay inside [0, n) of their chain: gaps of sentinel bits (NaN in the input) before, between
    and behind the chains keep their bits, every sample is bit-exact.  17 blocks = 8 704 samples: 67 iterations and 3 groups,
    19 blocks: 75 iterations and 3 groups"""
    import open_headstage_amd as ohs
    from open_headstage_amd import _ffi, synth
    exp_tuning.DEFAULTS.setdefault("eq_form", "0")
    exp_tuning("eq_form", 3)
    lib = _ffi.experiments_lib()
    S = port.S
    frames = blocks * 512
    lead, cgap, sgap, tail = port._LAYOUTS["gaps"]
    ss, cs, total, mask = port._layout(frames, lead, cgap, sgap, tail)
    irs = synth.hrir_set(512)
    coeffs, en = port._tables(ohs, False)
    x = synth.white_noise(range(90, 90 + S), frames)
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

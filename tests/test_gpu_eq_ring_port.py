"""The wave ring's I/O port (csrc/eq_ring64_body.hpp): four groups of 48 samples per loop iteration, a tail of 0 .. 3 groups,
stores and loads through buffer resources over the launch's n samples of a chain (row 0's offset lies beyond every launch's
num_records, so its stores are dropped and its loads return 0; loads past the launch's last sample return 0).

Bit for bit against the oracle with the wave-ring form forced (experiments build, Tuning::eq_form = 2): call lengths around the
iteration's edges and the tail's four sizes, 8 191 .. 8 193, a headline-length call split unevenly; shared and per-stream tables.
Guard bands: one allocation per buffer with gaps before, between and after every chain, filled with sentinel bits; after the
call every gap still holds its sentinel (nothing stored outside [0, n) of a chain, row 0 included) and every sample is
bit-exact -- in place and out of place, and with the last chain ending exactly at the end of its allocation."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS = 48000.0


@pytest.fixture()
def wave_ring(exp_tuning, monkeypatch):
    """StereoParametricEQ objects of the experiments library, k_eq_ring's wave-ring form forced"""
    from open_headstage_amd import _ffi, dsp
    monkeypatch.setattr(dsp, "lib", _ffi.experiments_lib)
    exp_tuning.DEFAULTS.setdefault("eq_form", "0")
    exp_tuning("eq_form", 2)
    return exp_tuning


def _pair(oracle, bands):
    import open_headstage_amd as ohs
    eg = ohs.StereoParametricEQ.new(len(bands), FS)
    eo = oracle.StereoParametricEQ(len(bands), FS)
    for i, b in enumerate(bands):
        eg.update_band_coeffs(i, FS, b)
        c, en = eg.get_band_coeffs(i)
        eo.set_band_coeffs(i, c, en)
    return eg, eo


def _same_bits(eg, eo, x, sizes):
    o = 0
    for n in sizes:
        gl, gr = x[0, o:o + n].copy(), x[1, o:o + n].copy()
        ol, orr = gl.copy(), gr.copy()
        eg.process_block(gl, gr)
        eo.process_block(ol, orr)
        assert np.array_equal(gl.view(np.uint32), ol.view(np.uint32)), ("L", n, o)
        assert np.array_equal(gr.view(np.uint32), orr.view(np.uint32)), ("R", n, o)
        o += n


# 192 = one loop iteration (four groups).  A launch of n samples runs groups 1 .. n // 48 - 1 in asm: 192 k - 1 leaves a tail
# of 2 groups, 192 k and 192 k + 1 .. + 47 a tail of 3, + 48 / + 49 none, + 96 one, + 144 two.
_EDGES = sorted({192 * k + d for k in (1, 2, 3, 4, 5, 44) for d in (-1, 0, 1, 47, 48, 49, 96, 144)})


@pytest.mark.parametrize("n", _EDGES + [8191, 8192, 8193])
def test_call_lengths_around_the_loop_iteration(oracle, wave_ring, n):
    from open_headstage_amd import synth
    eg, eo = _pair(oracle, synth.eq_table())
    x = synth.white_noise([41], 3 * n + 5)[0]
    _same_bits(eg, eo, x, [n, 5, n, n])        # the state carries from call to call


def test_headline_length_split_unevenly(oracle, wave_ring):
    from open_headstage_amd import synth
    eg, eo = _pair(oracle, synth.eq_table())
    sizes = [200017, 97, 8192, 271950]          # 480 256 samples, the headline's call length
    x = synth.white_noise([42], sum(sizes))[0]
    _same_bits(eg, eo, x, sizes)


# -- guard bands through the batch (EQ -> convolution -> gain): the EQ writes d_out, the convolution runs on it in place; the
#    reference is a batch with the EQ off fed with the oracle's EQ output in the same layout (the convolution is a function of
#    the bits it is fed, so one differing EQ bit would show) --------------------------------------------------------------

S = 3
SENT_IN = np.uint32(0x7FA5A5A5)         # a NaN: an input gap that leaked into a chain would poison its output
SENT_OUT = np.uint32(0xDEADBEEF)


def _tables(ohs, per_stream, nb=10):
    """coeffs [S][nb][5], enabled [S][nb]: one table for every stream, or a different one per stream"""
    from open_headstage_amd import synth
    from open_headstage_amd.dsp import FilterType
    rng = np.random.default_rng(5)
    coeffs = np.zeros((S, nb, 5), np.float32)
    en = np.ones((S, nb), bool)
    for s in range(S):
        for b in range(nb):
            fc = min(35.0 * 2.0 ** (b * 0.9 + 0.11 * s), 18000.0)
            coeffs[s, b] = ohs.biquad_coefficients(FilterType.Peak, synth.FS, fc, 0.9, float(rng.uniform(-8, 8)))
    if per_stream:
        en[1, 3] = False
        en[2, 6:] = False
    else:
        coeffs[:] = coeffs[0]
    return coeffs, en


def _oracle_eq(oracle, coeffs, en, x):
    q = oracle.StereoParametricEQ(coeffs.shape[0], FS)
    for b in range(coeffs.shape[0]):
        q.set_band_coeffs(b, coeffs[b], bool(en[b]))
    l, r = x[0].copy(), x[1].copy()
    q.process_block(l, r)
    return np.stack([l, r])


def _layout(frames, lead, cgap, sgap, tail):
    cs = frames + cgap
    ss = 2 * cs + sgap
    total = lead + (S - 1) * ss + cs + frames + tail
    mask = np.zeros(total, bool)            # True: a sample of some chain
    for s in range(S):
        for c in range(2):
            o = lead + s * ss + c * cs
            mask[o:o + frames] = True
    return ss, cs, total, mask


def _place(buf, x, lead, ss, cs, frames):
    for s in range(S):
        for c in range(2):
            o = lead + s * ss + c * cs
            buf[o:o + frames] = x[s, c]


def _take(buf, lead, ss, cs, frames):
    return np.stack([np.stack([buf[lead + s * ss + c * cs:lead + s * ss + c * cs + frames] for c in range(2)]) for s in range(S)])


def _batch(ohs, lib, irs, coeffs, en, eq_on, per_stream):
    bp = ohs.BatchProcessor(S, num_bands=coeffs.shape[1], library=lib)
    for p in range(4):
        bp.set_ir(p, irs[p])
    bp.set_conv_plan(1)
    bp.set_gain(0.75)
    bp.set_eq_enabled(eq_on)
    for b in range(coeffs.shape[1]):
        if per_stream:
            for s in range(S):
                bp.set_stream_band_coeffs(s, b, coeffs[s, b], bool(en[s, b]))
        else:
            bp.set_band_coeffs(b, coeffs[0, b], bool(en[0, b]))
    return bp


def _run(bp, x, lead, ss, cs, total, frames, in_place):
    """x [S][2][frames] into a fresh sentinel-filled allocation laid out by (lead, ss, cs); returns (out buffer, in buffer)"""
    import torch
    hin = np.full(total, SENT_IN, np.uint32).view(np.float32)
    _place(hin, x, lead, ss, cs, frames)
    d_in = torch.from_numpy(hin.copy()).cuda()
    if in_place:
        d_out = d_in
    else:
        d_out = torch.from_numpy(np.full(total, SENT_OUT, np.uint32).view(np.float32)).cuda()
    bp.process_ptr(d_in.data_ptr() + 4 * lead, d_out.data_ptr() + 4 * lead, frames // 512, ss, cs,
                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_in.cpu().numpy(), hin


# (lead, channel gap, stream gap, tail gap) in samples; tail 0: the last chain ends exactly at the end of its allocation
_LAYOUTS = {"gaps": (37, 61, 129, 83), "ends_at_allocation_end": (64, 1, 48, 0)}


@pytest.mark.parametrize("per_stream", [False, True], ids=["shared", "per_stream"])
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("layout", list(_LAYOUTS))
@pytest.mark.parametrize("blocks", [17, 19, 70])
def test_guard_bands(oracle, exp_tuning, per_stream, in_place, layout, blocks):
    """17 blocks = 8 704 samples: 180 asm groups (no tail), 19 blocks: 201 (a tail of 1), 70 blocks: the EQ || convolution
    overlap splits the call into six EQ launches (each with its own num_records)"""
    import open_headstage_amd as ohs
    from open_headstage_amd import _ffi, synth
    exp_tuning.DEFAULTS.setdefault("eq_form", "0")
    exp_tuning("eq_form", 2)
    lib = _ffi.experiments_lib()
    frames = blocks * 512
    lead, cgap, sgap, tail = _LAYOUTS[layout]
    ss, cs, total, mask = _layout(frames, lead, cgap, sgap, tail)
    irs = synth.hrir_set(512)
    coeffs, en = _tables(ohs, per_stream)
    x = synth.white_noise(range(70, 70 + S), frames)
    xe = np.stack([_oracle_eq(oracle, coeffs[s], en[s], x[s]) for s in range(S)])

    bp = _batch(ohs, lib, irs, coeffs, en, True, per_stream)
    out, inb, hin = _run(bp, x, lead, ss, cs, total, frames, in_place)
    ref = _batch(ohs, lib, irs, coeffs, en, False, per_stream)
    rout, _, _ = _run(ref, xe, lead, ss, cs, total, frames, False)

    gap = ~mask
    sent = SENT_IN if in_place else SENT_OUT
    assert np.all(out.view(np.uint32)[gap] == sent), np.flatnonzero(out.view(np.uint32)[gap] != sent)[:8]
    if not in_place:
        assert np.array_equal(inb.view(np.uint32), hin.view(np.uint32))        # the input is only read
    y, yr = _take(out, lead, ss, cs, frames), _take(rout, lead, ss, cs, frames)
    for s in range(S):
        assert np.array_equal(y[s].view(np.uint32), yr[s].view(np.uint32)), f"stream {s}"

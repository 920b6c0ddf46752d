"""tests/guard_bands.py can fail: a broken mask or a blind checker would make every guard-band test check nothing.  No library,
no GPU: the layout's bookkeeping, and three corruptions made by hand that gaps_intact must report with the right chain, offset and
length."""
import numpy as np
import pytest

from tests.guard_bands import SENT_IN, SENT_OUT, GapDamage, filled, gaps_intact, layout, place, take

# (S, frames, (lead, channel gap, stream gap, tail), alignment of every chain start in floats)
LAYOUTS = [(3, 512, (1, 1, 0, 1), 1), (3, 1536, (37, 61, 129, 83), 1), (5, 2048, (2, 2, 0, 2), 2), (5, 1536, (1574, 1566, 10, 1578), 2),
           (3, 1024, (4, 4, 0, 4), 4), (2, 4096, (8228, 8252, 20, 8276), 4), (1, 512, (3, 5, 7, 9), 1)]


def _audio(S, frames, seed=1):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (S, 2, frames)).astype(np.float32)


@pytest.mark.parametrize("S,frames,gaps,align", LAYOUTS)
def test_mask_chains_alignment_and_round_trip(S, frames, gaps, align):
    lead, cgap, sgap, tail = gaps
    ss, cs, total, mask = layout(S, frames, *gaps)
    assert mask.shape == (total,) and int(mask.sum()) == S * 2 * frames         # exactly the audio, nothing else
    starts = [lead + s * ss + c * cs for s in range(S) for c in range(2)]
    for k, o in enumerate(starts):
        assert o % align == 0 and ss % align == 0 and cs % align == 0, (k, o, ss, cs)
        assert mask[o:o + frames].all() and not mask[o - 1] and not mask[o + frames]      # a gap on both sides of every chain
        if k:
            assert o >= starts[k - 1] + frames + 1                                          # chains are disjoint and apart
    assert starts[0] == lead and total - (starts[-1] + frames) == tail
    # every sample of x lands on a mask position of its own (disjoint chains), and comes back
    x = _audio(S, frames)
    buf = filled(total, SENT_IN)
    place(buf, x, lead, ss, cs)
    assert np.array_equal(take(buf, S, frames, lead, ss, cs).view(np.uint32), x.view(np.uint32))
    assert np.array_equal(buf[mask].view(np.uint32), x.ravel().view(np.uint32))
    assert (buf.view(np.uint32)[~mask] == SENT_IN).all()
    counts = np.zeros(total, np.int32)
    for o in starts:
        counts[o:o + frames] += 1
    assert counts.max() == 1


@pytest.mark.parametrize("gaps", [(0, 1, 0, 1), (1, 0, 5, 1), (1, 1, 0, 0)])
def test_an_empty_gap_is_refused(gaps):
    with pytest.raises(AssertionError):
        layout(3, 512, *gaps)


@pytest.mark.parametrize("sentinel", [SENT_IN, SENT_OUT])
@pytest.mark.parametrize("S,frames,gaps,align", LAYOUTS)
def test_an_intact_buffer_passes(S, frames, gaps, align, sentinel):
    ss, cs, total, mask = layout(S, frames, *gaps)
    buf = filled(total, sentinel)
    place(buf, _audio(S, frames), gaps[0], ss, cs)
    gaps_intact(buf.view(np.uint32), mask, sentinel)
    # audio that happens to hold the sentinel's bits, or anything else, is no damage: only the gaps are looked at
    buf.view(np.uint32)[mask] = np.uint32(0x12345678)
    gaps_intact(buf.view(np.uint32), mask, sentinel)


def _damaged(S, frames, gaps, sentinel, lo, hi, value=0x3F800000):
    ss, cs, total, mask = layout(S, frames, *gaps)
    buf = filled(total, sentinel)
    place(buf, _audio(S, frames), gaps[0], ss, cs)
    assert not mask[lo:hi].any()            # (the corruption lies in a gap)
    buf.view(np.uint32)[lo:hi] = np.uint32(value)
    with pytest.raises(GapDamage) as e:
        gaps_intact(buf.view(np.uint32), mask, sentinel, "case")
    return e.value, ss, cs


@pytest.mark.parametrize("s,c", [(0, 0), (0, 1), (1, 1), (2, 0)])
def test_one_sample_directly_behind_a_chain(s, c):
    S, frames, gaps = 3, 1536, (37, 61, 129, 83)
    ss, cs, _, _ = layout(S, frames, *gaps)
    end = gaps[0] + s * ss + c * cs + frames
    err, _, _ = _damaged(S, frames, gaps, SENT_OUT, end, end + 1)
    assert err.runs == [(s, c, "behind", 0, 1)] and err.n_runs == 1
    msg = str(err)
    assert f"1 sample(s) behind chain (s={s}, c={c}), offset +0 from its end" in msg and "3f800000" in msg and "deadbeef" in msg


def test_one_sample_directly_in_front_of_the_first_chain():
    S, frames, gaps = 3, 1536, (37, 61, 129, 83)
    err, _, _ = _damaged(S, frames, gaps, SENT_IN, gaps[0] - 1, gaps[0])
    assert err.runs == [(0, 0, "in front of", -1, 1)]
    assert "1 sample(s) in front of chain (s=0, c=0), offset -1 from its start" in str(err)


@pytest.mark.parametrize("off", [0, 5])
def test_a_run_of_1536_samples_behind_the_last_chain(off):
    S, frames, gaps = 3, 512, (1574, 1566, 10, 1578)
    ss, cs, total, _ = layout(S, frames, *gaps)
    end = gaps[0] + (S - 1) * ss + cs + frames
    assert end + gaps[3] == total
    err, _, _ = _damaged(S, frames, gaps, SENT_OUT, end + off, end + off + 1536, value=0)
    assert err.runs == [(S - 1, 1, "behind", off, 1536)]
    assert f"1536 sample(s) behind chain (s={S - 1}, c=1), offset +{off} from its end" in str(err)


def test_a_run_nearer_to_the_next_chain_is_named_in_front_of_it_and_many_runs_are_counted():
    S, frames, gaps = 3, 512, (600, 600, 0, 600)
    ss, cs, total, mask = layout(S, frames, *gaps)
    buf = filled(total, SENT_OUT)
    place(buf, _audio(S, frames), gaps[0], ss, cs)
    u = buf.view(np.uint32)
    start_11 = gaps[0] + ss + cs                    # chain (1, 1)
    u[start_11 - 512:start_11] = 0                  # a whole block stored in front of it
    for k in range(9):                              # nine single words behind chain (2, 1)
        u[total - 600 + 3 + 2 * k] = 7
    with pytest.raises(GapDamage) as e:
        gaps_intact(u, mask, SENT_OUT)
    assert e.value.runs[0] == (1, 1, "in front of", -512, 512)
    assert e.value.runs[1] == (2, 1, "behind", 3, 1) and e.value.n_runs == 10 and "more run(s)" in str(e.value)


def test_the_wrong_sentinel_or_a_mask_of_another_shape_fails():
    ss, cs, total, mask = layout(3, 512, 4, 4, 0, 4)
    buf = filled(total, SENT_IN)
    with pytest.raises(GapDamage):
        gaps_intact(buf.view(np.uint32), mask, SENT_OUT)
    with pytest.raises(AssertionError):
        gaps_intact(buf.view(np.uint32)[:-1], mask, SENT_IN)
    with pytest.raises(AssertionError):
        gaps_intact(buf, mask, SENT_IN)             # float32: the comparison must be on the bits (a NaN equals nothing)

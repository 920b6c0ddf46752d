"""Guard bands for tests of kernels that read and write strided [stream][channel][frame] buffers: one allocation per buffer with a
gap in front of the first chain, between every two chains and behind the last one, every gap filled with sentinel bits.  After a
call every gap word must still hold its sentinel, and a failure says WHERE it does not: whoever reads it has no debugger and no
second run.  (A chain is one channel of one stream: `frames` consecutive samples.)  Pure numpy; checked by
tests/test_cpu_guard_bands.py."""
import numpy as np

SENT_IN = np.uint32(0x7FA5A5A5)         # a NaN: a gap sample of the input that enters arithmetic poisons the output
SENT_OUT = np.uint32(0xDEADBEEF)

MAX_REPORTED = 6                        # damaged runs named in a failure message


def layout(S, frames, lead, cgap, sgap, tail):
    """S streams x 2 channels x `frames` samples in one allocation: `lead` samples in front of chain (0, 0), `cgap` between a
    stream's two chains, `cgap + sgap` between one stream's second chain and the next stream's first, `tail` behind the last.
    -> (stream stride, channel stride, samples of the allocation, mask [total] bool: True = a sample of some chain).
    Every gap is non-empty -- tail = 0 is not offered: a chain that ends at the end of the allocation proves nothing here."""
    assert S >= 1 and frames >= 1
    assert lead >= 1 and cgap >= 1 and sgap >= 0 and tail >= 1, (lead, cgap, sgap, tail)
    cs = frames + cgap
    ss = 2 * cs + sgap
    total = lead + (S - 1) * ss + cs + frames + tail
    mask = np.zeros(total, bool)
    for s in range(S):
        for c in range(2):
            o = lead + s * ss + c * cs
            assert not mask[o:o + frames].any() and (o == 0 or not mask[o - 1])
            mask[o:o + frames] = True
    assert not mask[0] and not mask[-1] and int(mask.sum()) == S * 2 * frames
    return ss, cs, total, mask


def place(buf, x, lead, ss, cs):
    """x [S][2][frames] into the chains of the 1-D buffer"""
    S, _, frames = x.shape
    for s in range(S):
        for c in range(2):
            o = lead + s * ss + c * cs
            buf[o:o + frames] = x[s, c]


def take(buf, S, frames, lead, ss, cs):
    """the chains of the 1-D buffer -> [S][2][frames] (a copy)"""
    return np.stack([np.stack([buf[lead + s * ss + c * cs:lead + s * ss + c * cs + frames] for c in range(2)]) for s in range(S)])


def filled(total, sentinel):
    """a float32 buffer of `total` samples, every word the sentinel"""
    return np.full(total, sentinel, np.uint32).view(np.float32)


class GapDamage(AssertionError):
    """gaps_intact's failure; .runs: [(s, c, side, offset, length)] of the damaged runs it names, .n_runs: all of them"""

    def __init__(self, message, runs, n_runs):
        super().__init__(message)
        self.runs, self.n_runs = runs, n_runs


def _runs(flags):
    """[(first, one past the last)] of the runs of True"""
    d = np.diff(np.concatenate(([0], flags.astype(np.int8), [0])))
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def gaps_intact(buf_u32, mask, sentinel, what=""):
    """Every word of buf_u32 outside the chains (mask False) still holds `sentinel`, or GapDamage (an AssertionError).  The message
    names, for the first few damaged runs, the chain (s, c) the run lies behind or in front of -- the nearer one --, the offset of
    the run's first sample from that chain's END (behind: 0 = the sample directly behind the chain's last) or from its START (in
    front: -1 = the sample directly in front of the chain's first), its length in samples and the first words found there."""
    buf_u32 = np.asarray(buf_u32)
    assert buf_u32.dtype == np.uint32 and buf_u32.shape == mask.shape, (buf_u32.dtype, buf_u32.shape, mask.shape)
    bad = ~mask & (buf_u32 != np.uint32(sentinel))
    if not bad.any():
        return
    chains = _runs(mask)                    # in address order: chain k is (s, c) = (k // 2, k % 2)
    starts = np.array([a for a, _ in chains])
    runs = _runs(bad)
    named, lines = [], []
    for a, b in runs[:MAX_REPORTED]:
        k = int(np.searchsorted(starts, a, side="right")) - 1      # the last chain that starts in front of the run
        behind = None if k < 0 else a - chains[k][1]
        front = None if k + 1 >= len(chains) else a - chains[k + 1][0]
        if front is None or (behind is not None and behind <= -front - (b - a)):
            kk, side, off = k, "behind", behind
        else:
            kk, side, off = k + 1, "in front of", front
        named.append((kk // 2, kk % 2, side, int(off), b - a))
        words = " ".join(f"{int(v):08x}" for v in buf_u32[a:min(b, a + 4)])
        lines.append(f"  {b - a} sample(s) {side} chain (s={kk // 2}, c={kk % 2}), offset {int(off):+d} from its "
                     f"{'end' if side == 'behind' else 'start'} (buffer index {a}): {words}{' ...' if b - a > 4 else ''}")
    more = f"\n  ... and {len(runs) - MAX_REPORTED} more run(s)" if len(runs) > MAX_REPORTED else ""
    raise GapDamage(f"{what + ': ' if what else ''}{int(bad.sum())} gap word(s) in {len(runs)} run(s) no longer hold "
                    f"{int(sentinel):08x}:\n" + "\n".join(lines) + more, named, len(runs))

"""Where a stream sits in the batch, and where its buffers sit in memory: neither may change a bit of its output.

Two twins, both compared bit for bit, every stream, after every call (tests/test_gpu_stream_placement.py):

* a PERMUTED twin: handle B carries handle A's streams through a seeded derangement pi -- B's stream j has everything of A's stream
  pi(j): input, rows, previous rows, gains, tables, object indices and weights.  out_B[j] must equal out_A[pi(j)].  A kernel that
  reads the row, the table or the input of another stream (the chunk arithmetic `gw / chunks`, a ragged last workgroup, the XCD
  renumbering, the planes of rows `L.stream` apart, chains in pairs or rows of four) serves two different streams in the two
  handles, and the twins differ;
* a FAR twin: the same calls through the pointer entries on chains that lie beyond 2^31 and 2^32 bytes from the base (layouts F1
  and F2), inside one allocation filled with tests/guard_bands.py's sentinels and with a lead long enough that an offset truncated to
  32 bits or sign-extended lands in sentinel inside the allocation: NaN output or a damaged gap, never an access outside it.

numpy and torch helpers; nothing here touches the GPU at import, and everything that compares takes numpy arrays as well as torch
tensors, so that tests/test_cpu_stream_placement.py can hold the comparison and the reporting to fake libraries written in numpy."""
import numpy as np

from tests.guard_bands import GapDamage, gaps_intact

BLOCK = 512
MODULI = (2, 4, 8, 16, 64)      # the residue classes a stream's place is decoded from: pairs, rows of four, XCDs, 16-wave workgroups, waves
MIN_CLASS_CHANGE = 1.0 / 3.0
MAX_NAMED = 4                   # differing streams named in full in a failure message
FAR_LEAD = (1 << 29) + 4096     # floats in front of the first chain of a far buffer: more than 2^31 bytes
F1_STREAM_STRIDE = (1 << 29) + 1028
F2_CHANNEL_STRIDE = (1 << 30) + 2052
F1W_STREAM_STRIDE = (1 << 30) + 1028


# ---- the permutation ------------------------------------------------------------------------------------------------------------
def class_change(pi, m):
    """the share of the streams j whose twin pi(j) lies in another residue class mod m"""
    pi = np.asarray(pi)
    return float(np.mean(pi % m != np.arange(len(pi)) % m))


def is_derangement(pi):
    pi = np.asarray(pi)
    return sorted(pi.tolist()) == list(range(len(pi))) and not bool((pi == np.arange(len(pi))).any())


def derangement(S, seed=0):
    """pi [S]: a seeded permutation without a fixed point in which, for every m of MODULI, at least a third of the streams change
    their residue class mod m.  Seeded numpy permutations have both properties with room (45 - 52 % change class mod 2, more for the
    larger moduli); the loop only throws the rare one with a fixed point away."""
    assert S >= 4, S
    for attempt in range(1000):
        pi = np.random.default_rng([seed, S, attempt]).permutation(S)
        if is_derangement(pi) and all(class_change(pi, m) >= MIN_CLASS_CHANGE for m in MODULI):
            return pi.astype(np.int64)
    raise AssertionError(f"no derangement of {S} streams with the class changes found")


def _indexed(params, idx, exact):
    if params is None:
        return None
    if isinstance(params, dict):
        return {k: _indexed(v, idx, exact) for k, v in params.items()}
    if isinstance(params, (list, tuple)):
        return type(params)(_indexed(v, idx, exact) for v in params)
    a = np.asarray(params)
    assert a.ndim >= 1 and (a.shape[0] == len(idx) if exact else a.shape[0] > int(np.max(idx))), (a.shape, len(idx))
    return np.ascontiguousarray(a[idx])


def permuted(params, pi):
    """per-stream parameters (arrays whose first axis is the stream, or lists / tuples / dicts of such; None stays None) as handle B
    gets them: entry j is entry pi(j)"""
    return _indexed(params, np.asarray(pi), True)


def taken(params, streams):
    """the same parameters of a sample of streams only, in the sample's order (what a host model of len(streams) streams is given)"""
    return _indexed(params, np.asarray(streams), False)


# ---- the stream counts and the sample ---------------------------------------------------------------------------------------------
def stream_counts(cus=256):
    """(wave ring, row ring at one wave per workgroup, row ring at four waves per workgroup) for a device of `cus` compute units:
    * 67: odd and prime -- a ragged last workgroup for 16 and for 4 waves, more than eight workgroups (the XCD renumbering wraps);
      its 134 chains are at most 2 * cus, the wave ring's condition at 8192 frames (any device of 67 CUs or more);
    * cus + 1: 2 * cus + 2 chains, more than 2 * cus -- the row ring; fewer waves of four chains than CUs -- one wave per workgroup;
    * 2 * cus + 3: cus + 2 waves of four chains, at least cus -- four waves per workgroup.
    256 CUs: (67, 257, 515)."""
    assert cus >= 67, cus
    return 67, cus + 1, 2 * cus + 3


def expected_eq_form(S, frames, cus=256):
    """what csrc/eq_plan.h's rule gives a one-table or per-stream-table launch of 2 S chains over `frames` frames at strides the
    ring forms reach -> (form, waves per workgroup)"""
    chains = 2 * S
    if chains <= 2 * cus and frames >= 8192:
        return "wave_ring", 1
    return "row_ring", (4 if (chains + 3) // 4 >= cus else 1)


def sample_streams(S, seed=0, n_random=3, at_most=None):
    """the streams held to the host models: 0, 1, S - 2, S - 1, the two on either side of the multiple of 16 nearest S / 2, and
    n_random seeded ones.  at_most (never below 4): the first stream, the last one and both sides of the 16-boundary come first."""
    b = 16 * int(round(S / 2 / 16))
    b = min(max(b, 1), S - 1)
    core = [0, S - 1, b - 1, b]
    rest = [1, S - 2]
    rng = np.random.default_rng([seed, S])
    for s in rng.permutation(S).tolist():
        if len(rest) >= 2 + n_random:
            break
        if s not in core and s not in rest:
            rest.append(s)
    out = []
    for s in core + rest:
        if 0 <= s < S and s not in out:
            out.append(s)
    if at_most is not None:
        assert at_most >= 4, "the sample never goes below the first stream, the last one and both sides of the 16-boundary"
        out = out[:at_most]
    return out


# ---- the comparison ---------------------------------------------------------------------------------------------------------------
class PlacementMismatch(AssertionError):
    """.streams: every differing j (B's numbering), .pairs: [(j, pi(j))] of the named ones"""

    def __init__(self, message, streams, pairs):
        super().__init__(message)
        self.streams, self.pairs = streams, pairs


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def _bits(a):
    """[S][C][frames] float32 -> the same as int32 words (torch: on the array's device, no copy)"""
    if _is_torch(a):
        import torch
        assert a.dtype == torch.float32
        return a.view(torch.int32)
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.view(np.int32)


def _residues(s):
    return ", ".join(f"{s % m} mod {m}" for m in (2, 4, 8, 16))


def differing_streams(got, want):
    """got, want [S][C][frames] float32 (numpy or torch, both the same) -> the streams in which any bit differs (one reduction where
    the arrays live, one small download)"""
    g, w = _bits(got), _bits(want)
    assert tuple(g.shape) == tuple(w.shape), (tuple(g.shape), tuple(w.shape))
    if _is_torch(g):
        return (g != w).flatten(1).any(dim=1).nonzero().flatten().cpu().tolist()
    return np.flatnonzero((g != w).reshape(g.shape[0], -1).any(axis=1)).tolist()


def _first_last(got_s, want_s):
    """one stream [C][frames] -> (number of differing samples, first (channel, frame), last (channel, frame))"""
    g, w = _bits(got_s), _bits(want_s)
    if _is_torch(g):
        g, w = g.cpu().numpy(), w.cpu().numpy()
    bad = np.argwhere(g != w)
    return len(bad), tuple(bad[0].tolist()), tuple(bad[-1].tolist())


def assert_permuted_twin(out_b, out_a, pi, what=""):
    """out_B[j] == out_A[pi(j)] bit for bit for every j, or PlacementMismatch: the number of differing streams and, for the first
    few, j, pi(j), their residues mod 2, 4, 8 and 16 and the first and last differing (channel, frame)"""
    pi = np.asarray(pi)
    if _is_torch(out_a):
        import torch
        want = out_a[torch.as_tensor(pi, device=out_a.device)]
    else:
        want = np.asarray(out_a)[pi]
    bad = differing_streams(out_b, want)
    if not bad:
        return
    lines, pairs = [], []
    for j in bad[:MAX_NAMED]:
        n, first, last = _first_last(out_b[j], want[j])
        pairs.append((j, int(pi[j])))
        lines.append(f"  stream {j} ({_residues(j)}) of the twin != stream {int(pi[j])} ({_residues(int(pi[j]))}): {n} samples, first "
                     f"(channel, frame) {first}, last {last}")
    more = f"\n  ... and {len(bad) - MAX_NAMED} more: {bad[MAX_NAMED:MAX_NAMED + 24]}" if len(bad) > MAX_NAMED else ""
    raise PlacementMismatch(f"{what + ': ' if what else ''}{len(bad)} of {len(pi)} streams differ from the stream they carry:\n"
                            + "\n".join(lines) + more, bad, pairs)


def assert_same_streams(got, want, what=""):
    """the far twin's comparison: stream s of `got` equals stream s of `want` bit for bit, every stream (the same report)"""
    assert_permuted_twin(got, want, np.arange(got.shape[0]), what)


def repeated_streams(out):
    """[(s, t)], s < t: streams of `out` with bit-identical output (a 64-bit position-weighted sum of the words per stream finds the
    candidates where the array lives; candidates are then compared in full)"""
    b = _bits(out)
    S = b.shape[0]
    if _is_torch(b):
        import torch
        n = b[0].numel()
        wgt = (torch.arange(n, device=b.device, dtype=torch.int64) * 2654435761 + 40503) | 1
        key = (b.reshape(S, n).to(torch.int64) * wgt).sum(dim=1).cpu().numpy()
    else:
        n = b[0].size
        wgt = (np.arange(n, dtype=np.int64) * 2654435761 + 40503) | 1
        with np.errstate(over="ignore"):
            key = (b.reshape(S, n).astype(np.int64) * wgt).sum(axis=1)
    order = np.argsort(key, kind="stable")
    pairs = []
    for a, c in zip(order[:-1].tolist(), order[1:].tolist()):
        if key[a] == key[c] and not differing_streams(out[a:a + 1], out[c:c + 1]):
            pairs.append((min(a, c), max(a, c)))
    return sorted(pairs)


def assert_nobody_repeats(out, what=""):
    pairs = repeated_streams(out)
    assert not pairs, f"{what + ': ' if what else ''}{len(pairs)} pair(s) of streams with identical output, first {pairs[:6]}"


def rel_rms_per_block(got, ref):
    """got, ref [n][2][k * 512] -> relative RMS error per stream and block of 512 frames [n][k] (both ears together)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)

    def per_block(a):
        return np.sqrt(np.mean(a.reshape(a.shape[0], a.shape[1], -1, BLOCK) ** 2, axis=(1, 3)))
    rb = per_block(ref)
    assert (rb > 0).all(), "a silent reference block: the relative metric needs a signal"
    return per_block(got - ref) / rb


def assert_sample_within_bar(got, ref, streams, bar, what=""):
    """got, ref [len(streams)][2][k * 512]: relative RMS per stream and block of 512 at most `bar`; -> the worst figure"""
    got = np.asarray(got)
    assert np.isfinite(got).all(), f"{what}: non-finite samples in streams {[streams[i] for i in np.unique(np.argwhere(~np.isfinite(got))[:, 0])]}"
    err = rel_rms_per_block(got, ref)
    bad = np.argwhere(err > bar)
    assert bad.size == 0, (f"{what}: relative RMS {err[tuple(bad[0])]:.3e} in stream {streams[bad[0][0]]}, block {bad[0][1]} of "
                           f"{err.shape[1]} (bar {bar:.0e}); {len(bad)} (stream, block) above the bar: "
                           f"{[(streams[i], int(t)) for i, t in bad[:8]]}")
    return float(err.max())


# ---- far layouts ------------------------------------------------------------------------------------------------------------------
class FarLayout:
    """`channels` chains of `frames` floats per stream in one allocation: chain (s, c) starts at lead + s * ss + c * cs; every
    stride a multiple of 4 floats, the lead too (a 16-byte aligned base keeps the compact twin's alignment class)"""

    def __init__(self, name, S, channels, frames, ss, cs, lead=FAR_LEAD, tail=4096):
        assert all(v % 4 == 0 for v in (ss, cs, lead, tail)) and frames >= 1 and cs >= frames + 4 and (S == 1 or ss >= channels * cs)
        self.name, self.S, self.channels, self.frames, self.ss, self.cs, self.lead = name, S, channels, frames, ss, cs, lead
        self.total = lead + (S - 1) * ss + (channels - 1) * cs + frames + tail

    def start(self, s, c):
        """element offset of chain (s, c) from the allocation's base"""
        return self.lead + s * self.ss + c * self.cs

    def chains(self):
        return [(s, c, self.start(s, c)) for s in range(self.S) for c in range(self.channels)]

    def mask(self, lo, hi):
        """[hi - lo] bool: True = a sample of some chain, for the window [lo, hi) of the allocation"""
        m = np.zeros(hi - lo, bool)
        for _, _, o in self.chains():
            a, b = max(o, lo), min(o + self.frames, hi)
            if a < b:
                m[a - lo:b - lo] = True
        return m


def layout_f1(frames, channels=2, k=1):
    """F1: three streams, stream stride 2^29 + 1028 floats, channel stride frames + 4 k: stream 1 starts beyond 2^31 bytes from
    chain (0, 0), stream 2 beyond 2^32"""
    return FarLayout("F1", 3, channels, frames, F1_STREAM_STRIDE, frames + 4 * k)


def layout_f1w(frames, channels=2, k=1):
    """F1 with the streams twice as far apart (2^30 + 1028 floats): stream 1 already starts beyond 2^32 bytes.  F1 itself lies
    within the reach of the EQ's ring forms (ring_addressable), so the fallbacks behind that reach are run under this one and
    under F2"""
    return FarLayout("F1w", 3, channels, frames, F1W_STREAM_STRIDE, frames + 4 * k)


def ring_addressable(ss, cs, n):
    """csrc/eq_ring2_body.hpp's eq_ring2_addressable: the strides (floats) and frames the EQ ring forms' 32-bit lane offsets reach"""
    return ss >= 0 and cs >= 0 and (ss + cs + n + 1024) * 4 < (1 << 32)


def layout_f2(frames, channels=2):
    """F2: one stream, channel stride 2^30 + 2052 floats: channel 1 starts beyond 2^32 bytes from channel 0"""
    return FarLayout("F2", 1, channels, frames, channels * F2_CHANNEL_STRIDE, F2_CHANNEL_STRIDE)


def compact_layout(S, channels, frames):
    """the contiguous [S][channels][frames] tensor as a layout of the pointer entries (no lead, no gaps)"""
    lay = FarLayout.__new__(FarLayout)
    lay.name, lay.S, lay.channels, lay.frames, lay.ss, lay.cs, lay.lead = "compact", S, channels, frames, channels * frames, frames, 0
    lay.total = S * channels * frames
    return lay


def truncated_32(offset_floats):
    """what an element offset becomes in a kernel that keeps its BYTE offset in a signed 32-bit register: the mutant of the CPU
    tests, and the reason for the lead"""
    b = (4 * int(offset_floats)) & 0xFFFFFFFF
    return (b - (1 << 32) if b & 0x80000000 else b) // 4


def far_place(buf, x, lay):
    """x [S][channels][frames] into the chains of the 1-D buffer (numpy or torch, in place)"""
    for s, c, o in lay.chains():
        buf[o:o + lay.frames] = x[s, c]


def far_take(buf, lay):
    """the chains of the 1-D buffer -> [S][channels][frames] (a copy where the buffer lives)"""
    rows = [[buf[o:o + lay.frames] for c in range(lay.channels) for o in [lay.start(s, c)]] for s in range(lay.S)]
    if _is_torch(buf):
        import torch
        return torch.stack([torch.stack(r) for r in rows])
    return np.stack([np.stack(r) for r in rows])


WINDOW = 4096


def far_gaps_intact(buf, lay, sentinel, what="", chunk=1 << 27):
    """Every word of the 1-D float32 buffer outside the chains still holds `sentinel` (checked where the buffer lives, the whole
    buffer, in chunks); on failure only a window around the first offender is downloaded and handed to guard_bands' reporter.
    A float32 view of 32-bit words throughout: no arithmetic touches the NaN sentinel."""
    sent = int(np.array(sentinel, np.uint32).view(np.int32))
    words = _bits(buf)
    edges = sorted({0, lay.total} | {o for _, _, o in lay.chains()} | {o + lay.frames for _, _, o in lay.chains()})
    inside = {o for _, _, o in lay.chains()}
    for a, b in zip(edges[:-1], edges[1:]):
        if a in inside:
            continue
        for lo in range(a, b, chunk):
            hi = min(lo + chunk, b)
            bad = words[lo:hi] != sent
            if not bool(bad.any()):
                continue
            first = lo + int(bad.nonzero()[0][0] if not _is_torch(bad) else bad.nonzero()[0, 0])
            w0, w1 = max(0, first - WINDOW), min(lay.total, first + WINDOW)
            win = words[w0:w1]
            win = win.cpu().numpy() if _is_torch(win) else np.asarray(win)
            n_bad = int(bad.sum())
            in_win = [(s, c) for s, c, o in lay.chains() if o < w1 and o + lay.frames > w0]
            if not in_win:                      # far from every chain (the lead, where a sign-extended offset lands): no chain to name
                near = min(lay.chains(), key=lambda t: min(abs(first - t[2]), abs(first - t[2] - lay.frames)))
                raise GapDamage(f"{what}: layout {lay.name}, {n_bad} damaged word(s) in the gap [{a}, {b}) of the allocation, the first at "
                                f"element {first} (byte {4 * first:#x}), {first - near[2]:+d} from the start of the nearest chain "
                                f"(s={near[0]}, c={near[1]}): {' '.join(f'{int(v) & 0xFFFFFFFF:08x}' for v in win[first - w0:first - w0 + 4])}",
                                [(near[0], near[1], "far", first - near[2], n_bad)], 1)
            gaps_intact(win.view(np.uint32), lay.mask(w0, w1), sentinel,
                        f"{what}: layout {lay.name}, {n_bad} damaged word(s) in the gap [{a}, {b}) of the allocation, window [{w0}, {w1}) "
                        f"around the first one at element {first} (byte {4 * first:#x}; chains start at "
                        f"{[o for _, _, o in lay.chains()]}; the report counts the chains INSIDE the window, in address order: "
                        f"{in_win or 'none'})")
            raise AssertionError(f"{what}: damaged word at {first} not reported")      # (never: the window holds it)


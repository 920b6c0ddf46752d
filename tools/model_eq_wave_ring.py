#!/usr/bin/env python3
"""Lane-level CPU model of the wave-ring EQ (csrc/eq_ring64_body.hpp) with coefficient boundaries inside a launch.

64 lanes, one chain.  Band L (of nb <= 12 enabled bands, cascade order) has pre lane L and post lane L + 1; lanes 16 .. 63
are the conveyor (lane 63 - i holds sample 48 g + i of group g when it is injected).  Every step runs the kernel's six
operations on all lanes, in float32, every product and sum rounded by itself; `wave_ror:1` is np.roll(v, 1):

    O   X   = u0(ror 1) + s1            the band's output (a pass-on lane hands its neighbour's sample on: pb0 = 1, s1 = 0)
    T   t2  = u1(ror 1) + s2
    A   ao  = (a1, a2) * X
        [port, every 48th step: rows 1 .. 3 of X are stored, the next group's inputs injected]
    N   s1  = t2 - ao1 ;  s2 = b2x - ao2    (b2x: the PREVIOUS step's M)
    P   u   = (pb0, pb1) * X
    M   b2x = b2 * X(ror 1)

Steps count from 1; band L filters sample i in step i + L + 2 (O, T, A, N of its post lane L + 1).  The P that feeds that step
ran in step i + L + 1 on lane L, the M in step i + L + 1 on lane L + 1.

THE BOUNDARY RULE.  Sample B is the first one of a new table (`update_coefficients`: five new constants, s1 and s2 kept,
parametric_eq.rs:85-114).  Then, for lane l:

    a1, a2 (post lane of band l - 1)   new from the A of step B + l + 1
    pb0, pb1 (pre lane of band l)      new from the P of step B + l + 1
    b2 (post lane of band l - 1)       new from the M of step B + l

i.e. in step t the lane t - B - 1 takes its new (pb0, pb1, a1, a2) in front of A, and the lane t - B takes its new b2 in
front of M.  Lane 0 has no b2, so everything happens in steps B + 1 .. B + 13: for B a multiple of 512 (B mod 48 = 0, 16
or 32) these lie in ONE 48-step group, group B // 48.

check() compares the model's bits with the oracle's StereoParametricEQ, refreshed with set_band_coeffs in front of every
segment.  check_streams() does so for several chains with different band counts that follow different index rows (the
per-stream schedule of k_eq_ring_sched_streams: one chain per wave, every wave walks its own row, consecutive equal indices
are one run).  Run: python tools/model_eq_wave_ring.py
"""
import numpy as np

F = np.float32
LANES = 64
G = 48


def lane_constants(table):
    """table: float32 [nb][5] = {b0, b1, b2, a1, a2} of the enabled bands -> per-lane (pb0, pb1, b2, a1, a2), each [64]"""
    table = np.asarray(table, F).reshape(-1, 5)
    nb = table.shape[0]
    assert 1 <= nb <= 12
    pb0 = np.ones(LANES, F); pb1 = np.zeros(LANES, F)
    b2 = np.zeros(LANES, F); a1 = np.zeros(LANES, F); a2 = np.zeros(LANES, F)
    pb0[:nb] = table[:, 0]; pb1[:nb] = table[:, 1]
    b2[1:nb + 1] = table[:, 2]; a1[1:nb + 1] = table[:, 3]; a2[1:nb + 1] = table[:, 4]
    return [pb0, pb1, b2, a1, a2]


def ring_eq(x, tables, schedule, state=None):
    """One launch of the wave ring over x (float32 [n]).

    tables: list of [nb][5] coefficient tables (same nb); schedule: [(B, table index)], B ascending, the first entry at 0, the
    others inside (0, n); state: float32 [nb][2] (s1, s2) from the launch before (zeros if None).  Returns (y, new state)."""
    x = np.asarray(x, F)
    n = x.size
    nb = np.asarray(tables[0], F).reshape(-1, 5).shape[0]
    consts = [lane_constants(t) for t in tables]
    assert schedule[0][0] == 0
    c = [v.copy() for v in consts[schedule[0][1]]]
    bounds = list(schedule[1:])
    lane = np.arange(LANES)
    band = (lane >= 1) & (lane <= nb)
    conv = lane >= 16
    s_init = np.zeros((LANES, 2), F)
    if state is not None:
        s_init[1:nb + 1] = np.asarray(state, F)
    s_save = s_init.copy()

    def load_group(g):
        i = g * G + 63 - lane
        ok = conv & (i < n) & (i >= 0)
        out = np.zeros(LANES, F)
        out[ok] = x[i[ok]]
        return out

    y = np.zeros(n, F)
    X = np.where(conv, load_group(0), F(0)).astype(F)
    xnext = load_group(1)
    s1 = np.zeros(LANES, F); s2 = np.zeros(LANES, F)
    u0 = c[0] * X; u1 = c[1] * X                      # P
    b2x = c[2] * np.roll(X, 1)                        # M
    g_total = (n + 16 + G - 1) // G
    nxt = 0                                           # index of the boundary the ring meets next
    for stp in range(1, g_total * G + 1):
        g, k = divmod(stp - 1, G)
        while nxt < len(bounds) and stp > bounds[nxt][0] + 13:
            nxt += 1
        if nxt < len(bounds):
            B, ti = bounds[nxt]
            m = lane == stp - B - 1
            for q in (0, 1, 3, 4):
                c[q][m] = consts[ti][q][m]
        o = np.roll(u0, 1) + s1                       # O
        t2 = np.roll(u1, 1) + s2                      # T
        X = o
        ao1 = c[3] * o; ao2 = c[4] * o                # A
        if k == G - 1:                                # the port
            yi = g * G + 47 - lane
            ok = conv & (yi >= 0) & (yi < n)
            y[yi[ok]] = X[ok]
            X = np.where(conv, xnext, X).astype(F)
            xnext = load_group(g + 2)
        sn1 = t2 - ao1; sn2 = b2x - ao2               # N
        u0 = c[0] * X; u1 = c[1] * X                  # P
        if nxt < len(bounds):
            B, ti = bounds[nxt]
            m = lane == stp - B
            c[2][m] = consts[ti][2][m]
        b2x = c[2] * np.roll(X, 1)                    # M
        s1, s2 = sn1, sn2
        m = band & (lane == stp)                      # behind step L + 1: band L's first sample is next
        s1 = np.where(m, s_init[:, 0], s1); s2 = np.where(m, s_init[:, 1], s2)
        m = band & (lane == stp - n)                  # behind step n + L + 1: band L has filtered sample n - 1
        s_save[m, 0] = s1[m]; s_save[m, 1] = s2[m]
    return y, s_save[1:nb + 1].copy()


def oracle_eq(x, tables, schedule, fs=48000.0):
    """the oracle's StereoParametricEQ over x, set_band_coeffs for every band in front of every segment"""
    from oracle import ohs_oracle as orc
    x = np.asarray(x, F)
    nb = np.asarray(tables[0], F).reshape(-1, 5).shape[0]
    eq = orc.StereoParametricEQ(nb, fs)
    out = []
    edges = [b for b, _ in schedule] + [x.size]
    for (b, ti), e in zip(schedule, edges[1:]):
        for j in range(nb):
            eq.set_band_coeffs(j, np.asarray(tables[ti], F).reshape(-1, 5)[j], True)
        l = x[b:e].copy(); r = x[b:e].copy()
        eq.process_block(l, r)
        out.append(l)
    return np.concatenate(out)


def random_tables(rng, n_tables, nb, fs=48000.0):
    """stable peaking / shelving sections with all five constants different from table to table"""
    import open_headstage_amd as ohs
    tabs = []
    for _ in range(n_tables):
        t = np.zeros((nb, 5), F)
        for j in range(nb):
            t[j] = ohs.biquad_coefficients(int(rng.integers(0, 3)), fs, float(rng.uniform(40.0, 16000.0)),
                                           float(rng.uniform(0.4, 4.0)), float(rng.uniform(-9.0, 9.0)))
        tabs.append(t)
    return tabs


def check(nb, boundaries, n, n_tables=4, seed=0):
    """model == oracle, bit for bit, over two consecutive launches (state carried by the model's own state array)"""
    rng = np.random.default_rng(seed + 100 * nb)
    tabs = random_tables(rng, n_tables, nb)
    x = rng.standard_normal(2 * n).astype(F)
    sched = [(0, 0)] + [(b, (i + 1) % n_tables) for i, b in enumerate(boundaries)]
    last = sched[-1][1]
    sched2 = [(0, last)] + [(b, (last + i + 1) % n_tables) for i, b in enumerate(boundaries)]
    y1, st = ring_eq(x[:n], tabs, sched, None)
    y2, _ = ring_eq(x[n:], tabs, sched2, st)
    ref = oracle_eq(x, tabs, sched + [(n + b, t) for b, t in sched2])
    got = np.concatenate([y1, y2])
    return np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def row_schedule(row, seg_len, n, seg0=0, off0=0):
    """A stream's row of table indices (one per segment of seg_len samples) -> the schedule [(B, table)] of ONE launch of n
    samples that starts off0 samples into segment seg0.  Consecutive equal indices of the row are one run: the wave pays for
    the boundaries of its own row only (k_eq_ring_sched_streams)."""
    sched = [(0, int(row[seg0]))]
    B, seg = seg_len - off0, seg0 + 1
    while seg < len(row) and B < n:
        if int(row[seg]) != sched[-1][1]:
            sched.append((B, int(row[seg])))
        seg += 1
        B += seg_len
    return sched


def ring_eq_streams(xs, pools, rows, seg_len, states=None, seg0=0, off0=0):
    """One launch of the per-stream scheduled wave ring: chain c (one wave) filters xs[c] with the tables of pools[c] -- every
    chain its own number of bands -- along its own index row rows[c].  states: per chain [nb_c][2] or None.  -> (ys, states)"""
    ys, out_states = [], []
    for c, x in enumerate(xs):
        y, st = ring_eq(x, pools[c], row_schedule(rows[c], seg_len, len(x), seg0, off0), None if states is None else states[c])
        ys.append(y)
        out_states.append(st)
    return ys, out_states


def check_streams(band_counts, rows1, rows2, seg_len=512, n_tables=4, seed=0):
    """model == oracle, bit for bit, for chains with different band counts on different index rows over two consecutive launches
    (rows1, rows2: [chains][segments of the launch]); the oracle EQ of every chain is refreshed in front of EVERY segment"""
    rng = np.random.default_rng(seed)
    n1, n2 = len(rows1[0]) * seg_len, len(rows2[0]) * seg_len
    pools = [random_tables(rng, n_tables, nb) for nb in band_counts]
    xs = [rng.standard_normal(n1 + n2).astype(F) for _ in band_counts]
    y1, st = ring_eq_streams([x[:n1] for x in xs], pools, rows1, seg_len)
    y2, _ = ring_eq_streams([x[n1:] for x in xs], pools, rows2, seg_len, st)
    ok = True
    for c, x in enumerate(xs):
        every = [(k * seg_len, int(t)) for k, t in enumerate(list(rows1[c]) + list(rows2[c]))]
        ref = oracle_eq(x, pools[c], every)
        got = np.concatenate([y1[c], y2[c]])
        ok = ok and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    return ok


if __name__ == "__main__":
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for nb in range(1, 13):
        ok = check(nb, [512, 1024, 1536, 2560], 3072)
        print(f"{nb:2d} bands, boundaries at 512 1024 1536 2560 (mod 48: 32 16 0 16): {'bit-exact' if ok else 'MISMATCH'}")
        assert ok
    ok = check_streams([10, 7, 12], [[0, 1, 1, 2, 2, 2], [3, 3, 0, 0, 1, 2], [1, 2, 3, 0, 1, 2]],
                       [[2, 2, 3, 3, 0, 0], [0, 1, 1, 1, 1, 3], [3, 2, 1, 0, 3, 2]])
    print(f"three chains (10, 7, 12 bands) on their own index rows, two launches: {'bit-exact' if ok else 'MISMATCH'}")
    assert ok

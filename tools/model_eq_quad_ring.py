#!/usr/bin/env python3
"""Lane-level CPU model of the quad form of the wave-ring EQ: one band per aligned quad of lanes, FOUR VOP2+DPP instructions
per sample instead of the six of csrc/eq_ring64_body.hpp (modelled in tools/model_eq_wave_ring.py).

64 lanes, one chain.  Band k (of nb <= 12 enabled bands, cascade order) owns quad k = lanes 4k .. 4k+3 = (a, b, c, d); quads
nb .. 11 pass samples on; quads 12 .. 15 are the conveyor that the I/O port serves.  Per lane: Z0 / Z1 (alternating by step
parity), Zp, G, P and the constants C1, C2; per quad of a band C1 = (1, 1, a2, a1), C2 = (b2, b1, b0, 1), of a pass-on or
conveyor quad C1 = (1, 1, 0, 0), C2 = (0, 0, 1, 1).  A step (Zc = Z[step & 1], Zo = the other one), every result float32:

    alpha   Zc = Zp(wave_ror:1) + G             a: x = y of the quad in front + 0   b: m2 + 0   c: t = m1 + s2   d: y = m0 + s1
    delta   Zp = Zo(quad_perm 0,0,0,3) * C2     a: m2 = b2 x   b: m1 = b1 x   c: m0 = b0 x   d: 1.0 y  (the next quad's a takes it)
    <slot>  one issue slot that the DPP hazard leaves free: the port's instructions go here; a slot with nothing to carry
            holds a no-op or (group_program's fill) F = F(quad_perm 0,1,2,3) & F on a register that nothing else reads
    beta    P  = Zc(quad_perm 0,0,3,3) * C1     a, b: 1.0 x   c: p2 = a2 y   d: p1 = a1 y
    gamma   G  = Zc(quad_perm 0,0,1,2) - P      a, b: x - x = 0   c: s2' = m2 - p2   d: s1' = t - p1

This is the oracle's order (out = s1 + b0 x; s1 = s2 + b1 x - a1 out; s2 = b2 x - a2 out), s1 in G of lane d, s2 in G of
lane c.  A quad has a latency of four steps and four samples in flight; in a pass-on quad a sample goes a -> c -> d.

Timeline (steps count from 1): sample i is in Zc of lane 0 at step i + 1, in lane a of quad q at step i + 1 + 4q, in its lane
d (filtered, if the quad is a band) at step i + 3 + 4q.  The ring is 64 steps round.

The port.  Samples of even and of odd index never share a register: behind alpha of step m, Zc holds in lanes a and d of
the conveyor quads the eight outputs m - 49, m - 51 .. m - 63, and behind delta of step m + 1 those eight sit in lanes c
and d of Zp, where alpha of step m + 2 .. picks them up.  So a group is 16 steps and has two half ports:
    step 16g + 8    store B: lanes a, d of Zc               step 16g + 9   inject B: lanes c, d of Zp <- lanes a, b of x
    step 16g + 15   store A (of group g + 1)                step 16g + 16  inject A (of group g + 1): <- lanes c, d of x
    step 16g + 10   load x <- the 16 inputs of group g + K  step 16g + 14  wait for the x of group g + 1
(the inject is a v_cndmask with a quad_perm on x; DPP's bank_mask selects quads of a row, not lanes of a quad)
An inject at step n puts sample n + 60 - 4q into lane d and n + 62 - 4q into lane c of conveyor quad q (q = 12 .. 15); the x
register of group g holds, in quad q, (a, b, c, d) = samples 16g + (71, 69, 62, 60) - 4q.  Outputs leave 64 samples behind
the inputs that replace them, and an input is requested K groups before it is injected (K registers in rotation).
All port instructions sit in the free slots of different steps; the inject writes Zp two instructions (beta, gamma) ahead of
the alpha that reads it through DPP.

Head and tail.  The ring starts at zero one group early (step -15; nothing of it depends on a sample before the first: an
input that does not exist is a zero).  Band k's state of the launch before goes into G of its lanes c, d behind step
4k + 2, one step before its first sample's sums; it is taken out behind step n + 4k + 2, in which the band has filtered
sample n - 1.  The ring runs on zeros until the last output has been stored.

Where the port's memory instructions issue (group_program's `port`).  By default each of a group's two stores and its load
stands alone in the slot of its step (8, 15; 10).  The cluster variants C1 / C2 / C3 issue them behind one another -- a
vector-memory instruction alone between VALU instructions costs the wave about 8 ticks beyond its slot, one directly behind
another next to nothing -- and change nothing else: a store waits in a holding register, the load
issues up to 21 steps later, behind the inject B that consumed its register, with its deadline (the wait K - 1 groups on)
unchanged.  In-place safety: stores only move LATER, and so does the load, which is requested K groups before its samples'
outputs exist -- so a store never passes the load of the sample whose address it takes.  Ring(in_place=True) runs a launch
on one array and refuses a load of an address that a store has written.

The merged variants D1 / D2 / D1W / D2W issue FEWER memory instructions for the same bytes (the loop pays per instruction):
    D1   one store per group.  Step 8 parks Zc in H0 ("hold"), step 10's slot moves H0's lanes a, d to lanes b, c ("qmove":
         v_mov_b32_dpp quad_perm 0,0,3,3), step 15's slot takes Zc's lanes a, d into H0 ("merge": v_cndmask under a constant
         SGPR-pair mask -- a plain read of Zc, VCC stays the injects'), and one store ("mstore") carries the group's 16
         outputs, lanes b, c at the addresses of lanes a, d seven samples earlier.  Store and load issue in the NEXT group's
         step-1 slot; an iteration's last group issues its own in step 16 behind inject A.
    D2   one store and one load per two groups.  "xhalf" is v_permlane32_swap vdst, src: lanes 32 .. 63 of vdst change
         places with lanes 0 .. 31 of src.  With vdst = the even group's merged H0 and src = the odd group's H1, H1 holds the
         even group's outputs in row 1 and its own in row 3: one "pstore".  One "pload" fetches the even group's inputs into
         row 1 and the odd group's into row 3 of X; xhalf S, X brings row 1 to row 3 of S for the even group's injects.
    D1W / D2W   the same with the wait (and its 4-byte partner) directly in front of the cluster's memory instructions
         instead of in step 14's slot, which then carries nothing.
No holding register is live across the end of an iteration in any of them.  check_waits() walks the loop with the memory
instructions in flight and fails where an inject or an exchange reads a register whose load the waits have not covered.

hazards() walks the steady-state loop and gives, per DPP read, the distance in issue slots to the register's last VALU
writer; check_hazards() fails below 2 (gfx9 / CDNA: two wait states between a VALU write and a DPP read of a VGPR; the
same between a VALU write of either operand and a v_permlane32_swap).

Run: python tools/model_eq_quad_ring.py
"""
import numpy as np

F = np.float32
LANES = 64
G = 16                       # steps (= samples) per group
Q0 = 12                      # first conveyor quad
K_DEFAULT = 8                # groups between an input's request and its injection = x registers
LOOP_OWN_SLOTS = (11, 12)    # steps of an iteration's last group whose slot carries the loop's own instructions
TINY = np.finfo(F).tiny

_lane = np.arange(LANES)


def _perm(p):
    return (_lane & ~3) + np.asarray(p)[_lane & 3]


QP_DELTA, QP_BETA, QP_GAMMA = _perm([0, 0, 0, 3]), _perm([0, 0, 3, 3]), _perm([0, 0, 1, 2])
QP_INJECT = {"A": _perm([0, 1, 2, 3]), "B": _perm([0, 1, 0, 1])}
ROLE = _lane & 3             # 0 .. 3 = a .. d
QUAD = _lane >> 2
CONV = QUAD >= Q0
INJECT_LANES = CONV & (ROLE >= 2)
STORE_LANES = CONV & ((ROLE == 0) | (ROLE == 3))
X_SAMPLE = np.array([71, 69, 62, 60])[ROLE] - 4 * QUAD      # sample index of an x register's lane, from 16 g
STORE_SAMPLE = np.array([-1, 0, 0, -3])[ROLE] - 4 * QUAD    # sample index a store at step m finds in Zc, from m


def lane_constants(table):
    """table: float32 [nb][5] = {b0, b1, b2, a1, a2} of the enabled bands -> (C1, C2), each [64]"""
    table = np.asarray(table, F).reshape(-1, 5)
    nb = table.shape[0]
    assert 1 <= nb <= 12
    c1 = np.tile(np.array([1, 1, 0, 0], F), 16)
    c2 = np.tile(np.array([0, 0, 1, 1], F), 16)
    for k in range(nb):
        b0, b1, b2, a1, a2 = table[k]
        c1[4 * k:4 * k + 4] = (1, 1, a2, a1)
        c2[4 * k:4 * k + 4] = (b2, b1, b0, 1)
    return c1, c2


PORTS = (None, "C1", "C2", "C3", "D1", "D2", "D1W", "D2W")    # where and how the port's memory instructions issue (group_program)
HOLD = ("H0", "H1", "H2")           # holding registers of the cluster variants: a parked store's value
MERGED_PORTS = ("D1", "D1W")        # one store per group: both half ports' outputs merged in one register
PAIR_PORTS = ("D2", "D2W")          # one store and one load per two groups: two groups' registers exchanged by halves
WAIT_IN_CLUSTER = ("D1W", "D2W")    # the wait stands in front of the cluster's memory instructions, not in step 14's slot
ROW = _lane >> 4
MERGE_LANES = (ROLE == 0) | (ROLE == 3)     # the merge takes Zc here and keeps the holding register's lanes b, c
# a merged store behind step m (a group's step 15): lanes a, d hold step m's outputs, lanes b, c those of step m - 7
MSTORE_SAMPLE = np.array([-1, -8, -10, -3])[ROLE] - 4 * QUAD
# a pair's store behind step m (the odd group's step 15): row 3 as the merged store, row 1 what lane + 32 held 16 steps before
PAIR_LANES = (ROW == 1) | (ROW == 3)
PSTORE_SAMPLE = np.where(ROW == 3, MSTORE_SAMPLE, MSTORE_SAMPLE[(_lane + 32) % LANES] - G)
# a pair's load for the groups (e, e + 1), from 16 e: row 3 the inputs of group e + 1, row 1 those of group e as lane + 32 takes them
PX_SAMPLE = np.where(ROW == 3, X_SAMPLE + G, X_SAMPLE[(_lane + 32) % LANES])


def _memory_slots(g, K, port):
    """{s: instructions} of the slots of group g that carry the port's memory instructions, and of those the cluster
    variants leave empty.  A parked store keeps the step its value belongs to: ("store", that step, holding register)."""
    t = G * g
    x, xb = f"x{g % K}", f"x{(g - 1) % K}"
    if port is None:
        return {8: [("store", t + 8, "Z0")], 10: [("load", t + 10, x, g + K)], 15: [("store", t + 15, "Z1")]}
    if port == "C1":        # the load of the group before waits for this group's first store
        return {8: [("store", t + 8, "Z0"), ("load", t + 8, xb, g - 1 + K)], 10: [], 15: [("store", t + 15, "Z1")]}
    if port == "C2":        # one cluster per group: the first store's value waits in H0
        return {8: [("hold", t + 8, "H0", "Z0")], 10: [],
                15: [("store", t + 8, "H0"), ("store", t + 15, "Z1"), ("load", t + 15, x, g + K)]}
    assert port == "C3" and K % 2 == 0, (port, K)
    if g % 2 == 0:          # one cluster per two groups: the even group parks both of its values ...
        return {8: [("hold", t + 8, "H0", "Z0")], 10: [], 15: [("hold", t + 15, "H1", "Z1")]}
    return {8: [("hold", t + 8, "H2", "Z0")], 10: [],          # ... the odd one its first, and issues all six
            15: [("store", t - 8, "H0"), ("store", t - 1, "H1"), ("store", t + 8, "H2"), ("store", t + 15, "Z1"),
                 ("load", t + 15, xb, g - 1 + K), ("load", t + 15, x, g + K)] + ([("nop", t + 15)] if (g + 1) % K == 0 else [])}


def _merged_slots(g, K, port):
    """{s: instructions} of every slot of group g that carries something, for the variants D1 / D1W / D2 / D2W"""
    t = G * g
    first, last = g % K == 0, (g + 1) % K == 0
    inside = port in WAIT_IN_CLUSTER
    if port in MERGED_PORTS:
        x, xn, xb = f"x{g % K}", f"x{(g + 1) % K}", f"x{(g - 1) % K}"
        slots = {8: [("hold", t + 8, "H0", "Z0")], 9: [("inject", t + 9, "B", x)], 10: [("qmove", t + 10, "H0")],
                 15: [("merge", t + 15, "H0", "Z1")], 16: [("inject", t + 16, "A", xn)]}
        if not inside:
            slots[14] = [("wait", t + 14, xn), ("nop4", t + 14)]
        if not first:       # the group before's store and load
            slots[1] = ([("wait", t + 1, xn), ("nop4", t + 1)] if inside else []) + [("mstore", t - 1, "H0"), ("load", t + 1, xb, g - 1 + K)]
        if last:            # ... but the last group's own: no holding register is live across the end of an iteration
            slots[16] += (([("wait", t + 16, f"x{(g + 2) % K}"), ("nop4", t + 16)] if inside else []) +
                          [("mstore", t + 15, "H0"), ("load", t + 16, x, g + K)])
        return slots
    assert port in PAIR_PORTS and K % 2 == 0, (port, K)
    # (the wait in front of a cluster cannot cover that cluster's own load: with two registers in rotation it would have to)
    assert not inside or K >= 6, (port, K)
    K2 = K // 2
    j = (g % K) // 2
    X, Xn, Xb = f"X{j}", f"X{(j + 1) % K2}", f"X{(j - 1) % K2}"
    if g % 2 == 0:          # the even group: its inputs are in S, its merged outputs wait in H0 for the odd group's
        slots = {8: [("hold", t + 8, "H0", "Z0")], 9: [("inject", t + 9, "B", "S")], 10: [("qmove", t + 10, "H0")],
                 15: [("merge", t + 15, "H0", "Z1")], 16: [("inject", t + 16, "A", X)]}
        if not first:       # the pair before's: H1 takes H0's row 3 into its row 1; one store, one load for two groups
            slots[1] = [("xhalf", t + 1, "H0", "H1")]
            slots[2] = ([("wait", t + 2, Xn), ("nop4", t + 2)] if inside else []) + [("pstore", t - 1, "H1"), ("pload", t + 2, Xb, g - 2 + K)]
        return slots
    slots = {8: [("hold", t + 8, "H1", "Z0")], 9: [("inject", t + 9, "B", X)], 10: [("qmove", t + 10, "H1")],
             14: ([] if inside else [("wait", t + 14, Xn), ("nop4", t + 14)]) + [("xhalf", t + 14, "S", Xn)],   # S: the next even group's inputs
             15: [("merge", t + 15, "H1", "Z1")], 16: [("inject", t + 16, "A", "S")]}
    if last:                # (the store offsets' advance goes behind the last cluster: the slot's ("nop", step))
        slots[16] += ([("xhalf", t + 16, "H0", "H1")] + ([("wait", t + 16, f"X{(j + 2) % K2}"), ("nop4", t + 16)] if inside else []) +
                      [("pstore", t + 15, "H1"), ("pload", t + 16, X, g - 1 + K), ("nop", t + 16)])
    return slots


def group_program(g, K=K_DEFAULT, fill=False, port=None):
    """The instructions of group g (steps 16g + 1 .. 16g + 16) in issue order: (op, step, ...).  fill: a slot that carries
    nothing holds ("fill", step, "F") -- a VOP2+DPP instruction on a register F of its own, which keeps the vector unit for
    the step instruction's four cycles where a no-op lets a wave beside this one issue -- instead of ("nop", step).  (The
    experiments build's second loop; the product's has the no-ops: DESIGN.md 4.5, round 12.)  The two
    slots of an iteration's last group that carry the loop's own offset advances (steps 11 and 12) stay ("nop", step).

    port: where the two stores and the load issue.  None: each alone in the slot of its step (8, 10, 15).  The cluster
    variants put them behind one another, because a vector-memory instruction that stands alone between VALU instructions
    costs the wave about 12 cycles and one directly behind another about 4:
        "C1"  the load waits for step 8's store (of the next group): a pair and a lone store, 82 slots per group
        "C2"  step 8 parks Zc in the holding register H0 (("hold", step, "H0", Zc): a plain VALU move, no DPP, no hazard);
              step 15 issues store H0, store Zc, load x back to back: 83 slots, one cluster per group
        "C3"  groups in pairs (K even): the even group parks both values (H0, H1), the odd one its first (H2), and the odd
              group's step 15 issues four stores and two loads: 167 slots per two groups; in an iteration's last group the
              cluster is followed by the slot's ("nop", step): the store offsets' advance goes there, behind the stores
    Nothing else moves: same ring, same lanes, same injects.  A load only moves LATER, to a slot behind the inject B (step 9
    of its own or of the group before) that consumed its register, and its deadline -- the wait at step 14, K - 1 or K - 2
    groups on -- stays; wait_count(K, port) is the wait's new vmcnt.  A store only moves LATER as well, so it never passes
    the load of the sample whose place it takes (in place: an input is read K groups before it is injected, its output is
    stored 64 samples behind that) -- tests/test_cpu_eq_quad_port_cluster.py runs the launch on one array.  No holding
    register is live across the end of an iteration (K even), so the launch's C++ head and tail stay what they are."""
    prog = []
    own = (g + 1) % K == 0
    merged = _merged_slots(g, K, port) if port in MERGED_PORTS + PAIR_PORTS else None
    mem = _memory_slots(g, K, port) if merged is None else {}
    for s in range(1, G + 1):
        step = G * g + s
        zc, zo = f"Z{step & 1}", f"Z{(step - 1) & 1}"
        prog += [("alpha", step, zc), ("delta", step, zo)]
        if merged is not None:
            prog += merged.get(s) or [("fill", step, "F") if fill and not (own and s in LOOP_OWN_SLOTS) else ("nop", step)]
        elif mem.get(s):
            prog += mem[s]
        elif s == 9:
            prog.append(("inject", step, "B", f"x{g % K}"))
        elif s == 14:
            prog += [("wait", step, f"x{(g + 1) % K}"), ("nop4", step)]
        elif s == 16:
            prog.append(("inject", step, "A", f"x{(g + 1) % K}"))
        elif fill and not (own and s in LOOP_OWN_SLOTS):
            prog.append(("fill", step, "F"))
        else:
            prog.append(("nop", step))
        prog += [("beta", step, zc), ("gamma", step, zc), ("state", step)]
    return prog


def _program(g, K, fill=False, port=None):
    """group_program with the arguments it had before `port` wherever the port is the default one"""
    if port is not None:
        return group_program(g, K, fill, port=port)
    return group_program(g, K, True) if fill else group_program(g, K)


LOADS = ("load", "pload")
MEMORY = ("load", "store", "mstore", "pstore", "pload")


def wait_count(K=K_DEFAULT, port=None):
    """vmcnt of a group's wait: the memory instructions issued behind the load it waits for (they retire in issue order).
    Where the groups of a pair differ (C3), the smaller count: it is right for one and waits a little longer in the other."""
    prog = [i for g in range(0, 2 * K + 2) for i in _program(g, K, port=port)]
    counts = []
    waits = [j for j, i in enumerate(prog) if i[0] == "wait"]
    # (the merged variants: every wait of an iteration -- the last group's stands elsewhere than the others')
    for at in waits[-2:] if port not in MERGED_PORTS + PAIR_PORTS else [j for j in waits if prog[j][1] > G * (K + 2)]:
        reg = prog[at][2]
        ld = max(j for j, i in enumerate(prog[:at]) if i[0] in LOADS and i[2] == reg)
        counts.append(sum(1 for i in prog[ld + 1:at] if i[0] in MEMORY))
    return min(counts)


def check_waits(K=K_DEFAULT, port=None, count=None):
    """Walks the steady-state loop with the memory instructions in flight (they retire in issue order; a wait leaves the
    last `count` -- wait_count(K, port) -- of them) and fails where an inject or a half exchange reads a register whose
    load has not been waited for.  -> the number of reads checked"""
    count = wait_count(K, port) if count is None else count
    flight, reads = [], 0
    for g in range(0, 4 * K):
        for i in _program(g, K, port=port):
            if i[0] in MEMORY:
                flight.append(i[2] if i[0] in LOADS else None)
            elif i[0] == "wait":
                flight = flight[max(0, len(flight) - count):] if count else []
            elif i[0] in ("inject", "xhalf") and g >= 2 * K:
                for reg in ((i[3],) if i[0] == "inject" else i[2:4]):
                    assert reg not in flight, (i, "reads a register whose load is still in flight")
                    reads += 1
    return reads


def hazards(K=K_DEFAULT, extra=(), fill=False, port=None):
    """(reader, step, register, distance) for every DPP read of the steady-state loop: distance = issue slots between the
    register's last VALU write and the read.  `extra`: instructions (op, dpp-read register, written register) put behind the
    last step of every K groups (the loop's own: offset advances, counter).  fill: the program with the fill instruction."""
    prog = []
    for g in range(2 * K, 4 * K):
        prog += [i for i in _program(g, K, fill, port) if i[0] != "state"]
        if (g + 1) % K == 0:
            prog += list(extra)
    last_write, out = {}, []
    for pos, ins in enumerate(prog):
        op = ins[0]
        dpp_read = write = None
        if op == "alpha": dpp_read, write = "Zp", ins[2]
        elif op == "delta": dpp_read, write = ins[2], "Zp"
        elif op == "beta": dpp_read, write = ins[2], "P"
        elif op == "gamma": dpp_read, write = ins[2], "G"
        elif op == "inject": dpp_read, write = ins[3], "Zp"        # (x is written by a load: the wait covers it)
        elif op == "fill": dpp_read, write = ins[2], ins[2]
        elif op == "valu": dpp_read, write = ins[1], ins[2]
        elif op == "hold": write = ins[2]                          # (a plain VALU read of Zc: no wait states needed)
        elif op == "qmove": dpp_read, write = ins[2], ins[2]       # v_mov_b32_dpp on the holding register
        elif op == "merge": write = ins[2]                         # (v_cndmask under an SGPR mask: plain reads)
        elif op == "xhalf":
            # v_permlane32_swap: a VALU write of EITHER operand needs two wait states before it, as a DPP read does; it
            # writes both (a register that a load wrote is the wait's business: check_waits)
            for reg in ins[2:4]:
                if reg in last_write and pos >= len(prog) // 2:
                    out.append((op, ins[1], reg, pos - last_write[reg] - 1))
                last_write[reg] = pos
        if dpp_read is not None and dpp_read in last_write and pos >= len(prog) // 2:     # (the second pass: all writers seen)
            out.append((op, ins[1], dpp_read, pos - last_write[dpp_read] - 1))
        if write is not None:
            last_write[write] = pos
    return out


def check_hazards(K=K_DEFAULT, verbose=False, fill=False, port=None):
    worst = {}
    for op, step, reg, d in hazards(K, fill=fill, port=port):
        key = (op, reg[:1] if reg.startswith("Z") and reg != "Zp" else reg)
        worst[key] = min(worst.get(key, 99), d)
    for (op, reg), d in sorted(worst.items()):
        if verbose:
            print(f"  {op:6s} reads {reg:3s} through DPP: {d} issue slots behind its last VALU write")
        assert d >= 2, (op, reg, d)
    return worst


def _flush(v):
    return np.where(np.abs(v) < TINY, np.copysign(F(0), v), v).astype(F)


class Ring:
    """the registers of one wave and the interpreter of group_program's instructions"""

    def __init__(self, x, table, state=None, K=K_DEFAULT, mode=0, in_place=False):
        self.x = np.array(x, F)
        self.n = self.x.size
        tab = np.asarray(table, F).reshape(-1, 5)
        self.nb = tab.shape[0]
        self.C1, self.C2 = lane_constants(tab)
        self.K, self.mode = K, mode
        self.r = {k: np.zeros(LANES, F) for k in ["Z0", "Z1", "Zp", "G", "P"]}
        self.r["F"] = np.zeros(LANES, np.uint32)        # the fill's own register
        self.r.update({h: np.zeros(LANES, F) for h in HOLD})
        self.r.update({k: np.zeros(LANES, F) for k in ["S"] + [f"X{j}" for j in range(K // 2)]})   # the pair variants' inputs
        # in place the outputs go where the inputs are: load() then refuses an address that a store has written
        self.y = self.x if in_place else np.zeros(self.n, F)
        self.stored = np.zeros(self.n, np.int32)
        for g in range(-1, K - 1):
            self.r[f"x{g % K}"] = self.load(g)
        self.s_init = np.zeros((self.nb, 2), F) if state is None else np.asarray(state, F).reshape(self.nb, 2).copy()
        self.s_save = self.s_init.copy()

    def load(self, g):
        i = G * g + X_SAMPLE
        ok = CONV & (i >= 0) & (i < self.n)
        v = np.zeros(LANES, F)
        v[ok] = self.x[i[ok]]
        assert self.y is not self.x or not self.stored[i[ok]].any(), "an input is read after a store to its address"
        return v

    def pload(self, e):
        """a pair's load: row 1 the inputs of group e, row 3 those of group e + 1"""
        i = G * e + PX_SAMPLE
        ok = PAIR_LANES & (i >= 0) & (i < self.n)
        v = np.zeros(LANES, F)
        v[ok] = self.x[i[ok]]
        assert self.y is not self.x or not self.stored[i[ok]].any(), "an input is read after a store to its address"
        return v

    def op(self, f, a, b):
        # MODE.FP_DENORM (kernels.h, ohs_set_fp_mode): mode 1 flushes results, mode 2 operands as well
        if self.mode == 2:
            a, b = _flush(a), _flush(b)
        with np.errstate(invalid="ignore"):
            v = f(a, b).astype(F)
        return _flush(v) if self.mode else v

    def run(self, prog):
        r = self.r
        for ins in prog:
            o, step = ins[0], ins[1]
            if o == "alpha":
                r[ins[2]] = self.op(np.add, np.roll(r["Zp"], 1), r["G"])
            elif o == "delta":
                r["Zp"] = self.op(np.multiply, r[ins[2]][QP_DELTA], self.C2)
            elif o == "beta":
                r["P"] = self.op(np.multiply, r[ins[2]][QP_BETA], self.C1)
            elif o == "gamma":
                r["G"] = self.op(np.subtract, r[ins[2]][QP_GAMMA], r["P"])
            elif o == "store":
                i = step + STORE_SAMPLE
                ok = STORE_LANES & (i >= 0) & (i < self.n)
                self.y[i[ok]] = r[ins[2]][ok]
                self.stored[i[ok]] += 1
            elif o in ("mstore", "pstore"):     # one store for both half ports / for two groups
                i = step + (MSTORE_SAMPLE if o == "mstore" else PSTORE_SAMPLE)
                ok = (CONV if o == "mstore" else PAIR_LANES) & (i >= 0) & (i < self.n)
                self.y[i[ok]] = r[ins[2]][ok]
                self.stored[i[ok]] += 1
            elif o == "hold":
                r[ins[2]] = r[ins[3]].copy()
            elif o == "qmove":                  # lanes a, d of the parked value go to lanes b, c
                r[ins[2]] = r[ins[2]][QP_BETA]
            elif o == "merge":                  # lanes a, d take Zc, lanes b, c keep the parked value
                r[ins[2]] = np.where(MERGE_LANES, r[ins[3]], r[ins[2]]).astype(F)
            elif o == "xhalf":                  # lanes 32 .. 63 of the first change places with lanes 0 .. 31 of the second
                a, b = r[ins[2]].copy(), r[ins[3]].copy()
                a[32:], b[:32] = r[ins[3]][:32], r[ins[2]][32:]
                r[ins[2]], r[ins[3]] = a, b
            elif o == "pload":
                r[ins[2]] = self.pload(ins[3])
            elif o == "inject":
                r["Zp"] = np.where(INJECT_LANES, r[ins[3]][QP_INJECT[ins[2]]], r["Zp"]).astype(F)
            elif o == "load":
                r[ins[2]] = self.load(ins[3])
            elif o == "fill":
                r[ins[2]] = r[ins[2]][_perm([0, 1, 2, 3])] & r[ins[2]]
            elif o == "state":
                for k in range(self.nb):
                    if step == 4 * k + 2:
                        r["G"][4 * k + 3], r["G"][4 * k + 2] = self.s_init[k]
                    if step == self.n + 4 * k + 2:
                        self.s_save[k] = (r["G"][4 * k + 3], r["G"][4 * k + 2])


def n_groups(n):
    """groups -1 .. n_groups(n) - 1 run: the last output, sample n - 1, is stored by step n + 62 at the latest"""
    return (n + 62 + G - 1) // G


def ring_eq(x, table, state=None, K=K_DEFAULT, mode=0, fill=False, port=None, in_place=False):
    """One launch over x (float32 [n]) -> (y, new state [nb][2] = (s1, s2)); fill: the program with the fill instruction;
    port: the whole launch in that variant's program (C3: to the end of a pair of groups); in_place: on one array"""
    ring = Ring(x, table, state, K, mode, in_place)
    last = n_groups(ring.n)
    first = -1
    if port in MERGED_PORTS:        # a group's store issues in the group behind it
        last += 1
    elif port in PAIR_PORTS:        # whole pairs from an even group on, and the last pair's store issues in the pair behind it
        first, last = -2, last + last % 2 + 2
        ring.r["S"] = ring.load(-2)
        for p in range(-1, K // 2 - 1):
            ring.r[f"X{p % (K // 2)}"] = ring.pload(2 * p)
    for g in range(first, last + (last % 2 if port == "C3" else 0)):
        ring.run(_program(g, K, fill, port))
    assert np.all(ring.stored == 1), "every output is stored exactly once"
    return ring.y, ring.s_save


def oracle_eq(x, table, sizes, mode=0, fs=48000.0):
    """the oracle's StereoParametricEQ over x, one process_block per entry of sizes"""
    from oracle import ohs_oracle as orc
    tab = np.asarray(table, F).reshape(-1, 5)
    eq = orc.StereoParametricEQ(tab.shape[0], fs)
    for j in range(tab.shape[0]):
        eq.set_band_coeffs(j, tab[j], True)
    out, o = [], 0
    for n in sizes:
        l = np.asarray(x[o:o + n], F).copy(); r = l.copy()
        if mode:
            with orc.flush_denormals(mode):
                eq.process_block(l, r)
        else:
            eq.process_block(l, r)
        out.append(l)
        o += n
    return np.concatenate(out)


def random_table(rng, nb, fs=48000.0):
    import open_headstage_amd as ohs
    t = np.zeros((nb, 5), F)
    for j in range(nb):
        t[j] = ohs.biquad_coefficients(int(rng.integers(0, 3)), fs, float(rng.uniform(40.0, 16000.0)),
                                       float(rng.uniform(0.4, 4.0)), float(rng.uniform(-9.0, 9.0)))
    return t


def model_launches(x, table, sizes, K=K_DEFAULT, mode=0, fill=False):
    out, st, o = [], None, 0
    for n in sizes:
        y, st = ring_eq(x[o:o + n], table, st, K, mode, fill)
        out.append(y)
        o += n
    return np.concatenate(out)


def check(nb, sizes, seed=0, K=K_DEFAULT, mode=0, x=None):
    """model == oracle over consecutive launches of the given sizes (the state handed over by the model's own array): bit for
    bit in mode 0; in the flushing modes equal as numbers, differing bits only where both are zero (include/ohs_hip.h)"""
    rng = np.random.default_rng(seed + 100 * nb)
    tab = random_table(rng, nb)
    if x is None:
        x = rng.standard_normal(sum(sizes)).astype(F)
    got = model_launches(x, tab, sizes, K, mode)
    ref = oracle_eq(x, tab, sizes, mode)
    if mode == 0:
        return np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    d = got.view(np.uint32) != ref.view(np.uint32)
    return np.array_equal(got, ref) and bool(np.all(got[d] == 0.0) and np.all(ref[d] == 0.0))


def check_zero_corners(nb=10, n=3000, seed=5):
    """zeros and -0.0 in the input: equal as numbers everywhere, bit-exact wherever the oracle's output is not a zero, and a
    zero of the model that differs is +0.0 for the oracle's -0.0 (never the reverse)"""
    rng = np.random.default_rng(seed)
    tab = random_table(rng, nb)
    x = rng.standard_normal(n).astype(F)
    x[200:300] = -0.0
    x[700:900] = 0.0
    x[1500:] = -0.0
    got, ref = model_launches(x, tab, [n]), oracle_eq(x, tab, [n])
    d = got.view(np.uint32) != ref.view(np.uint32)
    return np.array_equal(got, ref) and bool(np.all(ref[d] == 0.0) and np.all(np.signbit(ref[d])) and not np.any(np.signbit(got[d])))


def check_nonfinite_reach(nb=10, n=6000, k=3001, seed=6):
    """a non-finite input sample k: bit-exact up to sample k - 64, non-finite from k on (include/ohs_hip.h: up to 64 early)"""
    rng = np.random.default_rng(seed)
    tab = random_table(rng, nb)
    ok = True
    for bad in (np.nan, np.inf):
        for kk in range(k, k + 16):
            x = rng.standard_normal(n).astype(F)
            x[kk] = bad
            got, ref = model_launches(x, tab, [n]), oracle_eq(x, tab, [n])
            ok = ok and np.array_equal(got[:kk - 64].view(np.uint32), ref[:kk - 64].view(np.uint32)) and not np.any(np.isfinite(got[kk:]))
    return ok


# ---- the launch as csrc/eq_quad_ring_body.hpp runs it: the C++ form around an interpreter of the generated asm TEXT ----------

def run_asm(lines, v, x, y, stored, n, iters, merge_lanes=None):
    """`iters` iterations of the generated loop (tools/gen_eq_quad_ring_asm.py: loop_asm) on the register file v (v[k]: 64
    lanes; uint32 for the offsets v0, v1, v9, v10, float32 elsewhere).  Buffer accesses are range-checked against 4 n as the
    hardware checks a raw buffer: VGPR offset + instruction offset >= num_records is dropped / reads 0.  VCC = every lane
    but c, d of the conveyor quads; %[mk], the merge's SGPR-pair mask = merge_lanes (MERGE_LANES).  Memory instructions
    retire in issue order and s_waitcnt vmcnt(N) leaves the last N in flight: an inject or a half exchange that reads a
    register whose load is still in flight is refused."""
    import re
    vcc = ~INJECT_LANES
    mk = MERGE_LANES if merge_lanes is None else merge_lanes
    flight = []             # the memory instructions in flight: the register a load writes, None for a store
    ops = {"v_add_f32_dpp": np.add, "v_mul_f32_dpp": np.multiply, "v_sub_f32_dpp": np.subtract}

    def dpp(src, ctrl):
        if ctrl == "wave_ror:1":
            return np.roll(src, 1)
        return src[_perm([int(c) for c in re.match(r"quad_perm:\[(\d),(\d),(\d),(\d)\]", ctrl).groups()])]

    for _ in range(iters):
        for l in lines:
            t = l.replace(",", " ").split()
            op = t[0]
            if op in ops:
                d, a, b = (int(r[1:]) for r in t[1:4])
                ctrl = "wave_ror:1" if "wave_ror:1" in l else re.search(r"quad_perm:\[[\d,]+\]", l).group(0)
                v[d] = ops[op](dpp(v[a], ctrl), v[b]).astype(F)
            elif op == "v_cndmask_b32_dpp":
                d, a, b = (int(r[1:]) for r in t[1:4])
                assert a not in flight, (l, "reads a register whose load is still in flight")
                v[d] = np.where(vcc, v[b], dpp(v[a], re.search(r"quad_perm:\[[\d,]+\]", l).group(0))).astype(F)
            elif op == "s_waitcnt":
                keep = int(re.search(r"vmcnt\((\d+)\)", l).group(1))
                flight = flight[max(0, len(flight) - keep):] if keep else []
            elif op == "v_mov_b32_dpp":         # the parked value's lanes a, d go to lanes b, c
                v[int(t[1][1:])] = dpp(v[int(t[2][1:])], re.search(r"quad_perm:\[[\d,]+\]", l).group(0))
            elif op == "v_cndmask_b32_e64":     # the merge: src1 where the mask is set
                d, a, b = (int(r[1:]) for r in t[1:4])
                assert t[4] == "%[mk]", l
                v[d] = np.where(mk, v[b], v[a]).astype(F)
            elif op == "v_permlane32_swap_b32":     # lanes 32 .. 63 of vdst change places with lanes 0 .. 31 of src
                d, a = int(t[1][1:]), int(t[2][1:])
                assert d not in flight and a not in flight, (l, "reads a register whose load is still in flight")
                vd, va = v[d].copy(), v[a].copy()
                vd[32:], va[:32] = v[a][:32], v[d][32:]
                v[d], v[a] = vd, va
            elif op in ("buffer_store_dword", "buffer_load_dword"):
                d, a = int(t[1][1:]), int(t[2][1:])
                flight.append(d if op == "buffer_load_dword" else None)
                off = v[a].astype(np.uint64) + int(re.search(r"offset:(\d+)", l).group(1))
                ok = off < 4 * n
                i = (off[ok] // 4).astype(np.int64)
                if op == "buffer_store_dword":
                    y[i] = v[d][ok]
                    stored[i] += 1
                else:
                    assert y is not x or not stored[i].any(), "an input is read after a store to its address"
                    w = np.zeros(LANES, F)
                    w[ok] = x[i]
                    v[d] = w
            elif op == "v_mov_b32_e64":         # a holding register of the cluster variants takes a value
                v[int(t[1][1:])] = v[int(t[2][1:])].copy()
            elif op == "v_add_u32_e64":
                d, a, b = (int(r[1:]) for r in t[1:4])
                v[d] = (v[a] + v[b]).astype(np.uint32)
            elif op == "v_and_b32_dpp":         # the fill: a register of its own, whatever it holds
                d, a, b = (int(r[1:]) for r in t[1:4])
                for k in (a, b):
                    v.setdefault(k, np.zeros(LANES, np.uint32))
                v[d] = dpp(v[a], re.search(r"quad_perm:\[[\d,]+\]", l).group(0)) & v[b]
            else:
                assert op in ("v_nop_e64", "s_nop", "s_add_u32"), l


def ring_eq_as_launched(x, table, state=None, lines=None, K=K_DEFAULT, port=None, in_place=False, mutate=None, merge_lanes=None):
    """One launch with the structure of eq_quad_ring_wave: groups -1 .. g0 - 1 in the C++ form (inputs requested two groups
    ahead: xcur, xnext), whole iterations of K groups through run_asm on the generated text with the kernel's offsets, the
    C++ form to the end.  -> (y, new state).  port: the variant `lines` were generated for (the C++ form is the default
    program in any case: its holding registers start from whatever they hold and none is live behind an iteration);
    in_place: inputs and outputs on one array, every load checked against the stores before it; mutate(v): a test's change
    to the register file the loop starts from; merge_lanes: run_asm's"""
    ring = Ring(x, table, state, K, in_place=in_place)
    n = ring.n
    xcur, xnext = ring.load(-1), ring.load(0)
    g_hi = (n + 1) // G
    iters = (g_hi - 5) // K if g_hi - 5 >= K else 0
    g0 = g_hi - iters * K if iters else -1
    xa = [ring.load(g0 + k) if iters else None for k in range(K)]      # (x0, x1 come from the head: checked below)
    xp = [ring.pload(g0 + 2 * j) for j in range(1, K // 2)] if iters and port in PAIR_PORTS else None

    def group_cpp(g):
        nonlocal xcur, xnext
        xnext2 = ring.load(g + 2)
        ring.r["xcur"], ring.r["xnext"] = xcur, xnext
        prog = []
        for ins in group_program(g, K):
            if ins[0] == "inject":
                prog.append(("inject", ins[1], ins[2], "xcur" if ins[2] == "B" else "xnext"))
            elif ins[0] != "load":
                prog.append(ins)
        ring.run(prog)
        xcur, xnext = xnext, xnext2

    g_total = n_groups(n)
    g = -1
    while g < (g0 if iters else g_total):
        group_cpp(g)
        g += 1
    if iters:
        assert np.array_equal(xcur, xa[0]) and np.array_equal(xnext, xa[1])
        r = ring.r
        st_off = np.where(STORE_LANES, (G * (g0 - 1) + 8 + STORE_SAMPLE) * 4, 0xFFFFF000).astype(np.uint32)
        ld_off = np.where(CONV, (G * g0 + X_SAMPLE) * 4, 0xFFFFF000).astype(np.uint32)
        assert np.all(st_off[STORE_LANES] < 2 ** 31)            # (g0 >= 5: no store offset of the run is negative)
        v = {0: st_off, 1: ld_off, 2: r["Z0"], 3: r["Z1"], 4: r["Zp"], 5: r["G"], 6: r["P"], 7: ring.C1, 8: ring.C2,
             9: np.where(CONV, 4 * G * K, 0).astype(np.uint32), 10: np.where(STORE_LANES, 4 * G * K, 0).astype(np.uint32),
             11: xcur, 12: xnext}
        for k in range(2, K):
            v[11 + k] = xa[k]
        if port in MERGED_PORTS:
            # one store per group: lanes b, c carry the outputs of step 8, seven samples in front of lane a's / d's of step 15
            v[0] = np.where(CONV, (G * (g0 - 1) + 15 + MSTORE_SAMPLE) * 4 - 28, 0xFFFFF000).astype(np.uint32)
            v[10] = v[9]
        elif port in PAIR_PORTS:
            # one store and one load per two groups, rows 1 and 3: v0 from the step 15 of group g0, v1 group g0's pair;
            # v11: S (group g0's inputs, row 3), v12 ..: X0 (row 3: group g0 + 1's) .. X(K/2 - 1)
            v[0] = np.where(PAIR_LANES, (G * g0 + 15 + PSTORE_SAMPLE) * 4, 0xFFFFF000).astype(np.uint32)
            v[1] = np.where(PAIR_LANES, (G * g0 + PX_SAMPLE) * 4, 0xFFFFF000).astype(np.uint32)
            v[9] = v[10] = np.where(PAIR_LANES, 4 * G * K, 0).astype(np.uint32)
            for k in range(2, K):
                del v[11 + k]
            for j in range(1, K // 2):
                v[12 + j] = xp[j - 1]
        if port is not None:
            assert np.all(v[0][v[0] != 0xFFFFF000] < 2 ** 31)
            # (holding registers: never read before the loop has written them)
            v.update({20 + k: np.full(LANES, np.nan, F) for k in range(len(HOLD))})
        if mutate is not None:
            mutate(v)
        run_asm(lines, v, ring.x, ring.y, ring.stored, n, iters, merge_lanes)
        r["Z0"], r["Z1"], r["Zp"], r["G"], r["P"] = v[2], v[3], v[4], v[5], v[6]
        xcur, xnext = v[11], v[12]
        g = g_hi
        while g < g_total:
            group_cpp(g)
            g += 1
    assert np.all(ring.stored == 1), "every output is stored exactly once"
    return ring.y, ring.s_save


if __name__ == "__main__":
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(f"DPP read distances of the steady-state loop (K = {K_DEFAULT}, wait: vmcnt({wait_count()})):")
    check_hazards(verbose=True)
    print("with the fill instruction in the slots that carry nothing:")
    check_hazards(verbose=True, fill=True)
    for nb in range(1, 13):
        ok = check(nb, [700, 1, 333, 64, 1000])
        print(f"{nb:2d} bands, launches of 700 1 333 64 1000 samples: {'bit-exact' if ok else 'MISMATCH'}")
        assert ok
    for n in list(range(1, 40)) + [47, 48, 49, 63, 64, 65, 127, 128, 129, 130, 143, 144, 145]:
        assert check(10, [n, n, 7, n]), n
    print("10 bands, every launch length 1 .. 39 and around the group and ring edges: bit-exact")
    for mode in (1, 2):
        x = np.random.default_rng(9).standard_normal(30000).astype(F)
        x[1500:] = 0.0
        ok = check(10, [1000, 9000, 20000], mode=mode, x=x)
        print(f"denormal mode {mode}, the state decaying behind the signal's end: {'equal' if ok else 'MISMATCH'}")
        assert ok
    assert check_zero_corners()
    print("zeros and -0.0 in the input: equal as numbers, only -0.0 -> +0.0")
    assert check_nonfinite_reach()
    print("a non-finite input sample: bit-exact up to 64 samples before it, non-finite from it on")

#!/usr/bin/env python3
"""Generates open_headstage_amd/csrc/eq_quad_ring_asm.inc: the steady-state loop of the quad form of the wave-ring EQ
(k_eq_ring's third body, csrc/eq_quad_ring_body.hpp), straight from the instruction list of the lane-level model
tools/model_eq_quad_ring.py (group_program): what the model interprets is what the kernel runs.

One iteration = K groups of 16 steps.  A step is alpha, delta, <slot>, beta, gamma -- four VOP2+DPP instructions and the issue
slot that the DPP read-after-write hazard leaves free between delta and beta; the port's instructions and the loop's own
sit in those slots, v_nop (VOP3: 8 bytes) where a slot has nothing to carry.  The second text, EQ_QUAD_RING_LOOP_FILL
(experiments build only: Tuning::eq_quad_fill), has the model's fill there instead: v_and_b32_dpp on v19, a VOP2+DPP
instruction that holds the vector unit for four cycles as a step instruction does, so that a wave beside this one cannot
start an instruction there -- measured: a tie, the convolution's waves cost the loop nothing.
Every encoding is 8 bytes and 8-byte aligned
except the group's s_waitcnt, which shares its slot with a 4-byte partner (s_nop, in the last group the counter's s_add):
81 issue slots per 16 samples.

Pinned registers:
    v0   store offsets: lanes a, d of the conveyor quads hold the byte offset of the sample they store at step
         16 (g0 - 1) + 8 (g0 = the iteration's first group), every other lane 0xFFFFF000 (beyond num_records: dropped)
    v1   load offsets: the conveyor's 16 lanes hold the byte offset of their sample of group g0's inputs, the others 0xFFFFF000
    v2 Z0   v3 Z1   v4 Zp   v5 G   v6 P   v7 C1   v8 C2
    v9 / v10   the iteration's advance of v1 / v0: 64 K bytes in the lanes that take part, 0 elsewhere
    v11 ..     x0 .. x(K-1): the inputs of the next K groups, reloaded in place K groups ahead
    v19        the fill's own register (EQ_QUAD_RING_LOOP_FILL only): no other instruction reads or writes it
    VCC  every lane but c, d of the conveyor quads (the inject is a v_cndmask with the quad_perm on x)

The cluster variants of the port (the model's group_program(port=...): the two stores and the load of a group issue behind
one another instead of each alone between VALU instructions) go to a second file, eq_quad_ring_cl_asm.inc, as
EQ_QUAD_RING_CL_LOOP; eq_quad_ring_asm.inc stays what it was.  Their holding registers are v20 .. v22 (H0 .. H2: a store's
value parked by a v_mov_b32 in VOP3 form, 8 bytes like everything else in the loop).  The offset of a store or a load is that
of the step its value or its register belongs to, less the iteration's advance where it issues behind the advance of v0 / v1.

The merged variants (D1 / D1W: one store per group; D2 / D2W: one store and one load per two groups) go to a third file,
eq_quad_ring_mg_asm.inc, as EQ_QUAD_RING_MG_LOOP, with MG_PORT the one the gate chose.  Their instructions beyond the above:
    v_mov_b32_dpp H, H quad_perm:[0,0,3,3]     the parked value's lanes a, d to lanes b, c (step 10's slot)
    v_cndmask_b32_e64 H, H, Zc, %[mk]          the merge: lanes a, d take Zc (step 15's slot; %[mk]: an SGPR pair, 0x9999...)
    v_permlane32_swap_b32 A, B                 lanes 32 .. 63 of A change places with lanes 0 .. 31 of B (D2 / D2W)
and their pinned registers differ so:
    D1 / D1W   v0 holds an offset in all 16 lanes of the conveyor: lanes a, d as above less 28 bytes -- every store carries
               the offset of its group's step 15 --, lanes b, c that of lane a / d seven samples before; v10 = v9
    D2 / D2W   v0 / v1 hold offsets in rows 1 and 3: row 3 the odd group's 16 lanes, row 1 what lane + 32 has in the even
               group; v0 counts from step 15 of group g0, v1 from group g0; v9 = v10: 64 K bytes in both rows.
               v11 S (the even group's inputs, row 3), v12 .. v(11 + K / 2) X0 ..: the pairs' inputs; H0, H1 = v20, v21.
               The advance of v0 stands behind the iteration's last cluster (step 16 of the last group).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import model_eq_quad_ring as model      # noqa: E402

FULL = "row_mask:0xf bank_mask:0xf"
REG = {"Z0": "v2", "Z1": "v3", "Zp": "v4", "G": "v5", "P": "v6", "C1": "v7", "C2": "v8", "F": "v19",
       "H0": "v20", "H1": "v21", "H2": "v22"}
CL_PORT = "C2"      # the variant eq_quad_ring_cl_asm.inc carries (the gate: DESIGN.md 4.5, round 15)
MG_PORT = "D1W"     # the variant eq_quad_ring_mg_asm.inc carries (the gate: DESIGN.md 4.5, round 17)
INJECT_PERM = {"A": "[0,1,2,3]", "B": "[0,1,0,1]"}


def loop_asm(K, fill=False, port=None):
    REG.update({f"x{k}": f"v{11 + k}" for k in range(K)})
    if port in model.PAIR_PORTS:
        REG.update({"S": "v11", **{f"X{j}": f"v{12 + j}" for j in range(K // 2)}})
    """One iteration = groups 0 .. K - 1 of the model's program as asm lines.  v0: store offsets (lanes a, d of the conveyor
    quads: the store of step 16 (g0 - 1) + 8, g0 = the iteration's first group), v1: load offsets (the conveyor's 16 lanes:
    group g0's inputs), v9 / v10: the iteration's advance of v1 / v0, 64 K bytes.  Other lanes hold 0xFFFFF000 (out of range) and advance by 0."""
    out = []
    wait = model.wait_count(K, port) if port else model.wait_count(K)
    adv_ld = adv_st = counted = False   # this iteration's advance of v1 / v0, the counter's add has issued
    # (C3: behind the last cluster, whose parked stores are two groups old; the pair variants: behind theirs likewise)
    s_adv_st = 15 if port == "C3" else 16 if port in model.PAIR_PORTS else 12
    for k in range(K):
        last = k == K - 1
        s = 0
        for ins in (model.group_program(k, K, fill, port=port) if port else model.group_program(k, K, fill)):
            op, step = ins[0], ins[1]
            if op == "alpha":
                s = step - model.G * k      # the step that issues (a parked store carries the step of its value)
                out.append(f"v_add_f32_dpp {REG[ins[2]]}, {REG['Zp']}, {REG['G']} wave_ror:1 {FULL}")
            elif op == "delta":
                out.append(f"v_mul_f32_dpp {REG['Zp']}, {REG[ins[2]]}, {REG['C2']} quad_perm:[0,0,0,3] {FULL}")
            elif op == "beta":
                out.append(f"v_mul_f32_dpp {REG['P']}, {REG[ins[2]]}, {REG['C1']} quad_perm:[0,0,3,3] {FULL}")
            elif op == "gamma":
                out.append(f"v_sub_f32_dpp {REG['G']}, {REG[ins[2]]}, {REG['P']} quad_perm:[0,0,1,2] {FULL}")
            elif op == "store":
                # behind the advance of v0 (slot 12 of the last group) the offsets are those of the next iteration
                kd, sd = divmod(step - 1, model.G)
                off = 64 * (kd + 1) + (28 if sd + 1 == 15 else 0) - (64 * K if adv_st else 0)
                assert sd + 1 in (8, 15) and 0 <= off < 4096, ins
                out.append(f"buffer_store_dword {REG[ins[2]]}, v0, %[rout], 0 offen offset:{off}")
            elif op in ("mstore", "pstore"):
                # mstore: v0 is the offset of step 15 of group g0 - 1, less 28; pstore (of an odd group): of step 15 of group g0
                kd = (step - 15) // model.G
                off = (64 * (kd + 1) + 28 if op == "mstore" else 64 * kd) - (64 * K if adv_st else 0)
                assert step == model.G * kd + 15 and 0 <= off < 4096, ins
                out.append(f"buffer_store_dword {REG[ins[2]]}, v0, %[rout], 0 offen offset:{off}")
            elif op == "qmove":
                out.append(f"v_mov_b32_dpp {REG[ins[2]]}, {REG[ins[2]]} quad_perm:[0,0,3,3] {FULL}")
            elif op == "merge":
                out.append(f"v_cndmask_b32_e64 {REG[ins[2]]}, {REG[ins[2]]}, {REG[ins[3]]}, %[mk]")
            elif op == "xhalf":
                out.append(f"v_permlane32_swap_b32 {REG[ins[2]]}, {REG[ins[3]]}")
            elif op == "inject":
                # VCC = every lane but c, d of the conveyor quads: those take x (through the quad_perm), the others keep Zp
                out.append(f"v_cndmask_b32_dpp {REG['Zp']}, {REG[ins[3]]}, {REG['Zp']}, vcc quad_perm:{INJECT_PERM[ins[2]]} {FULL}")
            elif op in ("load", "pload"):
                off = 64 * ins[3] - (64 * K if adv_ld else 0)
                assert 0 <= off < 4096, ins
                out.append(f"buffer_load_dword {REG[ins[2]]}, v1, %[rin], 0 offen offset:{off}")
            elif op == "hold":
                out.append(f"v_mov_b32_e64 {REG[ins[2]]}, {REG[ins[3]]}")
            elif op == "wait":
                out.append(f"s_waitcnt vmcnt({wait})")
            elif op == "nop4":
                # (the loop counter's add: the first 4-byte partner of the last group; a merged variant may have two there)
                out.append("s_add_u32 %[cnt], %[cnt], 1" if last and not counted else "s_nop 0")
                counted = counted or last
            elif op == "fill":
                out.append(f"v_and_b32_dpp {REG[ins[2]]}, {REG[ins[2]]}, {REG[ins[2]]} quad_perm:[0,1,2,3] {FULL}")
            elif op == "nop":
                if last and s == 11:
                    out.append("v_add_u32_e64 v1, v1, v9")
                    adv_ld = True
                elif last and s == s_adv_st:
                    out.append("v_add_u32_e64 v0, v0, v10")
                    adv_st = True
                else:
                    assert not fill, (k, s)
                    out.append("v_nop_e64")
    return out


def gen_loop(K=model.K_DEFAULT, fill=False, port=None):
    """the whole statement: VCC, the loop (%[cnt] counts up to 0), the wait for the last loads"""
    return (["s_mov_b32 vcc_lo, -1", "s_mov_b32 vcc_hi, 0x3333ffff", ".p2align 5", "1:"] + loop_asm(K, fill, port) +
            ["s_cbranch_scc0 1b", "s_waitcnt vmcnt(0)", "s_nop 1"])


def _macro(name, lines):
    return f"#define {name} \\\n" + " \\\n".join('    "' + l + '\\n"' for l in lines) + "\n"


def text(K=model.K_DEFAULT):
    return ("// generated by tools/gen_eq_quad_ring_asm.py -- do not edit\n"
            f"#define EQ_QUAD_RING_K {K}\n" + _macro("EQ_QUAD_RING_LOOP", gen_loop(K)) +
            "// the same loop with the fill instruction in the slots that carry nothing (Tuning::eq_quad_fill)\n"
            "#ifdef OHS_EXPERIMENTS\n" + _macro("EQ_QUAD_RING_LOOP_FILL", gen_loop(K, fill=True)) + "#endif\n")


def text_cl(K=model.K_DEFAULT, port=CL_PORT):
    """eq_quad_ring_cl_asm.inc: the loop with the port's memory instructions in clusters"""
    return ("// generated by tools/gen_eq_quad_ring_asm.py -- do not edit\n"
            f"// the steady-state loop of eq_quad_ring_asm.inc with the port variant {port} of tools/model_eq_quad_ring.py:\n"
            "// the group's stores and its load issue behind one another; holding registers from v20 on\n"
            f"#define EQ_QUAD_RING_CL_HOLD {len({i[2] for g in range(K) for i in model.group_program(g, K, port=port) if i[0] == 'hold'})}\n"
            + _macro("EQ_QUAD_RING_CL_LOOP", gen_loop(K, port=port)))


def text_mg(K=model.K_DEFAULT, port=MG_PORT):
    """eq_quad_ring_mg_asm.inc: the loop with both half ports' outputs merged into one store per group (or per two)"""
    hold = len({i[2] for g in range(K) for i in model.group_program(g, K, port=port) if i[0] == 'hold'})
    return ("// generated by tools/gen_eq_quad_ring_asm.py -- do not edit\n"
            f"// the steady-state loop of eq_quad_ring_asm.inc with the port variant {port} of tools/model_eq_quad_ring.py:\n"
            "// step 8's outputs wait in a holding register, move to lanes b, c and merge with step 15's: one store per group\n"
            f"#define EQ_QUAD_RING_MG_HOLD {hold}\n#define EQ_QUAD_RING_MG_PAIRS {int(port in model.PAIR_PORTS)}\n"
            + _macro("EQ_QUAD_RING_MG_LOOP", gen_loop(K, port=port)))


if __name__ == "__main__":
    model.check_hazards(model.K_DEFAULT)
    model.check_hazards(model.K_DEFAULT, fill=True)
    for port in (CL_PORT, MG_PORT):
        model.check_hazards(model.K_DEFAULT, port=port)
        model.check_waits(model.K_DEFAULT, port=port)
    csrc = os.path.join(os.path.dirname(HERE), "open_headstage_amd", "csrc")
    for name, t in (("eq_quad_ring_asm.inc", text()), ("eq_quad_ring_cl_asm.inc", text_cl()), ("eq_quad_ring_mg_asm.inc", text_mg())):
        open(os.path.join(csrc, name), "w").write(t)
        print("wrote", os.path.join(csrc, name))

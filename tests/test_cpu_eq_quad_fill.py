"""The fill instruction of the quad ring's steady-state loop (csrc/eq_quad_ring_body.hpp), the part that needs
no GPU.  In the experiments build's second loop (Tuning::eq_quad_fill) a slot that carries nothing holds a VOP2+DPP
instruction on a register of its own instead of a v_nop, so that the EQ wave keeps the vector unit between delta and beta.  The lane-level model (tools/model_eq_quad_ring.py,
group_program(fill=True)) runs that program: it must give the bits of the program without fills, every DPP read -- the fill's
own included -- must lie at least two issue slots behind the register's last VALU write, nothing else may touch the fill's
register, and the generated text must still be the launch the kernel runs."""
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LENGTHS = list(range(1, 36)) + [47, 48, 49, 63, 64, 65, 127, 128, 129, 143, 144, 145]


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def model():
    return _load("model_eq_quad_ring")


@pytest.fixture(scope="module")
def gen():
    return _load("gen_eq_quad_ring_asm")


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("nb", [1, 10, 12])
def test_fills_change_no_output_and_no_state(model, nb):
    """two launches of every length (1 .. 35, around the group of 16, the ring of 64, the iteration of 128), the second one
    starting from the first one's state: outputs and states of the program with fills == those of the program without"""
    rng = np.random.default_rng(40 + nb)
    tab = model.random_table(rng, nb)
    for n in LENGTHS:
        x = rng.standard_normal(2 * n).astype(np.float32)
        st_a = st_b = None
        for part in (x[:n], x[n:]):
            ya, st_a = model.ring_eq(part, tab, st_a)
            yb, st_b = model.ring_eq(part, tab, st_b, fill=True)
            assert np.array_equal(_bits(ya), _bits(yb)), (nb, n)
            assert np.array_equal(_bits(st_a), _bits(st_b)), (nb, n)


def test_the_program_with_fills_is_the_program(model):
    """the same instructions in the same order; the fill stands exactly where a slot carried nothing, and the two slots
    of an iteration's last group that carry the loop's offset advances keep theirs"""
    K = model.K_DEFAULT
    n_fill = 0
    for g in range(-1, 3 * K):
        plain, filled = model.group_program(g, K), model.group_program(g, K, fill=True)
        assert len(plain) == len(filled)
        for a, b in zip(plain, filled):
            if a == b:
                continue
            assert a[0] == "nop" and b == ("fill", a[1], "F"), (a, b)
            n_fill += 1
        own = [i[1] - model.G * g for i in filled if i[0] == "nop"]
        assert own == (list(model.LOOP_OWN_SLOTS) if (g + 1) % K == 0 else []), (g, own)
    # ten open slots per group (16 steps less two stores, two injects, the load and the wait), two of them the loop's own
    assert n_fill == (3 * K + 1) * 10 - 2 * 4         # (groups -1, K - 1, 2K - 1, 3K - 1 end an iteration)


@pytest.mark.parametrize("K", [4, 8])
def test_every_dpp_read_with_fills_is_two_slots_behind_its_writer(model, K):
    worst = model.check_hazards(K, fill=True)
    assert {op for op, _ in worst} == {"alpha", "beta", "gamma", "delta", "fill"}
    assert min(worst.values()) >= 2
    # consecutive fills are five slots apart (four instructions between them); the step's distances are what they were
    assert worst[("fill", "F")] == 4
    assert {k: v for k, v in worst.items() if k[0] != "fill"} == model.check_hazards(K)
    assert all(d >= 2 for _, _, _, d in model.hazards(K, fill=True))
    assert model.wait_count(K) == 3 * K - 3


def test_fill_hazard_check_has_teeth(model, monkeypatch):
    """two fills in neighbouring slots: the second reads F one slot behind its writer -- refused"""
    real = model.group_program

    def doubled(g, K=8, fill=False):
        out = []
        for i in real(g, K, fill):
            out.append(i)
            if i[0] == "fill" and i[1] % 16 == 1:
                out.append(i)
        return out
    monkeypatch.setattr(model, "group_program", doubled)
    with pytest.raises(AssertionError):
        model.check_hazards(8, fill=True)


def test_nothing_else_touches_the_fills_register(model, gen):
    K = model.K_DEFAULT
    for g in range(K):
        for ins in model.group_program(g, K, fill=True):
            assert ins[0] == "fill" or "F" not in ins[2:], ins
    freg = gen.REG["F"]
    lines = gen.gen_loop(fill=True)
    fills = [l for l in lines if l.startswith("v_and_b32_dpp")]
    assert len(fills) == 10 * K - 2 and len(set(fills)) == 1
    # VOP2 + DPP on the one register, all lanes enabled
    assert re.fullmatch(rf"v_and_b32_dpp {freg}, {freg}, {freg} quad_perm:\[0,1,2,3\] row_mask:0xf bank_mask:0xf", fills[0])
    for l in lines:
        if not l.startswith("v_and_b32_dpp"):
            assert freg not in re.findall(r"\bv\d+\b", l), l
    assert freg not in [v for k, v in gen.REG.items() if k != "F"] + ["v0", "v1", "v9", "v10"]
    # the loop's own instructions keep their slots, the wait pair stays, no v_nop is left; the second text is the v_nop loop
    assert sum(l.startswith("v_add_u32_e64") for l in lines) == 2 and not any(l.startswith("v_nop") for l in lines)
    assert sum(l.startswith("s_waitcnt vmcnt(") for l in lines) == K + 1
    nop = gen.gen_loop()
    assert len(nop) == len(lines)
    assert all(a == b or (a.startswith("v_and_b32_dpp") and b == "v_nop_e64") for a, b in zip(lines, nop))


@pytest.mark.parametrize("nb", [1, 10, 12])
def test_the_launch_on_the_generated_text_with_fills(oracle, model, gen, nb):
    """the kernel's structure (C++ head without fills, whole iterations of the generated text, C++ tail) on the text with
    fills: the oracle's bits, and those of the text with v_nop, the state handed over from launch to launch"""
    lines, nop = gen.loop_asm(model.K_DEFAULT, fill=True), gen.loop_asm(model.K_DEFAULT)
    assert any(l.startswith("v_and_b32_dpp") for l in lines)
    rng = np.random.default_rng(60 + nb)
    tab = model.random_table(rng, nb)
    for sizes in ([8192, 333], [206, 207, 208, 335, 336, 337], [1000 + 16 * t for t in range(8)]):
        x = rng.standard_normal(sum(sizes)).astype(np.float32)
        st_a = st_b = None
        out, o = [], 0
        for n in sizes:
            ya, st_a = model.ring_eq_as_launched(x[o:o + n], tab, st_a, lines)
            yb, st_b = model.ring_eq_as_launched(x[o:o + n], tab, st_b, nop)
            assert np.array_equal(_bits(ya), _bits(yb)) and np.array_equal(_bits(st_a), _bits(st_b)), (sizes, n)
            out.append(ya)
            o += n
        assert np.array_equal(_bits(np.concatenate(out)), _bits(model.oracle_eq(x, tab, sizes))), sizes

"""The quad ring's loop with the port's memory instructions in one cluster per group (csrc/eq_quad_ring_cl_asm.inc, DESIGN.md
4.5, round 15), the part that needs no GPU.  The model's port variant the generator ships (gen.CL_PORT; C2: step 8 parks Zc in
a holding register, step 15 issues store, store, load back to back) moves nothing but the slot the three instructions issue
in: every DPP read must still lie two issue slots behind its register's last VALU write, the wait's vmcnt in the generated
text must be the model's count, the committed .inc must be the generator's output with every 8-byte encoding 8-byte aligned,
the launch as the kernel runs it -- C++ head, whole iterations of the GENERATED TEXT, C++ tail -- must give the oracle's bits,
and on one array for input and output no input may be read after a store to its address."""
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# no asm run below n = 207, exactly one iteration at 207, two at 335; every remainder of the iteration count, one sample to
# either side of each group edge; around 8 192
SIZE_LISTS = ([206, 207, 208, 222, 223, 224, 335, 336, 337],
              [1000 + 16 * t + e for t in range(8) for e in (-1, 0, 1)],
              [8191, 8193])


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def gen():
    return _load("gen_eq_quad_ring_asm")


@pytest.fixture(scope="module")
def model(gen):
    return gen.model


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_the_shipped_variant_is_a_cluster_variant(model, gen):
    assert gen.CL_PORT in model.PORTS and gen.CL_PORT is not None
    # the default program is untouched by the argument
    for g in range(-1, 2 * model.K_DEFAULT):
        assert model.group_program(g, model.K_DEFAULT, port=None) == model.group_program(g, model.K_DEFAULT)


@pytest.mark.parametrize("K", [4, 8])
def test_every_dpp_read_is_two_slots_behind_its_writer(model, gen, K):
    assert all(d >= 2 for _, _, _, d in model.hazards(K, port=gen.CL_PORT))
    worst = model.check_hazards(K, port=gen.CL_PORT)
    assert {op for op, _ in worst} == {"alpha", "beta", "gamma", "delta"}
    # the memory instructions and the holding move stand where a slot was free: the step's distances are what they were
    assert worst == model.check_hazards(K)


def test_hazard_check_has_teeth(model, gen, monkeypatch):
    """a step without the free slot (alpha, delta, beta, gamma) puts beta one slot behind alpha: refused"""
    real = model.group_program
    monkeypatch.setattr(model, "group_program", lambda g, K=8, fill=False, port=None:
                        [i for i in real(g, K, fill, port=port) if i[0] not in ("nop", "nop4")])
    with pytest.raises(AssertionError):
        model.check_hazards(8, port=gen.CL_PORT)


def test_memory_instructions_only_move_later_and_stay_in_their_iteration(model, gen):
    """per group the same two stores (same steps' values) and the same load (same register, same inputs) as the default
    program, none issued earlier than there; a holding register is written and read inside one group of an iteration"""
    K = model.K_DEFAULT

    def issue(prog):        # (kind, value's step or loaded group, register the load writes) -> the step that issues it
        at, out = 0, {}
        for i in prog:
            if i[0] == "alpha":
                at = i[1]
            elif i[0] == "store":
                out[("store", i[1], None)] = at
            elif i[0] == "load":
                out[("load", i[3], i[2])] = at
        return out
    old = issue([i for g in range(0, 3 * K) for i in model.group_program(g, K)])
    new = issue([i for g in range(0, 3 * K) for i in model.group_program(g, K, port=gen.CL_PORT)])
    common = set(old) & set(new)
    assert len(common) >= 3 * (3 * K - 2)           # (all but those whose partner group lies outside the window)
    assert all(new[k] >= old[k] for k in common)
    # a holding register takes a value and gives it to a store inside one group
    for g in range(K):
        live = None
        for i in model.group_program(g, K, port=gen.CL_PORT):
            if i[0] == "hold":
                assert live is None
                live = i[2]
            elif i[0] == "store" and i[2] in model.HOLD:
                assert live == i[2]
                live = None
        assert live is None, "a holding register is live across the end of a group"


@pytest.mark.parametrize("K", [4, 8])
def test_wait_count_in_the_text_is_the_models(model, gen, K):
    want = model.wait_count(K, gen.CL_PORT)
    lits = [int(m.group(1)) for l in gen.loop_asm(K, port=gen.CL_PORT) for m in [re.match(r"s_waitcnt vmcnt\((\d+)\)", l)] if m]
    assert len(lits) == K and set(lits) == {want}
    if gen.CL_PORT == "C2":
        # the load is the last of its cluster, the wait stands K - 1 groups on in front of that group's cluster: K - 2 whole
        # clusters of three in between
        assert want == 3 * (K - 2)
    assert model.wait_count(K) == 3 * K - 3         # the default program's is what it was


def test_generated_file_is_the_generators_output_and_aligned(model, gen):
    inc = open(os.path.join(ROOT, "open_headstage_amd", "csrc", "eq_quad_ring_cl_asm.inc")).read()
    assert inc == gen.text_cl(), "eq_quad_ring_cl_asm.inc is not what tools/gen_eq_quad_ring_asm.py writes"
    lines = gen.gen_loop(port=gen.CL_PORT)
    body = lines[lines.index("1:") + 1:]            # (behind .p2align 5)
    four = ("s_waitcnt", "s_nop", "s_add_u32", "s_cbranch")
    at = 0
    for l in body:
        size = 4 if l.startswith(four) else 8
        assert size == 4 or at % 8 == 0, (at, l)
        at += size
    K = model.K_DEFAULT
    step = [l for l in body if l.startswith(("v_add_f32_dpp", "v_mul_f32_dpp", "v_sub_f32_dpp"))]
    assert len(step) == 4 * 16 * K
    mem = [l for l in body if l.startswith("buffer_")]
    assert len(mem) == 3 * K and sum(l.startswith("buffer_store_dword") for l in mem) == 2 * K
    # the holding registers are clear of every pinned register and of the fill's
    hold = {gen.REG[h] for h in model.HOLD}
    assert not hold & ({f"v{k}" for k in range(0, 20)})


@pytest.mark.parametrize("nb", [1, 10, 12])
def test_the_launch_on_the_generated_text(oracle, model, gen, nb):
    """bit for bit against the oracle, the state handed over from launch to launch"""
    lines = gen.loop_asm(model.K_DEFAULT, port=gen.CL_PORT)
    rng = np.random.default_rng(80 + nb)
    tab = model.random_table(rng, nb)
    for sizes in SIZE_LISTS:
        x = rng.standard_normal(sum(sizes)).astype(np.float32)
        st, out, o = None, [], 0
        for n in sizes:
            y, st = model.ring_eq_as_launched(x[o:o + n], tab, st, lines, port=gen.CL_PORT)
            out.append(y)
            o += n
        assert np.array_equal(_bits(np.concatenate(out)), _bits(model.oracle_eq(x, tab, sizes))), sizes


def test_in_place_no_input_is_read_after_a_store_to_its_address(oracle, model, gen):
    """inputs and outputs on ONE array: every load of the C++ form and of the generated text is checked against the stores
    issued before it (Ring.load, run_asm), and the outputs are still the oracle's; the whole launch in the variant's own
    program (ring_eq) likewise"""
    lines = gen.loop_asm(model.K_DEFAULT, port=gen.CL_PORT)
    rng = np.random.default_rng(77)
    tab = model.random_table(rng, 10)
    for sizes in SIZE_LISTS:
        x = rng.standard_normal(sum(sizes)).astype(np.float32)
        st, out, o = None, [], 0
        for n in sizes:
            y, st = model.ring_eq_as_launched(x[o:o + n], tab, st, lines, port=gen.CL_PORT, in_place=True)
            out.append(y)
            o += n
        assert np.array_equal(_bits(np.concatenate(out)), _bits(model.oracle_eq(x, tab, sizes))), sizes
    for n in (1, 17, 64, 129, 333, 1000):
        x = rng.standard_normal(n).astype(np.float32)
        y, _ = model.ring_eq(x, tab, port=gen.CL_PORT, in_place=True)
        assert np.array_equal(_bits(y), _bits(model.oracle_eq(x, tab, [n]))), n
    # the check has teeth: a load of an address that a store has written is refused
    ring = model.Ring(x, tab, in_place=True)
    ring.stored[:] = 1
    with pytest.raises(AssertionError):
        ring.load(0)

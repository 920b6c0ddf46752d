"""The quad ring's merged port, the part that needs no GPU.  Four variants of the model's
group_program(port=...): D1 (both half ports' outputs merged in one register: one store per group), D2 (two groups' registers
exchanged by halves: one store and one load per two groups), and D1W / D2W (the same with the group's wait in front of the
cluster's memory instructions instead of in step 14's slot).  Ring, lanes of the bands, injects, sample addresses and bits are
what they were; only where and how the port's memory instructions issue changes.  Per variant: every DPP read and every
operand of a half exchange lies two issue slots behind its last VALU write, no inject or exchange reads a register whose load
is still in flight, the launch in the variant's own program and the launch as the kernel runs it -- C++ head, whole iterations
of the GENERATED TEXT, C++ tail -- give the oracle's bits (1 / 10 / 12 bands, the three denormal modes, in place on one array,
launch sequences with odd and even group counts), the committed .inc is the generator's output, and the slot counts and
vmcnt values are the numbers written down here.  The default program and C1 .. C3 are byte for byte what they were.  Four
mutants must fail: the merge mask off by one lane role, the exchange's operands swapped, the wait one group late, a pair
store's row-1 offsets from the odd group's base."""
import hashlib
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("D1", "D1W", "D2", "D2W")

# the model's three size lists (tests/test_cpu_eq_quad_port_cluster.py): no asm run below n = 207, exactly one iteration at
# 207, two at 335; every remainder of the iteration count, one sample to either side of each group edge; around 8 192
SIZE_LISTS = ([206, 207, 208, 222, 223, 224, 335, 336, 337],
              [1000 + 16 * t + e for t in range(8) for e in (-1, 0, 1)],
              [8191, 8193])
# launches whose group count (n + 62 + 15) // 16 + 1 is odd, even, odd, even, ...: a pair variant's last pair is half empty
# in every other one, and the state goes from launch to launch
ODD_EVEN = [207 + 16 * k for k in range(6)]


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


def _launches(model, lines, port, x, tab, sizes, **kw):
    st, out, o = None, [], 0
    for n in sizes:
        y, st = model.ring_eq_as_launched(x[o:o + n].copy(), tab, st, lines, port=port, **kw)
        out.append(y)
        o += n
    return np.concatenate(out)


def test_the_variants_exist_and_the_shipped_one_is_one_of_them(model, gen):
    assert set(VARIANTS) <= set(model.PORTS) and gen.MG_PORT in VARIANTS
    assert set(model.MERGED_PORTS) | set(model.PAIR_PORTS) == set(VARIANTS)
    assert ODD_EVEN and {model.n_groups(n) % 2 for n in ODD_EVEN} == {0, 1}


def test_the_default_program_and_c1_to_c3_are_byte_identical(model, gen):
    """sha256 of the instruction lists (groups -1 .. 16) and of the generated statements, taken before the merged variants
    were added; the committed files of those loops are still the generator's output"""
    want = {(None, False): ("9a92f426b9b485df", "dcc701b9c58087b4", 21), (None, True): ("0435d32086a9d2e4", "ba375c9adc36e8b7", 21),
            ("C1", False): ("bb82d12344f74c8e", "f973d02211353ae6", 18), ("C2", False): ("ac5dda65900693cd", "7a450c157d2bdc6e", 18),
            ("C3", False): ("18277da2b3450ab2", "8d8a6e53dc72a7ee", 13)}
    for (port, fill), (h_prog, h_text, wait) in want.items():
        prog = repr([model.group_program(g, 8, fill, port=port) for g in range(-1, 17)])
        text = "\n".join(gen.gen_loop(8, fill=fill, port=port))
        assert hashlib.sha256(prog.encode()).hexdigest()[:16] == h_prog, (port, fill)
        assert hashlib.sha256(text.encode()).hexdigest()[:16] == h_text, (port, fill)
        assert model.wait_count(8, port) == wait
        model.check_waits(8, port)
    csrc = os.path.join(ROOT, "open_headstage_amd", "csrc")
    assert open(os.path.join(csrc, "eq_quad_ring_asm.inc")).read() == gen.text()
    assert open(os.path.join(csrc, "eq_quad_ring_cl_asm.inc")).read() == gen.text_cl()


@pytest.mark.parametrize("port", VARIANTS)
def test_hazards_and_waits(model, port):
    for K in (8,) if port == "D2W" else (4, 8):      # (D2W: the wait in front of a cluster needs three pairs in rotation)
        assert all(d >= 2 for _, _, _, d in model.hazards(K, port=port))
        worst = model.check_hazards(K, port=port)
        step = {k: v for k, v in worst.items() if k[0] in ("alpha", "beta", "gamma", "delta")}
        assert step == model.check_hazards(K)           # the step's own distances are what they were
        assert ("qmove", "H0") in worst                 # the quad move reads the holding register through DPP
        if port in model.PAIR_PORTS:
            assert {("xhalf", r) for r in ("H0", "H1", "S")} <= set(worst)
        assert model.check_waits(K, port) >= 4 * K


def test_the_half_exchange_rule_has_teeth(model, monkeypatch):
    """v_permlane32_swap directly behind the merge that wrote its operand: refused.  (In the last group of an iteration the
    exchange stands five slots behind the merge; here it is moved into the merge's own slot.)"""
    real = model.group_program

    def early(g, K=8, fill=False, port=None):
        prog = real(g, K, fill, port=port)
        if (g + 1) % K == 0:
            sw = next(i for i in prog if i[0] == "xhalf" and i[2] == "H0")
            prog.remove(sw)
            at = next(k for k, i in enumerate(prog) if i[0] == "merge")
            prog.insert(at + 1, sw)
        return prog
    monkeypatch.setattr(model, "group_program", early)
    with pytest.raises(AssertionError):
        model.check_hazards(8, port="D2")


@pytest.mark.parametrize("port,per_iteration,vmcnt,stores,loads", [("D1", 657, 12, 8, 8), ("D1W", 665, 10, 8, 8),
                                                                  ("D2", 655, 4, 4, 4), ("D2W", 655, 2, 4, 4)])
def test_slot_counts_and_vmcnt(model, gen, port, per_iteration, vmcnt, stores, loads):
    """instructions per iteration of K = 8 groups (128 samples; an s_waitcnt and its 4-byte partner count as two, as in the 81
    of the default loop and the 83 of C2), the memory instructions among them, and the wait's count"""
    K = 8
    lines = gen.loop_asm(K, port=port)
    assert len(lines) == per_iteration
    assert sum(l.startswith("buffer_store_dword") for l in lines) == stores
    assert sum(l.startswith("buffer_load_dword") for l in lines) == loads
    assert model.wait_count(K, port) == vmcnt
    lits = [int(m.group(1)) for l in lines for m in [re.match(r"s_waitcnt vmcnt\((\d+)\)", l)] if m]
    assert lits == [vmcnt] * (K if port in model.MERGED_PORTS else K // 2)
    per_group = [sum(1 for i in model.group_program(g, K, port=port) if i[0] != "state") for g in range(K, 2 * K)]
    if port == "D1":        # 80 + the wait + one more for store, load in one slot; the first group has no cluster, the last two
        assert per_group == [81] + [82] * 6 + [84]
    # one step = alpha, delta, slot, beta, gamma everywhere: the port changes slots only
    step = [l for l in lines if l.startswith(("v_add_f32_dpp", "v_mul_f32_dpp", "v_sub_f32_dpp"))]
    assert len(step) == 4 * 16 * K
    # the wait: in step 14's slot, or (W) in front of the memory instructions -- behind inject A in an iteration's last group
    for k, l in enumerate(lines):
        if l.startswith("s_waitcnt"):
            assert lines[k + 1].startswith(("s_nop 0", "s_add_u32")), (k, lines[k + 1])
            if port in model.WAIT_IN_CLUSTER:
                assert lines[k + 2].startswith("buffer_store_dword") and lines[k + 3].startswith("buffer_load_dword")


def test_generated_file_is_the_generators_output_and_aligned(model, gen):
    inc = open(os.path.join(ROOT, "open_headstage_amd", "csrc", "eq_quad_ring_mg_asm.inc")).read()
    assert inc == gen.text_mg(), "eq_quad_ring_mg_asm.inc is not what tools/gen_eq_quad_ring_asm.py writes"
    assert f"port variant {gen.MG_PORT} " in inc
    for port in VARIANTS:
        lines = gen.gen_loop(port=port)
        body = lines[lines.index("1:") + 1:]            # (behind .p2align 5)
        at = 0
        for l in body:
            size = 4 if l.startswith(("s_waitcnt", "s_nop", "s_add_u32", "s_cbranch")) else 8
            assert size == 4 or at % 8 == 0, (port, at, l)
            at += size
        assert sum(l.startswith("s_add_u32") for l in body) == 1        # the loop counter, once per iteration
        # the holding registers are clear of every pinned register and of the fill's; VCC is left to the injects
        used = set(re.findall(r"\bv(\d+)\b", "\n".join(body)))
        assert {"20"} <= used and (port in model.MERGED_PORTS) == ("21" not in used) and "19" not in used
        assert all("vcc" not in l for l in body if l.startswith("v_cndmask_b32_e64"))


@pytest.mark.parametrize("port", VARIANTS)
@pytest.mark.parametrize("nb", [1, 10, 12])
def test_the_launch_in_the_variants_own_program(oracle, model, port, nb):
    """ring_eq: the whole launch in the variant's program, out of place and in place on one array, the three denormal modes"""
    rng = np.random.default_rng(170 + nb)
    tab = model.random_table(rng, nb)
    for n in (1, 17, 64, 129, 333, 1000):
        x = rng.standard_normal(n).astype(np.float32)
        ref = model.oracle_eq(x, tab, [n])
        for in_place in (False, True):
            y, _ = model.ring_eq(x.copy(), tab, port=port, in_place=in_place)
            assert np.array_equal(_bits(y), _bits(ref)), (n, in_place)
    x = rng.standard_normal(3000).astype(np.float32) * np.float32(1e-30)
    x[400:] = 0.0               # the state decays through the subnormal range
    for mode in (1, 2):
        y, _ = model.ring_eq(x.copy(), tab, mode=mode, port=port)
        ref = model.oracle_eq(x, tab, [x.size], mode)
        d = _bits(y) != _bits(ref)
        assert np.array_equal(y, ref) and np.all(y[d] == 0.0) and np.all(ref[d] == 0.0), mode


@pytest.mark.parametrize("port", VARIANTS)
@pytest.mark.parametrize("nb", [1, 10, 12])
def test_the_launch_on_the_generated_text(oracle, model, gen, port, nb):
    """bit for bit against the oracle, the state handed over from launch to launch; the shipped variant and 10 bands: all
    three size lists, out of place and in place; otherwise the first list and the odd / even sequence"""
    lines = gen.loop_asm(model.K_DEFAULT, port=port)
    rng = np.random.default_rng(180 + nb)
    tab = model.random_table(rng, nb)
    full = nb == 10 or port == gen.MG_PORT
    for sizes in (SIZE_LISTS if full else SIZE_LISTS[:1]) + (ODD_EVEN,):
        x = rng.standard_normal(sum(sizes)).astype(np.float32)
        ref = model.oracle_eq(x, tab, sizes)
        for in_place in (False, True):
            got = _launches(model, lines, port, x, tab, sizes, in_place=in_place)
            assert np.array_equal(_bits(got), _bits(ref)), (sizes, in_place)


def test_in_place_check_has_teeth(model):
    rng = np.random.default_rng(7)
    ring = model.Ring(rng.standard_normal(300).astype(np.float32), np.ones((1, 5), np.float32), in_place=True)
    ring.stored[:] = 1
    with pytest.raises(AssertionError):
        ring.load(0)
    with pytest.raises(AssertionError):
        ring.pload(0)


# ---- mutants: each must fail ------------------------------------------------------------------------------------------------

def _fails(model, lines, port, x, tab, sizes, ref, **kw):
    """the launch raises (a check of the interpreter: a register read in flight, an output stored twice or never) or its
    bits differ from the oracle's"""
    try:
        got = _launches(model, lines, port, x, tab, sizes, **kw)
    except AssertionError:
        return True
    return not np.array_equal(_bits(got), _bits(ref))


@pytest.fixture(scope="module")
def case(oracle, model):
    rng = np.random.default_rng(99)
    tab = model.random_table(rng, 10)
    sizes = [335, 464]
    x = rng.standard_normal(sum(sizes)).astype(np.float32)
    return x, tab, sizes, model.oracle_eq(x, tab, sizes)


@pytest.mark.parametrize("port", VARIANTS)
def test_mutant_merge_mask_off_by_one_lane_role(model, gen, case, port):
    x, tab, sizes, ref = case
    lines = gen.loop_asm(model.K_DEFAULT, port=port)
    assert not _fails(model, lines, port, x, tab, sizes, ref)
    assert not _fails(model, lines, port, x, tab, sizes, ref, merge_lanes=model.MERGE_LANES.copy())
    for roles in ((1, 3), (0, 2), (0, 1), (1, 0)):      # a, d -> b, d / a, c / a, b / the mask shifted by one lane
        wrong = (model.ROLE == roles[0]) | (model.ROLE == roles[1])
        assert _fails(model, lines, port, x, tab, sizes, ref, merge_lanes=wrong), roles


@pytest.mark.parametrize("port", ["D2", "D2W"])
def test_mutant_swap_operands_exchanged(model, gen, case, port):
    x, tab, sizes, ref = case
    lines = gen.loop_asm(model.K_DEFAULT, port=port)
    flip = lambda l: re.sub(r"(v_permlane32_swap_b32) (v\d+), (v\d+)", r"\1 \3, \2", l)      # noqa: E731
    store_side = [flip(l) if l.startswith("v_permlane32_swap_b32 v20") else l for l in lines]
    load_side = [flip(l) if l.startswith("v_permlane32_swap_b32 v11") else l for l in lines]
    assert store_side != lines and load_side != lines
    assert _fails(model, store_side, port, x, tab, sizes, ref)
    assert _fails(model, load_side, port, x, tab, sizes, ref)


@pytest.mark.parametrize("port", VARIANTS)
def test_mutant_the_wait_one_group_late(model, gen, case, port):
    """a wait that stands one group (D2: one pair) further on leaves one more cluster's store and load in flight: vmcnt + 2.
    The model's walk and the interpreter of the text both refuse the inject (or exchange) that reads the register."""
    x, tab, sizes, ref = case
    K = model.K_DEFAULT
    count = model.wait_count(K, port)
    model.check_waits(K, port, count)
    with pytest.raises(AssertionError):
        model.check_waits(K, port, count + 2)
    lines = gen.loop_asm(K, port=port)
    late = [l.replace(f"vmcnt({count})", f"vmcnt({count + 2})") for l in lines]
    assert late != lines
    with pytest.raises(AssertionError, match="in flight"):
        _launches(model, late, port, x, tab, sizes)


@pytest.mark.parametrize("port", ["D2", "D2W"])
def test_mutant_pair_store_row_1_offset_from_the_odd_groups_base(model, gen, case, port):
    """row 1 of a pair's store carries the EVEN group's outputs, 16 samples in front of row 3's: with the odd group's base
    there they land on the odd group's addresses"""
    x, tab, sizes, ref = case
    lines = gen.loop_asm(model.K_DEFAULT, port=port)

    def wrong(v):
        row1 = model.ROW == 1
        v[0] = np.where(row1, v[0] + np.uint32(4 * model.G), v[0]).astype(np.uint32)
    assert _fails(model, lines, port, x, tab, sizes, ref, mutate=wrong)

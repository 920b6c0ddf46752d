"""The quad form of the wave-ring EQ (csrc/eq_quad_ring_body.hpp), the part that needs no GPU: the lane-level model
tools/model_eq_quad_ring.py -- 64 lanes, one band per quad, the four operations alpha delta beta gamma per step in float32,
the port, head, tail and state hand-over -- must give the oracle EQ's bits, and every DPP read of the steady-state loop must
lie at least two issue slots behind the register's last VALU write (the port's instructions included).  The generated asm
loop must be what the generator writes from the model's instruction list."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def model():
    return _load("model_eq_quad_ring")


@pytest.mark.parametrize("K", [4, 8])
def test_every_dpp_read_is_two_slots_behind_its_writer(model, K):
    worst = model.check_hazards(K)
    # the four step instructions read through DPP (the inject reads x, which a load writes: the group's wait covers it)
    assert {op for op, _ in worst} == {"alpha", "beta", "gamma", "delta"}
    assert min(worst.values()) >= 2
    # the inject writes Zp: alpha's distance is measured to it where it is the last writer
    assert worst[("alpha", "Zp")] == 2
    assert model.wait_count(K) == 3 * K - 3


def test_hazard_check_has_teeth(model, monkeypatch):
    """a step without the free slot (alpha, delta, beta, gamma) puts beta one slot behind alpha: refused"""
    real = model.group_program
    monkeypatch.setattr(model, "group_program", lambda g, K=8: [i for i in real(g, K) if i[0] not in ("nop", "nop4")])
    with pytest.raises(AssertionError):
        model.check_hazards(8)


@pytest.mark.parametrize("nb", list(range(1, 13)))
def test_model_matches_the_oracle_over_consecutive_launches(oracle, model, nb):
    assert model.check(nb, [700, 1, 333, 64, 1000], seed=1)


@pytest.mark.parametrize("n", list(range(1, 36)) + [47, 48, 49, 63, 64, 65, 79, 80, 81, 127, 128, 129, 143, 144, 145, 1000])
def test_model_every_length_around_the_edges(oracle, model, n):
    """lengths around the group of 16, the ring of 64 and the loop iteration of 128 steps, the state handed over three times"""
    assert model.check(10, [n, n, 7, n], seed=2)
    assert model.check(12, [n, 3, n], seed=3)


@pytest.mark.parametrize("K", [1, 4])
def test_model_other_lookahead_depths(oracle, model, K):
    assert model.check(10, [500, 37, 463], seed=4, K=K)


@pytest.mark.parametrize("mode", [1, 2])
def test_model_denormal_modes(oracle, model, mode):
    """the state decays through the subnormal range behind the signal's end: equal as numbers in the flushing modes, differing
    bits only where both are a zero (include/ohs_hip.h)"""
    x = np.random.default_rng(9).standard_normal(30000).astype(np.float32)
    x[1500:] = 0.0
    assert model.check(10, [1000, 9000, 20000], mode=mode, x=x)


def test_model_documented_corners(oracle, model):
    """include/ohs_hip.h, ohs_eq_process_block: a -0.0 may come out as +0.0 (never the reverse), a non-finite input sample
    shows up to 64 samples early; everything else bit-exact"""
    assert model.check_zero_corners()
    assert model.check_nonfinite_reach()


def test_model_tells_a_wrong_constant(oracle, model):
    rng = np.random.default_rng(3)
    tab = model.random_table(rng, 10)
    x = rng.standard_normal(600).astype(np.float32)
    ref = model.oracle_eq(x, tab, [600])
    y, _ = model.ring_eq(x, tab)
    assert np.array_equal(y.view(np.uint32), ref.view(np.uint32))
    tab2 = tab.copy()
    tab2[4, 2] = np.nextafter(tab2[4, 2], np.float32(2.0))
    y2, _ = model.ring_eq(x, tab2)
    assert not np.array_equal(y2.view(np.uint32), ref.view(np.uint32))


def test_lane_constants(model):
    t = np.arange(10, dtype=np.float32).reshape(2, 5) + 2        # (b0, b1, b2, a1, a2) = (2 .. 6), (7 .. 11)
    c1, c2 = model.lane_constants(t)
    assert list(c1[:12]) == [1, 1, 6, 5, 1, 1, 11, 10, 1, 1, 0, 0]
    assert list(c2[:12]) == [4, 3, 2, 1, 9, 8, 7, 1, 0, 0, 1, 1]


def test_generated_asm_is_the_generators_output():
    gen = _load("gen_eq_quad_ring_asm")
    inc = open(os.path.join(ROOT, "open_headstage_amd", "csrc", "eq_quad_ring_asm.inc")).read()
    assert inc == gen.text(), "eq_quad_ring_asm.inc is not what tools/gen_eq_quad_ring_asm.py writes"
    lines = gen.gen_loop()
    step = [l for l in lines if l.startswith(("v_add_f32_dpp", "v_mul_f32_dpp", "v_sub_f32_dpp"))]
    assert len(step) == 4 * 16 * gen.model.K_DEFAULT
    # every encoding inside the loop is 8 bytes but the 4-byte pairs (s_waitcnt + partner) and the closing branch
    four = [l for l in lines if l.startswith(("s_waitcnt", "s_nop", "s_add_u32", "s_cbranch"))]
    assert len(four) == 2 * gen.model.K_DEFAULT + 3


@pytest.mark.parametrize("nb", [1, 10, 12])
def test_the_launch_as_the_kernel_runs_it(oracle, model, nb):
    """csrc/eq_quad_ring_body.hpp's structure on the CPU: the C++ form for groups -1 .. g0 - 1 (inputs requested two groups
    ahead), whole iterations of the GENERATED asm text through an interpreter with the kernel's offset registers and a raw
    buffer's range check, the C++ form to the end -- lengths without an iteration, around the first one, with every remainder
    of the iteration count, around 8 192, the state handed over from launch to launch"""
    gen = _load("gen_eq_quad_ring_asm")
    lines = gen.loop_asm(model.K_DEFAULT)
    rng = np.random.default_rng(20 + nb)
    tab = model.random_table(rng, nb)
    for sizes in ([8192, 333, 700], [8191, 8193], [206, 207, 208, 222, 223, 224, 335, 336, 337],
                  [1000 + 16 * t + e for t in range(8) for e in (-1, 0, 1)]):
        x = rng.standard_normal(sum(sizes)).astype(np.float32)
        st, out, o = None, [], 0
        for n in sizes:
            y, st = model.ring_eq_as_launched(x[o:o + n], tab, st, lines)
            out.append(y)
            o += n
        ref = model.oracle_eq(x, tab, sizes)
        assert np.array_equal(np.concatenate(out).view(np.uint32), ref.view(np.uint32)), sizes

"""CPU suite: the EQ launch plan -- which form serves a launch, with which wave body, in what workgroups, on what grid.

open_headstage_amd/csrc/eq_plan.h is host-only C++: the one function every EQ launcher asks.  tools/check_eq_plan.cpp includes
that header and tuning.h alone; it is built here with AddressSanitizer + UBSan (g++, CPU only), once as the product build sees
the header and once with -DOHS_EXPERIMENTS, run as a child process over the full product of the cases below, and every field it
prints is compared with a numpy restatement of the rule as DOCUMENTED (csrc/kernels.h, csrc/tuning.h), not of the
C++."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, ROW_RING, WAVE_RING, CONVEYOR = 0, 1, 2, 3          # include/ohs_hip.h: OHS_EQ_FORM_*
IN = ["one_table", "addressable", "n", "n_chains", "n_bands", "exact", "xcd_lo", "xcd_n", "cus",
      "eq_form", "eq_conveyor", "eq_wg_waves", "eq_ring_v1", "eq_quad_fill", "eq_quad_lone_port", "eq_no_prio", "eq_lds"]
OUT = ["valid", "form", "body", "ring_v1", "wg_waves", "grid", "prio", "lds"]


@pytest.fixture(scope="module", params=[False, True], ids=["product", "experiments"])
def checker(request, tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("eq_plan") / "check_eq_plan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
           "-I" + os.path.join(ROOT, "open_headstage_amd", "csrc"), "-o", out, os.path.join(ROOT, "tools", "check_eq_plan.cpp")]
    if request.param:
        cmd.insert(1, "-DOHS_EXPERIMENTS=1")
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan not installed")
    assert r.returncode == 0, r.stderr[-2000:]
    return out, request.param


def _run(binary, words):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([binary], input=np.ascontiguousarray(words, np.int32).tobytes(), capture_output=True, env=env, timeout=300)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in err and "runtime error" not in err, (r.returncode, err[-3000:])
    return np.fromstring(r.stdout.decode(), np.int64, sep=" ").reshape(-1, len(OUT))


def _cases():
    """[N, 17]: the full product of the launch geometry, the XCD ranges and the tuning keys that the rule reads; the keys it only
    passes on (priority, LDS) and the experiments build's loop variants of the quad body vary from case to case"""
    rows = []
    for cus in (4, 256):
        dims = [(0, 1), (0, 1), (0, 512, 8191, 8192), (0, 2, 6, 2 * cus, 2 * cus + 2, 4 * cus - 2, 4 * cus), (0, 1, 12, 13, 16, 17),
                (0, 1), range(7), (cus,), (0, 1, 2, 3), (0, 1), (0, 2, 8), (0, 1)]
        g = np.stack(np.meshgrid(*[np.asarray(d, np.int32) for d in dims], indexing="ij"), axis=-1).reshape(-1, len(dims))
        rows.append(g)
    g = np.concatenate(rows)
    xcd = np.array([(0, 8), (0, 3), (3, 5), (7, 1), (0, 0), (4, 5), (-1, 2)], np.int32)[g[:, 6]]
    rng = np.random.default_rng(20240611)
    extra = rng.integers(0, 2, (len(g), 4)).astype(np.int32) * np.array([1, 1, 1, 4096], np.int32)
    return np.concatenate([g[:, :6], xcd, g[:, 7:], extra], axis=1)


def _expected(c, experiments):
    """The plan by the documents.  c: {name: [N] int64} -> [N, 8]"""
    one = c["one_table"] != 0
    addr, exact = c["addressable"] != 0, c["exact"] != 0
    n, chains, bands, cus = c["n"], c["n_chains"], c["n_bands"], c["cus"]
    nothing = (n <= 0) | (chains <= 0)                      # nothing to launch: valid, form NONE
    # round 2's ring kernel: the experiments build only, the launches of one table only (tuning.h)
    v1 = one & (c["eq_ring_v1"] != 0) if experiments else np.zeros(len(n), bool)
    # a pass holds 1 .. 16 bands; per-stream tables: both chains of every stream, and strides the ring form reaches
    refused = np.where(one, (bands < 1) | (bands > 16), (chains % 2 != 0) | ~addr) & ~nothing
    # kernels.h: the conveyor form serves more than 12 bands, the exact-specials mode, eq_conveyor and strides beyond the ring
    # form's 32-bit offsets (round 2's kernel carries 64-bit addresses); per-stream tables exist for the ring forms only
    conveyor = one & ~nothing & ~refused & ((bands > 12) | (c["eq_conveyor"] != 0) | exact | ~(addr | v1))
    ring = ~nothing & ~refused & ~conveyor
    # tuning.h eq_form: 1 = rows, 2 / 3 = one chain per wave; 0 = the library's choice -- DESIGN.md 4.5: the wave ring up to two
    # chains per CU and from 8192 samples
    wave = ring & ~v1 & ((c["eq_form"] >= 2) | ((c["eq_form"] == 0) & (chains <= 2 * cus) & (n >= 8192)))
    # the ring kernels (not round 2's) run on an XCD range inside [0, 8)
    xcd_bad = (c["xcd_n"] < 1) | (c["xcd_lo"] < 0) | (c["xcd_lo"] + c["xcd_n"] > 8)
    refused = refused | (ring & ~v1 & xcd_bad)
    ok = ~nothing & ~refused
    ring, wave, conveyor = ring & ok, wave & ok, conveyor & ok
    v1 = v1 & ring              # (reported where that kernel is what is launched)
    form = np.select([wave, ring, conveyor], [WAVE_RING, ROW_RING, CONVEYOR], NONE)
    # body: rows 0; one band per pair of lanes 1 (eq_form = 2, and the only wave body with per-stream tables); per quad 2 -- the
    # experiments build's loop variants of it: 3 = eq_quad_fill, else 4 = eq_quad_lone_port
    quad = np.where((c["eq_quad_fill"] != 0) & experiments, 3, np.where((c["eq_quad_lone_port"] != 0) & experiments, 4, 2))
    body = np.where(wave, np.where(~one | (c["eq_form"] == 2), 1, quad), 0)
    # waves: one per chain in the wave ring, else one per four chains; tuning.h eq_wg_waves: 0 = one wave per workgroup below one
    # wave per CU, else four (the wave ring: always one); round 2's kernel ignores a setting above four
    rows4 = (chains + 3) // 4
    waves = np.where(wave, chains, rows4)
    wg_set = np.where(v1 & (c["eq_wg_waves"] > 4), 0, c["eq_wg_waves"])
    wg = np.where(ring, np.where(wg_set != 0, wg_set, np.where(wave | (rows4 < cus), 1, 4)), 1)
    workgroups = -(-waves // wg)
    xn = np.where(xcd_bad, 8, c["xcd_n"])
    partitioned = np.where(xn == 8, workgroups, -(-workgroups // xn) * 8)        # kernels.h / eq_plan.h: xcd_grid
    grid = np.select([ring & ~v1, v1, conveyor], [partitioned, workgroups, rows4], 0)
    mine = ring & ~v1           # priority and the LDS reservation are the ring kernels'
    prio = np.where(mine & (c["eq_no_prio"] == 0), 1, 0)
    lds = np.where(mine, c["eq_lds"], 0)
    return np.stack([nothing | ok, form, body, v1, wg, grid, prio, lds], axis=1).astype(np.int64)


def test_plan_against_the_documents(checker):
    binary, experiments = checker
    cases = _cases()
    assert len(cases) == 2 * 2 * 2 * 4 * 7 * 6 * 2 * 7 * 4 * 2 * 3 * 2
    got = _run(binary, cases)
    c = {k: cases[:, i].astype(np.int64) for i, k in enumerate(IN)}
    want = _expected(c, experiments)
    assert got.shape == want.shape
    # the grid is xcd_grid(ceil(waves / wg_waves), xcd_n) of the plan's own fields, wherever a ring kernel is launched
    k = (got[:, 1] == ROW_RING) | (got[:, 1] == WAVE_RING)
    k &= got[:, 3] == 0
    waves = np.where(got[:, 1] == WAVE_RING, c["n_chains"], (c["n_chains"] + 3) // 4)
    wgs = -(-waves // got[:, 4])
    assert (got[k, 5] == np.where(c["xcd_n"] == 8, wgs, -(-wgs // np.maximum(c["xcd_n"], 1)) * 8)[k]).all()
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        i = int(bad[0])
        pytest.fail(f"{bad.size} of {len(want)} cases differ; first: {dict(zip(IN, cases[i].tolist()))}: "
                    f"got {dict(zip(OUT, got[i].tolist()))}, want {dict(zip(OUT, want[i].tolist()))}")


def test_the_cases_reach_every_outcome(checker):
    """the case set itself: every form, every body the build has, both workgroup shapes of the rows, refusals of each kind"""
    binary, experiments = checker
    cases = _cases()
    c = {k: cases[:, i].astype(np.int64) for i, k in enumerate(IN)}
    want = _expected(c, experiments)
    assert set(np.unique(want[:, 1])) == {NONE, ROW_RING, WAVE_RING, CONVEYOR}
    assert set(np.unique(want[:, 2])) == ({0, 1, 2, 3, 4} if experiments else {0, 1, 2})
    assert set(np.unique(want[:, 3])) == ({0, 1} if experiments else {0})
    assert {1, 2, 4, 8} <= set(np.unique(want[:, 4]))
    assert (want[:, 0] == 0).any() and ((want[:, 0] == 1) & (want[:, 1] == NONE)).any()
    # the thresholds lie between neighbouring cases: 8191 | 8192 samples, 2 cus | 2 cus + 2 chains, 12 | 13 bands
    auto = (c["one_table"] == 1) & (c["eq_form"] == 0) & (want[:, 0] == 1) & (c["n_bands"] == 12) & (c["eq_ring_v1"] == 0)
    for cus in (4, 256):
        at = auto & (c["cus"] == cus) & (want[:, 1] != CONVEYOR)
        assert set(want[at & (c["n"] == 8192) & (c["n_chains"] == 2 * cus), 1]) == {WAVE_RING}
        assert set(want[at & (c["n"] == 8191) & (c["n_chains"] == 2 * cus), 1]) == {ROW_RING}
        assert set(want[at & (c["n"] == 8192) & (c["n_chains"] == 2 * cus + 2), 1]) == {ROW_RING}
    live = (c["one_table"] == 1) & (c["n"] > 0) & (c["n_chains"] > 0) & (want[:, 0] == 1)
    assert set(want[live & (c["n_bands"] == 13), 1]) == {CONVEYOR} and CONVEYOR in set(want[live & (c["n_bands"] == 12), 1])
    assert {ROW_RING, WAVE_RING} <= set(want[live & (c["n_bands"] == 12), 1])

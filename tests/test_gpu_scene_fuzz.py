"""One BlendSceneProcessor, many calls: randomised sequences over both entries of libohs_scene2.so against ONE model of the handle.

Every call draws the plain or the blended entry, K from {1, 2, 3, 8, 33, 64}, 1 .. 7 blocks, seg_blocks from {1, 2, 3, 9}, CROSSFADE
or RING_OUT, one shared row or rows per stream, gains given or None, each prev_* given or None; between calls sometimes set_gain,
reset, or set_directions with a new 7-row table (which zeroes the overlap).  The model is tests/scene_blend_model.model_blend_f64
-- the plain entry is its weights at +0.0 --, with tail_in / with_tail carrying the 512-frame overlap across calls and across changes
of K; the overlap is kept at gain 1, as the handle keeps it (the gain is applied at the store).  After every call: the output within
1e-6 relative RMS per stream AND per 512-frame block (_within_bar: the project's FFT bar), and the launch record
equal to the model's plan.  3 streams, EQ off, four fixed seeds of twelve calls.  A failure names the seed and lists the calls.
tests/test_cpu_scene_blend.py holds the generator to what this paragraph names."""
import numpy as np
import pytest

from tests import scene_blend_model as bm
from tests.test_cpu_layout import BLOCK, make_layout
from tests.test_gpu_scene import _within_bar

pytestmark = pytest.mark.gpu

S, N_DIRS, N_CALLS = 3, 7, 12
SEEDS = (0, 1, 2, 3)
KS, SEGS = (1, 2, 3, 8, 33, 64), (1, 2, 3, 9)
GAINS = np.array([0.5, 0.75, 1.0, 1.25], np.float32)


def _walk(rng, first, n, draw, hold=0.6):
    """[n] entries after `first`: each object keeps its entry with probability `hold`, else draws a new one -> [n + 1][K]"""
    rows = [first]
    for _ in range(n):
        new = draw()
        rows.append(np.where(rng.random(first.shape) < hold, rows[-1], new).astype(first.dtype))
    return np.stack(rows)


def draw_call(rng):
    """-> dict: the arguments of one call (rows [R][n_segs][K] with R = 1 for a shared row; entry 0 of each walk is prev_*)"""
    K, blocks, seg = int(rng.choice(KS)), int(rng.integers(1, 8)), int(rng.choice(SEGS))
    n_segs = -(-blocks // min(seg, blocks))
    blended, fade, shared = bool(rng.integers(0, 2)), bool(rng.integers(0, 4) > 0), bool(rng.integers(0, 3) == 0)
    R = 1 if shared else S

    def weights():
        kind = rng.integers(0, 4, (R, K))
        return np.where(kind < 2, 0.0, np.where(kind == 2, 1.0, rng.uniform(0.05, 0.95, (R, K)))).astype(np.float32)
    walks = {"idx": _walk(rng, rng.integers(0, N_DIRS, (R, K)).astype(np.uint32), n_segs, lambda: rng.integers(0, N_DIRS, (R, K))),
             "idx1": _walk(rng, rng.integers(0, N_DIRS, (R, K)).astype(np.uint32), n_segs, lambda: rng.integers(0, N_DIRS, (R, K))),
             "weights": _walk(rng, weights(), n_segs, weights),
             "gains": _walk(rng, rng.choice(GAINS, (R, K)), n_segs, lambda: rng.choice(GAINS, (R, K)))}
    call = dict(K=K, blocks=blocks, seg=seg, blended=blended, fade=fade, shared=shared, x_seed=int(rng.integers(0, 1 << 30)))
    for name, w in walks.items():
        rows, prev = np.ascontiguousarray(np.moveaxis(w[1:], 0, 1)), np.ascontiguousarray(w[0])     # [R][n_segs][K], [R][K]
        call[name] = rows[0] if shared else rows
        call["prev_" + name] = (prev[0] if shared else prev) if rng.integers(0, 2) else None
    if rng.integers(0, 3) == 0:
        call["gains"] = None
    if not blended:
        for name in ("idx1", "weights", "prev_idx1", "prev_weights"):
            call[name] = None
    return call


def draw_sequence(seed):
    rng = np.random.default_rng(31000 + seed)
    ops = []
    for _ in range(N_CALLS):
        r = int(rng.integers(0, 8))
        if r == 0:
            ops.append(("set_gain", float(rng.choice([0.5, 0.7, 1.0]))))
        elif r == 1:
            ops.append(("reset",))
        elif r == 2:
            ops.append(("set_directions", int(rng.integers(1, 1000))))
        ops.append(("call", draw_call(rng)))
    return ops


def _describe(op):
    if op[0] != "call":
        return f"{op[0]}({', '.join(str(v) for v in op[1:])})"
    c = op[1]
    given = [k for k in ("gains", "prev_idx", "prev_gains", "prev_idx1", "prev_weights") if c[k] is not None]
    return (f"{'blended' if c['blended'] else 'plain'}(K {c['K']}, blocks {c['blocks']}, seg_blocks {c['seg']}, {'CROSSFADE' if c['fade'] else 'RING_OUT'}, "
            f"{'a shared row' if c['shared'] else 'rows per stream'}, given: {given})")


def _table(seed):
    return make_layout(N_DIRS, 512, seed=seed)


def run_sequence(seed):
    import torch

    import open_headstage_amd as ohs
    ops = draw_sequence(seed)
    h = ohs.BlendSceneProcessor(S, num_bands=10)
    dirs, gain, tail = _table(11), 1.0, None
    h.set_directions(dirs)
    done, n_calls, kinds = [], 0, set()
    for op in ops:
        done.append(_describe(op))
        where = f"seed {seed}, operation {len(done) - 1}: {done[-1]}; the sequence so far:\n  " + "\n  ".join(done)
        if op[0] == "set_gain":
            gain = op[1]
            h.set_gain(gain)
        elif op[0] == "reset":
            h.reset()
            tail = None
        elif op[0] == "set_directions":
            dirs, tail = _table(op[1]), None
            h.set_directions(dirs)
        if op[0] != "call":
            continue
        c = op[1]
        K, n = c["K"], c["blocks"]
        x = np.random.default_rng(c["x_seed"]).uniform(-1.0, 1.0, (S, K, n * BLOCK)).astype(np.float32)
        y = h.process(torch.from_numpy(x.copy()).cuda(), c["idx"], c["seg"], c["gains"], c["prev_idx"], c["prev_gains"], c["fade"], c["idx1"],
                      c["weights"], c["prev_idx1"], c["prev_weights"])
        torch.cuda.synchronize()
        y = y.cpu().numpy()
        # the plain entry is the blended rule at w = +0.0 (the second direction is never read, and is no change)
        idx1 = c["idx"] if c["idx1"] is None else c["idx1"]
        w = np.zeros(np.shape(c["idx"]), np.float32) if c["weights"] is None else c["weights"]
        m, tail = bm.model_blend_f64(x, dirs, c["idx"], idx1, w, c["seg"], c["gains"], c["prev_idx"], c["prev_idx1"], c["prev_weights"],
                                     c["prev_gains"], c["fade"], 1.0, tail, True)
        plan = bm.blend_plan(S, K, n, c["idx"], idx1, w, c["seg"], c["gains"], c["prev_idx"], c["prev_idx1"], c["prev_weights"], c["prev_gains"],
                             c["fade"])
        want = ((K + 1) // 2, bm.count_fading_passes(plan), bm.count_blended_passes(plan, K))
        rec = h.last_launch()
        try:
            assert (rec[0], rec[2], rec[3]) == want, f"the launch record {rec} against the model's (pairs, fading, blended) {want}"
            assert c["blended"] or rec[3] == 0
            _within_bar(y, gain * m, f"seed {seed}, operation {len(done) - 1}")
        except AssertionError as e:
            raise AssertionError(f"{where}\n{e}") from e
        n_calls += 1
        kinds.add((c["blended"], c["fade"], c["shared"], c["gains"] is None))
    return n_calls, kinds


@pytest.mark.parametrize("seed", SEEDS)
def test_one_handle_many_calls_against_the_model(seed):
    n_calls, kinds = run_sequence(seed)
    assert n_calls == N_CALLS
    print(f"scene fuzz seed {seed}: {n_calls} calls, {len(kinds)} combinations of (entry, switch mode, row form, gains)")


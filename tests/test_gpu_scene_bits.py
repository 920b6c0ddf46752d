"""The object scenes' output BITS across commits: tests/golden/scene_output_sha256.txt was written by `python tools/scene_hash.py` on an
MI355X, on the build of commit 29c4bd8 ("blend three directions per object over a triangle mesh") -- the one in front of the one
that folded the three object kernels' text into csrc/conv_objects_body.hpp --, and every build since has to give the same digests
through all six processing entries.  (The other scene tests compare two libraries of one build, which a change made alike to every
kernel passes.)  A deliberate change of the kernels' arithmetic needs the file regenerated, and says so here.

tools/scene_hash.py describes the scenes: 5 streams, K = 5 and K = 64, 512 taps, 64 directions, seg_blocks 2, CROSSFADE with every
prev_* row given -- gains present and rows per stream, flush mode 0, in one case, gains absent and one shared row, flush mode 1, in
the other -- and RING_OUT once.  Equal or not equal: there is no tolerance."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _tool():
    spec = importlib.util.spec_from_file_location("scene_hash", os.path.join(os.path.dirname(HERE), "tools", "scene_hash.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_scene_output_bits_are_those_of_the_three_separate_kernels():
    tool = _tool()
    want = {}
    with open(os.path.join(HERE, "golden", "scene_output_sha256.txt")) as f:
        for line in f:
            case, entry, digest = line.split()
            want[(case, entry)] = digest
    assert len(want) == len(tool.CASES) * len(tool.ENTRIES) == 18
    assert {c[1] for c in tool.CASES} == {5, 64} and {c[5] for c in tool.CASES} == {0, 1}
    assert {c[2:5] for c in tool.CASES} == {(True, True, False), (True, False, True), (False, True, False)}
    seen, bad = set(), []
    for case, entry, digest, launch, record in tool.hashes():
        print(case, entry, digest, launch)
        K, crossfade = next(c[1:3] for c in tool.CASES if c[0] == case)
        # more than one block range per stream; the record the scene was made for ...
        assert launch[1] > 1, (case, entry, launch)
        assert launch[:1] + launch[2:] == record, (case, entry, launch, record)
        # ... which, in the three-direction call, has two-row, four-row and six-row passes, and under CROSSFADE fading passes of each
        # kind: a pair of every kind in front of the odd last one, every pair fading once per segment
        if entry == "scene3_process_blended3":
            pairs, fading, four, six = record
            per_pair = tool.S * (tool.BLOCKS + (tool.N_SEGS if crossfade else 0))
            total = pairs * per_pair
            assert four > 0 and six > 0 and total - four - six > 0 and (four % per_pair, six % per_pair) == (0, 0), record
            assert fading == (tool.S * tool.N_SEGS * pairs if crossfade else 0), record
            # pairs of kind 0, 1, 2 (two, four, six rows): each pair's passes are its BLOCKS current ones and, under CROSSFADE, one
            # through the old entries per segment -- so the old halves of every kind are in the counts
            n = [len(range(kind, pairs, 3)) for kind in range(3)]
            assert min(n) > 0 and four == n[1] * per_pair and six == n[2] * per_pair and total - four - six == n[0] * per_pair, (record, n)
            if crossfade:
                assert four > tool.S * n[1] * tool.BLOCKS and six > tool.S * n[2] * tool.BLOCKS, record
        seen.add((case, entry))
        if digest != want[(case, entry)]:
            bad.append((case, entry))
    assert seen == set(want)
    assert not bad, f"object-scene output bits changed: {bad}"

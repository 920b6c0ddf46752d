"""bench.py --dump-outputs without a device: dump_outputs() on a host tensor shaped like a step's output.  The files are
float32, within the option's size budget, a function of the array alone (the sample's indices depend on the shape only),
and hold exactly the elements they name.  The GPU rehearsal of the whole option is tests/test_gpu_bench_rehearsal.py."""
import os

import numpy as np
import torch


def _dump(tmp_path, y, **kw):
    import bench
    d = str(tmp_path)
    bench.dump_outputs(d, y, **kw)
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_files_are_float32_and_name_their_elements(tmp_path):
    import bench
    g = torch.Generator().manual_seed(3)
    y = torch.randn(6, 2, 5000, generator=g)
    a = _dump(tmp_path / "a", y)
    assert sorted(a) == ["y_head", "y_sample", "y_tail"]
    assert all(v.dtype == np.float32 for v in a.values())
    k = a["y_head"].shape[2]
    assert a["y_head"].shape == a["y_tail"].shape == (6, 2, k) and 1 <= k <= 2500
    assert np.array_equal(a["y_head"], y[:, :, :k].numpy()) and np.array_equal(a["y_tail"], y[:, :, -k:].numpy())
    n = min(y.numel(), bench.DUMP_BYTES // 3 // 4)
    idx = np.unique(np.random.default_rng(bench.DUMP_SEED).integers(0, y.numel(), n, dtype=np.int64))
    assert idx.size == a["y_sample"].size and np.array_equal(a["y_sample"], y.reshape(-1).numpy()[idx])
    # same shape, other values: the same positions are sampled
    z = y * 2 + 1
    b = _dump(tmp_path / "b", z)
    assert np.array_equal(b["y_sample"], a["y_sample"] * 2 + 1)


def test_dump_outputs_stays_within_the_budget_at_the_headline_shape(tmp_path, monkeypatch):
    """the headline's [256, 2, 480 256] output (shrunk by the same factor as the budget, so the test stays small) and
    a two-rank share of it: all files together below the budget"""
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", bench.DUMP_BYTES // 64)
    y = torch.zeros(256, 2, 480256 // 64)
    for parts in (1, 2):
        d = tmp_path / f"p{parts}"
        _dump(d, y, parts=parts, suffix="_rank0" if parts > 1 else "")
        total = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
        assert total * parts <= bench.DUMP_BYTES * 1.01, (parts, total)
    assert bench.DUMP_BYTES * 64 <= 64_000_000

"""bench.py --dump-outputs on the host: what is written for a grid too large to dump whole (a fixed seeded sample with its cell indices) and for
a small one (x whole), within the 64 MB budget, the same in every run."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

INFO = {"rnorm0": 3.5, "rnorm": 1.25e-3}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_large_x_is_sampled_at_fixed_cells(tmp_path):
    n = 3 * bench.DUMP_CELLS + 17
    x = torch.arange(n, dtype=torch.float64) * 0.5
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), x, INFO, 0, 1)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == {"x_sample", "x_sample_index", "residual_norms"}
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 2 ** 20
    assert all(v.dtype == np.float64 for v in a.values())
    idx = a["x_sample_index"]
    assert idx.size == bench.DUMP_CELLS and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(a["x_sample"], idx * 0.5)                      # the values of x at those cells
    assert all(np.array_equal(a[k], b[k]) for k in a)                    # the same cells in every run
    assert np.array_equal(a["residual_norms"], [3.5, 1.25e-3])


def test_small_x_is_written_whole_and_ranks_are_apart(tmp_path):
    x = torch.linspace(-1.0, 1.0, 1000, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path), x, INFO, 0, 1)
    bench.dump_outputs(str(tmp_path), x + 1.0, INFO, 1, 2)
    d = _load(tmp_path)
    assert set(d) == {"x", "residual_norms", "x_rank1", "residual_norms_rank1"}
    assert np.array_equal(d["x"], x.numpy()) and np.array_equal(d["x_rank1"], x.numpy() + 1.0)

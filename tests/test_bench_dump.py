"""bench.py --dump-outputs: the files dump_outputs writes, checked on the host."""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import bench  # noqa: E402


def test_small_outputs_are_written_whole(tmp_path):
    g = torch.Generator().manual_seed(0)
    arrays = {"image": torch.rand(12, 16, 3, generator=g), "grad_means": torch.rand(50, 3, generator=g).double(),
              "count": torch.arange(7, dtype=torch.int32)}
    bench.dump_outputs(tmp_path, arrays)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["count.npy", "grad_means.npy", "image.npy"]
    img, gm, cnt = (np.load(tmp_path / f"{k}.npy") for k in ("image", "grad_means", "count"))
    assert img.dtype == np.float32 and np.array_equal(img, arrays["image"].numpy())
    assert gm.dtype == np.float64 and np.array_equal(gm, arrays["grad_means"].numpy())
    assert cnt.dtype == np.float32 and np.array_equal(cnt, np.arange(7, dtype=np.float32))


def test_large_outputs_are_a_fixed_sample_within_the_budget(tmp_path):
    n = bench.DUMP_BUDGET_BYTES // 4                     # each of the two large tensors alone fills the budget
    arrays = {"a": torch.arange(n, dtype=torch.float32), "b": -torch.arange(n + 5, dtype=torch.float32),
              "small": torch.ones(10)}
    bench.dump_outputs(tmp_path / "1", arrays)
    bench.dump_outputs(tmp_path / "2", arrays)
    total = sum(p.stat().st_size for p in (tmp_path / "1").iterdir())
    assert total <= bench.DUMP_BUDGET_BYTES + 4096 and total <= 64_000_000
    a = np.load(tmp_path / "1" / "a.npy")
    assert a.ndim == 1 and 0 < a.size < n
    assert np.all(np.diff(a) > 0)                        # sorted, no repeats, and the values are the sampled entries
    for name in arrays:
        assert np.array_equal(np.load(tmp_path / "1" / f"{name}.npy"), np.load(tmp_path / "2" / f"{name}.npy"))
    assert np.array_equal(np.load(tmp_path / "1" / "small.npy"), np.ones(10, dtype=np.float32))

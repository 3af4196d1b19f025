"""bench.py --dump-outputs: what a step returned, as float32 / float64 .npy files (no GPU: the batch is a stand-in holding CPU tensors)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _batch(n, od=57, idim=13):
    g = torch.Generator().manual_seed(0)
    return SimpleNamespace(obs=torch.rand((n, od), generator=g), term_obs=torch.rand((n, od), generator=g), reward=torch.rand(n, generator=g),
                           info=torch.randint(-5, 1 << 20, (n, idim), generator=g, dtype=torch.int32),
                           done=(torch.rand(n, generator=g) < 0.3).to(torch.uint8))


def test_dump_writes_every_output_exactly(tmp_path):
    G = _batch(64)
    bench.dump_outputs(G, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == sorted(f"{k}.npy" for k in bench.DUMP_NAMES)
    for k in bench.DUMP_NAMES:
        a = np.load(tmp_path / f"{k}.npy")
        assert a.dtype in (np.float32, np.float64) and a.shape == tuple(getattr(G, k).shape)
        np.testing.assert_array_equal(a, getattr(G, k).numpy())
    bench.dump_outputs(G, str(tmp_path), rank=1)
    np.testing.assert_array_equal(np.load(tmp_path / "rank1_obs.npy"), G.obs.numpy())


def test_dump_of_a_large_batch_is_a_fixed_sample_within_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100_000)
    G = _batch(1000)
    for d in ("a", "b"):
        bench.dump_outputs(G, str(tmp_path / d))
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 100_000 + 1024 * len(bench.DUMP_NAMES)
    idx = np.load(tmp_path / "a" / "env_index.npy").astype(np.int64)
    np.testing.assert_array_equal(idx, np.load(tmp_path / "b" / "env_index.npy"))
    assert len(idx) < 1000 and np.all(np.diff(idx) > 0)
    for k in bench.DUMP_NAMES:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f"{k}.npy"), getattr(G, k).numpy()[idx])

"""CPU suite: bench.py --dump-outputs writes float32 arrays within its size limit, the same ones for the same inputs."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_writes_float32_within_the_limit(tmp_path, monkeypatch):
    small = torch.randn(2, 4, 8, 8, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "a"), {"latents": small})
    got = np.load(tmp_path / "a" / "latents.npy")
    assert got.dtype == np.float32 and got.shape == (2, 4, 8, 8)
    assert np.array_equal(got, small.float().numpy())

    # above the limit: a fixed, seeded sample of the elements, the same on every call
    monkeypatch.setattr(bench, "DUMP_LIMIT", 4000)
    big = torch.arange(10000, dtype=torch.float32)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"latents": big})
    b, c = (np.load(tmp_path / d / "latents_sample.npy") for d in ("b", "c"))
    assert b.dtype == np.float32 and b.nbytes <= 4000 and b.size == 1000
    assert np.array_equal(b, c)
    assert np.all(np.diff(b) > 0) and np.isin(b, big.numpy()).all()
    assert not os.path.exists(tmp_path / "b" / "latents.npy")

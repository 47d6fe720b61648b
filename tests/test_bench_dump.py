"""bench.py --dump-outputs on the host: an output over the size cap is written as the same sample of rows in every run,
in their original order; smaller outputs are written whole, float32 or float64."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_samples_large_outputs_reproducibly(tmp_path):
    out = torch.randn(64, 1000, 256)                      # the default forward's encoder output shape
    out[..., 0] = torch.arange(64 * 1000, dtype=torch.float32).reshape(64, 1000)      # column 0: the row's own index
    loss = torch.tensor(2.5, dtype=torch.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"encoder_out": out, "loss": loss})
    a, b = np.load(tmp_path / "a" / "encoder_out.npy"), np.load(tmp_path / "b" / "encoder_out.npy")
    assert a.dtype == np.float32 and a.shape[1] == 256 and 0 < a.shape[0] < 64 * 1000
    assert np.array_equal(a, b)
    idx = a[:, 0].astype(np.int64)
    assert (np.diff(idx) > 0).all()
    assert np.array_equal(a, out.reshape(-1, 256).numpy()[idx])
    l = np.load(tmp_path / "a" / "loss.npy")
    assert l.dtype == np.float64 and l.shape == () and l == 2.5
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 10 ** 6


def test_dump_outputs_writes_small_outputs_whole(tmp_path):
    out = torch.randn(2, 50, 64).bfloat16()
    bench.dump_outputs(str(tmp_path), {"encoder_out": out})
    got = np.load(tmp_path / "encoder_out.npy")
    assert got.dtype == np.float32 and np.array_equal(got, out.float().numpy())

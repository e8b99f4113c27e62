"""bench.py's plain / --full split and --dump-outputs on CPU: the dump writes every array as
float32 / float64 .npy within its byte budget, whole when it fits and else as the same seeded sample
in every run; the options a plain run does not measure are refused without --full."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _arrays(scale=1.0):
    g = torch.Generator().manual_seed(7)
    return {"loss_terms": torch.tensor([1.5, 1.0, 0.5], dtype=torch.float64),
            "recon": torch.rand(4, 3, 8, 8, generator=g) * scale,
            "params": torch.randn(5001, generator=g) * scale,
            "grads": torch.randn(5001, generator=g) * scale}


def test_dump_outputs_whole_within_budget(tmp_path):
    import bench
    arrays = _arrays()
    bench.dump_outputs(str(tmp_path / "d"), arrays)
    assert sorted(os.listdir(tmp_path / "d")) == ["grads.npy", "loss_terms.npy", "params.npy", "recon.npy"]
    for name, t in arrays.items():
        a = np.load(tmp_path / "d" / (name + ".npy"))
        assert a.dtype == (np.float64 if name == "loss_terms" else np.float32)
        assert np.array_equal(a, t.reshape(-1).numpy())


def test_dump_outputs_samples_over_budget_the_same_way_every_run(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 20000)         # params and grads (20004 B each) do not fit
    bench.dump_outputs(str(tmp_path / "a"), _arrays())
    bench.dump_outputs(str(tmp_path / "b"), _arrays(2.0))
    total = 0
    for name, t in _arrays().items():
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        total += a.nbytes
        assert a.shape == b.shape
        if name == "loss_terms":
            continue
        assert np.array_equal(b, a * 2)                      # the same elements of both runs
        if name == "recon":
            assert np.array_equal(a, t.reshape(-1).numpy())  # small arrays stay whole
        else:
            assert 0 < a.size < t.numel() and np.isin(a, t.numpy()).all()
    assert total <= 20000


def test_kernel_breakdown_needs_full(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--kernel-breakdown"])
    with pytest.raises(SystemExit):
        bench.parse()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--kernel-breakdown", "--full", "--dump-outputs", "x"])
    args = bench.parse()
    assert args.full and args.dump_outputs == "x"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    args = bench.parse()
    assert not args.full and args.dump_outputs is None and args.steps == 3

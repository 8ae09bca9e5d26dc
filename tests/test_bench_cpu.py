"""bench.py's own plumbing without a GPU: the --steps / --warmup check and what --dump-outputs writes."""
import sys

import numpy as np
import pytest
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default_and_steps_must_be_positive(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "out")
    assert a.full and a.dump_outputs == "out"
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            _parse(monkeypatch, *bad)


def test_dump_outputs_writes_float32_and_a_seeded_sample_past_the_limit(tmp_path, monkeypatch):
    t = torch.randn(256, 512, generator=torch.Generator().manual_seed(0))
    bench.dump_outputs(tmp_path / "one", {"embeddings": t}, 0, 1)
    got = np.load(tmp_path / "one" / "embeddings.npy")
    assert got.dtype == np.float32 and np.array_equal(got, t.numpy())
    # two ranks share the limit: 100 rows each, the same rows in every run, in their original order
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2 * 100 * 512 * 4)
    for run in ("a", "b"):
        bench.dump_outputs(tmp_path / run, {"embeddings": t}, 1, 2)
    a, b = (np.load(tmp_path / run / "embeddings_rank1.npy") for run in ("a", "b"))
    assert a.shape == (100, 512) and a.nbytes <= bench.DUMP_LIMIT_BYTES // 2 and np.array_equal(a, b)
    rows = [int(np.flatnonzero((t.numpy() == r).all(axis=1))[0]) for r in a]
    assert rows == sorted(set(rows))

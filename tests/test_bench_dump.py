"""bench.py --dump-outputs writer: names, dtypes, determinism, size budget."""
import importlib.util
import os

import numpy as np
import torch

from arkflow_amd.batch import Column, MessageBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location(
        "bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _batch():
    return MessageBatch({
        "f": Column("numeric", torch.tensor([0.5, 1.5, 2.5])),
        "k": Column("numeric", torch.tensor([1, 2, (1 << 40) + 1])),
        "h": Column("numeric", torch.tensor([1.0, 2.0, 3.0],
                                            dtype=torch.bfloat16)),
        "s": Column.from_strings(["a", "bc", ""]),
    })


def test_dump_outputs_names_and_dtypes(tmp_path):
    bench = _bench()
    bench.dump_outputs([_batch()], str(tmp_path / "d"))
    got = {n: np.load(tmp_path / "d" / n) for n in os.listdir(tmp_path / "d")}
    assert sorted(got) == ["f.npy", "h.npy", "k.npy", "s.bytes.npy",
                           "s.offsets.npy"]
    assert got["f.npy"].dtype == np.float32
    assert got["h.npy"].dtype == np.float32
    assert got["k.npy"].dtype == np.float64  # int64 survives exactly
    assert got["k.npy"].tolist() == [1.0, 2.0, float((1 << 40) + 1)]
    assert got["f.npy"].tolist() == [0.5, 1.5, 2.5]
    assert got["s.bytes.npy"].tolist() == [97.0, 98.0, 99.0]
    assert got["s.offsets.npy"].tolist() == [0.0, 1.0, 3.0, 3.0]


def test_dump_outputs_budget_sample_is_fixed(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    outs = [
        MessageBatch({"a": Column(
            "numeric", torch.arange(5000, dtype=torch.float32))}),
        MessageBatch({"b": Column(
            "numeric", torch.arange(10, dtype=torch.float32))}),
    ]
    for d in ("x", "y"):
        bench.dump_outputs(outs, str(tmp_path / d))
    ax = np.load(tmp_path / "x" / "out0_a.npy")
    ay = np.load(tmp_path / "y" / "out0_a.npy")
    assert np.array_equal(ax, ay)              # same sample every run
    assert 0 < ax.size < 5000 and np.all(np.diff(ax) > 0)  # order kept
    assert np.load(tmp_path / "x" / "out1_b.npy").size == 10  # small: whole
    total = sum(os.path.getsize(tmp_path / "x" / n)
                for n in os.listdir(tmp_path / "x"))
    assert total <= 4096

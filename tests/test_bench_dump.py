"""bench.py --dump-outputs without a GPU: the writer keeps env order and the float dtypes, stays inside its byte budget, and
samples the same env rows every time it has to sample."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _outs(n, L=180):
    g = torch.Generator().manual_seed(3)
    return dict(obs_num=torch.rand(n, 10, generator=g), lasers=torch.rand(n, L, generator=g),
                target=torch.rand(n, 2, generator=g, dtype=torch.float64), reward=torch.rand(n, generator=g, dtype=torch.float64),
                done=torch.randint(0, 2, (n,), generator=g, dtype=torch.uint8), status=torch.randint(0, 9, (n, 3), generator=g, dtype=torch.uint8))


def test_dump_whole_batch(tmp_path):
    bench = _bench()
    outs = _outs(64)
    bench.dump_outputs(str(tmp_path), outs)
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in bench.DUMP_NAMES)
    for name, t in outs.items():
        a = np.load(tmp_path / (name + ".npy"))
        assert a.dtype == (np.float64 if t.dtype == torch.float64 else np.float32), name
        assert np.array_equal(a, t.numpy().astype(a.dtype)), name


def test_dump_samples_within_budget(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BUDGET", 1 << 20)
    outs = _outs(4096)                   # 3.3 MB of outputs against a 1 MB budget
    d1, d2 = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(d1), outs)
    bench.dump_outputs(str(d2), outs)
    assert sum(os.path.getsize(d1 / f) for f in os.listdir(d1)) <= 1 << 20
    rows = np.load(d1 / "env_index.npy")
    assert rows.dtype == np.float64 and len(rows) > 1000 and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, np.load(d2 / "env_index.npy"))
    idx = rows.astype(np.int64)
    for name, t in outs.items():
        a = np.load(d1 / (name + ".npy"))
        assert np.array_equal(a, t.numpy()[idx].astype(a.dtype)), name

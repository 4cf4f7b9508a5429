"""bench.py --dump-outputs (the last timed step's arrays as .npy, at most 64 MB) and the plain run's JSON line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def test_dump_outputs_writes_float32_arrays_in_their_shapes(tmp_path):
    import bench
    a = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    b = torch.linspace(0, 1, 5, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path), {"output": a, "grad.w": b})
    x, y = np.load(tmp_path / "output.npy"), np.load(tmp_path / "grad.w.npy")
    assert x.dtype == np.float32 and x.shape == (3, 4) and np.array_equal(x, a.numpy())
    assert y.dtype == np.float64 and np.array_equal(y, b.numpy())


def test_dump_outputs_samples_beyond_the_budget(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    big = torch.arange(10000, dtype=torch.float32)
    small = torch.ones(8)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"output": big, "grad.s": small})
    files = [tmp_path / "a" / f for f in ("output.npy", "grad.s.npy")]
    assert sum(os.path.getsize(f) for f in files) <= 4096
    x = np.load(files[0])
    assert 0 < x.size < big.numel() and np.all(np.diff(x) > 0)        # a subset of the elements, in index order
    assert np.array_equal(x, np.load(tmp_path / "b" / "output.npy"))  # the same sample every run
    assert np.array_equal(np.load(files[1]), small.numpy())             # arrays within their share are whole


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_and_dumps_the_step(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "edges/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["config"]["full"] is False   # the secondary legs need --full
    names = sorted(os.listdir(out))
    assert "output.npy" in names and any(n.startswith("grad.ent_encoder.") for n in names)
    total = 0
    for n in names:
        x = np.load(out / n)
        total += os.path.getsize(out / n)
        assert x.dtype == np.float32 and x.size > 0 and np.isfinite(x).all(), n
    assert total <= 64 * 10 ** 6
    assert np.abs(np.load(out / "output.npy")).max() > 0

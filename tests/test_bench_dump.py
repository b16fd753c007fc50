"""bench.py --dump-outputs DIR: what the last timed step computed, as DIR/<name>.npy in float32, large arrays as a fixed seeded sample
within the size budget; --steps sets the number of timed steps and the result line reports ms_per_step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


@pytest.fixture()
def bench_torch(monkeypatch):
    """bench's lazily loaded modules, put back to None afterwards (importing bench must not import torch: test_bench_launcher.py)."""
    monkeypatch.setattr(bench, "torch", torch)
    monkeypatch.setattr(bench, "F", F)


def _arrays():
    g = torch.Generator().manual_seed(5)
    return {"loss": torch.tensor(1.25), "logits": torch.randn(4, 3, generator=g),
            "grad.big": torch.randn(64, 50, generator=g), "grad.bigger": torch.randn(3, 1000, generator=g).double()}


def test_dump_writes_float32_and_samples_large_arrays_the_same_way_every_time(bench_torch, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 4 * 500)           # 500 elements per array
    arrays = _arrays()
    a = bench.dump_outputs(str(tmp_path / "a"), arrays)
    b = bench.dump_outputs(str(tmp_path / "b"), {k: v.clone() for k, v in reversed(list(arrays.items()))})
    assert a["arrays"] == 4 and sorted(a["sampled"]) == ["grad.big", "grad.bigger"]
    assert sorted(os.listdir(tmp_path / "a")) == sorted(k + ".npy" for k in arrays)
    for k, v in arrays.items():
        x, y = np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy"))
        assert x.dtype == np.float32 and np.array_equal(x, y), k
        if k in a["sampled"]:
            assert x.shape == (500,) and np.isin(x, v.float().numpy().ravel()).all() and len(np.unique(x)) == 500
        else:
            assert x.shape == tuple(v.shape) and np.array_equal(x, v.numpy())
    assert a["bytes"] == sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))


def test_dump_of_flagship_sized_gradients_stays_under_64_mb(bench_torch, tmp_path):
    """KAN-VGG11 has 26 parameter tensors, 316 MB of gradients; logits and loss come on top."""
    shapes = [(1024, 2048, 9)] + [(256, 256, 9)] * 25 + [(256, 10), ()]
    names = [f"grad.p{i}" for i in range(26)] + ["logits", "loss"]
    arrays = {n: torch.zeros(s) for n, s in zip(names, shapes)}
    out = bench.dump_outputs(str(tmp_path), arrays)
    assert out["bytes"] <= 64 << 20 and out["arrays"] == 28 and "grad.p0" in out["sampled"]


def test_one_step_keeps_the_logits_of_the_step(bench_torch):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(12, 5))
    x, t = torch.randn(8, 3, 2, 2), torch.randint(0, 5, (8,))
    keep = {}
    loss = bench.one_step(model, x, t, keep=keep)
    assert torch.equal(keep["logits"], model(x).detach()) and torch.equal(loss, F.cross_entropy(keep["logits"], t))
    assert not keep["logits"].requires_grad and model[1].weight.grad is not None


@pytest.mark.parametrize("bad", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked_before_anything_runs(bad):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + bad, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr and not r.stdout.strip()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_bench_dumps_the_last_timed_step(gpu_lib, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-aux",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=560, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    doc = json.loads(lines[0])
    assert doc["steps"] == 3 and doc["ms_per_step"] > 0 and doc["dump_outputs"]["arrays"] == 28
    files = sorted(os.listdir(tmp_path))
    assert len(files) == 28 and sum(os.path.getsize(tmp_path / f) for f in files) <= 64 << 20
    assert all(np.load(tmp_path / f).dtype == np.float32 for f in files)
    assert np.load(tmp_path / "logits.npy").shape == (256, 10)
    loss = float(np.load(tmp_path / "loss.npy"))
    assert abs(loss - doc["config"]["loss"]) <= 1e-6 and np.isfinite(loss)
    assert all(np.isfinite(np.load(tmp_path / f)).all() for f in files if f.startswith("grad."))

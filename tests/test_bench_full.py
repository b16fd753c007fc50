"""bench.py without --full does only what the headline needs (set-up, warm-up, timed steps, the result line); --full adds the
auxiliary legs and the CPU baseline after the timed steps."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric": "images/sec fwd+bwd KAN-VGG11 3x32x32 bs=256/GPU", "unit": "images/sec", "higher_is_better": True, "dtype": "f32"}
EXTRAS = ("with_optimizer", "other_workloads", "cpu_baseline")


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", *extra],
                       capture_output=True, text=True, timeout=560, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    doc = json.loads(lines[0])
    assert {k: doc[k] for k in HEADLINE} == HEADLINE and doc["value"] > 0 and doc["ms_per_step"] > 0 and doc["steps"] == 3
    assert doc["roofline"]["kernels"]
    return doc


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_measures_the_headline_only(gpu_lib):
    doc = _bench()
    assert doc["full"] is False and not [k for k in EXTRAS if k in doc]


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_full_run_adds_the_auxiliary_legs_and_the_cpu_baseline(gpu_lib):
    doc = _bench("--full", "--cpu-batch", "8", "--cpu-iters", "2", "--cpu-warmup", "1")
    assert doc["full"] is True and all(k in doc for k in EXTRAS)
    legs = dict(doc["other_workloads"], with_optimizer=doc["with_optimizer"])
    assert sorted(legs) == ["cheby_alexnet", "fastkan_layer", "kan_vgg11_inference", "split_precision_forward", "with_optimizer"]
    assert not {k: v["error"] for k, v in legs.items() if "error" in v}
    assert doc["with_optimizer"]["ms_per_step"] > 0 and doc["other_workloads"]["fastkan_layer"]["hip_graph"]["matches_eager_bitwise"] is True
    assert doc["cpu_baseline"]["value"] > 0 and doc["cpu_baseline"]["gpu_over_cpu"] > 0

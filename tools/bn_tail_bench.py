#!/usr/bin/env python3
"""KAN-VGG11 built as the reference's training script builds it -- kan_norm_layer=nn.BatchNorm2d (train.py:67-68) -- at batch 256:
forward + backward ms/step, and the time of the layer tails' own kernels per step.  bench.py keeps measuring the InstanceNorm model.

Two modes, so that the profiler never sits on the timed run:

  python tools/bn_tail_bench.py [--steps 30 --warmup 10 --windows 5]
      One JSON line: ms/step of each timed window (device events around `steps` steps), their median and their spread.  A step is
      zero_grad / forward / CrossEntropy / backward, as in bench.py.  Works at any commit that has the model.

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o st -- python tools/bn_tail_bench.py --steps 10 --warmup 3 --windows 1
  python tools/bn_tail_bench.py --kernel-stats DIR --profiled-steps 13
      One JSON line from the profiler's kernel_stats.csv: ms/step of every kernel that belongs to a layer tail -- the k_bn_* kernels of
      csrc/kan_bnorm.hip, or, at a commit without them, torch's batch-norm, PReLU and max-pool kernels; k_slab_reduce at both (without the
      k_bn_* kernels it also sums the forward's slabs) -- and their sum.
      For the k_bn_* kernels also the bytes each launch kind must move (from the layer shapes and the planner's slab counts) and the
      bandwidth that makes.  No GPU is needed for this mode."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH = 256
TAIL = re.compile(r"k_bn_|k_slab_reduce|batch_norm|BatchNorm|prelu|Prelu|PReLU|max_pool|MaxPool", re.I)
KINDS = ("k_bn_fwd_partials", "k_bn_fwd_finalise", "k_bn_fwd_apply", "k_bn_bwd_partials", "k_bn_bwd_finalise", "k_bn_bwd_apply")


def build():
    import torch
    import torch.nn as nn
    from convkan_amd.models import vggkan
    torch.manual_seed(0)
    return vggkan(3, 10, arch="VGG11", kan_conv="KAN", classifier_type="Linear", kan_norm_layer=nn.BatchNorm2d).cuda().train()


def timed(args):
    import torch
    import torch.nn.functional as F
    assert torch.cuda.is_available(), "this mode measures on the GPU: there is no CPU figure"
    model = build()
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(BATCH, 3, 32, 32, device="cuda", generator=g)
    t = torch.randint(0, 10, (BATCH,), device="cuda", generator=g)

    def step():
        model.zero_grad(set_to_none=True)
        F.cross_entropy(model(x), t).backward()
    for _ in range(args.warmup):
        step()
    windows = []
    for _ in range(args.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        windows.append(e0.elapsed_time(e1) / args.steps)
    print(json.dumps({"workload": "kan_vgg11 + BatchNorm2d, fwd + bwd", "batch": BATCH, "steps": args.steps, "warmup": args.warmup,
                      "ms_per_step_windows": [round(w, 4) for w in windows], "ms_per_step": round(statistics.median(windows), 4),
                      "spread_ms": round(max(windows) - min(windows), 4)}))


def tail_bytes():
    """{launch kind: bytes per step} the k_bn_* launches of the model must move, from shapes alone: the layers' output planes, the
    planner's forward slab counts, 4-byte data, one argmax byte per window, 8-byte workspace values (3 per plane forward, 5 backward)."""
    import torch.nn as nn
    from convkan_amd import KANConv2DLayer, ops
    from convkan_amd.models.kan_vgg import cfgs
    out = dict.fromkeys(KINDS, 0)
    spec = KANConv2DLayer(1, 1, 3, padding=1, base_activation=nn.SiLU).conv_spec()      # the model's layers: 3x3, pad 1, SiLU base branch
    cin, hw, entries = 3, 32, cfgs["VGG11"]
    for i, v in enumerate(entries):
        if v == "M":
            hw //= 2
            continue
        cout, pooled = int(v), i + 1 < len(entries) and entries[i + 1] == "M"
        slabs = ops._plan_cached(*ops._plan_key(spec, (BATCH, cin, hw, hw), cout))[2].fwd_splits
        n, planes = BATCH * cout * hw * hw, BATCH * cout
        y = n // 4 * 5 if pooled else n * 4                       # pooled: a quarter of the values plus their argmax bytes
        out["k_bn_fwd_partials"] += slabs * n * 4 + (n * 4 if slabs > 1 else 0) + planes * 24
        out["k_bn_fwd_finalise"] += planes * 24
        out["k_bn_fwd_apply"] += n * 4 + y
        out["k_bn_bwd_partials"] += n * 4 + y + planes * 40
        out["k_bn_bwd_finalise"] += planes * 40
        out["k_bn_bwd_apply"] += n * 4 + y + n * 4
        cin = cout
    return out


def kernel_stats(args):
    path = sorted(glob.glob(os.path.join(args.kernel_stats, "**", "*kernel_stats.csv"), recursive=True))[0]
    rows = [r for r in csv.DictReader(open(path)) if TAIL.search(r["Name"])]
    per_step = lambda ns: ns / args.profiled_steps / 1e6
    kernels = {r["Name"][:120]: round(per_step(float(r["TotalDurationNs"])), 4) for r in rows}
    res = {"source": "rocprofv3 --kernel-trace --stats", "profiled_steps": args.profiled_steps, "tail_kernels_ms_per_step": kernels,
           "tail_ms_per_step": round(sum(kernels.values()), 4)}
    if any("k_bn_" in r["Name"] for r in rows):
        need = tail_bytes()
        res["launches"] = {}
        for kind in KINDS:
            ms = per_step(sum(float(r["TotalDurationNs"]) for r in rows if kind in r["Name"]))
            res["launches"][kind] = {"ms_per_step": round(ms, 4), "mbytes_per_step": round(need[kind] / 1e6, 2),
                                     "tbytes_per_s": round(need[kind] / (ms * 1e-3) / 1e12, 3) if ms > 0 else None}
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --stats run of this tool")
    ap.add_argument("--profiled-steps", type=int, default=13, help="steps the profiled run made, warm-up included")
    a = ap.parse_args()
    kernel_stats(a) if a.kernel_stats else timed(a)

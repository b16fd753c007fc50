#!/usr/bin/env python3
"""What recording the optimizer into the step's HIP graph buys: three settings of the SAME training step in ONE process.

  python tools/full_graph_bench.py [--samples 20 --warmup 5 --out profiles/full_graph_step.json]

Settings (each on its own deep copy of the model, the same batch):
  eager              train_step: zero_grad / forward / loss / backward eager, FusedAdamW.step() eager
  graph_fwd_bwd      GraphedStep (forward / loss / backward replayed) + an eager FusedAdamW.step() after every replay -- the best before
                     FusedAdamW(capturable=True) existed, and the setting the third is compared with
  graph_full_step    GraphedStep(optimizer=FusedAdamW(capturable=True)): the optimizer step is part of the replay
Workloads: KAN-VGG11 (CIFAR shapes, torch's CrossEntropyLoss) at batch 4, 16 and 256, and the BASELINE config-2 step, one
FastKANConv2DLayer(3, 64, 3) on 256x3x32x32 whose backward starts from a fixed upstream gradient (here as the criterion sum(y * upstream), the same
in all three settings).

A sample is `inner` consecutive steps between two HIP events on the launch stream, divided by `inner` (the host may run ahead inside a sample, as it
does in a training loop); the settings are ALTERNATED sample by sample, never measured in blocks.  Reported per setting: median and min .. max of the
samples.  graph_full_step against graph_fwd_bwd: the difference of the medians, and whether the two min .. max ranges overlap -- only where they do
not is the difference called a gain (or a loss); otherwise it is reported as measured.
One JSON line on stdout; `--out` also writes it to a file.  There is no CPU figure: without a GPU the tool fails."""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = ("eager", "graph_fwd_bwd", "graph_full_step")


def _summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "samples": len(ms)}


def _against(base, s):
    """`s` against `base`: positive gain = `s` is faster; separated = the two min .. max ranges do not overlap."""
    return {"gain_ms": round(base["median_ms"] - s["median_ms"], 4), "speedup_median": round(base["median_ms"] / s["median_ms"], 3),
            "ranges_do_not_overlap": bool(s["max_ms"] < base["min_ms"] or base["max_ms"] < s["min_ms"])}


def _runners(base, data, target, criterion):
    """{setting: a callable running one step} -- every setting on its own copy of `base`."""
    import convkan_amd as K
    hyper = dict(lr=1e-3, weight_decay=1e-4)
    run = {}
    m0 = copy.deepcopy(base)
    o0 = K.FusedAdamW(m0.parameters(), **hyper)
    run["eager"] = lambda: K.train_step(m0, data, target, o0, criterion)
    m1 = copy.deepcopy(base)
    o1 = K.FusedAdamW(m1.parameters(), **hyper)
    s1 = K.GraphedStep(m1, data, target, criterion)

    def fwd_bwd_then_step():
        loss = s1(data, target)
        o1.step()
        return loss
    run["graph_fwd_bwd"] = fwd_bwd_then_step
    m2 = copy.deepcopy(base)
    o2 = K.FusedAdamW(m2.parameters(), **hyper, capturable=True)
    s2 = K.GraphedStep(m2, data, target, criterion, optimizer=o2)
    run["graph_full_step"] = lambda: s2(data, target)
    return run


def measure(name, base, data, target, criterion, args, inner):
    import torch
    run = _runners(base, data, target, criterion)
    for _ in range(args.warmup):
        for k in SETTINGS:
            run[k]()
    torch.cuda.synchronize()
    times = {k: [] for k in SETTINGS}
    for _ in range(args.samples):                                        # alternated sample by sample
        for k in SETTINGS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                run[k]()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / inner)
    res = {"workload": name, "batch": int(data.shape[0]), "steps_per_sample": inner}
    for k in SETTINGS:
        res[k] = _summary(times[k])
    res["graph_fwd_bwd"]["vs_eager"] = _against(res["eager"], res["graph_fwd_bwd"])
    res["graph_full_step"]["vs_eager"] = _against(res["eager"], res["graph_full_step"])
    res["graph_full_step"]["vs_graph_fwd_bwd"] = _against(res["graph_fwd_bwd"], res["graph_full_step"])
    return res


def main(args):
    import torch
    import torch.nn as nn
    import convkan_amd as K
    from convkan_amd.models import vggkan

    class Upstream(nn.Module):                                           # config 2 has no loss head: d(sum(y * upstream)) / dy = upstream
        def forward(self, y, upstream):
            return (y * upstream).sum()
    out = []
    g = torch.Generator(device="cuda").manual_seed(1)
    for bs in (4, 16, 256):
        torch.manual_seed(0)
        base = vggkan(3, 10, arch="VGG11", kan_conv="KAN", classifier_type="Linear").cuda().train()
        x = torch.randn(bs, 3, 32, 32, device="cuda", generator=g)
        t = torch.randint(0, 10, (bs,), device="cuda", generator=g)
        out.append(measure("kan_vgg11", base, x, t, nn.CrossEntropyLoss(), args, inner=2 if bs == 256 else 10))
        del base
        torch.cuda.empty_cache()
    torch.manual_seed(0)
    layer = K.FastKANConv2DLayer(3, 64, 3).cuda().train()
    x = torch.randn(256, 3, 32, 32, device="cuda", generator=g)
    with torch.no_grad():
        up = torch.randn(layer(x).shape, device="cuda", generator=g)
    out.append(measure("fastkan_layer (BASELINE config 2)", layer, x, up, Upstream(), args, inner=10))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5, help="untimed rounds of all three settings")
    ap.add_argument("--samples", type=int, default=20, help="timed samples of each setting")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU figure"
    res = {"tool": "tools/full_graph_bench.py", "device": torch.cuda.get_device_name(0), "workloads": main(a)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")

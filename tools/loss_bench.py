#!/usr/bin/env python3
"""A/B of the device-side criterion (K.CrossEntropyLoss, csrc/kan_loss.hip) against torch's nn.CrossEntropyLoss, in ONE process.

  python tools/loss_bench.py [--steps 20 --warmup 5 --inner 50 --out profiles/xent_bench_ab.json]

1. The criterion alone, forward + backward on fp32 logits [B, C] at (256, 10), (256, 100) and (128, 1000), under three settings: torch's,
   K.CrossEntropyLoss() and K.CrossEntropyLoss(metrics=m) (the counters of the test metrics in the same launches).  One sample = `--inner`
   forward + backward pairs between two HIP events on the launch stream (one pair is a few tens of microseconds: mostly the host's launch
   work, which is what a training step pays for it); reported per pair.
2. KAN-VGG11 at batch 256, K.train_step (forward, loss, backward, FusedAdamW) with either criterion; one sample = one step.
The settings are ALTERNATED sample by sample (never two blocks).  Reported per setting: median and min .. max; against torch's: the difference
of the medians and whether it exceeds the two spreads combined -- the project's rule for calling a difference separated; otherwise it is
reported as measured.  One JSON line on stdout; `--out` also writes it to a file.  There is no CPU figure: without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(256, 10), (256, 100), (128, 1000)]
BATCH = 256


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _summary(ms):
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5), "spread_ms": round(max(ms) - min(ms), 5),
            "samples": len(ms)}


def _against(base, s):
    """`s` against `base`: median difference (positive: `s` is faster) and the two-spreads rule."""
    gain = base["median_ms"] - s["median_ms"]
    return {"gain_ms": round(gain, 5), "speedup_median": round(base["median_ms"] / s["median_ms"], 3),
            "separated_by_more_than_both_spreads": bool(abs(gain) > base["spread_ms"] + s["spread_ms"])}


def _alternate(settings, args, per_sample=1):
    """{name: summary} of the callables in `settings`, warmed up and then timed in turn, sample by sample; times per unit of work."""
    import torch
    for _ in range(args.warmup):
        for fn in settings.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in settings}
    for _ in range(args.steps):
        for k, fn in settings.items():
            times[k].append(_timed(fn) / per_sample)
    res = {k: _summary(v) for k, v in times.items()}
    base = next(iter(settings))
    for k in list(settings)[1:]:
        res[k]["vs_" + base] = _against(res[base], res[k])
    return res


def criterion_ab(args, B, Cn):
    import torch
    import torch.nn as nn
    import convkan_amd as K
    g = torch.Generator(device="cuda").manual_seed(B + Cn)
    logits = (3.0 * torch.randn(B, Cn, device="cuda", generator=g)).requires_grad_(True)
    target = torch.randint(0, Cn, (B,), device="cuda", generator=g)
    crits = {"torch": nn.CrossEntropyLoss(), "kan": K.CrossEntropyLoss(), "kan_with_metrics": K.CrossEntropyLoss(metrics=K.ClassMetrics(Cn, "cuda"))}

    def pairs(crit):
        def run():
            for _ in range(args.inner):
                logits.grad = None
                crit(logits, target).backward()
        return run
    res = {"workload": "criterion fwd + bwd", "B": B, "C": Cn, "pairs_per_sample": args.inner, "unit": "ms per forward + backward pair"}
    res.update(_alternate({k: pairs(c) for k, c in crits.items()}, args, per_sample=args.inner))
    return res


def model_ab(args):
    import torch
    import torch.nn as nn
    import convkan_amd as K
    from convkan_amd.models import vggkan
    torch.manual_seed(0)
    model = vggkan(3, 10, arch="VGG11", kan_conv="KAN", classifier_type="Linear").cuda().train()
    opt = K.FusedAdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(BATCH, 3, 32, 32, device="cuda", generator=g)
    t = torch.randint(0, 10, (BATCH,), device="cuda", generator=g)
    crits = {"torch": nn.CrossEntropyLoss(), "kan_with_metrics": K.CrossEntropyLoss(metrics=K.ClassMetrics(10, "cuda"))}
    res = {"workload": "kan_vgg11 train_step (fwd + loss + bwd + FusedAdamW)", "batch": BATCH, "unit": "ms per step"}
    res.update(_alternate({k: (lambda c=c: K.train_step(model, x, t, opt, criterion=c)) for k, c in crits.items()}, args))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="timed samples of each setting")
    ap.add_argument("--inner", type=int, default=50, help="forward + backward pairs per sample of the criterion alone")
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU figure"
    res = {"tool": "tools/loss_bench.py", "device": torch.cuda.get_device_name(0), "criterion": [criterion_ab(a, B, Cn) for B, Cn in SHAPES]}
    if not a.skip_model:
        res["model"] = model_ab(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")

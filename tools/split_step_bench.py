#!/usr/bin/env python3
"""A/B of the opt-in split-precision TRAINING step (ops.split_precision_training) against the exact step and the split backward alone, in ONE process.

  python tools/split_step_bench.py [--steps 20 --warmup 5 --out profiles/split_training_step_ab.json]

KAN-VGG11, batch 256, forward + backward (no optimizer), under three settings -- exact, `ops.split_precision_backward()` (the two backward launches of the
layers in scope), `ops.split_precision_training()` (the forward launch as well) -- ALTERNATED step by step (never two blocks), each step between two HIP
events on the launch stream.  Reported per setting: median and min .. max; against the exact step and, for the training context, against the split
backward alone: the difference of the medians and whether it exceeds the two spreads combined -- the project's rule for calling a difference separated;
otherwise it is reported as measured.  Also: the max-normalised distance of the logits and of every conv-weight gradient of the training context from the
exact step, on the same batch.
One JSON line on stdout; `--out` also writes it to a file.  There is no CPU figure: without a GPU the tool fails."""
import argparse
import contextlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH = 256


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def _summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "spread_ms": round(max(ms) - min(ms), 4),
            "steps": len(ms)}


def _against(base, s):
    """`s` against `base`: median difference (positive: `s` is faster) and the two-spreads rule."""
    gain = base["median_ms"] - s["median_ms"]
    return {"gain_ms": round(gain, 4), "speedup_median": round(base["median_ms"] / s["median_ms"], 3),
            "separated_by_more_than_both_spreads": bool(abs(gain) > base["spread_ms"] + s["spread_ms"])}


def _relerr(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def model_ab(args):
    import torch
    import torch.nn.functional as F
    from convkan_amd import ops
    from convkan_amd.models import vggkan
    torch.manual_seed(0)
    model = vggkan(3, 10, arch="VGG11", kan_conv="KAN", classifier_type="Linear").cuda().train()
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(BATCH, 3, 32, 32, device="cuda", generator=g)
    t = torch.randint(0, 10, (BATCH,), device="cuda", generator=g)
    settings = {"exact": contextlib.nullcontext, "split_backward_context": ops.split_precision_backward, "split_training_context": ops.split_precision_training}

    def step(ctx):
        with ctx():
            model.zero_grad(set_to_none=True)
            y = model(x)
            F.cross_entropy(y, t).backward()
        return y
    for _ in range(args.warmup):
        for ctx in settings.values():
            step(ctx)
    torch.cuda.synchronize()
    times = {k: [] for k in settings}
    for _ in range(args.steps):                                      # alternated step by step
        for k, ctx in settings.items():
            times[k].append(_timed(lambda: step(ctx))[0])
    res = {"workload": "kan_vgg11 fwd + bwd", "batch": BATCH}
    for k in settings:
        res[k] = _summary(times[k])
    res["split_backward_context"]["vs_exact"] = _against(res["exact"], res["split_backward_context"])
    res["split_training_context"]["vs_exact"] = _against(res["exact"], res["split_training_context"])
    res["split_training_context"]["vs_split_backward"] = _against(res["split_backward_context"], res["split_training_context"])
    # distances on one batch, the dropout masks pinned by re-seeding before each step
    seen = {}
    for k in ("exact", "split_training_context"):
        torch.manual_seed(5)
        y = step(settings[k]).detach().clone()
        seen[k] = (y, {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.dim() == 4})
    torch.cuda.synchronize()
    res["split_training_vs_exact_maxnorm"] = {"logits": _relerr(seen["split_training_context"][0], seen["exact"][0]),
                                              "conv_weight_gradients": {n: _relerr(gr, seen["exact"][1][n]) for n, gr in seen["split_training_context"][1].items()}}
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="timed model steps of each setting")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU figure"
    res = {"tool": "tools/split_step_bench.py", "device": torch.cuda.get_device_name(0), "model": model_ab(a)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")

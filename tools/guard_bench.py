#!/usr/bin/env python3
"""What the device-side anomaly mode costs: the non-finite guard of FusedAdamW (opt.skip_nonfinite) and AnomalyProbe, in ONE process.

  python tools/guard_bench.py [--samples 15 --warmup 3 --out profiles/guard_bench.json]

Two workloads, each under settings ALTERNATED sample by sample (never two blocks), each sample between two HIP events on the launch stream:

  optimizer_step               FusedAdamW(capturable=True).step() on KAN-VGG11's parameters with fixed finite gradients, 50 calls per sample:
                               guard_off / guard_on, without clipping and with max_grad_norm = 1.0 (four optimizers on four copies of the model).
                               The probe hangs on the model, not on the optimizer: it has no figure here.
  kan_vgg11_bs256_recorded_step   GraphedStep(optimizer=...) at batch 256, 2 replays per sample: guard_off / guard_on / guard_and_probe_on
                               (three copies of the model, three recordings).

Reported per setting: median and min .. max; against guard_off: the difference of the medians and whether the two min .. max ranges overlap.
guard_off issues exactly the launches of a tree without this feature (the switch and the probe are opt-in), so its figure is the one to hold
against profiles/clip_bench.json and profiles/full_graph_step.json.  The counters are read once at the end, as a check that nothing was
skipped and the probe found nothing.  One JSON line on stdout; `--out` also writes it to a file.  There is no CPU figure: without a GPU the tool fails."""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH = 256


def _summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "samples": len(ms)}


def _against(base, s):
    """`s` against `base`: positive added_ms = `s` is slower."""
    return {"added_ms": round(s["median_ms"] - base["median_ms"], 4), "ratio_of_medians": round(s["median_ms"] / base["median_ms"], 4),
            "ranges_do_not_overlap": bool(s["max_ms"] < base["min_ms"] or base["max_ms"] < s["min_ms"])}


def _alternate(run, args, inner):
    import torch
    for _ in range(args.warmup):
        for fn in run.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in run}
    for _ in range(args.samples):
        for k, fn in run.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / inner)
    return {k: _summary(v) for k, v in times.items()}


def optimizer_step(base, args):
    import torch
    import convkan_amd as K
    run, opts = {}, {}
    for clip in (None, 1.0):
        for guard in (False, True):
            model = copy.deepcopy(base)
            opt = K.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, capturable=True, max_grad_norm=clip)
            opt.skip_nonfinite = guard
            g = torch.Generator(device="cuda").manual_seed(2)
            for p in model.parameters():
                p.grad = torch.randn(p.shape, device="cuda", generator=g) * 1e-3
            name = ("guard_on" if guard else "guard_off") + ("_clip" if clip is not None else "")
            run[name], opts[name] = opt.step, opt
    res = {"params": sum(p.numel() for p in base.parameters()), "calls_per_sample": 50, **_alternate(run, args, 50)}
    res["guard_on"]["vs_guard_off"] = _against(res["guard_off"], res["guard_on"])
    res["guard_on_clip"]["vs_guard_off_clip"] = _against(res["guard_off_clip"], res["guard_on_clip"])
    res["skipped_steps"] = {k: o.guard_report()["skipped_steps"] for k, o in opts.items() if o.skip_nonfinite}
    return res


def recorded_step(base, args):
    import torch
    import torch.nn as nn
    import convkan_amd as K
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(BATCH, 3, 32, 32, device="cuda", generator=g)
    t = torch.randint(0, 10, (BATCH,), device="cuda", generator=g)
    run, opts, probe = {}, {}, None
    for name, guard, with_probe in (("guard_off", False, False), ("guard_on", True, False), ("guard_and_probe_on", True, True)):
        model = copy.deepcopy(base)
        opt = K.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, capturable=True)
        opt.skip_nonfinite = guard
        if with_probe:
            probe = K.AnomalyProbe(model)
        step = K.GraphedStep(model, x, t, nn.CrossEntropyLoss(), optimizer=opt)
        run[name], opts[name] = (lambda s=step: s(x, t)), opt
    probe.reset()
    res = {"batch": BATCH, "replays_per_sample": 2, **_alternate(run, args, 2)}
    for k in ("guard_on", "guard_and_probe_on"):
        res[k]["vs_guard_off"] = _against(res["guard_off"], res[k])
    res["guard_and_probe_on"]["vs_guard_on"] = _against(res["guard_on"], res["guard_and_probe_on"])
    res["skipped_steps"] = {k: o.guard_report()["skipped_steps"] for k, o in opts.items() if o.skip_nonfinite}
    res["probe"] = {"slots": len(probe.slots), "ticks": int(probe.tick), "slots_with_a_non_finite_value": len(probe.report())}
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3, help="untimed rounds of all settings")
    ap.add_argument("--samples", type=int, default=15, help="timed samples of each setting")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU figure"
    from convkan_amd.models import vggkan
    torch.manual_seed(0)
    base = vggkan(3, 10, arch="VGG11", kan_conv="KAN", classifier_type="Linear").cuda().train()
    res = {"tool": "tools/guard_bench.py", "device": torch.cuda.get_device_name(0), "optimizer_step": optimizer_step(base, a)}
    torch.cuda.empty_cache()
    res["kan_vgg11_bs256_recorded_step"] = recorded_step(base, a)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")

#!/usr/bin/env python3
"""What gradient accumulation (FusedAdamW.accumulate_steps) costs per optimizer call, in ONE process.

  python tools/accum_bench.py [--samples 15 --warmup 3 --out profiles/accum_bench.json]

FusedAdamW.step() on KAN-VGG11's parameters with fixed finite gradients, k = 4, in both modes.  Per mode two optimizers on two copies of the
model: `plain` (accumulate_steps = 1: the launches of a tree without this feature) and one with accumulate_steps = 4, whose calls are told apart
by their place in the window -- `first` (m = 0: the accumulator is overwritten), `middle` (m = 1, 2: acc += g) and `boundary` (m = 3: the mean, then
the step).  The settings ALTERNATE sample by sample (never two blocks): a sample is `windows` rounds of [plain, first, middle, middle, boundary],
every call between two HIP events of its own on the launch stream.  Reported per setting: median and min .. max of the per-sample means.

Derived, and named for what they are -- CALL times over the bytes the algorithm needs, not kernel times (a call is one launch per parameter group
plus the host's work; run rocprofv3 --kernel-trace for the kernels alone):
  achieved_GBps        plain: 28 B per element (p, m, v read and written, g read); classic first: 8 B; classic middle: 12 B -- in the classic
                       mode a call inside the window launches the accumulate kernel and nothing else, so its time is that launch's
  idle_launches_ms     capturable middle - classic middle: what the statistics-free advance and step launches on an all-zero gated table cost in
                       the mode that decides on the device, and whether that is more than the accumulate launch itself
One JSON line on stdout; `--out` also writes it to a file.  There is no CPU figure: without a GPU the tool fails."""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K_STEPS = 4
ORDER = ("plain", "first", "middle", "middle", "boundary")


def _summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "samples": len(ms)}


def _against(base, s):
    """`s` against `base`: positive added_ms = `s` is slower."""
    return {"added_ms": round(s["median_ms"] - base["median_ms"], 4), "ratio_of_medians": round(s["median_ms"] / base["median_ms"], 4),
            "ranges_do_not_overlap": bool(s["max_ms"] < base["min_ms"] or base["max_ms"] < s["min_ms"])}


def _gbps(bytes_per_element, elements, s):
    return round(bytes_per_element * elements / (s["median_ms"] * 1e-3) / 1e9, 1)


def optimizer_calls(base, args, capturable):
    import torch
    import convkan_amd as K
    opts = {}
    for name, k in (("plain", 1), ("accum", K_STEPS)):
        model = copy.deepcopy(base)
        opt = K.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, capturable=capturable)
        opt.accumulate_steps = k
        g = torch.Generator(device="cuda").manual_seed(2)
        for p in model.parameters():
            p.grad = torch.randn(p.shape, device="cuda", generator=g) * 1e-3
        opts[name] = (model, opt)
    plain, accum = opts["plain"][1], opts["accum"][1]

    def round_of_calls(timed):
        for i, name in enumerate(ORDER):
            fn = plain.step if name == "plain" else accum.step
            if timed is None:
                fn()
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            timed.append((name, e0, e1))

    for _ in range(args.warmup):
        round_of_calls(None)
    torch.cuda.synchronize()
    assert accum.micro_step == 0
    times = {name: [] for name in dict.fromkeys(ORDER)}
    for _ in range(args.samples):
        timed = []
        for _ in range(args.windows):
            round_of_calls(timed)
        torch.cuda.synchronize()
        per = {name: [] for name in times}
        for name, e0, e1 in timed:
            per[name].append(e0.elapsed_time(e1))
        for name, v in per.items():
            times[name].append(sum(v) / len(v))
    assert accum.micro_step == 0
    res = {name: _summary(v) for name, v in times.items()}
    for name in ("first", "middle", "boundary"):
        res[name]["vs_plain"] = _against(res["plain"], res[name])
    steps = accum.state_dict()["state"][0]["step"]
    res["windows_run"] = int(steps)                                          # one step per window: warm-up rounds + samples x windows
    assert int(steps) == args.warmup + args.samples * args.windows, (int(steps), args)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3, help="untimed rounds of all settings")
    ap.add_argument("--samples", type=int, default=15, help="timed samples of each setting")
    ap.add_argument("--windows", type=int, default=10, help="rounds of [plain, first, middle, middle, boundary] per sample")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU figure"
    from convkan_amd.models import vggkan
    torch.manual_seed(0)
    base = vggkan(3, 10, arch="VGG11", kan_conv="KAN", classifier_type="Linear").cuda().train()
    elements = sum(p.numel() for p in base.parameters() if p.requires_grad)
    res = {"tool": "tools/accum_bench.py", "device": torch.cuda.get_device_name(0), "params": elements, "accumulate_steps": K_STEPS,
           "calls_per_sample": {"plain": a.windows, "first": a.windows, "middle": 2 * a.windows, "boundary": a.windows}}
    for mode, capturable in (("classic", False), ("capturable", True)):
        res[mode] = optimizer_calls(base, a, capturable)
        torch.cuda.empty_cache()
    c, d = res["classic"], res["capturable"]
    res["achieved_GBps_of_call_time"] = {"classic_plain_step_28B": _gbps(28, elements, c["plain"]),
                                         "classic_first_accumulate_8B": _gbps(8, elements, c["first"]),
                                         "classic_middle_accumulate_12B": _gbps(12, elements, c["middle"]),
                                         "capturable_plain_step_28B": _gbps(28, elements, d["plain"])}
    idle = round(d["middle"]["median_ms"] - c["middle"]["median_ms"], 4)
    res["idle_launches_ms"] = {"capturable_middle_minus_classic_middle": idle, "accumulate_launch_ms": c["middle"]["median_ms"],
                               "more_than_the_accumulate_launch": bool(idle > c["middle"]["median_ms"])}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")

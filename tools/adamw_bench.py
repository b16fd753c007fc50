"""HBM roofline of the fused AdamW step (28 B per element; 32 B with max_grad_norm: the gradient is read twice) and the cost of a full
training step with it on KAN-VGG11 bs 256, next to torch.optim.AdamW (foreach and fused) on the same model.
python tools/adamw_bench.py  [--json=out.json]  [--clip-json=profiles/clip_bench.json]

--clip-json: what clipping costs, measured in ONE process with the two settings ALTERNATED window by window: the optimizer step alone
(fused_flat against fused_flat_clip, max_grad_norm=1.0) and the recorded KAN-VGG11 bs 256 step (GraphedStep(optimizer=FusedAdamW(capturable=True)))
without and with clipping.  Per row the median and min .. max of the windows; the ratio of the medians next to what the bytes alone predict (32 / 28)."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import convkan_amd as K  # noqa: E402
from convkan_amd.models import vggkan  # noqa: E402

PEAK_GBS = 8000.0


def timed(fn, n=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def windows(fns, n, warm, rounds):
    """{name: [ms per call, one figure per window]}: the callables timed ALTERNATELY, `rounds` windows of `n` calls each."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, n=n, warm=0))
    return ms


def _row(ms, **extra):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), windows=len(ms), **extra)


def _pair(plain, clip, expected):
    ratio = clip["median_ms"] / plain["median_ms"]
    return dict(ratio_of_medians=round(ratio, 4), expected_from_bytes=round(expected, 4), added_ms=round(clip["median_ms"] - plain["median_ms"], 4),
                ranges_do_not_overlap=bool(plain["max_ms"] < clip["min_ms"] or clip["max_ms"] < plain["min_ms"]))


def clip_ab(path, max_grad_norm=1.0):
    x, t = torch.randn(256, 3, 32, 32, device="cuda"), torch.randint(0, 10, (256,), device="cuda")
    crit = torch.nn.CrossEntropyLoss()

    def model():
        torch.manual_seed(0)
        return vggkan(3, 10, arch="VGG11", kan_conv="KAN", classifier_type="Linear").cuda().train()
    out = {"tool": "tools/adamw_bench.py --clip-json", "device": torch.cuda.get_device_name(0), "max_grad_norm": max_grad_norm}
    steps = {}
    for name, kw in (("fused_flat", {}), ("fused_flat_clip", dict(max_grad_norm=max_grad_norm))):
        m = model()
        opt = K.FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-4, **kw)
        K.train_step(m, x, t, opt, crit)                       # gradients exist from here on
        steps[name] = opt.step
    nparam = sum(p.numel() for p in m.parameters())
    ms = windows(steps, n=200, warm=20, rounds=9)
    rows = {k: _row(v, algorithmic_GBps=round((32.0 if k.endswith("clip") else 28.0) * nparam / (statistics.median(v) * 1e-3) / 1e9, 1)) for k, v in ms.items()}
    out["optimizer_step"] = dict(params=nparam, calls_per_window=200, **rows, clip_vs_plain=_pair(rows["fused_flat"], rows["fused_flat_clip"], 32.0 / 28.0))
    print("optimizer_step", json.dumps(out["optimizer_step"]), flush=True)
    del steps, m, opt
    torch.cuda.empty_cache()
    replays = {}
    for name, kw in (("recorded_step", {}), ("recorded_step_clip", dict(max_grad_norm=max_grad_norm))):
        m = model()
        opt = K.FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-4, capturable=True, **kw)
        step = K.GraphedStep(m, x, t, crit, optimizer=opt)
        replays[name] = lambda step=step: step(x, t)
    ms = windows(replays, n=5, warm=3, rounds=9)
    rows = {k: _row(v) for k, v in ms.items()}
    plain_ms = out["optimizer_step"]["fused_flat"]["median_ms"]
    out["kan_vgg11_bs256_recorded_step"] = dict(calls_per_window=5, **rows, clip_vs_plain=_pair(
        rows["recorded_step"], rows["recorded_step_clip"], 1.0 + plain_ms * (32.0 / 28.0 - 1.0) / rows["recorded_step"]["median_ms"]))
    print("recorded_step", json.dumps(out["kan_vgg11_bs256_recorded_step"]), flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    for a in sys.argv:
        if a.startswith("--clip-json="):
            return clip_ab(a.split("=", 1)[1])
    out = {}
    torch.manual_seed(0)
    x, t = torch.randn(256, 3, 32, 32, device="cuda"), torch.randint(0, 10, (256,), device="cuda")
    crit = torch.nn.CrossEntropyLoss()
    for name in ("fused_flat", "fused_flat_clip", "torch_foreach", "torch_fused"):
        torch.manual_seed(0)
        m = vggkan(3, 10, arch="VGG11", kan_conv="KAN", classifier_type="Linear").cuda().train()
        nparam = sum(p.numel() for p in m.parameters())
        if name.startswith("fused_flat"):
            opt = K.FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0 if name == "fused_flat_clip" else None)
        else:
            opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4, foreach=name == "torch_foreach", fused=name == "torch_fused")
        K.train_step(m, x, t, opt, crit)                       # gradients exist from here on

        def fwd_bwd():
            opt.zero_grad()
            crit(m(x), t).backward()
        ms_step_only = timed(opt.step)
        ms_fb = timed(fwd_bwd, n=10, warm=3)
        ms_full = timed(lambda: K.train_step(m, x, t, opt, crit), n=10, warm=3)
        gbs = (32.0 if name == "fused_flat_clip" else 28.0) * nparam / (ms_step_only * 1e-3) / 1e9
        out[name] = dict(params=nparam, optimizer_step_ms=round(ms_step_only, 4), algorithmic_GBps=round(gbs, 1),
                         frac_of_hbm_peak=round(gbs / PEAK_GBS, 3), fwd_bwd_ms=round(ms_fb, 3), train_step_ms=round(ms_full, 3),
                         images_per_s=round(256 / (ms_full * 1e-3), 1))
        print(name, json.dumps(out[name]), flush=True)
        del m, opt
        torch.cuda.empty_cache()
    for a in sys.argv:
        if a.startswith("--json="):
            json.dump(out, open(a.split("=", 1)[1], "w"), indent=1)


if __name__ == "__main__":
    t0 = time.time()
    main()
    print(f"done in {time.time() - t0:.0f} s")

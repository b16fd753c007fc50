#!/usr/bin/env python3
"""A/B of the opt-in split-precision input gradient (kan_conv_bwd_data_split) against the exact fp32-MFMA bwd-data of the same library, in ONE process.

  python tools/split_bwd_data_bench.py [--launches 30 --warmup 5 --steps 20 --out profiles/split_bwd_data_bench_ab.json]

Per KAN-VGG11 layer in scope at batch 256 (64 -> 128 @ 16x16, 128 -> 256 @ 8x8, 256 -> 256 @ 8x8): the exact side is what the backward runs today --
`kan_conv_bwd_data` into the plan's slabs plus `kan_slab_reduce` where there is more than one -- the split side is `kan_conv_bwd_data_split` with cut
weights at hand.  The two are ALTERNATED launch by launch (never two blocks), each launch between two HIP events on the launch stream; reported: median
and min .. max of both, the useful TFLOP/s (2 * B * H * W * C * 9 planes * O * 9 taps over the median), the max-normalised distance of the two results,
and whether the split side wins by more than the two spreads combined.  The weight cut (`kan_split_pack_weights_bwd_data`) is timed on its own.
Then the KAN-VGG11 batch-256 forward + backward step with and without `ops.split_precision_backward_data()`, alternated step by step, the same way.
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
SHAPES = [(64, 128, 16), (128, 256, 8), (256, 256, 8)]


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
            "launches": len(ms)}


def layer_ab(C_, O_, PW, args):
    import torch
    import convkan_amd as K
    from convkan_amd import ops
    torch.manual_seed(C_ + PW)
    layer = K.KANConv2DLayer(C_, O_, 3, padding=1, base_activation=torch.nn.SiLU).cuda()
    spec, wb, ws = layer.conv_spec(), layer.base_conv[0].weight.detach(), layer.spline_conv[0].weight.detach()
    x = torch.randn(BATCH, C_, PW, PW, device="cuda")
    dz = torch.randn(BATCH, O_, PW, PW, device="cuda")
    _, packed, _, _, plan = ops._conv_forward(spec, x, None, [wb], [ws], True)
    exact = lambda: ops._conv_backward(spec, x, None, packed, dz, True, False, False)[0]      # kan_conv_bwd_data (+ kan_slab_reduce), as the backward runs it
    _, wcd = ops.kan_conv_bwd_data_split(spec, x, dz, wb, ws)
    split = lambda: ops.kan_conv_bwd_data_split(spec, x, dz, None, None, wcd)[0]
    for _ in range(args.warmup):
        exact(), split()
    torch.cuda.synchronize()
    t_exact, t_split = [], []
    for _ in range(args.launches):                                   # alternated, never two blocks
        ms, dx_e = _timed(exact); t_exact.append(ms)
        ms, dx_s = _timed(split); t_split.append(ms)
    geom, basis, _ = ops._plan_cached(*ops._plan_key(spec, x.shape, O_))
    t_cut = [_timed(lambda: ops._cut_weights_bwd_data(geom, basis, wb, ws, wcd))[0] for _ in range(args.launches)]
    e, s = _summary(t_exact), _summary(t_split)
    flop = 2.0 * BATCH * PW * PW * C_ * 9 * O_ * 9
    e["useful_tflops"], s["useful_tflops"] = round(flop / e["median_ms"] / 1e9, 1), round(flop / s["median_ms"] / 1e9, 1)
    return {"shape": f"{C_}->{O_} @{PW}x{PW} B={BATCH}", "exact_slabs": int(plan.bwd_data_splits), "exact": e, "split": s, "weight_cut": _summary(t_cut),
            "cut_weight_mbytes": round(wcd.numel() / 1e6, 2), "speedup_median": round(e["median_ms"] / s["median_ms"], 3),
            "split_faster_by_more_than_both_spreads": bool(e["median_ms"] - s["median_ms"] > e["spread_ms"] + s["spread_ms"]),
            "dx_split_vs_exact_maxnorm": float((dx_s - dx_e).abs().max() / dx_e.abs().max())}


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

    def step(ctx):
        with ctx():
            model.zero_grad(set_to_none=True)
            F.cross_entropy(model(x), t).backward()
    for _ in range(args.warmup):
        step(contextlib.nullcontext), step(ops.split_precision_backward_data)
    torch.cuda.synchronize()
    t_exact, t_split = [], []
    for _ in range(args.steps):
        t_exact.append(_timed(lambda: step(contextlib.nullcontext))[0])
        t_split.append(_timed(lambda: step(ops.split_precision_backward_data))[0])
    e, s = _summary(t_exact), _summary(t_split)
    return {"workload": "kan_vgg11 fwd + bwd", "batch": BATCH, "exact": e, "split_bwd_data_context": s, "speedup_median": round(e["median_ms"] / s["median_ms"], 3),
            "faster_by_more_than_both_spreads": bool(e["median_ms"] - s["median_ms"] > e["spread_ms"] + s["spread_ms"])}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30, help="timed launches of each side per layer (>= 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="timed model steps of each side")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU figure"
    res = {"tool": "tools/split_bwd_data_bench.py", "device": torch.cuda.get_device_name(0), "layers": [layer_ab(*s, a) for s in SHAPES], "model": model_ab(a)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")

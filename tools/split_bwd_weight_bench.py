#!/usr/bin/env python3
"""A/B of the opt-in split-precision weight gradient (kan_conv_bwd_weight_split) against the exact fp32-MFMA weight gradient of the same library, in ONE process.

  python tools/split_bwd_weight_bench.py [--launches 30 --warmup 5 --steps 20 --out profiles/split_bwd_weight_bench_ab.json]

Per KAN-VGG11 layer in scope at batch 256 (64 -> 128 @ 16x16, 128 -> 256 @ 8x8, 256 -> 256 @ 8x8): the exact side is what the backward runs today --
`kan_conv_bwd_weight` into the plan's packed slabs plus `kan_unpack_wgrad` -- the split side is the whole entry point: the dz cut, the contraction and the
fixed-order reduce of the depth splits, workspace allocation included.  The two are ALTERNATED launch by launch (never two blocks), each launch between two
HIP events on the launch stream; reported: median and min .. max of both, the useful TFLOP/s (2 * B * H * W * C * 9 planes * O * 9 taps over the median),
the max-normalised distance of the two results, and whether the split side wins by more than the two spreads combined -- the rule that decides whether a
shape stays in `ops.split_precision_backward_weight()`.
Then the KAN-VGG11 batch-256 forward + backward step under four settings -- exact, `split_precision_backward_data`, `split_precision_backward_weight`, both
(`split_precision_backward`) -- alternated step by step, the same way.
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


def _wins(e, s):
    return bool(e["median_ms"] - s["median_ms"] > e["spread_ms"] + s["spread_ms"])


def layer_ab(C_, O_, PW, args):
    import ctypes as C
    import torch
    import convkan_amd as K
    from convkan_amd import _lib as L
    from convkan_amd import ops
    torch.manual_seed(C_ + PW)
    layer = K.KANConv2DLayer(C_, O_, 3, padding=1, base_activation=torch.nn.SiLU).cuda()
    spec, wb, ws = layer.conv_spec(), layer.base_conv[0].weight.detach(), layer.spline_conv[0].weight.detach()
    x = torch.randn(BATCH, C_, PW, PW, device="cuda")
    dz = torch.randn(BATCH, O_, PW, PW, device="cuda")
    _, packed, _, _, plan = ops._conv_forward(spec, x, None, [wb], [ws], True)
    exact = lambda: ops._conv_backward(spec, x, None, packed, dz, False, False, True)[2:]      # kan_conv_bwd_weight + kan_unpack_wgrad, as the backward runs them
    split = lambda: ops.kan_conv_bwd_weight_split(spec, x, dz)
    for _ in range(args.warmup):
        exact(), split()
    torch.cuda.synchronize()
    t_exact, t_split = [], []
    for _ in range(args.launches):                                   # alternated, never two blocks
        ms, (db_e, ds_e) = _timed(exact); t_exact.append(ms)
        ms, (db_s, ds_s) = _timed(split); t_split.append(ms)
    geom, basis, _ = ops._plan_cached(*ops._plan_key(spec, x.shape, O_))
    e, s = _summary(t_exact), _summary(t_split)
    flop = 2.0 * BATCH * PW * PW * C_ * 9 * O_ * 9
    e["useful_tflops"], s["useful_tflops"] = round(flop / e["median_ms"] / 1e9, 1), round(flop / s["median_ms"] / 1e9, 1)
    return {"shape": f"{C_}->{O_} @{PW}x{PW} B={BATCH}", "exact_slabs": int(plan.bwd_weight_splits), "exact_reads_position_major_dz": bool(plan.dz_pm_wanted), "exact": e, "split": s,
            "workspace_mbytes": round(L.load().kan_split_bwd_weight_workspace_bytes(C.byref(geom), C.byref(basis)) / 1e6, 2),
            "speedup_median": round(e["median_ms"] / s["median_ms"], 3), "split_faster_by_more_than_both_spreads": _wins(e, s),
            "dw_base_split_vs_exact_maxnorm": float((db_s - db_e[0]).abs().max() / db_e[0].abs().max()),
            "dw_basis_split_vs_exact_maxnorm": float((ds_s - ds_e[0]).abs().max() / ds_e[0].abs().max())}


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
    settings = {"exact": contextlib.nullcontext, "split_bwd_data_context": ops.split_precision_backward_data,
                "split_bwd_weight_context": ops.split_precision_backward_weight, "split_backward_context": ops.split_precision_backward}

    def step(ctx):
        with ctx():
            model.zero_grad(set_to_none=True)
            F.cross_entropy(model(x), t).backward()
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
    for k in list(settings)[1:]:
        res[k]["speedup_median"] = round(res["exact"]["median_ms"] / res[k]["median_ms"], 3)
        res[k]["faster_by_more_than_both_spreads"] = _wins(res["exact"], res[k])
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30, help="timed launches of each side per layer (>= 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="timed model steps of each setting")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU figure"
    res = {"tool": "tools/split_bwd_weight_bench.py", "device": torch.cuda.get_device_name(0), "layers": [layer_ab(*s, a) for s in SHAPES], "model": model_ab(a)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")

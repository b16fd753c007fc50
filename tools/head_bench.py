#!/usr/bin/env python3
"""Forward + backward of ONE MLP KAN head layer (ChebyKAN), two routes to the same conv-stage kernels:

  layout   ChebyKANLayer as shipped: the [I, O, n] coefficients are packed / their gradient unpacked by kan_pack_weights_iod /
           kan_unpack_wgrad_iod (ConvSpec.w_layout = 1)
  permute  the baseline: ops.kan_conv on coeffs.permute(1, 0, 2).reshape(O, I * n, 1, 1) -- one extra read + write of the weights in the
           forward and of their gradient in the backward, around the conv-layout pack / unpack kernels

Shapes: 9216 -> 4096, degree 3, batch 128 (the AlexNet head) and 512 -> 10, degree 3, batch 256 (the VGG11 head).  Per route and shape:
ms/step of each timed window (device events around at least `steps` steps and 0.4 s of work, one synchronisation per window; the two
routes' windows alternate), their median and their spread (max - min).  Both routes pack on every call, so neither is helped by a cache.  One JSON line per run; --out also writes it to a file.

    python tools/head_bench.py [--steps 10 --warmup 3 --windows 5] [--out profiles/heads_bench_ab.json]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"alexnet_head": (128, 9216, 4096, 3), "vgg11_head": (256, 512, 10, 3)}      # B, I, O, degree


def window(step, steps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def measure(routes, args):
    """{route: figures}: the routes' windows alternate (the machine is shared: a drift hits both), each window at least args.min_window_ms long."""
    for step in routes.values():
        for _ in range(args.warmup):
            step()
    steps = {k: max(args.steps, int(args.min_window_ms / window(step, args.steps)) + 1) for k, step in routes.items()}
    windows = {k: [] for k in routes}
    for _ in range(args.windows):
        for k, step in routes.items():
            windows[k].append(window(step, steps[k]))
    return {k: {"steps_per_window": steps[k], "ms_per_step_windows": [round(t, 4) for t in w], "ms_per_step": round(statistics.median(w), 4),
                "spread_ms": round(max(w) - min(w), 4)} for k, w in windows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--min-window-ms", type=float, default=400.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import convkan_amd as K
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU figure"
    res = {"workload": "one ChebyKAN head layer, fwd + bwd", "windows": args.windows, "warmup": args.warmup, "shapes": {}}
    for tag, (B, I, O, degree) in SHAPES.items():
        torch.manual_seed(0)
        layer = K.ChebyKANLayer(I, O, degree).cuda()
        x = torch.randn(B, I, device="cuda", requires_grad=True)
        g = torch.randn(B, O, device="cuda")
        conv_layout = dataclasses.replace(layer.conv_spec(), w_layout=0)

        def layout():
            layer.cheby_coeffs.grad = x.grad = None
            layer(x).backward(g)

        def permute():
            layer.cheby_coeffs.grad = x.grad = None
            w = layer.cheby_coeffs.permute(1, 0, 2).reshape(O, I * (degree + 1), 1, 1)
            K.ops.kan_conv(conv_layout, x.reshape(B, I, 1, 1), None, [], [w]).view(B, O).backward(g)
        layout()
        ref = (layer.cheby_coeffs.grad.clone(), x.grad.clone())
        permute()
        same = bool(torch.equal(ref[0], layer.cheby_coeffs.grad) and torch.equal(ref[1], x.grad))      # one set of kernels, one summation order
        r = {"B": B, "I": I, "O": O, "degree": degree, "weight_mbytes": round(I * O * (degree + 1) * 4 / 1e6, 1), "routes_bit_identical": same,
             **measure({"layout": layout, "permute": permute}, args)}
        a, b = r["layout"], r["permute"]
        r["saved_ms"] = round(b["ms_per_step"] - a["ms_per_step"], 4)
        r["beats_combined_spread"] = bool(r["saved_ms"] > a["spread_ms"] + b["spread_ms"])
        res["shapes"][tag] = r
        del layer, x, g
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

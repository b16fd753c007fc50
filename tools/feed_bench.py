#!/usr/bin/env python3
"""First measurements of the batch-preparation kernel (csrc/kan_feed.hip, ops.prepare_batch) and of the training step fed by K.DeviceBatches, in ONE process.

  python tools/feed_bench.py [--steps 20 --warmup 5 --runs 2 --out profiles/feed_bench.json]

  (a) kernel    one launch over 10 000 CIFAR-sized channels_last images with the train transform (RandomCrop(32, padding=4) + flip): time per launch,
                achieved bytes/s with the bytes computed from the shapes, N * (H*W*C + 4*C*Ho*Wo + 16 + 16) (image read, fp32 written, table row read,
                label read + target written), and its share of the achievable HBM rate of MI355X_MICROARCH.md (6.3 TB/s; the spec peak is 8).  The
                10 000-image working set (154 MB) fits the 256 MB Infinity Cache, so the same launch over 50 000 images (770 MB) is timed beside it.
  (b) batch     one bs-256 launch (test transform, shuffled index) against the torch-eager device restatement of the same batch: advanced-indexing
                gather, permute, / 255, sub, div.  The ratio is reported, not gated.
  (c) step      KAN-VGG11 bs-256 ``train_step`` (FusedAdamW, torch's criterion) under three feeds ALTERNATED step by step: K.DeviceBatches over a
                50 000-image synthetic uint8 set (train transform); a resident list of pre-materialised fp32 batches; a host DataLoader over a
                TensorDataset of that fp32 list with num_workers=0 (the reference's transfer cost without its transforms).  The condition to meet:
                the DeviceBatches step is within the run-to-run spread of the resident step plus the kernel time of (b) -- otherwise the iteration
                path hides a host read or an allocation.
  --imagenet    the loader's ImageNet branch instead (csrc/kan_feed_resize.hip, ops.prepare_resized_batch, K.ResizedDeviceBatches), written to
                profiles/feed_resize_bench.json with `--out`:
                (d) kernel  one bs-128 launch of the CIFAR train transform (Resize(256) + RandomResizedCrop(224) + flip) over 50 000 resident
                            images, and of the test transform (CenterCrop: stage 2 the identity), against a same-process `fill_` of the same 77 MB
                            output (the write alone), alternated; bytes from the shapes, B * (H*W*C + 4*3*224*224 + 24 + 16), and the share of the
                            achievable HBM rate.
                (e) step    KAN-AlexNet (ChebyKAN degree 4) bs-128 ``train_step`` fed by K.ResizedDeviceBatches against the same step on resident
                            pre-materialised fp32 batches, alternated step by step.
Kernel windows are `--launches` launches between two HIP events on the launch stream; steps are one step between two events.  Every figure is given per
run (`--runs` repeats of the whole schedule) with median and min .. max.  One JSON line on stdout; `--out` also writes it.  There is no CPU figure:
without a GPU the tool fails."""
import argparse
import itertools
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH = 256
HBM_ACHIEVABLE = 6.3e12            # bytes/s, MI355X_MICROARCH.md ("8 TB/s peak (spec); about 6.3 TB/s achievable")
MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616)


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def _summary(ms, digits=4):
    return {"median_ms": round(statistics.median(ms), digits), "min_ms": round(min(ms), digits), "max_ms": round(max(ms), digits),
            "spread_ms": round(max(ms) - min(ms), digits), "samples": len(ms)}


def feed_bytes(N, H, W, C, Ho, Wo):
    return N * (H * W * C + 4 * C * Ho * Wo + 16 + 16)


def _synthetic(n, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randint(0, 256, (n, 32, 32, 3), device="cuda", generator=g, dtype=torch.uint8),
            torch.randint(0, 10, (n,), device="cuda", generator=g, dtype=torch.int64))


def kernel_rate(args):
    """(a): whole-set launches."""
    import torch
    import convkan_amd as K
    from convkan_amd import ops
    res = {}
    sets = {}
    for n in (10000, 50000):
        images, labels = _synthetic(n, n)
        table = K.device_batches("CIFAR10", True, images, labels, n).epoch_table(0)
        out = (torch.empty((n, 3, 32, 32), device="cuda"), torch.empty((n,), device="cuda", dtype=torch.int64))
        sets[n] = (images, labels, table, out)

    def window(n):
        images, labels, table, out = sets[n]
        for _ in range(args.launches):
            ops.prepare_batch(images, table, (32, 32), MEAN, STD, labels=labels, out=out)
    for n in sets:
        for _ in range(args.warmup):
            window(n)
    torch.cuda.synchronize()
    for n in sets:
        res[f"n{n}"] = {"images": n, "bytes_per_launch": feed_bytes(n, 32, 32, 3, 32, 32), "runs": []}
    for _ in range(args.runs):
        times = {n: [] for n in sets}
        for _ in range(args.steps):                                      # alternated window by window
            for n in sets:
                times[n].append(_timed(lambda: window(n))[0] / args.launches)
        for n in sets:
            s = _summary(times[n], 5)
            rate = res[f"n{n}"]["bytes_per_launch"] / (s["median_ms"] * 1e-3)
            s.update(bytes_per_s=round(rate, -6), share_of_achievable_hbm=round(rate / HBM_ACHIEVABLE, 3))
            res[f"n{n}"]["runs"].append(s)
    res["launches_per_window"] = args.launches
    res["hbm_achievable_bytes_per_s"] = HBM_ACHIEVABLE
    return res


def batch_vs_eager(args):
    """(b): one bs-256 launch against torch eager on the device, the same batch."""
    import torch
    import convkan_amd as K
    from convkan_amd import ops
    images, labels = _synthetic(50000, 7)
    db = K.device_batches("CIFAR10", False, images, labels, BATCH, shuffle=True)
    table = db.epoch_table(0)[:BATCH].contiguous()
    mean, std = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1), torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    out = (torch.empty((BATCH, 3, 32, 32), device="cuda"), torch.empty((BATCH,), device="cuda", dtype=torch.int64))

    def kernel():
        return ops.prepare_batch(images, table, (32, 32), MEAN, STD, labels=labels, out=out)

    def eager():
        idx = table[:, 0].long()
        x = images[idx].permute(0, 3, 1, 2).to(torch.float32).div(255)
        return x.sub_(mean).div_(std), labels[idx]
    (xk, tk), (xe, te) = kernel(), eager()
    torch.cuda.synchronize()
    settings = {"kernel": kernel, "eager": eager}

    def window(fn):
        for _ in range(args.launches):
            fn()
    for fn in settings.values():
        for _ in range(args.warmup):
            window(fn)
    torch.cuda.synchronize()
    res = {"batch": BATCH, "targets_equal": bool(torch.equal(tk, te)),
           "max_abs_difference_from_eager": float((xk - xe).abs().max()), "runs": []}         # torch's device div by a scalar multiplies by a reciprocal
    for _ in range(args.runs):
        times = {k: [] for k in settings}
        for _ in range(args.steps):
            for k, fn in settings.items():
                times[k].append(_timed(lambda: window(fn))[0] / args.launches)
        run = {k: _summary(times[k], 5) for k in settings}
        run["eager_over_kernel_median"] = round(run["eager"]["median_ms"] / run["kernel"]["median_ms"], 2)
        res["runs"].append(run)
    return res


def step_under_feeds(args, kernel_ms):
    """(c): the training step under three feeds."""
    import torch
    from torch.utils.data import DataLoader, TensorDataset
    import convkan_amd as K
    from convkan_amd.models import vggkan
    torch.manual_seed(0)
    model = vggkan(3, 10, arch="VGG11", kan_conv="KAN", classifier_type="Linear").cuda().train()
    opt = K.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    images, labels = _synthetic(50000, 11)
    db = K.device_batches("CIFAR10", True, images, labels, BATCH, drop_last=True)
    resident = [(x.clone(), t.clone()) for x, t in itertools.islice(iter(db), 16)]
    host = DataLoader(TensorDataset(torch.cat([x for x, _ in resident]).cpu(), torch.cat([t for _, t in resident]).cpu()), batch_size=BATCH,
                      shuffle=False, num_workers=0)

    def forever(make):
        while True:
            yield from make()
    feeds = {"device_batches": forever(lambda: iter(db)), "resident_fp32": forever(lambda: iter(resident)), "host_loader": forever(lambda: iter(host))}

    def step(feed):
        data, target = next(feed)
        return K.train_step(model, data.to("cuda"), target.to("cuda"), opt)
    for _ in range(args.warmup):
        for feed in feeds.values():
            step(feed)
    torch.cuda.synchronize()
    res = {"workload": "kan_vgg11 train_step (FusedAdamW)", "batch": BATCH, "runs": []}
    for _ in range(args.runs):
        times = {k: [] for k in feeds}
        for _ in range(args.steps):                                      # alternated step by step
            for k, feed in feeds.items():
                times[k].append(_timed(lambda: step(feed))[0])
        run = {k: _summary(times[k]) for k in feeds}
        extra = run["device_batches"]["median_ms"] - run["resident_fp32"]["median_ms"]
        allowed = run["device_batches"]["spread_ms"] + run["resident_fp32"]["spread_ms"] + kernel_ms
        run["device_batches_minus_resident_ms"] = round(extra, 4)
        run["allowed_ms"] = round(allowed, 4)                            # both spreads plus the kernel time of (b)
        run["within_spread_plus_kernel"] = bool(extra <= allowed)
        run["host_loader_minus_resident_ms"] = round(run["host_loader"]["median_ms"] - run["resident_fp32"]["median_ms"], 4)
        res["runs"].append(run)
    return res


IMAGENET_BATCH = 128


def resized_bytes(B, H, W, C, OC, Ho, Wo):
    return B * (H * W * C + 4 * OC * Ho * Wo + 24 + 16)


def resized_kernel(args):
    """(d): one bs-128 launch of the ImageNet-branch transforms against a fill of the same output."""
    import torch
    import convkan_amd as K
    from convkan_amd import ops
    images, labels = _synthetic(50000, 13)
    out = (torch.empty((IMAGENET_BATCH, 3, 224, 224), device="cuda"), torch.empty((IMAGENET_BATCH,), device="cuda", dtype=torch.int64))
    feeds = {"train": K.imagenet_device_batches("CIFAR10", True, images, labels, IMAGENET_BATCH),
             "test": K.imagenet_device_batches("CIFAR10", False, images, labels, IMAGENET_BATCH, shuffle=True)}
    tables = {k: d.epoch_table(0)[:IMAGENET_BATCH].contiguous() for k, d in feeds.items()}

    def launch(k):
        d = feeds[k]
        return lambda: ops.prepare_resized_batch(images, tables[k], d.resize, d.out_hw, d.mean, d.std, labels, True, d.out_channels, d.coeffs, out)
    settings = {"train": launch("train"), "test": launch("test"), "fill": lambda: out[0].fill_(0.5)}

    def window(fn):
        for _ in range(args.launches):
            fn()
    for fn in settings.values():
        for _ in range(args.warmup):
            window(fn)
    torch.cuda.synchronize()
    nbytes = resized_bytes(IMAGENET_BATCH, 32, 32, 3, 3, 224, 224)
    res = {"batch": IMAGENET_BATCH, "bytes_per_launch": nbytes, "output_bytes": out[0].numel() * 4, "launches_per_window": args.launches,
           "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "runs": []}
    for _ in range(args.runs):
        times = {k: [] for k in settings}
        for _ in range(args.steps):                                      # alternated window by window
            for k, fn in settings.items():
                times[k].append(_timed(lambda: window(fn))[0] / args.launches)
        run = {k: _summary(times[k], 5) for k in settings}
        for k in ("train", "test"):
            rate = nbytes / (run[k]["median_ms"] * 1e-3)
            run[k].update(bytes_per_s=round(rate, -6), share_of_achievable_hbm=round(rate / HBM_ACHIEVABLE, 3),
                          fill_over_kernel_median=round(run["fill"]["median_ms"] / run[k]["median_ms"], 3))
        res["runs"].append(run)
    return res


def resized_step(args):
    """(e): the KAN-AlexNet step under the resized feed and under resident fp32 batches."""
    import torch
    import convkan_amd as K
    from convkan_amd.models import alexnet_kan
    torch.manual_seed(0)
    model = alexnet_kan(num_classes=10, kan_conv="ChebyKAN", degree=4).cuda().train()
    opt = K.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    images, labels = _synthetic(50000, 17)
    db = K.imagenet_device_batches("CIFAR10", True, images, labels, IMAGENET_BATCH, drop_last=True)
    resident = [(x.clone(), t.clone()) for x, t in itertools.islice(iter(db), 8)]

    def forever(make):
        while True:
            yield from make()
    feeds = {"resized_device_batches": forever(lambda: iter(db)), "resident_fp32": forever(lambda: iter(resident))}

    def step(feed):
        data, target = next(feed)
        return K.train_step(model, data, target, opt)
    for _ in range(args.warmup):
        for feed in feeds.values():
            step(feed)
    torch.cuda.synchronize()
    res = {"workload": "kan_alexnet ChebyKAN degree 4 train_step (FusedAdamW)", "batch": IMAGENET_BATCH, "runs": []}
    for _ in range(args.runs):
        times = {k: [] for k in feeds}
        for _ in range(args.steps):                                      # alternated step by step
            for k, feed in feeds.items():
                times[k].append(_timed(lambda: step(feed))[0])
        run = {k: _summary(times[k]) for k in feeds}
        run["resized_minus_resident_ms"] = round(run["resized_device_batches"]["median_ms"] - run["resident_fp32"]["median_ms"], 4)
        run["images_per_s_resized"] = round(IMAGENET_BATCH / (run["resized_device_batches"]["median_ms"] * 1e-3), 1)
        res["runs"].append(run)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="timed windows (kernels) or steps (model) of each setting, per run")
    ap.add_argument("--launches", type=int, default=50, help="launches per timed kernel window")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--only", default="abc", help="which of a, b, c to run")
    ap.add_argument("--out", default=None)
    ap.add_argument("--imagenet", action="store_true", help="measure the ImageNet-branch feed (d, e) instead of a, b, c")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU figure"
    res = {"tool": "tools/feed_bench.py", "device": torch.cuda.get_device_name(0)}
    if a.imagenet:
        res["d_resized_kernel"] = resized_kernel(a)
        res["e_step_under_resized_feed"] = resized_step(a)
        a.only = ""
    if "a" in a.only:
        res["a_kernel_rate"] = kernel_rate(a)
    kernel_ms = 0.0
    if "b" in a.only:
        res["b_batch_vs_eager"] = batch_vs_eager(a)
        kernel_ms = max(r["kernel"]["median_ms"] for r in res["b_batch_vs_eager"]["runs"])
    if "c" in a.only:
        res["c_step_under_feeds"] = step_under_feeds(a, kernel_ms)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")

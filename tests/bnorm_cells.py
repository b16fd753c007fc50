"""The cell matrix of the BatchNorm (+ PReLU, + 2x2 max-pool) kernels (csrc/kan_bnorm.hip) and the plain-torch reference its rows are
judged against: F.batch_norm -> PReLU -> F.max_pool2d on the CPU, in fp64 and in fp32, gradients by autograd.

Each row is the smallest shape that crosses one boundary of the kernels (the `why` column).  The attributes the boundaries do not fix
vary across the rows: affine "" none | "gb" gamma and beta | "GB" both, every third gamma negative; slope "" none | "+" 0.25 | "-"
-0.25 (one per group); track=False a module without running statistics; kind "unaligned" the slabs start one float into their storage.

Conditioning is norm_cells' (same KINK, NEAR, MASK_CAP, same function): no upstream gradient within 1e-4 of the PReLU kink or on a
near-tied pool window, exact ties stay in, at most 1 % of a row's outputs masked -- a row over the cap gets another seed, never a
wider cap.  tests/test_bnorm_matrix.py keeps that on the CPU; tests/test_gpu_bnorm_matrix.py runs every row on the GPU."""
import functools
import math

import torch
import torch.nn.functional as F

from norm_cells import KINK, MASK_CAP, NEAR, conditioning  # noqa: F401  (KINK, NEAR: the constants `conditioning` applies)

EPS = 1e-5
MOMENTUM = 0.1


def row(B, C, H, W, S, groups, pool, training, why, affine="gb", slope="+", track=True, kind=None, seed=None):
    return dict(B=B, C=C, H=H, W=W, S=S, groups=groups, pool=pool, training=training, why=why, affine=affine, slope=slope, track=track,
                kind=kind, seed=seed)


# fmt: off
BNORM_CASES = [
    row(3, 7, 1, 1, 1, 1, None, True, "one-element planes"),
    row(5, 6, 2, 2, 1, 2, None, True, "grouped layer", affine="GB", slope="-"),
    row(3, 9, 3, 3, 2, 3, None, True, "two slabs, three groups", affine=""),
    row(3, 7, 5, 13, 5, 1, None, True, "odd plane, five slabs", slope="", kind="unaligned"),
    row(70, 3, 2, 2, 1, 1, None, True, "more than one wave of partials per channel"),
    row(2, 5, 33, 35, 3, 1, None, True, "plane > 1024 elements", affine="GB", slope="-"),
    row(3, 7, 2, 2, 4, 1, (2, 2), True, "pooled, four slabs"),
    row(5, 6, 4, 4, 1, 2, (2, 2), True, "pooled, grouped", slope="-"),
    row(3, 9, 6, 6, 1, 3, (2, 2), True, "pooled, three groups", affine="", track=False),
    row(2, 5, 34, 36, 2, 1, (2, 2), True, "pooled, plane > 1024 elements", affine="GB"),
    row(3, 7, 4, 4, 1, 1, None, False, "eval statistics"),
    row(3, 7, 6, 6, 2, 1, (2, 2), False, "eval statistics, pooled", affine="GB", slope="-"),
    row(2, 130, 8, 8, 1, 1, (2, 2), True, "more than 128 channels", slope=""),
]
# fmt: on


def case_id(case):
    i = BNORM_CASES.index(case)
    p = "-pool2" if case["pool"] else ""
    return f"{i}-{case['B']}x{case['C']}x{case['H']}x{case['W']}{p}-S{case['S']}-g{case['groups']}-{'train' if case['training'] else 'eval'}-" \
           f"{case['affine'] or 'noaff'}{case['slope'] or '0'}" + ("" if case["track"] else "-notrack") + (f"-{case['kind']}" if case["kind"] else "")


def make_inputs(case):
    """fp64 CPU tensors of a row, drawn from its seed (1000 + row index unless the row names another) in a fixed order: the slabs
    zs [S, B, C, H, W] with a per-channel scale and offset, gamma, beta, running_mean, running_var; then what the row's attributes keep of
    them, and its slopes."""
    i = BNORM_CASES.index(case)
    g = torch.Generator().manual_seed(1000 + i if case["seed"] is None else case["seed"])
    S, B, C, H, W = (case[k] for k in "SBCHW")
    rand = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    zs = randn(S, B, C, H, W) / math.sqrt(S)
    zs = zs * (0.5 + 1.5 * rand(C)).view(1, 1, C, 1, 1) + (3 * randn(C) / S).view(1, 1, C, 1, 1)
    gamma, beta = 1 + 0.5 * randn(C), 0.5 * randn(C)
    rmean, rvar = 0.3 * randn(C), 0.5 + rand(C)
    if case["affine"] == "GB":
        gamma[::3] *= -1
    if not case["affine"]:
        gamma = beta = None
    if not case["track"]:
        rmean = rvar = None
    slope = torch.full((case["groups"],), 0.25 if case["slope"] == "+" else -0.25, dtype=torch.float64) if case["slope"] else None
    return dict(zs=zs, gamma=gamma, beta=beta, slope=slope, rmean=rmean, rvar=rvar)


def _forward(case, inputs, dtype, graph=True):
    cast = lambda t: t.detach().to(dtype).clone() if t is not None else None          # (fresh leaves: the inputs are shared between dtypes)
    zs = cast(inputs["zs"]).requires_grad_(graph)
    gamma, beta, slope = (cast(inputs[k]).requires_grad_(graph) if inputs[k] is not None else None for k in ("gamma", "beta", "slope"))
    rmean, rvar = (cast(inputs[k]) for k in ("rmean", "rvar"))
    z = zs.sum(0)
    batch = case["training"] or rmean is None                    # torch.nn.BatchNorm's rule
    n = F.batch_norm(z, rmean, rvar, gamma, beta, batch, MOMENTUM, EPS)
    act = n
    if slope is not None:
        act = F.prelu(n, slope.repeat_interleave(case["C"] // case["groups"]))
    if graph:
        act.retain_grad()
    y = F.max_pool2d(act, 2, 2) if case["pool"] else act
    zd = z.detach()
    mean = zd.mean((0, 2, 3)) if batch else rmean
    rstd = 1.0 / torch.sqrt((zd.var((0, 2, 3), unbiased=False) if batch else rvar) + EPS)
    return dict(zs=zs, gamma=gamma, beta=beta, slope=slope, z=z, n=n, act=act, y=y, mean=mean, rstd=rstd, rmean=rmean, rvar=rvar)


def _backward(case, f, go):
    f["y"].backward(go.to(f["y"].dtype))
    n = f["n"].detach()
    grad = lambda p: p.grad if p is not None else None
    out = dict(y=f["y"].detach(), z=f["z"].detach(), dz=f["zs"].grad[0], mean=f["mean"], rstd=f["rstd"], running_mean=f["rmean"],
               running_var=f["rvar"], dgamma=grad(f["gamma"]), dbeta=grad(f["beta"]), dslope=grad(f["slope"]))
    if f["slope"] is not None:
        # a slope gradient is judged against sum |n g| over its elements on the negative side: its net value may cancel
        w = (n * f["act"].grad).abs() * (n <= 0)
        out["dslope_scale"] = w.sum((0, 2, 3)).reshape(case["groups"], -1).sum(1)
    return out


@functools.lru_cache(maxsize=2)
def reference_pair(idx):
    """Row BNORM_CASES[idx]: (inputs, go, mask, pidx, fp64 results, fp32 results) -- computed once, shared, never modified."""
    case = BNORM_CASES[idx]
    inputs = make_inputs(case)
    f64 = _forward(case, inputs, torch.float64)
    mask, pidx = conditioning(case, f64["n"].detach(), f64["act"].detach())
    go = torch.randn(f64["y"].shape, generator=torch.Generator().manual_seed(99)) * (~mask).float()
    return inputs, go, mask, pidx, _backward(case, f64, go), _backward(case, _forward(case, inputs, torch.float32), go)


def mask_share(case):
    """(share, count, outputs) of the row's outputs its conditioning masks, from the fp64 forward alone."""
    f = _forward(case, make_inputs(case), torch.float64, graph=False)
    mask = conditioning(case, f["n"], f["act"])[0]
    return float(mask.float().mean()), int(mask.sum()), mask.numel()

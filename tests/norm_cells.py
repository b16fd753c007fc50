"""The cell matrix of the InstanceNorm (+ PReLU, + max-pool) kernels: which kernel variant `kan_norm_route` picks for a tensor, one
row per variant and per side of every switch point, and the plain-torch reference the rows are judged against.

A cell is what `kan_norm_route` (the function the six kan_instnorm_prelu* entry points dispatch from) decides for a launch:
direction, kernel (generic / register), G, EPL, PPI, NT, the pool mode, and for the generic kernels whether the plane is staged in
LDS and whether the backward holds it in registers between its two passes.  `norm_key` spells a route out, e.g.
`fwd-REGS-G64-E4-P2-NT256-pool2`, `bwd-GEN-G64-reread-poolk-nolds`, `bwd-REGS-G4-E1-P4-NT1024-strided`.  `-strided` (the grid is
capped and a workgroup runs its grid-stride loop more than once) is a property of the launcher, not of the variant: every capped
launcher has one row just past its cap (`launcher_of`), instead of one per variant -- a generic-backward variant whose plane does
not fit LDS would need a 100 MB tensor to stride.  tests/test_norm_matrix.py keeps the table complete on the CPU;
tests/test_gpu_norm_matrix.py runs every row against `reference(case, torch.float64)`.

Conditioning (all from the fp64 reference, never from the kernel): an output whose normalised value lies within 1e-4 of the
PReLU kink gets no upstream gradient (helpers.check_vs_oracle's rule); so does a pool window in which some value lies within
1e-4 of the maximum without being equal to it (fp32 may order the two the other way and route the gradient to another pixel),
or whose maximum lies within 1e-4 of the kink.  Exact ties stay in: equal z give equal activations in any precision, and the
first maximum in scan order must win, as in torch.  At most MASK_CAP of a row's outputs may be masked; a row that breaks the
cap gets another seed, not a wider cap."""
import ctypes
import functools

import torch
import torch.nn.functional as F

EPS = 1e-5
KINK = 1e-4            # |normalised value| <= KINK: on the PReLU kink (helpers.check_vs_oracle)
NEAR = 1e-4            # 0 < max - value < NEAR: a near-tie of a pool window
MASK_CAP = 0.01        # at most this share of a row's outputs may be masked


def norm_key(r, bwd):
    """Readable id of a KanNormRoute."""
    s = ("bwd" if bwd else "fwd") + ("-REGS" if r.kernel else "-GEN") + f"-G{r.G}"
    if r.kernel:
        s += f"-E{r.EPL}-P{r.PPI}-NT{r.NT}"
    elif bwd:
        s += "-twopass" if r.held else "-reread"
    if r.pool == 1:
        s += "-pool2"
    elif r.pool == 2:
        s += "-poolk" + ("-lds" if r.lds else "-nolds")
    return s + ("-strided" if r.strided else "")


def cell_of(key):
    """The variant alone: the key without the launcher's `-strided`."""
    return key[:-len("-strided")] if key.endswith("-strided") else key


def launcher_of(key):
    """The capped launcher a key belongs to (None: the generic forward, whose grid has no cap)."""
    p = key.split("-")
    if p[1] == "REGS":
        return "fwd_regs" if p[0] == "fwd" else "bwd_regs_" + p[5]
    return "bwd_generic" if p[0] == "bwd" else None


def pool_args(pool, H, W):
    """(pool2x2, pool_k, pool_s) as ops._norm_fwd resolves `pool`: (2, 2) on an even plane is the 2x2 mode."""
    if not pool:
        return 0, 0, 0
    if tuple(pool) == (2, 2) and H % 2 == 0 and W % 2 == 0:
        return 1, 0, 0
    return 0, pool[0], pool[1]


def route(bwd, B, C, H, W, S=1, pool=None, aligned=True):
    """`kan_norm_route` of the library for a dense [S][B][C][H][W] tensor, as ops._norm_fwd / _norm_bwd would launch it."""
    from convkan_amd import _lib as L
    r = L.KanNormRoute()
    p2, pk, ps = pool_args(pool, H, W)
    L.check(L.load().kan_norm_route(int(bwd), B, C, H, W, C * H * W, S, B * C * H * W, p2, pk, ps, int(aligned), ctypes.byref(r)), "kan_norm_route")
    return r


def case_route(case, bwd):
    return route(bwd, case["B"], case["C"], case["H"], case["W"], case["S"], case["pool"], case["kind"] != "unaligned")


def row(fwd, bwd, B, C, H, W, S=1, groups=1, affine="gb", slope="+", pool=None, kind=None, seed=0):
    """affine: "" none | "gb" gamma and beta | "g" / "b" one of them | "GB" both, every third gamma negative;
    slope: "" none (the instance_norm op) | "+" around 0.25 | "-" around -0.25;  groups > 1: one slope per C / groups channels;
    kind: "unaligned" z starts one float into its storage | "const" every plane constant (every window an all-tie) |
    "ties" image 2 repeats each even row in the row below it, image 3 each even column in the column right of it: windows
    with exactly two maxima, the first of them anywhere in the window."""
    return dict(fwd=fwd, bwd=bwd, B=B, C=C, H=H, W=W, S=S, groups=groups, affine=affine, slope=slope, pool=pool, kind=kind, seed=seed)


# fmt: off
NORM_CASES = [
    # no pool: one row each side of every switch point of the register variants (HW = 4 ... 1024), then the generic kernel
    row("fwd-REGS-G4-E1-P4-NT256", "bwd-REGS-G4-E1-P4-NT1024", 3, 7, 1, 1),
    row("fwd-REGS-G4-E1-P4-NT256", "bwd-REGS-G4-E1-P4-NT1024", 5, 6, 2, 2, groups=2, affine="GB"),
    row("fwd-REGS-G8-E1-P4-NT256", "bwd-REGS-G8-E1-P4-NT1024", 3, 7, 1, 5, affine=""),
    row("fwd-REGS-G8-E1-P4-NT256", "bwd-REGS-G8-E1-P4-NT1024", 5, 13, 2, 4, slope=""),
    row("fwd-REGS-G16-E1-P4-NT256", "bwd-REGS-G16-E1-P4-NT1024", 3, 9, 3, 3, S=2, groups=3, affine="GB", slope="-"),
    row("fwd-REGS-G16-E1-P4-NT256", "bwd-REGS-G16-E1-P4-NT1024", 5, 13, 2, 8, affine="", slope=""),
    row("fwd-REGS-G32-E1-P4-NT256", "bwd-REGS-G32-E1-P4-NT1024", 3, 7, 1, 17, affine="g"),
    row("fwd-REGS-G32-E1-P4-NT256", "bwd-REGS-G32-E1-P4-NT1024", 5, 6, 4, 8, groups=2, affine="b", slope="-"),
    row("fwd-REGS-G16-E4-P2-NT256", "bwd-REGS-G16-E4-P2-NT1024", 3, 7, 3, 11, affine="", slope="-"),
    row("fwd-REGS-G16-E4-P2-NT256", "bwd-REGS-G16-E4-P2-NT1024", 3, 9, 4, 16, groups=3),
    row("fwd-REGS-G64-E2-P2-NT256", "bwd-REGS-G64-E2-P2-NT1024", 3, 7, 5, 13, S=5),
    row("fwd-REGS-G64-E2-P2-NT256", "bwd-REGS-G64-E2-P2-NT1024", 5, 6, 8, 16, groups=2, affine="GB"),
    row("fwd-REGS-G64-E4-P2-NT256", "bwd-REGS-G64-E4-P2-NT1024", 3, 7, 3, 43, affine=""),
    row("fwd-REGS-G64-E4-P2-NT256", "bwd-REGS-G64-E4-P2-NT1024", 5, 13, 8, 32, slope=""),
    row("fwd-REGS-G64-E8-P1-NT256", "bwd-REGS-G64-E8-P1-NT1024", 3, 9, 1, 257, groups=3, affine="GB", slope="-"),
    row("fwd-REGS-G64-E8-P1-NT256", "bwd-REGS-G64-E8-P1-NT1024", 5, 13, 8, 64, affine="", slope=""),
    row("fwd-REGS-G64-E16-P1-NT256", "bwd-REGS-G64-E16-P1-NT256", 3, 7, 19, 27, S=9, affine="g"),
    row("fwd-REGS-G64-E16-P1-NT256", "bwd-REGS-G64-E16-P1-NT256", 5, 6, 16, 64, S=32, groups=2, affine="b", slope="-"),
    row("fwd-GEN-G64", "bwd-GEN-G64-reread", 3, 7, 25, 41, S=5, affine="", slope="-"),
    row("fwd-GEN-G64", "bwd-GEN-G64-reread", 3, 9, 56, 56, S=2, groups=3),
    # MaxPool2d(2, 2) on even planes: the register variants each side of nwin = 4 ... 128, then the generic 2x2 mode above 1024 pixels
    row("fwd-REGS-G4-E4-P2-NT256-pool2", "bwd-REGS-G4-E1-P4-NT1024-pool2", 3, 7, 2, 2, S=32, pool=(2, 2)),
    row("fwd-REGS-G4-E4-P2-NT256-pool2", "bwd-REGS-G16-E1-P4-NT1024-pool2", 5, 6, 4, 4, groups=2, affine="GB", pool=(2, 2)),
    row("fwd-REGS-G4-E4-P2-NT256-pool2", "bwd-REGS-G16-E1-P4-NT1024-pool2", 3, 7, 2, 6, affine="b", slope="", pool=(2, 2)),
    row("fwd-REGS-G8-E4-P2-NT256-pool2", "bwd-REGS-G32-E1-P4-NT1024-pool2", 3, 7, 2, 10, affine="", pool=(2, 2)),
    row("fwd-REGS-G8-E4-P2-NT256-pool2", "bwd-REGS-G32-E1-P4-NT1024-pool2", 5, 13, 4, 8, slope="", pool=(2, 2)),
    row("fwd-REGS-G16-E4-P2-NT256-pool2", "bwd-REGS-G16-E4-P2-NT1024-pool2", 3, 9, 6, 6, groups=3, affine="GB", slope="-", pool=(2, 2)),
    row("fwd-REGS-G16-E4-P2-NT256-pool2", "bwd-REGS-G16-E4-P2-NT1024-pool2", 5, 13, 8, 8, S=3, affine="", slope="", pool=(2, 2)),
    row("fwd-REGS-G32-E4-P2-NT256-pool2", "bwd-REGS-G64-E2-P2-NT1024-pool2", 3, 7, 2, 34, affine="g", pool=(2, 2)),
    row("fwd-REGS-G32-E4-P2-NT256-pool2", "bwd-REGS-G64-E2-P2-NT1024-pool2", 5, 6, 8, 16, groups=2, affine="b", slope="-", pool=(2, 2)),
    row("fwd-REGS-G64-E4-P2-NT256-pool2", "bwd-REGS-G64-E4-P2-NT1024-pool2", 3, 7, 6, 22, affine="", slope="-", pool=(2, 2)),
    row("fwd-REGS-G64-E4-P2-NT256-pool2", "bwd-REGS-G64-E4-P2-NT1024-pool2", 3, 9, 16, 16, S=2, groups=3, pool=(2, 2)),
    row("fwd-REGS-G64-E8-P1-NT256-pool2", "bwd-REGS-G64-E8-P1-NT1024-pool2", 3, 7, 10, 26, pool=(2, 2)),
    row("fwd-REGS-G64-E8-P1-NT256-pool2", "bwd-REGS-G64-E8-P1-NT1024-pool2", 5, 6, 16, 32, S=5, groups=2, affine="GB", pool=(2, 2)),
    row("fwd-REGS-G64-E16-P1-NT256-pool2", "bwd-REGS-G64-E16-P1-NT256-pool2", 3, 7, 6, 86, affine="", pool=(2, 2)),
    row("fwd-REGS-G64-E16-P1-NT256-pool2", "bwd-REGS-G64-E16-P1-NT256-pool2", 5, 13, 32, 32, S=9, slope="", pool=(2, 2)),
    row("fwd-GEN-G64-pool2", "bwd-GEN-G64-reread-pool2", 3, 9, 34, 34, S=9, groups=3, affine="GB", slope="-", pool=(2, 2)),
    row("fwd-GEN-G64-pool2", "bwd-GEN-G64-reread-pool2", 5, 13, 2, 514, S=2, affine="", slope="", pool=(2, 2)),
    # general MaxPool2d(k, s): every G, LDS and no LDS, two-pass and re-read, Hp / Wp = 1, kernels up to 15
    row("fwd-GEN-G16-poolk-lds", "bwd-GEN-G16-twopass-poolk-lds", 3, 7, 13, 13, S=2, affine="g", pool=(3, 2)),
    row("fwd-GEN-G64-poolk-lds", "bwd-GEN-G64-twopass-poolk-lds", 5, 6, 27, 27, groups=2, affine="b", slope="-", pool=(3, 2)),
    row("fwd-GEN-G64-poolk-lds", "bwd-GEN-G64-reread-poolk-lds", 3, 7, 55, 55, S=32, affine="", slope="-", pool=(3, 2)),
    row("fwd-GEN-G64-poolk-nolds", "bwd-GEN-G64-reread-poolk-nolds", 3, 9, 57, 56, S=5, groups=3, pool=(3, 2)),
    row("fwd-GEN-G64-poolk-nolds", "bwd-GEN-G64-reread-poolk-nolds", 3, 7, 57, 57, pool=(2, 2)),
    row("fwd-GEN-G16-poolk-lds", "bwd-GEN-G16-twopass-poolk-lds", 5, 6, 13, 11, groups=2, affine="GB", pool=(2, 2)),
    row("fwd-GEN-G16-poolk-lds", "bwd-GEN-G16-twopass-poolk-lds", 3, 7, 12, 14, affine="", pool=(3, 1)),
    row("fwd-GEN-G32-poolk-lds", "bwd-GEN-G32-twopass-poolk-lds", 5, 13, 17, 17, slope="", pool=(5, 3)),
    row("fwd-GEN-G16-poolk-lds", "bwd-GEN-G16-twopass-poolk-lds", 3, 9, 9, 20, groups=3, affine="GB", slope="-", pool=(7, 1)),
    row("fwd-GEN-G64-poolk-lds", "bwd-GEN-G64-twopass-poolk-lds", 5, 13, 31, 17, affine="", slope="", pool=(15, 4)),
    row("fwd-GEN-G64-poolk-lds", "bwd-GEN-G64-twopass-poolk-lds", 3, 7, 15, 31, affine="g", pool=(15, 15)),
    row("fwd-GEN-G4-poolk-lds", "bwd-GEN-G4-twopass-poolk-lds", 5, 6, 3, 3, groups=2, affine="b", slope="-", pool=(3, 2)),
    row("fwd-GEN-G4-poolk-lds", "bwd-GEN-G4-twopass-poolk-lds", 3, 7, 9, 4, affine="", slope="-", pool=(3, 2)),
    row("fwd-GEN-G4-poolk-lds", "bwd-GEN-G4-twopass-poolk-lds", 3, 9, 2, 9, groups=3, pool=(2, 1)),
    row("fwd-GEN-G4-poolk-lds", "bwd-GEN-G4-twopass-poolk-lds", 3, 7, 5, 5, pool=(3, 2)),
    row("fwd-GEN-G8-poolk-lds", "bwd-GEN-G8-twopass-poolk-lds", 5, 6, 7, 9, groups=2, affine="GB", pool=(3, 2)),
    row("fwd-GEN-G32-poolk-lds", "bwd-GEN-G32-twopass-poolk-lds", 3, 7, 19, 19, S=9, affine="", pool=(3, 2)),
    # one row per capped launcher, the smallest tensor that makes a workgroup run its grid-stride loop twice: fwd_regs (8192 blocks x 4 groups
    # x 64 planes) and with it bwd_regs at NT = 1024; bwd_regs at NT = 256 (2048 blocks x 4 planes); the generic backward (512 blocks x 4 planes)
    row("fwd-REGS-G4-E1-P4-NT256-strided", "bwd-REGS-G4-E1-P4-NT1024-strided", 3, 699051, 2, 2),
    row("fwd-REGS-G64-E16-P1-NT256", "bwd-REGS-G64-E16-P1-NT256-strided", 3, 2731, 19, 27, affine="GB", slope="-"),
    row("fwd-GEN-G64", "bwd-GEN-G64-reread-strided", 3, 683, 25, 41, affine=""),
    # the forward's alignment fallback: z starts one float into its storage, so the float2 kernels are off and the generic 2x2 mode runs, every G
    row("fwd-GEN-G4-pool2", "bwd-REGS-G4-E1-P4-NT1024-pool2", 5, 6, 2, 2, groups=2, affine="GB", pool=(2, 2), kind="unaligned"),
    row("fwd-GEN-G8-pool2", "bwd-REGS-G8-E1-P4-NT1024-pool2", 3, 9, 2, 4, groups=3, affine="GB", slope="-", pool=(2, 2), kind="unaligned"),
    row("fwd-GEN-G16-pool2", "bwd-REGS-G16-E1-P4-NT1024-pool2", 5, 6, 4, 4, groups=2, affine="b", slope="-", pool=(2, 2), kind="unaligned"),
    row("fwd-GEN-G32-pool2", "bwd-REGS-G32-E1-P4-NT1024-pool2", 5, 13, 2, 10, pool=(2, 2), kind="unaligned"),
    row("fwd-GEN-G64-pool2", "bwd-REGS-G16-E4-P2-NT1024-pool2", 3, 7, 8, 8, slope="", pool=(2, 2), kind="unaligned"),
    # exact ties, on the generic and on the register kernels: constant planes (every window an all-tie; rows of their own, because their
    # rstd = 1 / sqrt(eps) and dz are ~300 x those of an ordinary plane and would set the scale of a shared tensor), and planes with
    # repeated rows / columns (partial ties: two maxima per window, the first one at any position, the later one must lose)
    row("fwd-GEN-G16-poolk-lds", "bwd-GEN-G16-twopass-poolk-lds", 3, 7, 13, 13, pool=(3, 2), kind="const"),
    row("fwd-REGS-G16-E4-P2-NT256-pool2", "bwd-REGS-G16-E4-P2-NT1024-pool2", 3, 7, 8, 8, slope="-", pool=(2, 2), kind="const"),
    row("fwd-GEN-G16-poolk-lds", "bwd-GEN-G16-twopass-poolk-lds", 4, 5, 13, 13, pool=(3, 2), kind="ties"),
    row("fwd-REGS-G16-E4-P2-NT256-pool2", "bwd-REGS-G16-E4-P2-NT1024-pool2", 4, 5, 8, 8, slope="-", pool=(2, 2), kind="ties"),
]
# fmt: on


def case_id(case):
    p = f"-pool{case['pool'][0]}s{case['pool'][1]}" if case["pool"] else ""
    return f"{case['B']}x{case['C']}x{case['H']}x{case['W']}{p}-S{case['S']}-g{case['groups']}-{case['affine'] or 'noaff'}{case['slope'] or '0'}" + \
        (f"-{case['kind']}" if case["kind"] else "")


def case_ids(cases):
    return [case_id(c) for c in cases]


# ------------------------------------------------------------------------------------------ inputs and the reference
def make_inputs(case):
    """fp32 CPU tensors of a row: slabs zs [S, B, C, H, W] (randn plus a per-plane offset of at most 1, so that the mean does not
    dwarf the spread), gamma / beta / slope or None."""
    g = torch.Generator().manual_seed(1000 + case["seed"])
    S, B, C, H, W = (case[k] for k in "SBCHW")
    zs = torch.randn(S, B, C, H, W, generator=g)
    zs[0] += 2 * torch.rand(B, C, 1, 1, generator=g) - 1
    if case["kind"] == "const":
        zs[:] = zs[:, :, :, :1, :1]                                         # (needs beta: the normalised value is 0 on the kink otherwise)
    if case["kind"] == "ties":
        assert B >= 4
        zs[:, 2, :, 1::2] = zs[:, 2, :, 0:2 * (H // 2):2]                   # row 2i + 1 = row 2i: both lie in the window that starts at row 2i
        zs[:, 3, :, :, 1::2] = zs[:, 3, :, :, 0:2 * (W // 2):2]             # column 2j + 1 = column 2j
    a = case["affine"]
    gamma = 1 + 0.2 * torch.randn(C, generator=g) if a in ("gb", "g", "GB") else None
    beta = 0.5 + 0.2 * torch.rand(C, generator=g) if a in ("gb", "b", "GB") else None
    if beta is not None:
        beta[1::2] *= -1
    if a == "GB":
        gamma[::3] *= -1
    slope = None
    if case["slope"]:
        slope = (0.25 + 0.1 * (torch.rand(case["groups"], generator=g) - 0.5)) * (1 if case["slope"] == "+" else -1)
    return zs, gamma, beta, slope


def _windows(t, k, s):
    """[planes, k*k, Q] values of every pool window, in scan order."""
    B, C, H, W = t.shape
    return F.unfold(t.reshape(B * C, 1, H, W), k, stride=s)


def _instance_norm(z, gamma, beta):
    if z.shape[2] * z.shape[3] > 1:
        return F.instance_norm(z, weight=gamma, bias=beta, eps=EPS)
    # torch refuses a single-pixel plane ("expected more than 1 spatial element"): the same formula, spelled out
    n = (z - z.mean((2, 3), keepdim=True)) * torch.rsqrt(z.var((2, 3), unbiased=False, keepdim=True) + EPS)
    n = n * gamma.view(1, -1, 1, 1) if gamma is not None else n
    return n + beta.view(1, -1, 1, 1) if beta is not None else n


def _forward(case, inputs, dtype, graph=True):
    """The row's forward in `dtype` (graph kept for `_backward` unless graph=False): a dict of the leaves and of z, n (pre-PReLU),
    act (pre-pool), y."""
    zs, gamma, beta, slope = inputs
    zs = zs.to(dtype).requires_grad_(graph)
    gamma, beta, slope = (p.to(dtype).requires_grad_(graph) if p is not None else None for p in (gamma, beta, slope))
    z = zs.sum(0)
    n = _instance_norm(z, gamma, beta)
    act = n
    if slope is not None:
        act = F.prelu(n, slope.repeat_interleave(case["C"] // case["groups"]) if case["groups"] > 1 else slope.expand(case["C"]))
    if graph:
        act.retain_grad()
    y = F.max_pool2d(act, case["pool"][0], case["pool"][1]) if case["pool"] else act
    return dict(zs=zs, gamma=gamma, beta=beta, slope=slope, z=z, n=n, act=act, y=y)


def conditioning(case, n64, act64):
    """(mask [shape of y]: outputs that get no upstream gradient; pidx [shape of y] uint8 or None: the first maximum of every window in
    scan order, dh * k + dw), from the fp64 forward."""
    if not case["pool"]:
        return n64.abs() <= KINK, None
    k, s = case["pool"]
    u, un = _windows(act64, k, s), _windows(n64, k, s)
    d = u.max(1, keepdim=True).values - u
    near = ((d > 0) & (d < NEAR)).any(1)
    first = torch.where(d == 0, torch.arange(k * k).view(1, -1, 1), k * k).min(1).values      # first maximum in scan order
    kink = un.gather(1, first.unsqueeze(1)).squeeze(1).abs() <= KINK
    B, C, H, W = act64.shape
    shape = (B, C, (H - k) // s + 1, (W - k) // s + 1)
    return (near | kink).reshape(shape), first.to(torch.uint8).reshape(shape)


def _backward(case, f, go):
    f["y"].backward(go.to(f["y"].dtype))
    zd, n = f["z"].detach(), f["n"].detach()
    grad = lambda p: p.grad if p is not None else None
    out = dict(y=f["y"].detach(), z=zd, dz=f["zs"].grad[0], mean=zd.mean((2, 3)).reshape(-1),
               rstd=(1.0 / torch.sqrt(zd.var((2, 3), unbiased=False) + EPS)).reshape(-1),
               dgamma=grad(f["gamma"]), dbeta=grad(f["beta"]), dslope=grad(f["slope"]))
    if f["slope"] is not None:
        # what a slope gradient is judged against: sum |n g| over the elements on the negative side, per slope -- its net value may
        # cancel to nothing (see the comment above route_cells.ROUTE_CASES)
        w = (n * f["act"].grad).abs() * (n <= 0)
        out["dslope_scale"] = w.sum((0, 2, 3)).reshape(case["groups"], -1).sum(1)
    return out


@functools.lru_cache(maxsize=2)
def reference_pair(idx):
    """Row NORM_CASES[idx]: (inputs, go, mask, pidx, fp64 results, fp32 results) -- computed once, shared, never modified."""
    case = NORM_CASES[idx]
    inputs = make_inputs(case)
    f64 = _forward(case, inputs, torch.float64)
    mask, pidx = conditioning(case, f64["n"].detach(), f64["act"].detach())
    go = torch.randn(f64["y"].shape, generator=torch.Generator().manual_seed(99)) * (~mask).float()
    return inputs, go, mask, pidx, _backward(case, f64, go), _backward(case, _forward(case, inputs, torch.float32), go)


def reference(case, dtype):
    """y, dz, dgamma, dbeta, dslope (None where the row has no such parameter), mean, rstd = 1 / sqrt(var + eps) and the summed z of
    the row, in `dtype`, plain torch on the CPU: z = slabs.sum(0); F.instance_norm; PReLU with the per-channel expansion of the
    per-group slopes; F.max_pool2d when pooled; backward by autograd from the seeded, masked `go`."""
    ref = reference_pair(NORM_CASES.index(case))
    return ref[4] if dtype == torch.float64 else ref[5]


def mask_share(case):
    """Share of the row's outputs its conditioning masks, from the fp64 forward alone."""
    f = _forward(case, make_inputs(case), torch.float64, graph=False)
    return float(conditioning(case, f["n"], f["act"])[0].float().mean())


def tie_stats(case):
    """Of a pooled row, from the fp64 forward, over the unmasked windows: (windows with more than one but not k*k maxima, those of them
    whose first maximum is not the window's first element)."""
    f = _forward(case, make_inputs(case), torch.float64, graph=False)
    mask, first = conditioning(case, f["n"], f["act"])
    u = _windows(f["act"], *case["pool"])
    count = (u == u.max(1, keepdim=True).values).sum(1).reshape(mask.shape)
    partial = (count > 1) & (count < case["pool"][0] ** 2) & ~mask
    return int(partial.sum()), int((partial & (first > 0)).sum())

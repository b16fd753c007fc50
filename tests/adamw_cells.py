"""The cell matrix of the AdamW kernels (csrc/kanconv.hip, section "optimizer step": k_adamw behind kan_adamw_step, k_adamw_seg behind
kan_adamw_step_segments), the plain-torch reference its rows are judged against, and the judge.

Reference: one AdamW step as a function of (p, g, m, v, lr, betas, eps, weight_decay, step, grad_scale) on torch CPU tensors, in the
formula order of torch's single-tensor path (torch/optim/adam.py: mul_, lerp_ -- ATen's two-branch lerp --, mul_ + addcmul_, sqrt / div / add_,
addcdiv_), run in fp64 as the reference and in fp32 as the noise measure.  tests/test_adamw_matrix.py anchors the fp64 run to
torch.optim.AdamW, the optimizer the reference project builds (generic_train.py:24).

Rows: FLAT rows call kan_adamw_step at the smallest sizes on each side of every launch boundary (1024 elements per workgroup, at most 4096
workgroups, a tail of < 4 elements); SEGMENT rows call kan_adamw_step_segments with tables the test builds itself (layout()).  Each row
declares its cell as an explicit key; flat_key() / seg_key() restate the launch arithmetic and must reproduce it.  The attributes the
boundaries do not fix -- hyper-parameter set, step, grad_scale, starting state -- vary across the rows of both classes.

Inputs (make_inputs): drawn in fp64 from the row's seed, rounded to fp32 once; both references start from the rounded values.  Gradients
have magnitude (1..10) x 10 ** randint(-6, 3) per element, 5 % exact zeros; a third of the parameters start at 0, a third at ~1e-3, a third at
~1.  Random starting moments draw their magnitude from the same distribution, independently of the gradient (a running average of
gradients whose size varies from step to step), times grad_scale; v0 = m-scale^2 x (0.5 .. 1.5) >= 0.  The smallest squared and scaled
gradient is (1e-6 / 128)^2 x (1 - 0.999) = 6e-20: nothing is subnormal.

Judge (judge()): parameters in two classes -- those that started at 0, where the update is not hidden under the rounding of p, and the
rest -- each normalised by the fp64 reference's largest element of the class; m elementwise against max(|m0|, |g grad_scale|); v elementwise
relative to the fp64 value (a sum of non-negative terms), exactly 0 where the reference is exactly 0.  Tolerance per tensor: max(FLOOR,
4 x the error of the fp32 CPU execution against fp64, measured live); FLOOR = 2e-6 is the data floor of tests/test_gpu_norm_matrix.py.  No row
masks anything today; a row that has to names the reason in `mask`, and at most MASK_CAP of its elements may go.

Not covered: a segment offset above 2^31 elements (seg_off is 64-bit, `off` in k_adamw_seg is long long) would need three blocks of more
than 8 GB each, over 24 GB of device memory, for one test; it is left out."""
import functools
import math

import numpy as np
import torch

FLOOR = 2e-6
MASK_CAP = 0.01
WG_ELEMS, MAX_WGS = 1024, 4096          # kanconv.hip:3296-3297: 256 threads x float4 per workgroup, at most 256 * 16 workgroups

# (lr, betas, eps, weight_decay)
HYPER = {
    "default": (1e-3, (0.9, 0.999), 1e-8, 1e-4),        # what the reference project trains with (train.py defaults into generic_train.py:24)
    "wd2": (1e-2, (0.9, 0.999), 1e-8, 1e-2),
    "all": (3e-2, (0.5, 0.9), 1e-3, 0.3),               # every term matters
    "b00": (1e-3, (0.0, 0.0), 1e-8, 1e-2),
    "b39": (1e-3, (0.3, 0.9), 1e-8, 1e-2),
}
STEPS = (1, 7, 1000, 100000)
GSCALES = (1.0, 1.0 / 128)


def flat(n, hyper, step, gscale, state, why, key):
    return dict(kind="flat", n=n, hyper=hyper, step=step, gscale=gscale, state=state, why=why, key=key, mask=None)


def seg(chunk, segs, hyper, step, gscale, state, why, key, bucket=False, bias=None, flatten=False):
    """segs: (elements, gradient offset in floats into its storage | None = null gradient) per segment; bias: per-segment step counts."""
    return dict(kind="seg", chunk=chunk, segs=segs, hyper=hyper, step=step if bias is None else max(bias), gscale=gscale, state=state, why=why,
                key=key, bucket=bucket, bias=bias, flatten=flatten, mask=None)


def _tiny_segs():
    return [(1 + i % 7, None if i % 11 == 5 else i % 4) for i in range(3000)]


_C3 = {4: 11, 1024: 3069, 8192: 20483}   # three chunks, the last one ragged and no multiple of 4: 4+4+3, 2*1024+1021, 2*8192+4099

# fmt: off
ADAMW_CASES = [
    # ---- flat rows: key = ("flat", "f4" | "tailonly", grid-stride trips of the busiest thread, tail length)
    flat(1, "default", 1, 1.0, "zero", "tail only", ("flat", "tailonly", 0, 1)),
    flat(2, "b39", 7, 1 / 128, "rand", "tail only", ("flat", "tailonly", 0, 2)),
    flat(3, "all", 1000, 1.0, "rand", "tail only", ("flat", "tailonly", 0, 3)),
    flat(4, "b39", 100000, 1 / 128, "zero", "one float4", ("flat", "f4", 1, 0)),
    flat(1023, "wd2", 7, 1.0, "rand", "last size of one workgroup", ("flat", "f4", 1, 3)),
    flat(1024, "b00", 1, 1.0, "zero", "one full workgroup", ("flat", "f4", 1, 0)),
    flat(1025, "all", 7, 1 / 128, "rand", "tail behind a full workgroup", ("flat", "f4", 1, 1)),
    flat(99998, "b00", 1000, 1.0, "rand", "98 workgroups, tail of 2", ("flat", "f4", 1, 2)),
    flat(MAX_WGS * WG_ELEMS, "default", 1000, 1 / 128, "rand", "last size without a second grid-stride trip", ("flat", "f4", 1, 0)),
    flat(MAX_WGS * WG_ELEMS + 4, "b00", 100000, 1.0, "rand", "one float4 in the second trip", ("flat", "f4", 2, 0)),
    flat(MAX_WGS * WG_ELEMS + 7, "wd2", 1, 1.0, "zero", "second trip plus tail", ("flat", "f4", 2, 3)),
    # ---- segment rows: key = ("seg", chunk_elems, "bias" | "nobias", "all" | "some" | "none" null segments, segment cells);
    #      a segment cell is path:chunks(3 = three or more):tail of the last chunk, "tailonly" when the float4 loop has no trip
    seg(4, [(1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (11, 0), (11, 1), (7, 2), (3, 3), (9, None)], "default", 1, 1.0, "zero",
        "one thread per chunk", ("seg", 4, "nobias", "some",
                                 ("f4:c1:t0", "f4:c1:t1:tailonly", "f4:c1:t2:tailonly", "f4:c1:t3:tailonly", "f4:c2:t1", "f4:c2:t2", "f4:c2:t3", "f4:c3:t3",
                                  "null:c3", "scalar:c1", "scalar:c2", "scalar:c3"))),
    seg(1024, [(1, 0), (3, 0), (1020, 0), (1021, 0), (1022, 0), (1023, 0), (1024, 0), (1025, 0), (_C3[1024], 0)], "all", 7, 1 / 128, "rand",
        "exactly one loop trip; separate gradient allocations",
        ("seg", 1024, "nobias", "none", ("f4:c1:t0", "f4:c1:t1", "f4:c1:t1:tailonly", "f4:c1:t2", "f4:c1:t3", "f4:c1:t3:tailonly", "f4:c2:t1", "f4:c3:t1"))),
    seg(1024, [(1023, 1), (1025, 2), (_C3[1024], 3), (8, 0)], "b00", 1000, 1.0, "rand", "scalar path at offsets 1, 2, 3; views of one bucket",
        ("seg", 1024, "nobias", "none", ("f4:c1:t0", "scalar:c1", "scalar:c2", "scalar:c3")), bucket=True),
    seg(8192, [(1, 0), (2, 0), (8188, 0), (8189, 0), (8190, 0), (8191, 0), (8192, 0), (8193, 0), (_C3[8192], 0)], "default", 100000, 1 / 128, "rand",
        "eight loop trips (the optimizer's chunk); views of one bucket",
        ("seg", 8192, "nobias", "none", ("f4:c1:t0", "f4:c1:t1", "f4:c1:t1:tailonly", "f4:c1:t2", "f4:c1:t2:tailonly", "f4:c1:t3", "f4:c2:t1", "f4:c3:t3")),
        bucket=True),
    seg(8192, [(_C3[8192], 1), (8193, 2), (5, 3), (_C3[8192], 0)], "b39", 7, 1.0, "zero", "scalar path on multi-chunk segments",
        ("seg", 8192, "nobias", "none", ("f4:c3:t3", "scalar:c1", "scalar:c2", "scalar:c3"))),
    seg(8192, [(5, None), (20003, 0), (_C3[8192], None), (64, 0), (8192, None)], "wd2", 7, 1.0, "rand",
        "null gradient in the first, a multi-chunk middle and the last segment",
        ("seg", 8192, "nobias", "some", ("f4:c1:t0", "f4:c3:t3", "null:c1", "null:c3"))),
    seg(1024, [(5, None), (_C3[1024], None), (1024, None)], "default", 1, 1.0, "rand", "all gradients null: every workgroup returns",
        ("seg", 1024, "nobias", "all", ("null:c1", "null:c3"))),
    seg(8192, [(_C3[8192], 0), (_C3[8192], 1), (5, 0), (8193, 0), (_C3[8192], None)], "all", None, 1 / 128, "rand",
        "bias table, per-segment step counts differ, multi-chunk segments",
        ("seg", 8192, "bias", "some", ("f4:c1:t1", "f4:c2:t1", "f4:c3:t3", "null:c3", "scalar:c3")), bias=[1, 7, 1000, 100000, 3]),
    seg(1024, [(_C3[1024], 2), (1024, 0), (7, 0)], "b39", None, 1.0, "zero", "bias table at the one-trip chunk",
        ("seg", 1024, "bias", "none", ("f4:c1:t0", "f4:c1:t3", "scalar:c3")), bias=[2, 5, 1], bucket=True),
    seg(4, _tiny_segs(), "default", 1000, 1.0, "rand", "3000 tiny segments in one launch",
        ("seg", 4, "nobias", "some", ("f4:c1:t0", "f4:c1:t1:tailonly", "f4:c1:t2:tailonly", "f4:c1:t3:tailonly", "f4:c2:t1", "f4:c2:t2", "f4:c2:t3",
                                      "null:c1", "null:c2", "scalar:c1", "scalar:c2")), bucket=True),
    seg(8192, [(20003, 0), (5, 0), (64, 0), (8192, 0)], "default", 7, 1 / 128, "rand", "tables from FusedAdamW._flatten",
        ("seg", 8192, "nobias", "none", ("f4:c1:t0", "f4:c1:t1", "f4:c3:t3")), flatten=True),
]
# fmt: on

# every reachable cell the matrix must hold a row for.  Flat: the tail runs after the loop whatever the trip count, so each tail length is
# listed once per loop state the boundary sizes reach; two trips need a 4 Mi-element row each and are listed for tail 0 and 3 only.
REACHABLE_FLAT = [("flat", "tailonly", 0, t) for t in (1, 2, 3)] + [("flat", "f4", 1, t) for t in (0, 1, 2, 3)] + [("flat", "f4", 2, 0), ("flat", "f4", 2, 3)]
# Segment: (chunk_elems, bias table, segment cell)
REACHABLE_SEG = (
    [(4, False, c) for c in ("f4:c1:t0", "f4:c1:t1:tailonly", "f4:c1:t2:tailonly", "f4:c1:t3:tailonly", "f4:c2:t1", "f4:c2:t2", "f4:c2:t3", "f4:c3:t3")]
    + [(ch, False, c) for ch in (1024, 8192) for c in ("f4:c1:t0", "f4:c1:t1", "f4:c1:t2", "f4:c1:t3", "f4:c1:t1:tailonly", "f4:c2:t1")]
    + [(1024, False, "f4:c1:t3:tailonly"), (8192, False, "f4:c1:t2:tailonly"), (1024, False, "f4:c3:t1"), (8192, False, "f4:c3:t3")]
    + [(ch, False, c) for ch in (4, 1024, 8192) for c in ("scalar:c1", "scalar:c2", "scalar:c3")]
    + [(4, False, "null:c1"), (4, False, "null:c3"), (1024, False, "null:c1"), (1024, False, "null:c3"), (8192, False, "null:c1"), (8192, False, "null:c3")]
    + [(8192, True, c) for c in ("f4:c1:t1", "f4:c3:t3", "scalar:c3", "null:c3")] + [(1024, True, "scalar:c3"), (1024, True, "f4:c1:t0")]
)


def case_id(case):
    i = ADAMW_CASES.index(case)
    gs = "gs128" if case["gscale"] != 1.0 else "gs1"
    if case["kind"] == "flat":
        return f"{i}-flat-n{case['n']}-{case['hyper']}-s{case['step']}-{gs}-{case['state']}"
    extra = ("-bias" if case["bias"] else "") + ("-bucket" if case["bucket"] else "") + ("-flatten" if case["flatten"] else "")
    return f"{i}-seg-c{case['chunk']}-{len(case['segs'])}segs-{case['hyper']}-s{case['step']}-{gs}-{case['state']}{extra}"


def n_elems(case):
    return case["n"] if case["kind"] == "flat" else sum(n for n, _ in case["segs"])


# --------------------------------------------------------------------------------------------------------------- launch arithmetic
def flat_key(n):
    """Restates kan_adamw_step's launch (kanconv.hip:3296-3299) and k_adamw's loop and tail (kanconv.hip:2677-2685)."""
    n4 = n >> 2                                                         # :2677
    blocks = min(max((n4 + 255) // 256, 1), 256 * 16)                   # :3296-3298
    trips = -(-n4 // (blocks * 256))                                    # :2679: i += gridDim.x * blockDim.x, busiest thread
    return ("flat", "f4" if n4 else "tailonly", trips, n - (n4 << 2))   # :2684-2685


def layout(case):
    """The tables of a segment row as Python lists, and where everything lives: seg_off (multiples of 4 elements, with gaps of 0 / 4 / 8
    elements plus the alignment padding between segments; a `flatten` row: FusedAdamW's 64-element alignment), the block length n_blk, the
    chunk table, elem_off (first element of each segment in the row's dense input vectors) and grad_pos (first element of each gradient in
    the one flat bucket of a `bucket` row, so that the view starts `offset` floats past a 16-byte boundary)."""
    align = 64 if case["flatten"] else 4
    seg_off, seg_n, chunk_seg, chunk_start, elem_off, grad_pos = [], [], [], [], [], []
    cur = e = b = 0
    for i, (n, goff) in enumerate(case["segs"]):
        cur = -(-cur // align) * align + (0 if case["flatten"] else 4 * (i % 3))
        seg_off.append(cur); seg_n.append(n); elem_off.append(e)
        cur += n; e += n
        for s0 in range(0, n, case["chunk"]):
            chunk_seg.append(i); chunk_start.append(s0)
        if goff is None:
            grad_pos.append(None)
        else:
            b = -(-b // 4) * 4 + goff
            grad_pos.append(b)
            b += n
    return dict(seg_off=seg_off, seg_n=seg_n, chunk_seg=chunk_seg, chunk_start=chunk_start, elem_off=elem_off, grad_pos=grad_pos,
                n_blk=-(-cur // align) * align, n_bucket=b + 4)


def seg_key(chunk, seg_n, chunk_seg, chunk_start, grad_addr, has_bias):
    """Restates k_adamw_seg (kanconv.hip:2696-2713) per workgroup from the tables and the gradient addresses (0 = null)."""
    cells = {}
    for sg, start in zip(chunk_seg, chunk_start):                       # :2696
        c = cells.setdefault(sg, dict(chunks=0, path=None, tail=0, trips=0))
        c["chunks"] += 1
        if not grad_addr[sg]:                                           # :2698
            c["path"] = "null"
            continue
        n = min(chunk, seg_n[sg] - start)                               # :2700
        c["path"] = "f4" if (grad_addr[sg] + 4 * start) & 15 == 0 else "scalar"      # :2702-2703
        if c["path"] == "f4":
            c["trips"] = max(c["trips"], -(-(n >> 2) // 256))           # :2704
            c["tail"] = max(c["tail"], n & 3)                           # :2709-2710
    out = set()
    for c in cells.values():
        s = f"{c['path']}:c{min(c['chunks'], 3)}"
        if c["path"] == "f4":
            s += f":t{c['tail']}" + ("" if c["trips"] else ":tailonly")
        out.add(s)
    nulls = [not grad_addr[sg] for sg in sorted(cells)]
    return ("seg", chunk, "bias" if has_bias else "nobias", "all" if all(nulls) else "some" if any(nulls) else "none", tuple(sorted(out)))


def fake_grad_addresses(case, lay):
    """Addresses with the alignment the GPU test's gradient buffers have (their bases are 16-byte aligned), for the CPU key check."""
    if case["bucket"]:
        return [0 if p is None else 1 << 20 | 4 * p for p in lay["grad_pos"]]
    return [0 if goff is None else (i + 1) << 20 | 4 * goff for i, (_, goff) in enumerate(case["segs"])]


def elem_steps(case):
    """Per-element step counts of a bias-table row (int64 tensor), else the row's scalar step."""
    if case["kind"] == "flat" or case["bias"] is None:
        return case["step"]
    return torch.cat([torch.full((n,), st, dtype=torch.int64) for (n, _), st in zip(case["segs"], case["bias"])])


def active_elems(case):
    """bool per element: False inside a segment whose gradient is null (torch skips it: nothing may change)."""
    if case["kind"] == "flat":
        return torch.ones(case["n"], dtype=torch.bool)
    return torch.cat([torch.full((n,), goff is not None, dtype=torch.bool) for n, goff in case["segs"]])


def bias_table(hyper, steps):
    """{ -lr / (1 - beta1^step_s), 1 / sqrt(1 - beta2^step_s) } per segment, as include/kanconv.h defines seg_bias and optim.py builds it."""
    lr, (b1, b2), _, _ = HYPER[hyper]
    return [[-lr / (1.0 - b1 ** st), 1.0 / (1.0 - b2 ** st) ** 0.5] for st in steps]


# --------------------------------------------------------------------------------------------------------------- inputs and reference
def make_inputs(case):
    """fp32 CPU tensors p, g, m, v over the row's elements (segments back to back), drawn in fp64 from seed 2000 + row index."""
    N = n_elems(case)
    gen = torch.Generator().manual_seed(2000 + ADAMW_CASES.index(case))
    rand = lambda: torch.rand(N, generator=gen, dtype=torch.float64)
    randn = lambda: torch.randn(N, generator=gen, dtype=torch.float64)
    mag = lambda: 10.0 ** torch.randint(-6, 3, (N,), generator=gen).double()
    g = mag() * (1 + 9 * rand()) * torch.where(rand() < 0.5, -1.0, 1.0) * (rand() >= 0.05)
    cls = torch.arange(N) % 3
    p = randn() * torch.where(cls == 0, 0.0, torch.where(cls == 1, 1e-3, 1.0))
    scale = mag() * case["gscale"]
    m, v = randn() * scale, scale * scale * (0.5 + rand())
    if case["state"] == "zero":
        m, v = torch.zeros_like(m), torch.zeros_like(v)
    return dict(p=p.float(), g=g.float(), m=m.float(), v=v.float())


def torch_order_step(p, g, m, v, hyper, step, gscale):
    """One AdamW step, out of place, in the dtype of its arguments: the formulas of torch's single-tensor path in their order
    (torch/optim/adam.py _single_tensor_adam with decoupled weight decay), grad_scale folded into the gradient first."""
    lr, (b1, b2), eps, wd = hyper
    g = g * gscale
    p = p * (1 - lr * wd)
    m = torch.lerp(m, g, 1 - b1)                                        # ATen: weight < 0.5 ? m + w (g - m) : g - (g - m)(1 - w)
    v = (v * b2).addcmul(g, g, value=1 - b2)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = (v.sqrt() / bc2 ** 0.5).add(eps)
    return p.addcdiv(m, denom, value=-lr / bc1), m, v


def reference(case, inp, dtype, step_fn=torch_order_step):
    """dict(p, m, v) of the row after its step in `dtype`; elements of null segments keep their input values."""
    lr_etc, steps, act = HYPER[case["hyper"]], elem_steps(case), active_elems(case)
    t = {k: x.to(dtype) for k, x in inp.items()}
    out = {k: t[k].clone() for k in "pmv"}
    groups = [(int(s), act & (steps == s)) for s in steps.unique()] if torch.is_tensor(steps) else [(steps, act)]
    for st, sel in groups:
        if not bool(sel.any()):
            continue
        whole = bool(sel.all())
        args = [t[k] if whole else t[k][sel] for k in "pgmv"]
        for k, r in zip("pmv", step_fn(*args, lr_etc, st, case["gscale"])):
            if whole:
                out[k] = r
            else:
                out[k][sel] = r
    return out


@functools.lru_cache(maxsize=2)
def reference_pair(idx):
    """Row ADAMW_CASES[idx]: (inputs, fp64 results, fp32 results) -- computed once, shared, never modified."""
    case = ADAMW_CASES[idx]
    inp = make_inputs(case)
    return inp, reference(case, inp, torch.float64), reference(case, inp, torch.float32)


# --------------------------------------------------------------------------------------------------------------- the kernel's arithmetic in fp32
def _f32(x):
    with np.errstate(all="ignore"):
        return float(np.float32(x))


def kernel_args(hyper, step, gscale, wrong=None):
    """adam_args (kanconv.hip:2716-2723): every scalar formed in double, rounded to fp32 once."""
    lr, (b1, b2), eps, wd = hyper
    st = step - 1 if wrong == "bias_from_step_minus_1" else step
    with np.errstate(all="ignore"):
        bc1, bc2 = np.float64(1.0) - np.float64(b1) ** st, np.float64(1.0) - np.float64(b2) ** st
        a = dict(decay=_f32(1.0 - lr * wd), w1=_f32(1.0 - b1), b1=_f32(b1), b2=_f32(b2), w2=_f32(1.0 - b2), gscale=_f32(gscale),
                 inv_bc2_sqrt=_f32(1.0 / np.sqrt(bc2)), eps=_f32(eps), neg_step=_f32(-lr / bc1))
    if wrong == "one_minus_float_beta2":
        a["w2"] = float(np.float32(1.0) - np.float32(b2))
    return a


WRONG = ("eps_inside_sqrt", "bias_from_step_minus_1", "decay_after_update", "one_minus_float_beta2", "gscale_missing_from_v", "bias_pair_swapped",
         "one_branch_lerp")


def kernel_restatement(case, inp, wrong=None):
    """adam1 (kanconv.hip, section "optimizer step") in fp32 torch arithmetic, one rounding per operation (no fused multiply-add), over the
    row's elements; `wrong` names one deliberate mistake.  Returns dict(p, m, v); null segments keep their inputs."""
    assert wrong is None or wrong in WRONG
    a = kernel_args(HYPER[case["hyper"]], case["step"], case["gscale"], wrong)
    p, g0, m, v = (inp[k].clone() for k in "pgmv")
    neg, inv = a["neg_step"], a["inv_bc2_sqrt"]
    if case["kind"] == "seg" and case["bias"] is not None:              # k_adamw_seg: seg_bias[2 sg], seg_bias[2 sg + 1]
        tab = torch.tensor(bias_table(case["hyper"], case["bias"]), dtype=torch.float32)
        if wrong == "bias_pair_swapped":
            tab = tab.flip(1)
        per = torch.cat([tab[i].expand(n, 2) for i, (n, _) in enumerate(case["segs"])])
        neg, inv = per[:, 0].contiguous(), per[:, 1].contiguous()
    g = g0 * a["gscale"]
    pd = p * a["decay"]
    if wrong == "one_branch_lerp":
        m1 = m + (g - m) * a["w1"]
    else:
        m1 = g - (g - m) * a["b1"] if a["w1"] >= 0.5 else m + (g - m) * a["w1"]
    gv = g0 if wrong == "gscale_missing_from_v" else g
    v1 = v * a["b2"] + a["w2"] * gv * gv
    if wrong == "eps_inside_sqrt":
        denom = torch.sqrt(v1 * inv * inv + a["eps"])
    else:
        denom = torch.sqrt(v1) * inv + a["eps"]
    p1 = (p + neg * (m1 / denom)) * a["decay"] if wrong == "decay_after_update" else pd + neg * (m1 / denom)
    act = active_elems(case)
    return dict(p=torch.where(act, p1, p), m=torch.where(act, m1, m), v=torch.where(act, v1, v))


# --------------------------------------------------------------------------------------------------------------- judge
def judged_elems(case, inp, r64):
    """bool per element: True = judged.  Every row judges every element; a row that cannot names its reason in case["mask"]."""
    assert case["mask"] is None
    return torch.ones(n_elems(case), dtype=torch.bool)


def _errors(case, inp, res, r64, keep):
    """{tensor: largest normalised error of `res` against the fp64 reference}; NaN anywhere makes the figure NaN."""
    d = lambda t: t.detach().double().cpu().reshape(-1)
    out = {}
    zero = (inp["p"] == 0) & keep
    for name, sel in (("p(from 0)", zero), ("p(rest)", ~zero & keep)):
        if bool(sel.any()):
            out[name] = float(((d(res["p"]) - r64["p"])[sel].abs() / (r64["p"][sel].abs().max() + 1e-300)).max())
    if bool(keep.any()):
        mscale = torch.maximum(inp["m"].double().abs(), (inp["g"].double() * case["gscale"]).abs())
        out["m"] = float(((d(res["m"]) - r64["m"]).abs() / (mscale + 1e-300))[keep].max())
        out["v"] = float(((d(res["v"]) - r64["v"]).abs() / (r64["v"] + 1e-300))[keep].max())       # (reference 0: any other value is an error of 1e300)
    return out


def judge(case, inp, got, r64, r32):
    """Judges dict(p, m, v) `got` (any float dtype, the row's element order).  Returns (lines, bad): one "<tensor> <err> (tol, fp32
    reference)" string per judged tensor, and the failures."""
    keep = judged_elems(case, inp, r64)
    err, noise = _errors(case, inp, got, r64, keep), _errors(case, inp, r32, r64, keep)
    lines, bad = [], []
    for name, e in err.items():
        tol = max(FLOOR, 4.0 * noise[name])
        lines.append(f"{name} {e:.1e} (tol {tol:.1e}, fp32 reference {noise[name]:.1e})")
        if not e <= tol:
            bad.append(f"{name}: error {e:.3e} > {tol:.3e} (fp32 reference {noise[name]:.3e})")
    return lines, bad


# --------------------------------------------------------------------------------------------------------------- special values
SPECIAL_HYPER, SPECIAL_STEP = "all", 7


def special_inputs():
    """19 elements (four float4 and a tail of three): g = 0 on zero moments; NaN, +inf and -inf each alone in its float4 and in the tail;
    |g| = 1e20 (v overflows: (1 - 0.9) x 1e40).  Returns (inputs, poisoned: bool per element)."""
    nan, inf = float("nan"), float("inf")
    g = torch.tensor([0.0, nan, 1.0, -2.0, 1e-3, 3.0, inf, 0.5, -inf, 1.0, 2.0, 1e20, -1e20, 4.0, 0.0, 1.0, 1.0, nan, -3.0])
    p = torch.linspace(-1.0, 1.0, 19)
    m, v = torch.full((19,), 0.25), torch.full((19,), 0.5)
    m[0] = v[0] = m[14] = v[14] = 0.0
    return dict(p=p, g=g, m=m, v=v), ~torch.isfinite(g)


def special_reference(inp):
    return dict(zip("pmv", torch_order_step(inp["p"], inp["g"], inp["m"], inp["v"], HYPER[SPECIAL_HYPER], SPECIAL_STEP, 1.0)))


def judge_special(inp, poisoned, got, r32):
    """By class against the fp32 CPU run: a poisoned element is non-finite in p, m and v; every other element has the fp32 run's class
    (+-inf, exact 0, finite) and, where finite, its value to FLOOR relative."""
    bad = []
    for k in "pmv":
        a, b = got[k].detach().float().cpu(), r32[k]
        if bool(torch.isfinite(a[poisoned]).any()):
            bad.append(f"{k}: a NaN / inf gradient left a finite value at {torch.isfinite(a) & poisoned}")
        for i in (~poisoned).nonzero().flatten().tolist():
            x, y = float(a[i]), float(b[i])
            ok = x == y if (math.isinf(y) or y == 0.0) else math.isfinite(x) and abs(x - y) <= FLOOR * abs(y)
            if not ok:
                bad.append(f"{k}[{i}]: {x} vs {y} (g = {float(inp['g'][i])})")
    return bad

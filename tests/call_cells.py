"""The calling-condition matrix of the autograd ops (convkan_amd/ops.py): SUBJECTS x CONDITIONS, and the judge.

Every fp64 matrix of this suite calls the ops one way: a contiguous fp32 input made on the default stream, every parameter and the input
asking for a gradient, a contiguous incoming gradient, one backward.  This matrix leaves that one calling condition.  A cell runs a subject
under a condition and compares it with THE SAME subject under the canonical call -- the call the existing matrices already judge against
fp64 -- so the op, the shapes and the launch plan are the same on both sides and the expected result is bit equality (`torch.equal`).

Subjects: one per code path of ops.py, each of them a row of an existing table (route_cells.ROUTE_CASES and order_cells.ORDER_CASES looked up by key and index, the
fixtures of tests/golden/heads, tests/golden/mlp_tiny, a wav_cells row, the two smallest draws of test_gpu_fuzz's 1-D and 3-D tests), so
the canonical call is oracle-checked by an existing test; tests/test_call_matrix.py holds the table to that on the CPU.

Conditions: `CONDITIONS` maps each of the eleven conditions to its variants; `EXCLUSIONS` lists, with one line of reason each, the
(condition or variant, subject) pairs that make no sense.  Nothing else is left out: every other pair is a test of
tests/test_gpu_call_matrix.py.

The judge (`same`): which class a tensor falls in is decided by `klass` alone, never per cell.
  bits    y, dx, every parameter gradient with dim() >= 3 that is not a phase (the W_IOD coefficient gradients among them), dlogits, lse,
          the loss, the metric counters, the running statistics, and every gradient of a BatchNorm subject (its kernels have no float
          atomics: test_gpu_bnorm_matrix).
  atomic  the float-atomic sums -- scalar PReLU slopes, InstanceNorm gamma / beta gradients, phase and Gram-coefficient gradients; by the
          rule dim() < 3 of helpers.check_vs_oracle -- get the bound the project already uses for them, 2e-5 max-normalised
          (split_cells.same_but_slopes, test_gpu_route_matrix._run draws the same line).
Every variant compares y bitwise and dx or a dim() >= 3 gradient bitwise (`same` refuses a comparison that would not), except the
refusals, which assert the exception type and that no tensor reached `.grad`.

The same condition code runs on the CPU over a toy pure-torch Function with planted defects (test_call_matrix.py): each defect must be
caught, the correct version must pass."""
import contextlib
import copy
import random

import torch
import torch.nn as nn

ATOMIC_TOL = 2e-5
INPLACE = "modified by an inplace operation"
ONCE = "once_differentiable"


# ================================================================================================ subjects
def _s(sid, kind, path, **kw):
    return dict(id=sid, kind=kind, path=path, **kw)


_KAN = "FAST_BSPLINE_SILU HALO TAP-RB HALO"
SUBJECTS = [
    # 1: KANConv2DLayer SiLU, 3x3 pad 1, B 8, C 2, O 128, 4x4 -- single group, cacheable: the persistent packed layouts of `_pack`
    _s("kan-silu", "route", "cached pack; _KanConvInPrelu, InstanceNorm tail", key=_KAN, index=0, shape=(8, 2, 128, 4, 1)),
    _s("kan-silu-affine", "route", "cached pack; _KanConvInPrelu, affine InstanceNorm tail", key=_KAN, index=0, shape=(8, 2, 128, 4, 1), affine=True),
    # 2: the same layer with norm_layer=BatchNorm2d
    _s("kan-bn-train", "route", "_KanConvInPrelu, BatchNorm tail, batch statistics", key=_KAN, index=0, shape=(8, 2, 128, 4, 1), bn=True, training=True,
       stateful=True),
    _s("kan-bn-eval", "route", "_KanConvInPrelu, BatchNorm tail, running statistics", key=_KAN, index=0, shape=(8, 2, 128, 4, 1), bn=True, training=False),
    # 3 - 6
    _s("cheby-grouped", "route", "grouped: fresh() pack; no base branch", key="FAST_CHEBY5 BAND TAP BAND", index=1, shape=(17, 6, 2, 5, 2)),
    _s("relu-phases", "route", "kan_conv_phased, ReLU-KAN phases", key="FAST_RELU8 TAP TAP TAP-PM", index=0, shape=(17, 6, 2, 3, 2)),
    _s("gram-coeffs", "route", "kan_conv_phased, Gram coefficients", key="FAST_GRAM4 TAP TAP TAP-PM", index=0, shape=(17, 2, 32, 3, 2)),
    _s("legendre-xn", "route", "second input xn", key="FAST_POLY4 TAP TAP TAP", index=1, shape=(17, 3, 40, 2, 1)),
    # 7: the smallest (B * C * O * pixels) B-spline draws of test_gpu_fuzz.test_random_1d_vs_oracle / test_random_3d_vs_oracle
    _s("kan-1d", "fuzz1d", "1-D shim: weight.unsqueeze(2) views", seed=16),
    _s("kan-3d", "fuzz3d", "3-D shim: one launch set per depth tap over gathered slices", seed=7),
    # 8: the smallest wav_cells row a WavKANConv2DLayer can be built from (plain row, int kernel / stride / padding / dilation)
    _s("wav", "wav", "_WavStage", row=27),
    # 9: the W_IOD heads, from tests/golden/heads
    _s("head-cheby", "head", "W_IOD, 130 outputs", name="cheby_o130"),
    _s("head-lucas", "head", "W_IOD, 300 inputs: 9 forward slabs", name="lucas_i300"),
    # 10: KANLayer(7, 3), tests/golden/mlp_tiny
    _s("mlp-kan", "mlp", "1x1 plane with a base branch", name="mlp_tiny"),
    # 11: the norm ops called directly, B 3, C 5, 4x6, affine
    _s("instance-norm", "normop", "_InstanceNorm", shape=(3, 5, 4, 6)),
    _s("batch-norm", "normop", "_InstanceNorm with BatchStats", shape=(3, 5, 4, 6), bn=True, training=True, stateful=True),
    # 12: the loss
    _s("xent-5x10", "loss", "_CrossEntropy", shape=(5, 10), metrics=False),
    _s("xent-5x10-metrics", "loss", "_CrossEntropy with ClassMetrics", shape=(5, 10), metrics=True, stateful=True),
    _s("xent-257x100", "loss", "_CrossEntropy, more than one block", shape=(257, 100), metrics=False),
    _s("xent-257x100-metrics", "loss", "_CrossEntropy with ClassMetrics, more than one block", shape=(257, 100), metrics=True, stateful=True),
    # 13: the 8x8 tile orders KanPlan does not show, rows of order_cells.ORDER_CASES (key: spec class, orders, groups, the three routes): the smallest row
    # whose forward runs half-plane row blocks and whose weight gradient takes its own 8x8 entry (B 4, C 2, O 256), and the smallest row whose bwd-data runs
    # the 32-image row-segment tiles from a dz_pm that `_conv_backward` builds for them alone (B 32, C 1, O 16), the latter under the BatchNorm tail
    _s("kan8-rowblk-pos8bw", "order", "k_conv_fwd_halo row blocks; kan_conv_bwd_weight_rowgroups + kan_unpack_wgrad_rowgroups",
       key="FAST_BSPLINE_SILU POS8_BWD_WEIGHT+ROWBLK8_FWD G1 HALO TAP HALO", index=0, shape=(4, 2, 256, 8, 1)),
    _s("kan8-pos8bd-bn", "order", "dz_pm built for bwd-data alone (_pos8_bwd_data); BatchNorm tail, batch statistics",
       key="FAST_BSPLINE_SILU POS8_BWD_DATA G1 BAND TAP BAND", index=0, shape=(32, 1, 16, 8, 1), bn=True, training=True, stateful=True),
]
SUBJECT = {s["id"]: s for s in SUBJECTS}


def order_row_key(subject):
    """The order_cells key an `order` subject names: "spec orders G<n> fwd bwd-data bwd-weight"."""
    spec, orders, grouped, *routes = subject["key"].split()
    return (spec, tuple(sorted(orders.split("+"))), grouped != "G1") + tuple(routes)


def route_row(subject):
    """The ROUTE_CASES row of a `route` subject, the ORDER_CASES row of an `order` subject: the `index`-th row whose key is `key`."""
    if subject["kind"] == "order":
        from order_cells import ORDER_CASES
        rows = [c for c in ORDER_CASES if c["key"] == order_row_key(subject)]
        return rows[subject["index"]]
    from route_cells import ROUTE_CASES
    rows = [c for c in ROUTE_CASES if c["key"] == tuple(subject["key"].split())]
    return rows[subject["index"]]


def fuzz_1d(seed):
    """The draw of test_gpu_fuzz.test_random_1d_vs_oracle(seed), restated (seed % 4 == 0: the B-spline layer)."""
    r = random.Random(9000 + seed)
    G = r.choice([1, 1, 2, 3])
    C, O = r.choice([1, 2, 3, 8]) * G, r.choice([1, 4, 16, 64, 128]) * G
    k = r.choice([1, 3, 3, 5, 7])
    s_, d = r.choice([1, 1, 2, 3]), r.choice([1, 1, 2])
    p = r.choice([0, 1, d * (k - 1) // 2, d * (k - 1)])
    Lx = r.choice([4, 9, 16, 33, 64, 200, 1000])
    if (Lx + 2 * p - d * (k - 1) - 1) // s_ + 1 < 4:
        p, s_ = d * (k - 1), 1
    B = r.choice([1, 2, 5, 16]) if O * Lx <= 65536 else r.choice([1, 2])
    return dict(G=G, C=C, O=O, k=k, s=s_, d=d, p=p, dims=(Lx,), B=B)


def fuzz_3d(seed):
    """The draw of test_gpu_fuzz.test_random_3d_vs_oracle(seed), restated (seed % 7 == 0: the B-spline layer)."""
    r = random.Random(11000 + seed)
    G = r.choice([1, 1, 2])
    C, O = r.choice([1, 2, 3, 6]) * G, r.choice([1, 4, 16, 64]) * G
    k = r.choice([1, 3, 3])
    s_, d = r.choice([1, 1, 2]), r.choice([1, 1, 2])
    p = r.choice([0, 1, 2])
    D, H, W = r.choice([1, 2, 3, 5, 8]), r.choice([3, 4, 6, 8]), r.choice([3, 4, 7, 8])

    def out(n):
        return (n + 2 * p - d * (k - 1) - 1) // s_ + 1
    if min(out(D), out(H), out(W)) <= 0 or out(D) * out(H) * out(W) < 4:
        p, s_ = d * (k - 1), 1
        if out(D) * out(H) * out(W) < 4:
            H, W = 4, 4
    B = r.choice([1, 2, 5])
    return dict(G=G, C=C, O=O, k=k, s=s_, d=d, p=p, dims=(D, H, W), B=B)


def fuzz_size(c):
    n = c["B"] * c["C"] * c["O"]
    for v in c["dims"]:
        n *= v
    return n


def wav_rows():
    """The wav_cells rows a layer can be built from, with their size."""
    from wav_cells import WAV_CASES
    return [(i, c["B"] * c["C"] * c["O"] * c["H"] * c["W"]) for i, c in enumerate(WAV_CASES)
            if c["kind"] is None and all(isinstance(c[n], int) for n in ("k", "s", "p", "d"))]


class _NormOp(nn.Module):
    """`ops.instance_norm` / `ops.batch_norm` called directly, as a module so that the conditions find its parameters and buffers."""

    def __init__(self, C, bn, gen):
        super().__init__()
        self.bn = bn
        self.gamma = nn.Parameter(1.0 + 0.2 * torch.randn(C, generator=gen))
        self.beta = nn.Parameter(0.2 * torch.randn(C, generator=gen))
        if bn:
            self.register_buffer("running_mean", 0.1 * torch.randn(C, generator=gen))
            self.register_buffer("running_var", 1.0 + 0.1 * torch.rand(C, generator=gen))

    def forward(self, x, gamma=None, beta=None):
        from convkan_amd import ops
        gamma, beta = self.gamma if gamma is None else gamma, self.beta if beta is None else beta
        if self.bn:
            return ops.batch_norm(x, gamma, beta, self.running_mean, self.running_var, self.training)
        return ops.instance_norm(x, gamma, beta)


class _Loss(nn.Module):
    """`ops.cross_entropy` against a fixed target; the counters of a ClassMetrics are a buffer (restored before every run)."""

    def __init__(self, target, classes, metrics):
        super().__init__()
        from convkan_amd.loss import ClassMetrics
        self.register_buffer("target", target)
        if metrics:
            self.register_buffer("counters", ClassMetrics(classes, device="cpu").buffer)

    def forward(self, logits, target=None):
        from convkan_amd import ops
        return ops.cross_entropy(logits, self.target if target is None else target, getattr(self, "counters", None))


def _perturb(layer, affine, gen):
    """Trainable basis parameters and an affine norm away from their init (test_gpu_route_matrix._perturb)."""
    with torch.no_grad():
        if hasattr(layer, "phase_low"):
            layer.phase_low.add_(0.06 * torch.randn(layer.phase_low.shape, generator=gen))
            layer.phase_high.add_(0.06 * torch.randn(layer.phase_high.shape, generator=gen))
        if hasattr(layer, "beta_weights"):
            layer.beta_weights.copy_(0.2 * torch.randn(layer.beta_weights.shape, generator=gen))
        if affine:
            for m in layer.layer_norm:
                m.weight.add_(0.2 * torch.randn(m.weight.shape, generator=gen))
                m.bias.add_(0.2 * torch.randn(m.bias.shape, generator=gen))


def build(subject):
    """(module, x) of a subject on the CPU, the same on every call (seeded)."""
    import convkan_amd as K
    kind = subject["kind"]
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(1)
    if kind in ("route", "order"):
        from route_cells import LAYERS, SHAPES, case_layer
        case = dict(route_row(subject))
        if subject.get("affine"):
            case["affine"] = True
        if subject.get("bn"):
            cls, kw = LAYERS[case["layer"]]
            m = getattr(K, cls)(case["C"], case["O"], norm_layer=nn.BatchNorm2d, **dict(kw, groups=case["G"], **SHAPES[case["shape"]]))
            with torch.no_grad():
                for n in m.layer_norm:
                    n.weight.add_(0.2 * torch.randn(n.weight.shape, generator=gen))
                    n.bias.add_(0.2 * torch.randn(n.bias.shape, generator=gen))
                    n.running_mean.add_(0.1 * torch.randn(n.running_mean.shape, generator=gen))
                    n.running_var.add_(0.1 * torch.rand(n.running_var.shape, generator=gen))
        else:
            m = case_layer(case)
            _perturb(m, case.get("affine"), gen)
        x = torch.randn(case["B"], case["C"], case["H"], case["W"], generator=gen) * case.get("scale", 1.0)
    elif kind in ("fuzz1d", "fuzz3d"):
        c = fuzz_1d(subject["seed"]) if kind == "fuzz1d" else fuzz_3d(subject["seed"])
        cls = K.KANConv1DLayer if kind == "fuzz1d" else K.KANConv3DLayer
        m = cls(c["C"], c["O"], c["k"], groups=c["G"], stride=c["s"], dilation=c["d"], padding=c["p"])
        x = torch.randn(c["B"], c["C"], *c["dims"], generator=gen)
    elif kind == "wav":
        from wav_cells import WAV_CASES
        c = WAV_CASES[subject["row"]]
        m = K.WavKANConv2DLayer(c["C"], c["O"], c["k"], stride=c["s"], padding=c["p"], dilation=c["d"], wavelet_type=c["wavelet"], norm_layer=nn.InstanceNorm2d)
        x = torch.randn(c["B"], c["C"], c["H"], c["W"], generator=gen)
    elif kind == "head":
        from heads_cases import build_head, load_head, state_dict_of
        d = load_head(subject["name"])
        m = build_head(d["cfg"])
        m.load_state_dict(state_dict_of(d))
        x = torch.from_numpy(d["x"]).clone()
    elif kind == "mlp":
        from conftest import load_golden
        from helpers import ACTS
        d = load_golden(subject["name"])
        c = d["cfg"]
        m = K.KANLayer(c["I"], c["O"], grid_size=c["G"], spline_order=c["S"], base_activation=ACTS[c["act"]], grid_range=c["rng"])
        m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in d.items() if k.startswith("sd.")})
        x = torch.from_numpy(d["x"]).clone()
    elif kind == "normop":
        B, C, H, W = subject["shape"]
        m = _NormOp(C, bool(subject.get("bn")), gen)
        x = torch.randn(B, C, H, W, generator=gen)
    elif kind == "loss":
        B, C = subject["shape"]
        m = _Loss(torch.randint(0, C, (B,), generator=gen), C, subject["metrics"])
        x = 3.0 * torch.randn(B, C, generator=gen)
    else:
        raise KeyError(kind)
    m.train(bool(subject.get("training", True)))
    return m, x


# ================================================================================================ a live subject and its runs
def group_of(name):
    """Which `needs_input_grad` subset a parameter belongs to."""
    if name.startswith(("phase", "beta_weights")) or name.endswith((".scale", ".translation")):
        return "phase"
    if name.startswith(("base_conv", "base_weight")):
        return "base"
    if "layer_norm" in name or name.startswith(("prelu", "gamma", "beta")):
        return "affine"
    return "conv"


class Result:
    """What one call left behind, cloned: y, dx (None: not asked for), dw {parameter: gradient or None}, state {buffer and extra tensors}."""

    def __init__(self, y, dx, dw, state):
        self.y, self.dx, self.dw, self.state = y, dx, dw, state


class Live:
    """A subject on a device: the module, the canonical input and incoming gradient, and the canonical Result (computed once, shared,
    never modified)."""

    functions = None                # the autograd Functions whose backwards `cell_needs` watches (None: those of convkan_amd.ops)
    peek = True                     # state_of may read the node's saved tensors (not under checkpoint: that would start its recomputation)

    def __init__(self, subject, module, x, device, call=None, sync=None):
        self.subject, self.sid, self.device = subject, subject["id"], torch.device(device)
        self.module, self.x = module.to(device), x.to(device).contiguous()
        self.call = call if call is not None else (lambda m, t: m(t))
        self.sync = sync if sync is not None else ((lambda: torch.cuda.synchronize()) if self.device.type == "cuda" else (lambda: None))
        self.buffers0 = {n: b.clone() for n, b in self.module.named_buffers()}
        with torch.no_grad():
            shape = self.call(self.module, self.x).shape
        self.restore()
        self.go = torch.randn(shape, generator=torch.Generator().manual_seed(2)).to(device)
        self._canon = None

    @property
    def bits_only(self):
        return bool(self.subject.get("bn"))

    @property
    def params(self):
        return dict(self.module.named_parameters())

    def restore(self):
        with torch.no_grad():
            for n, b in self.module.named_buffers():
                b.copy_(self.buffers0[n])

    def fresh(self):
        """An equal subject of its own: new Parameters (so new cache entries and version counters), same values, same x and go."""
        other = copy.copy(self)
        other.module = copy.deepcopy(self.module)
        other.restore()
        other._canon = self._canon
        return other

    @property
    def canon(self):
        if self._canon is None:
            self._canon = run(self)
        return self._canon


def prepare(live, need=None, need_x=True, x=None):
    """Buffers restored, gradients cleared, requires_grad set (`need`: None = every parameter, else the set of names); returns the input leaf
    (a detached alias of `x`: same storage, same strides)."""
    live.restore()
    for n, p in live.module.named_parameters():
        p.requires_grad_(need is None or n in need)
        p.grad = None
    xg = (live.x if x is None else x).detach()
    xg.requires_grad_(need_x)
    return xg


def state_of(live, y):
    """Buffers (running statistics, metric counters) after the call, and the loss's lse (saved on the node)."""
    st = {"buf." + n: b.detach().clone() for n, b in live.module.named_buffers()}
    if live.peek and live.subject["kind"] == "loss" and y.grad_fn is not None and hasattr(y.grad_fn, "saved_tensors"):
        st["lse"] = y.grad_fn.saved_tensors[2].detach().clone()
    return st


def collect(live, xg, y, state=None):
    live.sync()
    dx = xg.grad.detach().clone() if xg.grad is not None else None
    dw = {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in live.module.named_parameters()}
    return Result(y.detach().clone(), dx, dw, state if state is not None else {})


def run(live, x=None, go=None, need=None, need_x=True, ctx=contextlib.nullcontext):
    """One forward and backward.  `ctx`: a context manager factory the whole call runs inside."""
    xg = prepare(live, need, need_x, x)
    with ctx():
        y = live.call(live.module, xg)
        state = state_of(live, y)
        if y.requires_grad:
            y.backward(live.go if go is None else go)
    return collect(live, xg, y, state)


# ================================================================================================ the judge
def klass(live, name):
    """`bits` or `atomic` for a parameter's gradient: the one place that decides."""
    if live.bits_only:
        return "bits"
    p = live.params[name]
    return "bits" if p.dim() >= 3 and not name.startswith("phase") else "atomic"


def _close(a, b, scale=None):
    ref = float(b.abs().max()) if scale is None else scale
    return float((a.double() - b.double()).abs().max()) <= ATOMIC_TOL * max(ref, 1e-30) if ref > 0 else bool((a == b).all())


def same(live, want, got, what, grads=True, state=True, factor=1.0):
    """`got` equals `want` by the class rule.  `factor`: the gradients of `got` are `factor` times those of `want` (exactly, for a power of
    two).  Raises AssertionError naming every tensor that differs; refuses to pass a comparison without a bitwise gradient."""
    bad, bitwise, scal_w, scal_g = [], 0, [], []
    if not torch.equal(want.y, got.y):
        bad.append(f"y (max |diff| {float((want.y.double() - got.y.double()).abs().max()):.3e})")
    if grads:
        if (want.dx is None) != (got.dx is None):
            bad.append("dx: one is None")
        elif want.dx is not None:
            bitwise += 1
            if not torch.equal(want.dx * factor, got.dx):
                bad.append(f"dx (max |diff| {float((want.dx.double() * factor - got.dx.double()).abs().max()):.3e})")
        for n, w in want.dw.items():
            g = got.dw[n]
            if (w is None) != (g is None):
                bad.append(f"{n}: one is None")
            elif w is None:
                continue
            elif klass(live, n) == "bits":
                bitwise += 1
                if not torch.equal(w * factor, g):
                    bad.append(f"{n} (max |diff| {float((w.double() * factor - g.double()).abs().max()):.3e})")
            elif w.numel() == 1:                            # the per-group scalar slopes are judged together, as split_cells.same_but_slopes
                scal_w.append(w.reshape(-1) * factor)       # and helpers.check_vs_oracle judge them
                scal_g.append(g.reshape(-1))
            elif not _close(g, w * factor):
                bad.append(f"{n} (atomic class: max |diff| {float((w.double() * factor - g.double()).abs().max()):.3e} of max {float(w.abs().max() * factor):.3e})")
        if scal_w and not _close(torch.cat(scal_g), torch.cat(scal_w)):
            bad.append(f"scalar slopes (atomic class: {torch.cat(scal_g).tolist()} vs {torch.cat(scal_w).tolist()})")
        assert bitwise, f"{live.sid} {what}: a comparison with no bitwise gradient (vacuous cell)"
    if state:
        missing = [n for n in want.state if n.startswith("buf.") and n not in got.state]
        assert not missing, f"{live.sid} {what}: no {missing} to compare"
        bad += [f"{n}" for n in want.state if n in got.state and not torch.equal(want.state[n], got.state[n])]
    assert not bad, f"{live.sid} {what}: differs from the canonical call in {bad}"


def oracle_judge(live, got, what):
    """A route subject's result against the fp64 oracle by helpers.check_vs_oracle's rule: per tensor max(stated tolerance, 4 x the fp32
    oracle's own error against fp64).  For a tensor a condition legitimately cannot reproduce bit for bit (ORACLE_JUDGED)."""
    from helpers import TOL_DW, TOL_DX, TOL_Y, oracle_run, relerr
    from route_cells import case_cfg
    case = route_row(live.subject)
    layer = copy.deepcopy(live.module).cpu()
    cfg, x, go = case_cfg(case, layer), live.x.cpu(), live.go.cpu()
    y32, dx32, dw32, _ = oracle_run(cfg, layer, x, go, torch.float32)
    y64, dx64, dw64, _ = oracle_run(cfg, layer, x, go, torch.float64)
    rows = [("y", got.y, y32, y64, TOL_Y), ("dx", got.dx, dx32, dx64, TOL_DX)]
    rows += [(n, g, dw32[n], dw64[n], TOL_DW if live.params[n].dim() >= 3 else ATOMIC_TOL) for n, g in got.dw.items() if g is not None]
    bad = {}
    for n, g, a32, a64, base in rows:
        err, own = relerr(g, a64), relerr(a32, a64)
        if not err <= max(base, 4.0 * own):
            bad[n] = (err, max(base, 4.0 * own), own)
    assert not bad, f"{live.sid} {what}: (error, tolerance, fp32 oracle's own error) vs the fp64 oracle: {bad}"


def no_grads(live, xg=None):
    left = [n for n, p in live.module.named_parameters() if p.grad is not None] + (["x"] if xg is not None and xg.grad is not None else [])
    assert not left, f"{live.sid}: a refused call left gradients in {left}"


# ================================================================================================ strided forms
def permuted(t):
    """The values of `t` in another memory order: channels_last (4-D), channels_last_3d (5-D), the transposed view of a transposed
    copy (2-D and 3-D).  The storage holds exactly numel elements."""
    if t.dim() == 4:
        return t.contiguous(memory_format=torch.channels_last)
    if t.dim() == 5:
        return t.contiguous(memory_format=torch.channels_last_3d)
    return t.transpose(-1, -2).contiguous().transpose(-1, -2)


def cols2(t):
    """Every second column of a buffer twice as wide (2 x numel elements of storage; the other columns hold a value no result may show)."""
    buf = torch.full(t.shape[:-1] + (2 * t.shape[-1],), 1e4, dtype=t.dtype, device=t.device)
    v = buf[..., ::2]
    v.copy_(t)
    return v


def bstride0(t):
    """Batch stride 0 over a full-size storage: every image reads image 0 (the rest of the storage holds other values)."""
    buf = t.contiguous().clone()
    return buf.as_strided(t.shape, (0,) + tuple(buf.stride()[1:]))


def offset4(t):
    """A contiguous view that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 5, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ================================================================================================ conditions
def _x_form(form):
    def cell(live):
        same(live, live.canon, run(live, x=form(live.x)), f"x as {form.__name__}")
    return cell


def _go_form(form):
    def cell(live):
        go = form(live.go)
        want = live.canon if torch.equal(go, live.go) else run(live, go=go.contiguous().clone())
        same(live, want, run(live, go=go), f"incoming gradient as {form.__name__}")
    return cell


def ops_functions():
    """The autograd Functions of convkan_amd.ops."""
    from convkan_amd import ops
    return [v for v in vars(ops).values() if isinstance(v, type) and issubclass(v, torch.autograd.Function) and v is not torch.autograd.Function]


@contextlib.contextmanager
def watched(functions, returned):
    """Inside: every backward of `functions` appends (name, ctx.needs_input_grad, [which returned values are tensors]) to `returned`.  (The node
    calls `cls.backward` when it runs, so the class attribute is what to wrap; autograd itself drops a gradient nobody asked for, so `.grad`
    cannot show one.)"""
    saved = {}
    for cls in functions:
        orig = saved[cls] = cls.__dict__["backward"]

        def spy(ctx, *grads, _orig=orig.__func__, _name=cls.__name__):
            out = _orig(ctx, *grads)
            tup = out if isinstance(out, tuple) else (out,)
            returned.append((_name, tuple(ctx.needs_input_grad), [g is not None for g in tup]))
            return out
        cls.backward = staticmethod(spy)
    try:
        yield
    finally:
        for cls, orig in saved.items():
            cls.backward = orig


def needs_subsets(live):
    names = list(live.params)
    out = {"x": (set(), True)}
    for grp in ("conv", "base", "affine", "phase"):
        sel = {n for n in names if group_of(n) == grp}
        if sel:
            out[grp] = (sel, False)
    out["nothing"] = (set(), False)
    return out


def cell_needs(live):
    """Every subset: the gradients asked for equal the canonical ones, the others are None -- as `.grad` and as what each custom backward
    returned (`watched`) -- and nothing frozen gets a `.grad`."""
    canon, bitwise = live.canon, 0
    for tag, (need, need_x) in needs_subsets(live).items():
        xg = prepare(live, need, need_x)
        y = live.call(live.module, xg)
        state = state_of(live, y)
        if tag == "nothing":
            assert not y.requires_grad and y.grad_fn is None, f"{live.sid}: everything frozen, yet y requires grad"
        else:
            returned = []
            assert y.requires_grad, f"{live.sid} needs={tag}: y does not require grad"
            with watched(live.functions if live.functions is not None else ops_functions(), returned):
                y.backward(live.go)
            assert returned or not need_x, f"{live.sid} needs={tag}: no backward of the ops was seen"      # (a layer's own torch modules after the op may be all that asks)
            extra = [(name, i) for name, needs, has in returned for i, (nd, h) in enumerate(zip(needs, has)) if h and not nd]
            assert not extra, f"{live.sid} needs={tag}: a backward returned a tensor for inputs that asked for none: {extra}"
        got = collect(live, xg, y, state)
        part = Result(canon.y, canon.dx if need_x else None, {n: (g if n in need else None) for n, g in canon.dw.items()}, canon.state)
        has_bits = need_x or any(klass(live, n) == "bits" for n in need)
        same(live, part, got, f"needs={tag}", grads=has_bits)
        if not has_bits:                                    # only atomic-class gradients asked for: judged by their rule, None-ness exactly
            assert got.dx is None
            asked = [n for n, w in part.dw.items() if w is not None]
            assert [n for n, g in got.dw.items() if g is not None] == asked, f"{live.sid} needs={tag}: gradients of other parameters than {asked}"
            scalars = [n for n in asked if part.dw[n].numel() == 1]                 # judged together, as in `same`
            assert all(_close(got.dw[n], part.dw[n]) for n in asked if n not in scalars), f"{live.sid} needs={tag}: a gradient differs"
            assert not scalars or _close(torch.cat([got.dw[n].reshape(-1) for n in scalars]), torch.cat([part.dw[n].reshape(-1) for n in scalars])), \
                f"{live.sid} needs={tag}: the scalar slopes differ"
        bitwise += int(has_bits)
    assert bitwise, f"{live.sid}: no subset with a bitwise gradient"


def cell_grad_mode(live):
    """Forward under no_grad and under inference_mode (first on a subject of its own, whose caches are then made inside inference mode):
    the canonical forward bits and state; the training call after them is still the canonical one."""
    own = live.fresh()
    for ctx in (torch.inference_mode, torch.no_grad):
        xg = prepare(own, need_x=False)
        with ctx():
            y = own.call(own.module, xg)
            state = state_of(own, y)
        assert not y.requires_grad
        same(own, live.canon, collect(own, xg, y, state), ctx.__name__, grads=False)
    same(own, live.canon, run(own), "the training call after inference-mode and no-grad forwards")


def cell_retain(live):
    """backward(retain_graph=True) twice: the same bits both times; two backwards without zero_grad: g + g exactly."""
    xg = prepare(live)
    y = live.call(live.module, xg)
    state = state_of(live, y)
    y.backward(live.go, retain_graph=True)
    first = collect(live, xg, y, state)
    same(live, live.canon, first, "first backward of a retained graph")
    y.backward(live.go)
    same(live, live.canon, collect(live, xg, y, state), "two backwards without zero_grad (g + g)", factor=2.0)


def second_input(live):
    if live.subject["kind"] == "loss":
        return live.x.flip(1).contiguous()
    return (0.5 * live.x + 0.25).contiguous()


def cell_two_inputs(live):
    """One layer applied to two inputs in one graph: each y and dx as in a run of its own, the parameter gradients their sum (one fp32
    add).  State is not compared (a stateful subject has then run twice)."""
    xb = second_input(live)
    ra, rb = live.canon, run(live, x=xb)
    xa_g = prepare(live)
    xb_g = xb.detach().requires_grad_(True)
    ya, yb = live.call(live.module, xa_g), live.call(live.module, xb_g)
    torch.autograd.backward([ya, yb], [live.go, live.go])
    got_a = collect(live, xa_g, ya)
    got_b = Result(yb.detach().clone(), xb_g.grad.detach().clone(), got_a.dw, {})
    summed = {n: (None if g is None else g + rb.dw[n]) for n, g in ra.dw.items()}
    same(live, Result(ra.y, ra.dx, summed, {}), got_a, "first of two inputs in one graph", state=False)
    same(live, Result(rb.y, rb.dx, summed, {}), got_b, "second of two inputs in one graph", state=False)


def cell_checkpoint(live):
    from torch.utils.checkpoint import checkpoint
    call = live.call
    ck = copy.copy(live)
    ck.call = lambda m, t: checkpoint(lambda u: call(m, u), t, use_reentrant=False)
    ck.peek = False
    same(live, live.canon, run(ck), "torch.utils.checkpoint(use_reentrant=False)", state=live.subject["kind"] != "loss")


def step_names(live):
    """The parameters an in-place weight step touches: the conv and base weights; a subject without any, all its parameters."""
    names = [n for n in live.params if group_of(n) in ("conv", "base")]
    return names or list(live.params)


def _backward_or_raise(y, go):
    try:
        y.backward(go)
    except RuntimeError as e:
        assert INPLACE in str(e), f"a RuntimeError that is not torch's in-place check: {e}"
        return "raises"
    return "consistent"


def _pinned(live, cond, outcome):
    want = live.subject.get("stale", {}).get(cond) or STALE[cond].get(live.sid, STALE[cond]["*"])
    assert outcome == want, f"{live.sid} {cond}: the backward {outcome}, pinned as {want} (both satisfy the contract; the table states which)"


def cell_stale_x(live):
    """x.add_(1) after the forward."""
    own = live.fresh()
    xg = prepare(own, x=live.x.clone())
    y = own.call(own.module, xg)
    state = state_of(own, y)
    with torch.no_grad():
        xg.add_(1.0)
    outcome = _backward_or_raise(y, live.go)
    if outcome == "consistent":
        same(own, live.canon, collect(own, xg, y, state), "backward after x.add_(1): the gradient of the forward that ran")
    _pinned(live, "stale-x", outcome)
    same(own, live.canon, run(own), "the canonical call afterwards")


def cell_stale_w(live):
    """An in-place weight step after the forward, no second forward."""
    own = live.fresh()
    xg = prepare(own)
    y = own.call(own.module, xg)
    state = state_of(own, y)
    with torch.no_grad():
        for n in step_names(own):
            own.params[n].add_(0.01)
    outcome = _backward_or_raise(y, live.go)
    if outcome == "consistent":
        same(own, live.canon, collect(own, xg, y, state), "backward after a weight step: the gradient of the forward that ran")
    _pinned(live, "stale-w", outcome)
    with torch.no_grad():
        for n in step_names(own):
            own.params[n].copy_(live.params[n])
    same(own, live.canon, run(own), "the canonical call at the old weights afterwards")


def cell_stale_refwd(live):
    """Forward A, weight step, forward B of the same layer and shape, then backward of A: raises, or A's gradient -- never a mix; B's
    backward is that of a clean run at the new weights."""
    own = live.fresh()
    xg = prepare(own)
    ya = own.call(own.module, xg)
    state_a = state_of(own, ya)
    with torch.no_grad():
        for n in step_names(own):
            own.params[n].add_(0.01)
    clean = own.fresh()
    xb = live.x.detach().requires_grad_(True)
    yb = own.call(own.module, xb)
    outcome = _backward_or_raise(ya, live.go)
    if outcome == "consistent":
        same(own, live.canon, collect(own, xg, ya, state_a), "backward of the first graph after a step and a second forward", state=not live.subject.get("stateful"))
    _pinned(live, "stale-refwd", outcome)
    want_b = run(clean)
    for p in own.module.parameters():
        p.grad = None
    yb.backward(live.go)
    same(own, want_b, collect(own, xb, yb), "backward of the second graph vs a clean run at the new weights", state=False)


def cell_side_stream(live):
    s = torch.cuda.Stream(device=live.device)
    s.wait_stream(torch.cuda.current_stream(live.device))

    @contextlib.contextmanager
    def on_stream():
        with torch.cuda.stream(s):
            yield
        torch.cuda.current_stream(live.device).wait_stream(s)
    same(live, live.canon, run(live, ctx=on_stream), "forward and backward on a side stream")


def _refused(live, x, what, types, **call_kw):
    xg = prepare(live, x=x, need_x=x.is_floating_point())
    try:
        live.call(live.module, xg, **call_kw) if call_kw else live.call(live.module, xg)
    except types:
        no_grads(live, xg)
        return
    raise AssertionError(f"{live.sid}: {what} was not refused")


def cell_refuse_dtype(live):
    from convkan_amd._lib import KanConvError
    for dt in (torch.float64, torch.float16, torch.bfloat16):
        _refused(live, live.x.to(dt), f"x in {dt}", KanConvError)
    if live.subject["kind"] == "loss":
        _refused(live, live.x, "an int32 target", KanConvError, target=live.module.target.to(torch.int32))


def cell_refuse_cpu_weights(live):
    """x on the device, the parameters on the CPU: refused on the host (torch refuses first where a host op of the layer meets them)."""
    own = live.fresh()
    own.module = own.module.cpu()
    own.buffers0 = {n: b.cpu() for n, b in own.buffers0.items()}
    _refused(own, live.x, "parameters on the CPU", RuntimeError)


def _autocast():
    return torch.autocast("cuda", dtype=torch.bfloat16)


def cell_autocast_fp32(live):
    """Under autocast(bf16) an fp32 x gives the canonical bits: autocast does not cast a custom Function's inputs."""
    same(live, live.canon, run(live, ctx=_autocast), "fp32 x under autocast(bf16)")


def cell_autocast_upstream(live):
    """The bf16 output of an upstream autocast layer is refused."""
    from convkan_amd._lib import KanConvError
    ac = _autocast
    c = live.x.shape[1]
    up = {2: nn.Linear(c, c), 3: nn.Conv1d(c, c, 1), 4: nn.Conv2d(c, c, 1), 5: nn.Conv3d(c, c, 1)}[live.x.dim()].to(live.device)
    with ac():
        h = up(live.x)
        assert h.dtype == torch.bfloat16
        _refused(live, h.detach(), "the bf16 output of an upstream autocast layer", KanConvError)


def cell_norm_params(live):
    """ops.instance_norm / batch_norm with a strided gamma or beta: as with its contiguous clone; fp64 and CPU forms are refused."""
    from convkan_amd._lib import KanConvError
    m = live.module
    for which in ("gamma", "beta"):
        p = getattr(m, which).detach()
        for bad, what in ((p.double(), "fp64"), (p.cpu(), "on the CPU")):
            _refused(live, live.x, f"{which} {what}", KanConvError, **{which: bad})
        v = cols2(p).requires_grad_(True)
        assert not v.is_contiguous()
        xg = prepare(live)
        y = live.call(m, xg, **{which: v})
        state = state_of(live, y)
        y.backward(live.go)
        got = collect(live, xg, y, state)
        got.dw[which] = v.grad.detach().clone()
        same(live, live.canon, got, f"a strided {which}")


def cell_double_backward(live):
    """create_graph=True: the first-order gradients are the canonical bits, and differentiating them raises torch's once-differentiable
    error -- never a silent zero or None second-order term."""
    import pytest
    xg = prepare(live)
    y = live.call(live.module, xg)
    state = state_of(live, y)
    names = list(live.params)
    grads = torch.autograd.grad(y, [xg] + [live.params[n] for n in names], live.go, create_graph=True, allow_unused=True)
    live.sync()
    got = Result(y.detach().clone(), grads[0].detach().clone(), {n: (None if g is None else g.detach().clone()) for n, g in zip(names, grads[1:])}, state)
    if live.sid in ORACLE_JUDGED:
        same(live, live.canon, got, "forward under create_graph=True", grads=False)
        oracle_judge(live, got, "first-order gradients under create_graph=True")
    else:
        same(live, live.canon, got, "first-order gradients under create_graph=True")
    assert grads[0].requires_grad, f"{live.sid}: dx under create_graph=True carries no graph: a second-order term would silently be dropped"
    with pytest.raises(RuntimeError, match=ONCE):
        grads[0].sum().backward()


def cell_empty_batch(live):
    """B = 0 is refused on the host (kan_plan's non-positive dimension, the norm and wavelet ops' own check, the loss at B < 1)."""
    from convkan_amd._lib import KanConvError
    kw = {"target": live.module.target[:0]} if live.subject["kind"] == "loss" else {}
    _refused(live, live.x[:0], "an empty batch", EMPTY_RAISES.get(live.sid, KanConvError), **kw)
    same(live, live.canon, run(live), "the canonical call afterwards")


def refuse_on_cpu(subject):
    """x (and everything else) on the CPU: refused on the host, with no device needed; nothing reaches `.grad`."""
    from convkan_amd._lib import KanConvError
    m, x = build(subject)
    x.requires_grad_(True)
    try:
        m(x)
    except KanConvError:
        left = [n for n, p in m.named_parameters() if p.grad is not None] + (["x"] if x.grad is not None else [])
        assert not left, f"{subject['id']}: a refused call left gradients in {left}"
        return
    raise AssertionError(f"{subject['id']}: a CPU input was not refused")


# condition -> {variant: cell}.  `GPU_ONLY` variants need a device API (streams, autocast("cuda"), two devices).
CONDITIONS = {
    "1-input-layout": {"x-permuted": _x_form(permuted), "x-cols2": _x_form(cols2)},
    "2-gradient-layout": {"go-permuted": _go_form(permuted), "go-cols2": _go_form(cols2), "go-bstride0": _go_form(bstride0)},
    "3-offset": {"x-offset4": _x_form(offset4), "go-offset4": _go_form(offset4)},
    "4-needs": {"needs": cell_needs},
    "5-grad-mode": {"grad-mode": cell_grad_mode},
    "6-reuse": {"retain": cell_retain, "two-inputs": cell_two_inputs, "checkpoint": cell_checkpoint},
    "7-stale": {"stale-x": cell_stale_x, "stale-w": cell_stale_w, "stale-refwd": cell_stale_refwd},
    "8-side-stream": {"side-stream": cell_side_stream},
    "9-refusals": {"refuse-dtype": cell_refuse_dtype, "refuse-cpu-weights": cell_refuse_cpu_weights, "autocast-fp32": cell_autocast_fp32, "autocast-upstream": cell_autocast_upstream,
                   "norm-params": cell_norm_params},
    "10-double-backward": {"double-backward": cell_double_backward},
    "11-empty-batch": {"empty-batch": cell_empty_batch},
}
GPU_ONLY = {"side-stream", "refuse-cpu-weights", "autocast-fp32", "autocast-upstream"}
VARIANT = {v: (c, fn) for c, vs in CONDITIONS.items() for v, fn in vs.items()}

_LOSS = tuple(s["id"] for s in SUBJECTS if s["kind"] == "loss")
_NOT_NORMOP = tuple(s["id"] for s in SUBJECTS if s["kind"] != "normop")
# (variant, subject, reason): the pairs that make no sense.
EXCLUSIONS = (
    [(v, s, "the incoming gradient of the loss is a scalar: it has no layout") for v in ("go-permuted", "go-cols2", "go-bstride0") for s in _LOSS]
    + [("checkpoint", "kan-bn-train", "the forward runs twice, so the running statistics update twice, as torch's would"),
       ("checkpoint", "batch-norm", "the forward runs twice, so the running statistics update twice, as torch's would"),
       ("checkpoint", "kan8-pos8bd-bn", "the forward runs twice, so the running statistics update twice, as torch's would"),
       ("checkpoint", "xent-5x10-metrics", "the forward runs twice, so the counters add the batch twice"),
       ("checkpoint", "xent-257x100-metrics", "the forward runs twice, so the counters add the batch twice")]
    + [(v, s, "the loss has no parameters to step") for v in ("stale-w", "stale-refwd", "refuse-cpu-weights") for s in _LOSS]
    + [("autocast-fp32", s, "the layer's own nn.PReLU after the op is on autocast's lower-precision list: torch runs it in bf16") for s in ("kan-3d", "mlp-kan")]
    + [("norm-params", s, "gamma and beta are arguments of the public norm ops alone") for s in _NOT_NORMOP]
)

# Condition 11: who refuses B = 0 where it is not an op of ops.py.
EMPTY_RAISES = {"legendre-xn": IndexError}      # the layer's own min / max normalisation of x (torch.amin over an empty dim) comes before any op

# Condition 10: the subjects whose first-order gradients under create_graph=True are judged against the fp64 oracle, not bitwise.  Same
# launches of ops.py, another incoming gradient: the layer's own nn.SiLU after the norm (`_norm_act`) takes torch's differentiable
# backward formula under create_graph=True, whose last bit differs from its fused silu_backward.
ORACLE_JUDGED = ("relu-phases", "gram-coeffs", "legendre-xn")

# Condition 7: what the backward does -- "raises" torch's in-place error, or returns the "consistent" gradient of the forward that ran.
# By reading ops.py; "*" is the default.
STALE = {
    # every Function saves the x it was given (or a view of it); the 3-D shim gathers depth slices into a copy first
    "stale-x": {"*": "raises", "kan-3d": "consistent"},
    # the conv Functions save packed layouts, not the weights: a step the forward never sees leaves the saved layouts as they were.  The
    # phased stage saves its basis weights (views of the Parameters), the wavelet stage its weights, the norm op gamma
    "stale-w": {"*": "consistent", "relu-phases": "raises", "gram-coeffs": "raises", "wav": "raises", "instance-norm": "raises", "batch-norm": "raises"},
    # the cached layouts are re-packed in place by the second forward, with a version bump (`_pack`): the first graph raises.  Every
    # fresh() pack leaves the first graph its own layouts (the grouped layers, the one-channel band layer kan8-pos8bd-bn, the W_IOD heads, the MLP layer with its host-applied
    # activation and second input); the subjects that raise under stale-w raise here for the same reason.  The 3-D subject has one depth
    # tap: its weight slice is a contiguous view of the Parameter, so it takes the cached path
    "stale-refwd": {"*": "consistent", "kan-silu": "raises", "kan-silu-affine": "raises", "kan-bn-train": "raises", "kan-bn-eval": "raises",
                    "kan8-rowblk-pos8bw": "raises", "kan-3d": "raises", "relu-phases": "raises", "gram-coeffs": "raises", "wav": "raises", "instance-norm": "raises",
                    "batch-norm": "raises"},
}


def excluded(variant, sid):
    return any(v == variant and s == sid for v, s, _ in EXCLUSIONS)


def cells(gpu):
    """[(variant, subject id)] of the matrix: all of it on a device, the device-free variants otherwise."""
    return [(v, s["id"]) for v in VARIANT for s in SUBJECTS if not excluded(v, s["id"]) and (gpu or v not in GPU_ONLY)]


_LIVE = {}


def live_of(sid, device="cuda"):
    """The shared Live of a subject (its canonical Result is computed once)."""
    if (sid, device) not in _LIVE:
        m, x = build(SUBJECT[sid])
        call = None
        if SUBJECT[sid]["kind"] in ("normop", "loss"):
            call = lambda mod, t, **kw: mod(t, **kw)
        _LIVE[(sid, device)] = Live(SUBJECT[sid], m, x, device, call=call)
    return _LIVE[(sid, device)]

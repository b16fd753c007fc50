"""CPU half of the calling-condition matrix (tests/call_cells.py): the tables are consistent, every subject is the row of an existing
table it claims to be and still plans to the path it is there for, a CPU input is refused by every subject, and the judge can fail -- the
condition code of the GPU matrix, run over a toy pure-torch autograd.Function, rejects each planted defect and passes the correct version."""
import weakref

import pytest
import torch
import torch.nn as nn

import call_cells as CC
from call_cells import CONDITIONS, EXCLUSIONS, GPU_ONLY, SUBJECT, SUBJECTS, VARIANT


# ------------------------------------------------------------------------------------------------ the tables
def test_tables_are_consistent():
    ids = [s["id"] for s in SUBJECTS]
    assert len(set(ids)) == len(ids)
    variants = [v for vs in CONDITIONS.values() for v in vs]
    assert len(set(variants)) == len(variants) and len(CONDITIONS) == 11
    assert GPU_ONLY <= set(variants)
    for v, s, reason in EXCLUSIONS:
        assert v in VARIANT and s in SUBJECT and reason.strip(), (v, s, reason)
    assert len(set((v, s) for v, s, _ in EXCLUSIONS)) == len(EXCLUSIONS)
    for cond, vs in CONDITIONS.items():
        applied = {s for s in ids if any(not CC.excluded(v, s) for v in vs)}
        assert len(applied) >= 8, f"{cond} is applied to {len(applied)} subjects only"
    for cond, pins in CC.STALE.items():
        assert cond in VARIANT and set(pins) - {"*"} <= set(ids) and set(pins.values()) <= {"raises", "consistent"}
    assert set(CC.ORACLE_JUDGED) | set(CC.EMPTY_RAISES) <= {s["id"] for s in SUBJECTS if s["kind"] == "route"}
    assert len(CC.cells(True)) == len(variants) * len(ids) - len(EXCLUSIONS)


# ------------------------------------------------------------------------------------------------ the subjects are rows of existing tables
@pytest.mark.parametrize("sid", [s["id"] for s in SUBJECTS if s["kind"] == "route"])
def test_route_subject_is_its_row_and_plans_to_its_path(sid):
    from convkan_amd import _lib as L, ops
    from route_cells import ROUTE_CASES, case_structs, route_key, second_input
    s = SUBJECT[sid]
    case = CC.route_row(s)
    assert any(case is c for c in ROUTE_CASES)
    assert (case["B"], case["C"], case["O"], case["H"], case["G"]) == s["shape"] and case["W"] == case["H"]
    layer, x = CC.build(s)
    assert tuple(x.shape) == (case["B"], case["C"], case["H"], case["W"])
    g, b, p = case_structs(case, layer)
    assert route_key(g, b, p) == case["key"] == tuple(s["key"].split())
    spec = layer.conv_spec()
    cacheable = ops._cacheable(ops._plan_key(spec, x.shape, case["O"] // case["G"]))
    if sid.startswith("kan-"):                                   # subjects 1 and 2: one group, cached layouts, the fused tail
        assert spec.groups == 1 and cacheable and spec.has_base
        assert type(layer.layer_norm[0]) is (nn.BatchNorm2d if s.get("bn") else nn.InstanceNorm2d)
        assert layer.layer_norm[0].affine == bool(s.get("affine") or s.get("bn")) and layer.training == bool(s.get("training", True))
    elif sid == "cheby-grouped":
        assert spec.groups == 2 and not spec.has_base and spec.kind == L.BASIS_CHEBY and spec.n_basis == 5
    elif sid == "relu-phases":
        assert spec.kind == L.BASIS_RELU and spec.groups == 2 and hasattr(layer, "phase_low")
    elif sid == "gram-coeffs":
        assert spec.kind == L.BASIS_GRAM and spec.groups == 2 and hasattr(layer, "beta_weights")
    elif sid == "legendre-xn":
        assert second_input(b) and type(layer).__name__ == "LegendreKANConv2DLayer"
    else:
        raise AssertionError(sid)


@pytest.mark.parametrize("sid", [s["id"] for s in SUBJECTS if s["kind"] == "order"])
def test_order_subject_is_its_row_and_plans_to_its_path(sid):
    """The two subjects on the 8x8 tile orders: each is the row of order_cells.ORDER_CASES it names, the smallest row that has its orders, and its layer
    still plans to them -- so that its canonical call is the one tests/test_gpu_order_matrix.py judges against fp64."""
    from convkan_amd import ops
    from order_cells import ORDER_CASES, order_key, work
    from route_cells import case_structs
    s = SUBJECT[sid]
    case = CC.route_row(s)
    assert any(case is c for c in ORDER_CASES) and case["key"] == CC.order_row_key(s)
    assert (case["B"], case["C"], case["O"], case["H"], case["G"]) == s["shape"] and case["W"] == case["H"] == 8
    want = {"kan8-rowblk-pos8bw": lambda o: set(o) == {"ROWBLK8_FWD", "POS8_BWD_WEIGHT"}, "kan8-pos8bd-bn": lambda o: "POS8_BWD_DATA" in o}[sid]
    assert want(case["key"][1]) and work(case) == min(work(c) for c in ORDER_CASES if want(c["key"][1]))
    layer, x = CC.build(s)
    assert tuple(x.shape) == (case["B"], case["C"], 8, 8)
    g, b, p = case_structs(case, layer)
    assert order_key(g, b, p) == case["key"]
    spec = layer.conv_spec()
    # the halo layouts are kept between calls; the band layouts of the one-channel layer have pad rows to clear and are packed afresh on every call
    assert spec.groups == 1 and spec.has_base and ops._cacheable(ops._plan_key(spec, x.shape, case["O"])) == (sid == "kan8-rowblk-pos8bw")
    assert CC.STALE["stale-refwd"].get(sid, "consistent") == ("raises" if sid == "kan8-rowblk-pos8bw" else "consistent")
    assert type(layer.layer_norm[0]) is (nn.BatchNorm2d if s.get("bn") else nn.InstanceNorm2d) and layer.training == bool(s.get("training", True))
    if sid == "kan8-rowblk-pos8bw":                              # the weight gradient bypasses the plan's halo route; no dz_pm is ever built
        assert ops._row_blocks8_forward(g, p) and ops._pos8_bwd_weight(g, p) and not ops._pos8_bwd_data(g, p) and not p.dz_pm_wanted and p.pos8_bw_slabs == 1
    else:                                                        # dz_pm is built for bwd-data alone: not when x asks for no gradient
        assert ops._pos8_bwd_data(g, p) and not ops._pos8_bwd_weight(g, p) and not p.dz_pm_wanted


def test_fuzz_subjects_are_the_smallest_draws():
    for sid, draw, seeds in (("kan-1d", CC.fuzz_1d, range(0, 24, 4)), ("kan-3d", CC.fuzz_3d, range(0, 18, 7))):
        sizes = {seed: CC.fuzz_size(draw(seed)) for seed in seeds}
        assert SUBJECT[sid]["seed"] == min(sizes, key=lambda k: (sizes[k], k)), sizes
        layer, x = CC.build(SUBJECT[sid])
        c = draw(SUBJECT[sid]["seed"])
        assert type(layer).__name__ == ("KANConv1DLayer" if sid == "kan-1d" else "KANConv3DLayer")
        assert tuple(x.shape) == (c["B"], c["C"]) + c["dims"] and layer.groups == c["G"]


def test_wav_subject_is_the_smallest_row():
    rows = CC.wav_rows()
    assert SUBJECT["wav"]["row"] == min(rows, key=lambda r: (r[1], r[0]))[0]
    layer, x = CC.build(SUBJECT["wav"])
    assert type(layer).__name__ == "WavKANConv2DLayer" and x.dim() == 4


def test_head_and_mlp_subjects_are_their_fixtures():
    from convkan_amd import ops
    from heads_cases import load_head
    for sid, want in (("head-cheby", (4, 9, 130, 2)), ("head-lucas", (2, 300, 5, 3))):
        cfg = load_head(SUBJECT[sid]["name"])["cfg"]
        assert (cfg["B"], cfg["I"], cfg["O"], cfg["degree"]) == want
        layer, x = CC.build(SUBJECT[sid])
        spec = layer.conv_spec()
        assert spec.w_layout == ops.W_IOD and tuple(x.shape) == want[:2]
        plan = ops._plan_cached(*ops._plan_key(spec, (want[0], want[1], 1, 1), want[2]))[2]
        assert plan.fwd_splits == (9 if sid == "head-lucas" else 1)
    layer, x = CC.build(SUBJECT["mlp-kan"])
    spec = layer.conv_spec()
    assert tuple(x.shape)[1] == 7 and layer.base_weight.shape == (3, 7) and spec.has_base and spec.kernel == (1, 1) and spec.w_layout == 0


def test_norm_and_loss_subjects():
    from norm_cells import NORM_CASES, norm_key, route
    B, C, H, W = SUBJECT["instance-norm"]["shape"]
    assert (B, C, H, W) == (3, 5, 4, 6) == SUBJECT["batch-norm"]["shape"]
    plain = [c for c in NORM_CASES if c["pool"] is None]          # the kernel variant of the op's launch is a cell of the norm matrix (the slope is a runtime pointer)
    assert norm_key(route(False, B, C, H, W), False) in {c["fwd"] for c in plain}
    assert norm_key(route(True, B, C, H, W), True) in {c["bwd"] for c in plain}
    assert sorted((s["shape"], s["metrics"]) for s in SUBJECTS if s["kind"] == "loss") == [((5, 10), False), ((5, 10), True), ((257, 100), False),
                                                                                          ((257, 100), True)]


@pytest.mark.parametrize("sid", [s["id"] for s in SUBJECTS])
def test_cpu_input_is_refused_on_the_host(sid):
    """Condition 9, the part that needs no device: x (with everything else) on the CPU."""
    CC.refuse_on_cpu(SUBJECT[sid])


# ------------------------------------------------------------------------------------------------ the judge must be able to fail
DEFECTS = {
    "storage-x": {"x-permuted", "x-cols2"},                      # reads its input in storage order, ignoring strides
    "storage-go": {"go-permuted", "go-cols2", "go-bstride0"},    # reads the incoming gradient that way
    "grad-not-none": {"needs"},                                  # returns a tensor where needs_input_grad is False
    "stale-pack": {"stale-refwd"},                               # a second forward overwrites the packed weight without a version bump
    "silent-double": {"double-backward"},                        # its backward is silently differentiable to nothing
}
_PACKS = {}


def _raw(t):
    """`t` read as if it were contiguous: numel elements in storage order from its first element."""
    strides, n = [], 1
    for d in reversed(t.shape):
        strides.append(n)
        n *= d
    return torch.as_strided(t, t.shape, tuple(reversed(strides)), t.storage_offset())


def _toy_function(defect):
    from convkan_amd._lib import KanConvError
    from convkan_amd.ops import _once                             # once_differentiable as the ops apply it

    def packed_of(w):
        ent = _PACKS.get(id(w))
        if ent is None:
            with torch.inference_mode(False):
                ent = _PACKS[id(w)] = [w.detach().clone(), w._version]
            weakref.finalize(w, _PACKS.pop, id(w), None)
        elif ent[1] != w._version:
            if defect == "stale-pack":
                with torch.autograd._unsafe_preserve_version_counter(ent[0]):
                    ent[0].copy_(w.detach())
            else:
                ent[0].copy_(w.detach())                          # in place: bumps the version a graph that saved it will check
            ent[1] = w._version
        return ent[0]

    def forward(ctx, x, w, b):
        if x.dtype != torch.float32 or x.numel() == 0:
            raise KanConvError(f"x must be non-empty float32, got {x.dtype} {tuple(x.shape)}")
        xr = _raw(x) if defect == "storage-x" and not x.is_contiguous() else x.contiguous()
        packed = packed_of(w)
        ctx.save_for_backward(xr, packed)
        return xr * packed + b.view(1, -1, 1, 1)

    def backward(ctx, dy):
        xr, packed = ctx.saved_tensors
        g = _raw(dy) if defect == "storage-go" and not dy.is_contiguous() else dy.contiguous()
        if defect == "silent-double":
            g, xr, packed = g.detach(), xr.detach(), packed.detach()
        nx, nw, nb = ctx.needs_input_grad
        dw = (g * xr).sum((0, 2, 3)).view_as(packed) if nw else (torch.zeros_like(packed) if defect == "grad-not-none" else None)
        return (g * packed if nx else None), dw, (g.sum((0, 2, 3)) if nb else None)

    body = {"forward": staticmethod(forward), "backward": staticmethod(backward if defect == "silent-double" else _once(backward))}
    return type("Toy", (torch.autograd.Function,), body)


class _ToyLayer(nn.Module):
    def __init__(self, fn, C):
        super().__init__()
        gen = torch.Generator().manual_seed(3)
        self.fn = fn
        self.weight = nn.Parameter(torch.randn(C, 1, 1, generator=gen))                   # dim() >= 3: the bitwise class
        self.layer_norm_bias = nn.Parameter(torch.randn(C, generator=gen))                # the atomic class

    def forward(self, x):
        return self.fn.apply(x, self.weight, self.layer_norm_bias)


def _toy_live(defect):
    subject = dict(id="toy" + ("-" + defect if defect else ""), kind="toy", path="toy",
                   stale={"stale-x": "raises", "stale-w": "consistent", "stale-refwd": "raises"})
    x = torch.randn(3, 5, 4, 6, generator=torch.Generator().manual_seed(4))
    fn = _toy_function(defect)
    live = CC.Live(subject, _ToyLayer(fn, 5), x, "cpu")
    live.functions = [fn]
    return live


TOY_VARIANTS = [v for v in VARIANT if v not in GPU_ONLY and v != "norm-params"]


def _rejecting(defect):
    out = set()
    live = _toy_live(defect)
    for v in TOY_VARIANTS:
        try:
            VARIANT[v][1](live)
        except (AssertionError, pytest.fail.Exception) as e:
            out.add(v)
            print(f"[{defect}] {v}: {str(e)[:200]}")
    return out


def test_correct_toy_passes_every_condition():
    assert _rejecting(None) == set()


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_planted_defect_is_rejected(defect):
    assert _rejecting(defect) == DEFECTS[defect]

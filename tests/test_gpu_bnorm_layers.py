"""Layers built with norm_layer=BatchNorm run their norm on the BatchNorm kernels (csrc/kan_bnorm.hip), never on torch's batch norm.

Each layer is run for two steps (forward + backward, no optimizer) on the GPU with torch.nn.functional.batch_norm patched to raise, and
compared with the fp64 CPU oracle of the same layer (tests/helpers.oracle_forward: torch's conv, batch norm, PReLU, then F.max_pool2d
for pool=True) run for the same two steps: the output, dx, every parameter gradient, and after the second step the running buffers and
num_batches_tracked of every group.

Tolerance, per tensor: max(stated, 4 x the fp32 oracle's own error against fp64, measured live) -- helpers.check_vs_oracle's rule and
stated bounds (TOL_Y, TOL_DX, TOL_DW; 2e-5 for the vectors).  The running buffers are blends of the per-channel mean and variance of
the conv stage's output and inherit its bound, TOL_Y.  Conditioning is norm_cells': no upstream gradient on the PReLU kink, nor on a
near-tied pool window."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import convkan_amd as K
from helpers import TOL_DW, TOL_DX, TOL_Y, check_vs_oracle, oracle_forward, relerr
from norm_cells import conditioning

pytestmark = pytest.mark.gpu


def _cfg(kind, C, O, groups=1, **kw):
    return dict(kind=kind, C=C, O=O, k=3, s=1, p=1, d=1, groups=groups, **kw)


def _randomise_norm(layer, seed):
    """Affine parameters and running buffers away from their initial 1 / 0, as after some training."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in layer.layer_norm:
            if m.affine:
                m.weight.add_(0.3 * torch.randn(m.weight.shape, generator=g))
                m.bias.add_(0.3 * torch.randn(m.bias.shape, generator=g))
            if m.running_mean is not None:
                m.running_mean.add_(0.3 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.mul_(0.5 + torch.rand(m.running_var.shape, generator=g))


def _steps(run, layer, x, go, steps):
    """`steps` times zero_grad / forward / backward; returns (y, dx, {parameter gradients}, {buffers}) after the last."""
    for _ in range(steps):
        layer.zero_grad(set_to_none=True)
        xs = x.clone().requires_grad_(True)
        y = run(layer, xs)
        if go is None:
            return y.detach(), None, {}, {}
        y.backward(go.to(y.dtype).to(y.device))
    return (y.detach(), xs.grad, {n: p.grad for n, p in layer.named_parameters() if p.grad is not None},
            {n: b.detach().clone() for n, b in layer.named_buffers() if n.startswith("layer_norm.")})


def _oracle(cfg, layer, x, go, dtype, pool, steps):
    l2 = copy.deepcopy(layer).to(dtype)
    if hasattr(l2, "grid") and isinstance(l2.grid, torch.Tensor):
        l2.grid = l2.grid.to(dtype)

    def run(m, xs):
        y = oracle_forward(cfg, m, xs)
        return F.max_pool2d(y, 2, 2) if pool else y
    return _steps(run, l2, x.to(dtype), go, steps)


def _upstream(cfg, layer, x, pool):
    """The seeded upstream gradient, zero where norm_cells' conditioning says so (from the fp64 oracle alone)."""
    l2 = copy.deepcopy(layer).double()
    if hasattr(l2, "grid") and isinstance(l2.grid, torch.Tensor):
        l2.grid = l2.grid.double()
    pre = []
    with torch.no_grad():
        y = oracle_forward(cfg, l2, x.double(), pre)
        y = F.max_pool2d(y, 2, 2) if pool else y
        go = torch.randn(y.shape, generator=torch.Generator().manual_seed(99))
        if hasattr(layer, "prelus") and len(pre) == cfg["groups"]:
            norms = copy.deepcopy(layer.layer_norm).double()            # (a fresh copy: step 1's statistics)
            n = torch.cat([norms[g](z) for g, z in enumerate(pre)], 1)
            act = torch.cat([F.prelu(p, l2.prelus[g].weight) for g, p in enumerate(n.chunk(cfg["groups"], 1))], 1)
            go = go * (~conditioning(dict(pool=(2, 2) if pool else None), n, act)[0]).float()
    return go


def _check(monkeypatch, layer, cfg, x, pool=False, steps=2):
    go = _upstream(cfg, layer, x, pool)
    y64, dx64, dw64, buf64 = _oracle(cfg, layer, x, go, torch.float64, pool, steps)
    y32, dx32, dw32, buf32 = _oracle(cfg, layer, x, go, torch.float32, pool, steps)
    dev = copy.deepcopy(layer).cuda()

    def boom(*a, **k):
        raise AssertionError("the layer reached torch.nn.functional.batch_norm")
    with monkeypatch.context() as mp:
        mp.setattr(F, "batch_norm", boom)
        y, dx, dw, buf = _steps((lambda m, xs: m(xs, pool=True)) if pool else (lambda m, xs: m(xs)), dev, x.cuda(), go, steps)
        torch.cuda.synchronize()

    def judge(name, a, b32, b64, stated):
        err, noise = relerr(a, b64), relerr(b32, b64)
        return name, err, max(stated, 4.0 * noise), noise
    rows = [judge("y", y, y32, y64, TOL_Y), judge("dx", dx, dx32, dx64, TOL_DX)]
    assert set(dw) == set(dw64), set(dw) ^ set(dw64)
    slopes = [n for n in dw64 if dw64[n].numel() == 1]                    # per-group PReLU slopes: judged together (one scalar each)
    if slopes:
        cat = lambda d: torch.cat([d[n].reshape(-1).cpu() for n in slopes])
        rows.append(judge("prelus", cat(dw), cat(dw32), cat(dw64), 2e-5))
    rows += [judge(n, dw[n], dw32[n], dw64[n], TOL_DW if dw64[n].dim() >= 3 else 2e-5) for n in dw64 if n not in slopes]
    assert set(buf) == set(buf64), set(buf) ^ set(buf64)
    for n in buf64:
        if n.endswith("num_batches_tracked"):
            assert int(buf[n]) == int(buf64[n]) == (steps if layer.training else 0), (n, int(buf[n]), int(buf64[n]))
        else:
            rows.append(judge(n, buf[n], buf32[n], buf64[n], TOL_Y))
    print(f"[bnorm layer] {cfg} pool={pool} train={layer.training}: " + "; ".join(f"{n} {e:.1e} (tol {t:.1e})" for n, e, t, _ in rows))
    bad = [r for r in rows if not r[1] <= r[2]]
    assert not bad, f"{cfg}: (tensor, error, tolerance, fp32 oracle's own error) {bad}"


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("groups", [1, 2])
def test_bspline_batchnorm_tail(groups, train, pool, gpu_lib, monkeypatch):
    torch.manual_seed(10 + groups)
    C = 3 if groups == 1 else 4
    layer = K.KANConv2DLayer(C, 8, 3, padding=1, groups=groups, norm_layer=nn.BatchNorm2d).train(train)
    _randomise_norm(layer, 5)
    _check(monkeypatch, layer, _cfg("bspline", C, 8, groups), torch.randn(4, C, 8, 8), pool=pool)


def test_bspline_without_running_stats(gpu_lib, monkeypatch):
    """track_running_stats=False: batch statistics in eval mode too, no buffers at all."""
    torch.manual_seed(3)
    layer = K.KANConv2DLayer(3, 8, 3, padding=1, norm_layer=nn.BatchNorm2d, track_running_stats=False, affine=False).eval()
    assert not dict(layer.layer_norm.named_buffers())
    _check(monkeypatch, layer, _cfg("bspline", 3, 8), torch.randn(4, 3, 8, 8), pool=True)


@pytest.mark.parametrize("name", ["cheby", "rbf", "gram", "bspline1d", "bspline3d"])
def test_other_families_batchnorm(name, gpu_lib, monkeypatch):
    """ChebyKAN (no PReLU), FastKAN (the norm sits on the input of the RBFs), GRAM ("norm, then activation"), a 1-D and a 3-D layer."""
    torch.manual_seed(20)
    if name == "cheby":
        layer, cfg, x = K.ChebyKANConv2DLayer(3, 8, 3, padding=1, groups=1, norm_layer=nn.BatchNorm2d), _cfg("cheby", 3, 8, degree=3), torch.randn(4, 3, 8, 8)
    elif name == "rbf":
        layer, cfg, x = K.FastKANConv2DLayer(4, 8, 3, padding=1, groups=2, norm_layer=nn.BatchNorm2d), _cfg("rbf", 4, 8, 2, act="silu"), torch.randn(4, 4, 8, 8)
    elif name == "gram":
        layer, cfg, x = K.GRAMKANConv2DLayer(3, 8, kernel_size=3, padding=1, degree=2, norm_layer=nn.BatchNorm2d), _cfg("gram", 3, 8, degree=2), torch.randn(4, 3, 8, 8)
        with torch.no_grad():
            layer.beta_weights.normal_(0.0, 0.2)
    elif name == "bspline1d":
        layer, cfg, x = K.KANConv1DLayer(3, 8, 3, padding=1, norm_layer=nn.BatchNorm1d), _cfg("bspline", 3, 8, ndim=1), torch.randn(4, 3, 19)
    else:
        layer, cfg, x = K.KANConv3DLayer(2, 4, 3, padding=1, groups=2, norm_layer=nn.BatchNorm3d), _cfg("bspline", 2, 4, 2, ndim=3), torch.randn(3, 2, 3, 4, 5)
    _randomise_norm(layer, 6)
    _check(monkeypatch, layer.train(), cfg, x)


class _GroupNorm(nn.GroupNorm):
    def __init__(self, channels):
        super().__init__(2, channels)


@pytest.mark.parametrize("norm", ["momentum_none", "groupnorm"])
def test_other_norms_stay_on_torch(norm, gpu_lib):
    """momentum=None (the cumulative average) and any other norm class keep the caller's own module (test_bnorm_matrix.py: `_fusable_batchnorm`
    refuses them), and stay correct."""
    torch.manual_seed(4)
    if norm == "momentum_none":
        layer = K.KANConv2DLayer(3, 8, 3, padding=1, norm_layer=nn.BatchNorm2d, momentum=None)
    else:
        layer = K.KANConv2DLayer(3, 8, 3, padding=1, norm_layer=_GroupNorm)
    check_vs_oracle(layer, _cfg("bspline", 3, 8), torch.randn(4, 3, 8, 8))


def test_graphed_batchnorm_steps_equal_eager_steps_bitwise(gpu_lib):
    """Two KAN-VGG11 training steps (bs 4) with kan_norm_layer=BatchNorm2d under train.GraphedStep leave exactly the losses, weights and
    buffers (running statistics, num_batches_tracked) of two eager steps: the running-buffer updates and the counter's in-place add are
    recorded into the graph."""
    from convkan_amd.models import vggkan
    torch.manual_seed(7)
    base = vggkan(3, 10, arch="VGG11", kan_conv="KAN", dropout_linear=0.0, kan_norm_layer=nn.BatchNorm2d).cuda().train()
    assert all(type(m) is nn.BatchNorm2d for f in base.features if hasattr(f, "layer_norm") for m in f.layer_norm)
    start = copy.deepcopy(base.state_dict())
    g = torch.Generator(device="cuda").manual_seed(3)
    batches = [(torch.randn(4, 3, 32, 32, device="cuda", generator=g), torch.randint(0, 10, (4,), device="cuda", generator=g)) for _ in range(2)]
    out = {}
    for mode in ("eager", "graph"):
        model = copy.deepcopy(base)
        opt = K.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
        losses = []
        if mode == "eager":
            for d, t in batches:
                losses.append(float(K.train_step(model, d, t, opt)))
        else:
            step = K.GraphedStep(model, batches[0][0], batches[0][1])
            model.load_state_dict(start)                                 # the warm-up steps moved the running buffers
            for d, t in batches:
                losses.append(float(step(d, t)))
                opt.step()
        torch.cuda.synchronize()
        out[mode] = (losses, {n: t.detach().clone() for n, t in model.state_dict().items()})
    assert out["eager"][0] == out["graph"][0], (out["eager"][0], out["graph"][0])
    for n, a in out["eager"][1].items():
        assert torch.equal(a, out["graph"][1][n]), n
    tracked = [n for n in out["eager"][1] if n.endswith("num_batches_tracked")]
    assert tracked and all(int(out["graph"][1][n]) == 2 for n in tracked)
    assert any(not torch.equal(out["graph"][1][n], start[n]) for n in out["graph"][1] if n.endswith("running_mean"))

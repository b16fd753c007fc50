"""What the tests of the opt-in split-precision launches share (ops.py, section "opt-in split precision"): the stage they are built
around, the cases the library puts out of scope, spies on the three public entry points, and one KAN-VGG11 training step with its bit-for-bit comparison.
tests/test_split*.py use the host half on the CPU, tests/test_gpu_split*.py all of it on the GPU."""
import contextlib

import torch

ENTRY_POINTS = ("kan_conv_fwd_split", "kan_conv_bwd_data_split", "kan_conv_bwd_weight_split")

# what `kan_split_supported` refuses (tests/test_gpu_split.py::test_split_forward_scope_is_enforced): 4x4 planes, another spec, 64 outputs, odd batch on 8x8,
# GELU base branch -- as keyword arguments of `stage_spec` / `geom_basis`
OUT_OF_SCOPE = [dict(C_=16, O_=128, H=4), dict(C_=16, O_=128, H=8, nb=11), dict(C_=16, O_=64, H=8), dict(C_=16, O_=128, H=8, B=3),
                dict(C_=16, O_=128, H=8, act="gelu")]


def stage_spec(nb=8, act="silu", **over):
    """The ConvSpec of a 3x3 / stride 1 / pad 1 B-spline layer as the layers build it; `over`: ConvSpec fields to replace."""
    from convkan_amd import _lib as L
    from convkan_amd import ops
    table = tuple(float(v) for v in torch.linspace(-2.2, 2.2, nb + 4).tolist())
    kw = dict(kind=L.BASIS_BSPLINE, n_basis=nb, order=3, act={"silu": L.ACT_SILU, "gelu": L.ACT_GELU, "none": L.ACT_NONE}[act], p0=0.0, p1=0.0, table=table,
              kernel=(3, 3), stride=(1, 1), padding=(1, 1), dilation=(1, 1))
    kw.update(over)
    return ops.ConvSpec(**kw)


def geom_basis(C_, O_, H, B=2, nb=8, act="silu"):
    """(geom, basis) as the ops build them for the stage of `stage_spec` on a [B, C_, H, H] input with O_ outputs."""
    from convkan_amd import ops
    g, b, _ = ops._plan_cached(stage_spec(nb, act), B, C_, H, H, O_, C_, O_)
    return g, b


def split_layer(C_, O_, **kw):
    """(layer on the GPU, its spec, base weights, spline weights) of a KANConv2DLayer as models/kan_vgg.py builds it: SiLU base branch unless `kw` says otherwise."""
    import convkan_amd as K
    kw.setdefault("base_activation", torch.nn.SiLU)
    layer = K.KANConv2DLayer(C_, O_, 3, padding=1, **kw).cuda()
    return layer, layer.conv_spec(), layer.base_conv[0].weight.detach(), layer.spline_conv[0].weight.detach()


@contextlib.contextmanager
def spies():
    """Record the x shape of every call of the three module-level split entry points."""
    from convkan_amd import ops
    calls = {n: [] for n in ENTRY_POINTS}
    orig = {n: getattr(ops, n) for n in ENTRY_POINTS}

    def spy(name):
        return lambda *a, **k: (calls[name].append(tuple(a[1].shape)), orig[name](*a, **k))[1]
    for n in ENTRY_POINTS:
        setattr(ops, n, spy(n))
    try:
        yield calls
    finally:
        for n in ENTRY_POINTS:
            setattr(ops, n, orig[n])


def vgg_step(model, x, target, fwd_ctx=None, bwd_ctx=None):
    """(logits, gradients by name) of one cross-entropy step: forward and loss inside `fwd_ctx`; the backward there too, or inside `bwd_ctx` when given."""
    model.zero_grad(set_to_none=True)
    with fwd_ctx if fwd_ctx is not None else contextlib.nullcontext():
        y = model(x)
        loss = torch.nn.functional.cross_entropy(y, target)
        if bwd_ctx is None:
            loss.backward()
    if bwd_ctx is not None:
        with bwd_ctx:
            loss.backward()
    return y.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def same_but_slopes(g0, g1, names):
    """Bit-equal on every tensor of `names` with more than one element.  The scalar PReLU slopes are summed by float atomics across workgroups (their last
    bits differ between two runs of the EXACT step as well): judged together under the project's bound for these scalars, 2e-5 max-normalised.  Returns
    the slopes' distance (0.0 without slopes)."""
    from helpers import relerr
    slopes = [n for n in names if g0[n].numel() == 1]
    others = [n for n in names if g0[n].numel() > 1]
    assert others and all(torch.equal(g0[n], g1[n]) for n in others), [n for n in others if not torch.equal(g0[n], g1[n])]
    if not slopes:
        return 0.0
    e = relerr(torch.cat([g1[n].reshape(-1) for n in slopes]), torch.cat([g0[n].reshape(-1) for n in slopes]))
    assert e <= 2e-5, e
    return e

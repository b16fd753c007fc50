"""OPT-IN split-precision TRAINING forward (ops.split_precision_forward / split_precision_training, train_step / GraphedStep `split_precision=`; DESIGN.md
section 10): inside the context the conv stage of a layer in scope runs kan_conv_fwd_split with grad mode on, and hands its backward what an exact one needs.

Asserted: the bare stage equals the direct kan_conv_fwd_split call bit for bit, sits <= 1e-5 (max-normalised) from the exact stage and from the fp64 oracle's
pre-norm sum, and its backward is the exact backward bit for bit (A); whole layers with InstanceNorm / BatchNorm tails against the fp64 oracle under the
project's one rule (B); routing, no-grad equivalence with split_precision_inference, the decision at forward time and the composition of the three contexts on
KAN-VGG11 (C); stages out of scope untouched (D); cut weights that follow the optimizer (E) and a recorded step (F); runs of images deciding one by one, and the
cache entry dying with its weights.  Every run prints the measured errors.

Measured on an MI355X (max-normalised): bare stage vs fp64 5.9e-7 .. 3.8e-6 (the deepest, 256 -> 256 @ 8x8), the exact kernel 1.9 .. 3.2e-7; whole layers vs fp64: y 0.8 ..
2.2e-6, dx 2.6 .. 3.7e-7, weight gradients 2.2 .. 4.9e-7, slope gradient 0.2 .. 1.1e-6; KAN-VGG11 bs 8: logits 8.0e-6 from the exact step's, conv-weight gradients
1.5 .. 3.1e-4 (DESIGN.md section 10 has the table and the bs-256 step times)."""
import contextlib
import copy
import gc

import pytest
import torch

from helpers import check_vs_oracle, relerr
from split_cells import ENTRY_POINTS
from split_cells import same_but_slopes as _same_but_slopes
from split_cells import spies as _spies
from split_cells import split_layer as _layer
from split_cells import vgg_step as _vgg_step

pytestmark = pytest.mark.gpu

SILU = torch.nn.SiLU
BARE = [(8, 128, 2, 8), (128, 256, 4, 8), (256, 256, 2, 8), (16, 256, 2, 16), (64, 128, 3, 16)]       # C, O, B, plane (an odd batch is in scope on 16x16)
LAYERS = [(8, 128, 2, 8), (64, 256, 2, 8), (16, 256, 2, 16), (64, 128, 2, 16)]
IN_CONTEXT = [(8, 64, 16, 16), (8, 128, 8, 8), (8, 256, 8, 8)]        # x shapes of the KAN-VGG11 bs-8 layers the context takes, in forward order


def _bare(spec, x, dz, wb, ws, ctx):
    """z, dx, dw_base, dw_basis of ops.kan_conv, the forward inside `ctx`."""
    from convkan_amd import ops
    xg, wbg, wsg = x.clone().requires_grad_(True), wb.clone().requires_grad_(True), ws.clone().requires_grad_(True)
    with ctx:
        z = ops.kan_conv(spec, xg, None, [wbg], [wsg])
    z.backward(dz)
    return z.detach(), xg.grad, wbg.grad, wsg.grad


# ------------------------------------------------------------------------------------------ A: the bare stage
@pytest.mark.parametrize("C_,O_,B,PW", BARE)
def test_bare_stage_forward_is_the_split_launch_and_backward_the_exact_one(C_, O_, B, PW, gpu_lib):
    from convkan_amd import ops
    from oracle import kan_oracle as O
    torch.manual_seed(C_ + B)
    layer, spec, wb, ws = _layer(C_, O_)
    x = torch.randn(B, C_, PW, PW, device="cuda")
    dz = torch.randn(B, O_, PW, PW, device="cuda")
    with _spies() as calls:
        exact = _bare(spec, x, dz, wb, ws, contextlib.nullcontext())
        assert calls["kan_conv_fwd_split"] == []
        split = _bare(spec, x, dz, wb, ws, ops.split_precision_forward())
        assert calls == {"kan_conv_fwd_split": [tuple(x.shape)], "kan_conv_bwd_data_split": [], "kan_conv_bwd_weight_split": []}, calls
    direct = ops.kan_conv_fwd_split(spec, x, wb, ws)[0]
    torch.cuda.synchronize()
    assert torch.equal(split[0], direct)
    pre = []
    O.kan_conv2d(x.double().cpu(), [wb.double().cpu()], [ws.double().cpu()], [torch.tensor([0.25], dtype=torch.float64)],
                 knots=layer.grid.double().cpu(), spline_order=3, act=torch.nn.functional.silu, padding=1, pre_norm_out=pre)
    ref = pre[0]
    scale = float(ref.abs().max())
    e_split = float((split[0].double().cpu() - ref).abs().max()) / scale
    e_exact = float((exact[0].double().cpu() - ref).abs().max()) / scale
    e_pair = float((split[0] - exact[0]).abs().max()) / scale
    print(f"[split training fwd {C_}->{O_} @{PW}x{PW} B={B}] z vs fp64: split {e_split:.2e}  exact kernel {e_exact:.2e};  split vs exact {e_pair:.2e}")
    assert e_split <= 1e-5 and e_pair <= 1e-5, (e_split, e_exact, e_pair)
    # a conv stage's backward reads x, W and dz only, and the launches are the exact ones
    for name, a, b in zip(("dx", "dw_base", "dw_basis"), split[1:], exact[1:]):
        assert torch.equal(a, b), (name, relerr(a, b))


# ------------------------------------------------------------------------------------------ B: whole layers against the fp64 oracle
# The largest condition number of the scalar slope gradient a draw may have.  From the reference and the number formats alone: a forward error of delta
# (max-normalised; the split forward's recorded 2.6e-6 at these depths, test_gpu_split.py) lands on each of the N ~ B O H W / 2 = 2^13 .. 2^16 terms with a
# random sign, so the sum moves by about kappa * delta * (max |z| / rms |z| ~ 4) / sqrt(N) = kappa * 4e-8 .. 1.2e-7 of its value; under kappa = 150 that stays
# below the 2e-5 bound of helpers.check_vs_oracle for these scalars.  Computed on the fp64 oracle only -- nothing the kernels return enters the choice.
KAPPA_MAX = 150.0


def _slope_condition(layer, cfg, x):
    """sum |dy n| / |sum dy n| over the outputs with n < 0 (n: the normalised pre-activation), with check_vs_oracle's own upstream gradient, in fp64."""
    from helpers import oracle_run
    y0, _, _, pre = oracle_run(cfg, layer, x, None, torch.float64)
    go = torch.randn(y0.shape, generator=torch.Generator().manual_seed(99)).double()
    with torch.no_grad():
        n = copy.deepcopy(layer.layer_norm).double()[0](pre[0].detach())
    terms = (go * (n.abs() > 1e-4))[n < 0] * n[n < 0]
    return float(terms.abs().sum() / terms.sum().abs())


@pytest.mark.parametrize("norm", ["in", "bn"])
@pytest.mark.parametrize("C_,O_,B,PW", LAYERS)
def test_layer_inside_the_context_vs_fp64_oracle(C_, O_, B, PW, norm, gpu_lib):
    """y, dx and every parameter gradient under check_vs_oracle's rule, unchanged.  The draw (weights and x) is the first of the seeds C + plane, + 1, ... whose
    PReLU slope gradient is well conditioned ON THE fp64 ORACLE (`_slope_condition` <= KAPPA_MAX): that gradient is ONE scalar, a signed sum over ~B O H W / 2
    outputs, and any forward error reaches it multiplied by kappa.  Measured on an MI355X at the ill-conditioned draws this skips -- 16 -> 256 @ 16x16,
    BatchNorm, seed 32, kappa 6411: slope gradient 3.4e-5 against the 2e-5 bound (y 1.2e-6, every other tensor <= 5e-7); the EXACT path at 64 -> 128 @ 16x16,
    seed 80, kappa 7920: 1.6e-5 -- the distance follows kappa (about 5e-9 kappa on both paths), not the path."""
    import convkan_amd as K
    from convkan_amd import ops
    kw = dict(norm_layer=torch.nn.BatchNorm2d, affine=True) if norm == "bn" else {}
    cfg = dict(kind="bspline", groups=1, k=3, s=1, p=1, d=1, act="silu")
    for seed in range(C_ + PW, C_ + PW + 32):
        torch.manual_seed(seed)
        layer = K.KANConv2DLayer(C_, O_, 3, padding=1, base_activation=SILU, **kw)    # on the host: check_vs_oracle runs the oracle first, then moves it
        x = torch.randn(B, C_, PW, PW)
        kappa = _slope_condition(layer, cfg, x)
        if kappa <= KAPPA_MAX:
            break
    else:
        pytest.fail(f"no draw with a slope-gradient condition number <= {KAPPA_MAX} in 32 seeds")
    print(f"[split training fwd layer {norm} {C_}->{O_} @{PW}x{PW} B={B}] seed {seed}: slope-gradient condition number {kappa:.0f}")
    with _spies() as calls, ops.split_precision_forward():
        errs = check_vs_oracle(layer, cfg, x, tag=f"split training fwd {norm} {C_}->{O_} @{PW}x{PW} B={B}", fallback=False)
    print(f"[split training fwd layer {norm} {C_}->{O_} @{PW}x{PW} B={B}] (error, tolerance, fp32 oracle's own) " +
          "  ".join(f"{k} {v[0]:.1e}/{v[1]:.1e}/{v[2]:.1e}" for k, v in errs.items()))
    assert calls["kan_conv_fwd_split"] == [(B, C_, PW, PW)], calls


# ------------------------------------------------------------------------------------------ C: KAN-VGG11
def test_contexts_on_kan_vgg11(gpu_lib):
    """One training step of KAN-VGG11 (bs 8) inside ops.split_precision_forward() runs the split forward for exactly the layers of IN_CONTEXT and no split
    backward; its logits are those of split_precision_inference under no_grad bit for bit, within 1e-4 of the exact step's (SURVEY 8(c)'s model tolerance);
    the decision is the forward's; split_precision_training() is the three contexts nested; outside, the step is the exact one.  The conv-weight gradient
    distances from the exact step are printed, not bounded: this model's gradients answer 1e-6 activation noise with up to 1e-2 (VERDICT weak #1), and the
    backward itself is pinned by the bare-stage and layer tests above."""
    from convkan_amd import ops
    from convkan_amd.models import vggkan
    torch.manual_seed(1)
    m = vggkan(3, 10, arch="VGG11", kan_conv="KAN", dropout_linear=0.0).cuda().train()
    x = torch.randn(8, 3, 32, 32, device="cuda")
    t = torch.randint(0, 10, (8,), device="cuda")
    fwd, bwd_x, bwd_w = ENTRY_POINTS
    with _spies() as calls:
        y0, g0 = _vgg_step(m, x, t)
        assert all(c == [] for c in calls.values()), calls
        # routing
        y1, g1 = _vgg_step(m, x, t, ops.split_precision_forward())
        assert calls[fwd] == IN_CONTEXT and calls[bwd_x] == [] and calls[bwd_w] == [], calls
        # logits
        with torch.no_grad(), ops.split_precision_inference():
            y_inf = m(x)
        assert torch.equal(y1, y_inf)
        err = relerr(y1, y0)
        print(f"[split training fwd KAN-VGG11 bs 8] logits vs the exact step: {err:.2e}")
        assert 0.0 < err <= 1e-4, err
        # gradients
        assert all(bool(torch.isfinite(g).all()) for g in g1.values()) and not all(torch.equal(g0[n], g1[n]) for n in g0)
        convw = [n for n in g0 if g0[n].dim() == 4]
        print("[split training fwd KAN-VGG11 bs 8] conv-weight gradient distance from the exact step (max-normalised, forward split only): " +
              "  ".join(f"{n} {relerr(g1[n], g0[n]):.1e}" for n in convw))
        # decided at forward time: a backward run outside the context is the same backward
        y2, g2 = _vgg_step(m, x, t, ops.split_precision_forward(), contextlib.nullcontext())
        assert torch.equal(y1, y2)
        _same_but_slopes(g1, g2, list(g1))
        # composition: split_precision_training() is the three contexts nested by hand, 3 launches of each entry point
        for c in calls.values():
            c.clear()
        y3, g3 = _vgg_step(m, x, t, ops.split_precision_training())
        assert calls[fwd] == IN_CONTEXT and calls[bwd_x] == IN_CONTEXT[::-1] and calls[bwd_w] == IN_CONTEXT[::-1], calls
        with ops.split_precision_forward():
            with ops.split_precision_backward_data():
                y4, g4 = _vgg_step(m, x, t, ops.split_precision_backward_weight())
        assert all(len(c) == 2 * len(IN_CONTEXT) for c in calls.values()), calls
        assert torch.equal(y3, y4) and torch.equal(y3, y1)
        _same_but_slopes(g3, g4, list(g3))
        assert any(not torch.equal(g3[n], g1[n]) for n in g1)              # and the backward did go split as well
        print("[split training KAN-VGG11 bs 8] conv-weight gradient distance from the exact step (max-normalised, all three launches split): " +
              "  ".join(f"{n} {relerr(g3[n], g0[n]):.1e}" for n in convw))
        # outside any context: the exact step
        n_calls = {k: len(c) for k, c in calls.items()}
        y5, g5 = _vgg_step(m, x, t)
        assert {k: len(c) for k, c in calls.items()} == n_calls and torch.equal(y0, y5)
        _same_but_slopes(g0, g5, list(g0))


# ------------------------------------------------------------------------------------------ D: out of scope inside the context
def _out_of_scope():
    import convkan_amd as K
    return [("4x4 planes", K.KANConv2DLayer(16, 128, 3, padding=1, base_activation=SILU), (2, 16, 4, 4)),
            ("grid_size 8", K.KANConv2DLayer(16, 128, 3, padding=1, grid_size=8, base_activation=SILU), (2, 16, 8, 8)),
            ("64 outputs", K.KANConv2DLayer(16, 64, 3, padding=1, base_activation=SILU), (2, 16, 8, 8)),
            ("odd batch on 8x8", K.KANConv2DLayer(16, 128, 3, padding=1, base_activation=SILU), (3, 16, 8, 8)),
            ("GELU base", K.KANConv2DLayer(16, 128, 3, padding=1), (2, 16, 8, 8))]


@pytest.mark.parametrize("case", range(5), ids=["4x4", "grid8", "O64", "odd_batch_8x8", "gelu"])
def test_out_of_scope_stages_are_untouched(case, gpu_lib):
    """The bare stage and the whole layer, forward and backward, inside split_precision_training(): the same bits as outside, no split launch."""
    from convkan_amd import ops
    torch.manual_seed(case)
    _, layer, shape = _out_of_scope()[case]
    layer = layer.cuda().train()
    spec, wb, ws = layer.conv_spec(), layer.base_conv[0].weight.detach(), layer.spline_conv[0].weight.detach()
    x = torch.randn(*shape, device="cuda")
    dz = torch.randn(shape[0], wb.shape[0], shape[2], shape[3], device="cuda")

    def whole(ctx):
        layer.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        with ctx:
            y = layer(xg)
            y.backward(dz)
        return y.detach(), {"dx": xg.grad, **{n: p.grad.clone() for n, p in layer.named_parameters()}}
    with _spies() as calls:
        outside, inside = _bare(spec, x, dz, wb, ws, contextlib.nullcontext()), _bare(spec, x, dz, wb, ws, ops.split_precision_training())
        for name, a, b in zip(("z", "dx", "dw_base", "dw_basis"), inside, outside):
            assert torch.equal(a, b), name
        (y0, g0), (y1, g1) = whole(contextlib.nullcontext()), whole(ops.split_precision_training())
        assert torch.equal(y0, y1)
        _same_but_slopes(g0, g1, list(g0))
        assert all(c == [] for c in calls.values()), calls


# ------------------------------------------------------------------------------------------ E: weights changed between steps
def test_cut_weights_follow_the_optimizer_and_train_step_is_the_context(gpu_lib):
    import convkan_amd as K
    from convkan_amd import ops
    torch.manual_seed(11)
    base = torch.nn.Sequential(_layer(16, 128)[0]).train()
    x = torch.randn(4, 16, 8, 8, device="cuda").requires_grad_(True)      # (an input gradient to compute: all three launches run)
    target = torch.randn(4, 128, 8, 8, device="cuda")
    mse = torch.nn.MSELoss()
    model, by_hand = copy.deepcopy(base), copy.deepcopy(base)
    opt, opt_h = (K.FusedAdamW(m.parameters(), lr=1e-2, weight_decay=1e-4) for m in (model, by_hand))
    with _spies() as calls:
        loss = K.train_step(model, x, target, opt, mse, split_precision=True)
        assert all(c == [tuple(x.shape)] for c in calls.values()), calls
        opt_h.zero_grad()                                                 # the same step written with the context by hand
        with ops.split_precision_training():
            loss_h = mse(by_hand(x), target)
            loss_h.backward()
        opt_h.step()
        torch.cuda.synchronize()
        assert torch.equal(loss, loss_h.detach())
        p, ph = dict(model.named_parameters()), dict(by_hand.named_parameters())
        _same_but_slopes({n: v.detach() for n, v in p.items()}, {n: v.detach() for n, v in ph.items()}, list(p))
        assert any(not torch.equal(v.detach(), dict(base.named_parameters())[n].detach()) for n, v in p.items())
        # after the optimizer step the context multiplies the weights as they are now
        layer = model[0]
        spec, wb, ws = layer.conv_spec(), layer.base_conv[0].weight, layer.spline_conv[0].weight
        with torch.no_grad(), ops.split_precision_forward():
            z = ops.kan_conv(spec, x, None, [wb], [ws])
        fresh = ops.kan_conv_fwd_split(spec, x, wb.detach().clone(), ws.detach().clone())[0]
        stale = ops.kan_conv_fwd_split(spec, x, base[0].base_conv[0].weight.detach(), base[0].spline_conv[0].weight.detach())[0]
        assert torch.equal(z, fresh) and not torch.equal(z, stale)
        for c in calls.values():
            c.clear()
        loss2 = K.train_step(model, x, target, opt, mse, split_precision=True)
        assert all(c == [tuple(x.shape)] for c in calls.values()), calls
        with torch.no_grad(), ops.split_precision_forward():
            z2 = ops.kan_conv(spec, x, None, [wb], [ws])
        assert torch.equal(z2, ops.kan_conv_fwd_split(spec, x, wb.detach().clone(), ws.detach().clone())[0]) and not torch.equal(z2, z)
        assert bool(torch.isfinite(loss2)) and float(loss2) != float(loss)
    assert ops._SPLIT == ops.SplitMode()


# ------------------------------------------------------------------------------------------ F: a recorded step
def test_graphed_steps_with_split_precision_equal_eager_steps_bitwise(gpu_lib):
    """A GraphedStep(..., split_precision=True), FusedAdamW outside the graph, two batches: losses and weights equal two eager steps inside
    split_precision_training() -- the forward's weight cut is recorded (ops.always_pack) and re-run at every replay on the weights the optimizer wrote, into
    the address it was recorded with -- and differ from two exact steps."""
    import convkan_amd as K
    from convkan_amd import ops
    from convkan_amd.models import vggkan
    torch.manual_seed(7)
    base = vggkan(3, 10, arch="VGG11", kan_conv="KAN", dropout_linear=0.0).cuda().train()
    g = torch.Generator(device="cuda").manual_seed(3)
    batches = [(torch.randn(8, 3, 32, 32, device="cuda", generator=g), torch.randint(0, 10, (8,), device="cuda", generator=g)) for _ in range(2)]
    out = {}
    for mode in ("eager", "graph", "exact"):
        model = copy.deepcopy(base)
        opt = K.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
        losses = []
        if mode == "eager":
            with ops.split_precision_training():
                for d, t in batches:
                    losses.append(float(K.train_step(model, d, t, opt)))
        elif mode == "graph":
            step = K.GraphedStep(model, batches[0][0], batches[0][1], split_precision=True)
            assert ops._SPLIT == ops.SplitMode()
            for d, t in batches:
                losses.append(float(step(d, t)))
                opt.step()
        else:
            for d, t in batches:
                losses.append(float(K.train_step(model, d, t, opt)))
        torch.cuda.synchronize()
        out[mode] = (losses, {n: p.detach().clone() for n, p in model.named_parameters()})
    assert out["eager"][0] == out["graph"][0], (out["eager"][0], out["graph"][0])
    for n, a in out["eager"][1].items():
        assert torch.equal(a, out["graph"][1][n]), n
    assert out["exact"][0] != out["eager"][0]
    assert any(not torch.equal(a, out["exact"][1][n]) for n, a in out["eager"][1].items())


# ------------------------------------------------------------------------------------------ runs of images, the cache
def test_runs_of_images_decide_one_by_one(gpu_lib, monkeypatch):
    """A batch cut into runs of whole images (here by a lowered launch limit): 3 images on 8x8 planes are out of scope as one launch; cut into 2 + 1, the
    even run takes the split forward and the odd one the exact one."""
    from convkan_amd import ops
    torch.manual_seed(2)
    _, spec, wb, ws = _layer(16, 128)
    x = torch.randn(3, 16, 8, 8, device="cuda")
    monkeypatch.setattr(ops, "MAX_TENSOR_BYTES", 2 * 4 * 128 * 64)        # two images' outputs
    with _spies() as calls, torch.no_grad():
        exact = ops.kan_conv(spec, x, None, [wb], [ws])
        with ops.split_precision_forward():
            z = ops.kan_conv(spec, x, None, [wb], [ws])
        assert calls["kan_conv_fwd_split"] == [(2, 16, 8, 8)], calls
    assert torch.equal(z[:2], ops.kan_conv_fwd_split(spec, x[:2].contiguous(), wb, ws)[0]) and not torch.equal(z[:2], exact[:2])
    assert torch.equal(z[2:], exact[2:])


def test_forward_cut_weight_cache_entry_dies_with_its_weights(gpu_lib):
    """The forward's cut-weight cache is keyed by weight addresses and version stamps.  A later model's weights can land on a dead model's addresses with equal
    stamps (fresh Parameters: version 0), and a step would then multiply the dead model's cut weights: the entry must go when its weights do -- on the
    training path and on the inference path, which share the cache."""
    from convkan_amd import ops
    for ctx in (ops.split_precision_forward, ops.split_precision_inference):
        layer = _layer(16, 128)[0].eval()
        x = torch.randn(2, 16, 8, 8, device="cuda")
        with torch.no_grad(), ctx():
            layer(x)
        key = (layer.base_conv[0].weight.data_ptr(), layer.spline_conv[0].weight.data_ptr(), x.device.index)
        assert key in ops._CUT_FWD.entries
        del layer
        gc.collect()
        assert key not in ops._CUT_FWD.entries

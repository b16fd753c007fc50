"""OPT-IN split-precision weight gradient (kan_conv_bwd_weight_split, ops.split_precision_backward_weight / split_precision_backward).

The expanded plane values (the exact kernels' own) and dz are cut into three bf16 pieces, six bf16 MFMA products per 16-deep block are accumulated in fp32,
images are the inner depth index, and depth-split partial sums are added in a fixed order.  Asserted per shape and for BOTH gradient tensors: split vs the
fp64 oracle <= max(TOL_DW, 4 x the fp32 oracle's own error) -- the project's one rule -- and split vs the exact HIP kernels <= TOL_DW; bit-identical repeats;
a derived 2^-21 bound on inputs that isolate every one of the six products; that nothing outside the two gradients is written (guards around the workspace
too); and, on KAN-VGG11, that the context changes the weight gradients of the layers in scope and nothing else, eagerly, under GraphedStep and through
registered gradient sinks.  Every run prints the measured errors.

Measured on an MI355X over SHAPES + MULTI_UNIT (max-normalised against fp64, dw_base / dw_basis): split 2.4e-7 .. 8.0e-7 / 2.2e-7 .. 6.8e-7, the exact kernels
1.7e-7 .. 6.2e-7 / 1.5e-7 .. 3.7e-7, the fp32 CPU oracle 2.7e-7 .. 4.4e-6 / 2.4e-7 .. 1.3e-6; split against exact 2.8e-7 .. 1.0e-6 / 2.0e-7 .. 7.6e-7 (the largest of each on
256 -> 256 @ 8x8, B 24; the table per shape: DESIGN.md section 10).  Every product: 3.8e-8 .. 8.7e-8
against the 2^-21 = 4.8e-7 bound.  KAN-VGG11, bs 8: the six weight gradients 3.5e-7 .. 5.9e-7 from the exact step's."""
import copy
import ctypes as C
import weakref

import pytest
import torch

from helpers import TOL_DW, relerr
from split_cells import same_but_slopes as _same_but_slopes
from split_cells import spies
from split_cells import split_layer as _layer
from split_cells import vgg_step as _vgg_step

pytestmark = pytest.mark.gpu

# the last two: several depth units, an odd number of image pairs, batch tails that fill neither an 8- nor a 16-image group
SHAPES = [(8, 128, 2, 8), (16, 128, 4, 8), (64, 256, 2, 8), (256, 256, 2, 8), (8, 128, 1, 16), (24, 128, 3, 16), (64, 128, 2, 16), (8, 128, 34, 8), (8, 128, 9, 16)]
# The depth units of a (channel, output tile) are dealt to KS = min(32, ceil(512 / (C O / 128)), units) workgroups, so every shape above runs ONE unit per
# workgroup.  These make a workgroup run several -- the steady state of the batch-256 launches: the x values fetched one unit ahead, the next unit's first dz
# block copied during the last block of this one, dz buffer 1 reused as expansion scratch, the halo tile rewritten between units.
#   (8, 128, 264, 8)    33 units on KS = 32: one run of two octets
#   (64, 256, 34, 8)    5 units on KS = 4, the last octet a tail of two images
#   (256, 256, 24, 8)   3 units on KS = 1: one workgroup runs them all, as at 256 -> 256, batch 256
#   (8, 128, 72, 16)    36 units on KS = 32: runs of two quarter planes, some inside an image octet, some across two
#   (64, 256, 10, 16)   8 units on KS = 4: upper and lower half of an octet (the row offset moves, the octet stays)
MULTI_UNIT = [(8, 128, 264, 8), (64, 256, 34, 8), (256, 256, 24, 8), (8, 128, 72, 16), (64, 256, 10, 16)]
IN_CONTEXT = [(8, 256, 8, 8), (8, 128, 8, 8), (8, 64, 16, 16)]        # x shapes of the KAN-VGG11 bs-8 layers the context takes, in backward order


def _exact_dw(spec, x, dz, wb, ws):
    from convkan_amd import ops
    wbg, wsg = wb.clone().requires_grad_(True), ws.clone().requires_grad_(True)
    ops.kan_conv(spec, x, None, [wbg], [wsg]).backward(dz)
    return wbg.grad, wsg.grad


def test_multi_unit_shapes_do_run_several_units_per_workgroup():
    """The premise of MULTI_UNIT, restated from the header's KS rule (tests/test_split_bwd_weight.py holds the library to it)."""
    for shapes, several in ((SHAPES, False), (MULTI_UNIT, True)):
        for C_, O_, B, PW in shapes:
            units = -(-B // 8) * (1 if PW == 8 else 4)
            ks = min(32, -(-512 // (C_ * (O_ // 128))), units)
            assert (units > ks) == several, (C_, O_, B, PW, units, ks)


@pytest.mark.parametrize("C_,O_,B,PW", SHAPES + MULTI_UNIT)
def test_split_bwd_weight_vs_fp64_oracle_and_exact_kernel(C_, O_, B, PW, gpu_lib):
    from convkan_amd import ops
    from oracle import kan_oracle as O
    torch.manual_seed(C_ + B)
    layer, spec, wb, ws = _layer(C_, O_)
    knots = layer.grid.detach().float().cpu().reshape(-1)
    x = 1.5 * torch.randn(B, C_, PW, PW)
    flat = x.view(-1)
    plant = torch.cat([knots, torch.tensor([-2.2000002, 2.2000002, -2.5, 2.5, -7.0, 7.0, 0.0])])      # exact knots, both sides of the range, far outside
    flat[torch.randperm(flat.numel())[:plant.numel()]] = plant
    x = x.cuda()
    dz = torch.randn(B, O_, PW, PW, device="cuda")
    split = ops.kan_conv_bwd_weight_split(spec, x, dz)
    again = ops.kan_conv_bwd_weight_split(spec, x, dz)
    exact = _exact_dw(spec, x, dz, wb, ws)
    torch.cuda.synchronize()
    ref = {}
    for dt in (torch.float64, torch.float32):
        wbo, wso = wb.to(dt).cpu().requires_grad_(True), ws.to(dt).cpu().requires_grad_(True)
        pre = []
        O.kan_conv2d(x.to(dt).cpu(), [wbo], [wso], [torch.tensor([0.25], dtype=dt)], knots=layer.grid.to(dt).cpu(), spline_order=3,
                     act=torch.nn.functional.silu, padding=1, pre_norm_out=pre)
        pre[0].backward(dz.to(dt).cpu())
        ref[dt] = (wbo.grad, wso.grad)
    for i, name in enumerate(("dw_base", "dw_basis")):
        assert split[i].shape == exact[i].shape == ref[torch.float64][i].shape
        noise = relerr(ref[torch.float32][i], ref[torch.float64][i])
        e_split, e_exact, e_pair = relerr(split[i], ref[torch.float64][i]), relerr(exact[i], ref[torch.float64][i]), relerr(split[i], exact[i])
        print(f"[split bwd-weight {C_}->{O_} @{PW}x{PW} B={B}] {name} vs fp64: split {e_split:.2e}  exact kernel {e_exact:.2e}  fp32 oracle {noise:.2e};  split vs exact {e_pair:.2e}")
        assert torch.isfinite(split[i]).all()
        assert torch.equal(split[i], again[i]), name
        assert e_split <= max(TOL_DW, 4.0 * noise), (name, e_split, e_exact, noise)
        assert e_pair <= TOL_DW, (name, e_pair, e_split, e_exact)


@pytest.mark.parametrize("PW,B", [(8, 2), (16, 1)])
def test_every_product_is_present(PW, B, gpu_lib):
    """v = 1 + 2^-9 + 2^-18 cuts into hi 1, mid 2^-9, lo 2^-18.  One dz element = v, all others 0: every dW entry is a single product v * E, E the plane value
    the tap reaches (x = 1.5 randn: E has all three pieces).  E comes exactly from the exact path with that dz element = 1.0, the reference is v * E in fp64.
    CPU emulation of this construction puts the complete six-product sum at 2^-24 .. 2^-25 of max |v E| and any single missing product at >= 2^-18; the
    bound 2^-21 sits 8 x from both.  Where the exact result is 0 (other outputs, taps that leave the plane) the split result must be exactly 0."""
    from convkan_amd import ops
    C_, O_ = 8, 128
    v = 1.0 + 2.0 ** -9 + 2.0 ** -18
    torch.manual_seed(PW)
    _, spec, wb, ws = _layer(C_, O_)
    x = 1.5 * torch.randn(B, C_, PW, PW, device="cuda")
    e = PW - 1
    worst = [0.0, 0.0]
    for (h, w) in ((0, 0), (0, e), (e, 0), (e, e), (PW // 2 - 1, PW // 2)):
        for o in (0, 7, 8, 127):
            dz = torch.zeros(B, O_, PW, PW, device="cuda")
            dz[B - 1, o, h, w] = 1.0
            E = _exact_dw(spec, x, dz, wb, ws)
            dz[B - 1, o, h, w] = v
            split = ops.kan_conv_bwd_weight_split(spec, x, dz)
            for i in range(2):
                want = v * E[i].double()
                err = float((split[i].double() - want).abs().max()) / float(want.abs().max())
                worst[i] = max(worst[i], err)
                assert float(want.abs().max()) > 0 and err <= 2.0 ** -21, (h, w, o, i, err)
                assert bool((split[i][E[i] == 0] == 0).all()), (h, w, o, i)
            assert bool((E[1] == 0).any())                            # (other outputs at least)
    print(f"[split bwd-weight every product @{PW}x{PW}] worst |split - v E| / max |v E|: dw_base {worst[0]:.2e}  dw_basis {worst[1]:.2e}  (bound {2.0 ** -21:.2e})")


@pytest.mark.parametrize("C_,O_,B,PW", [(8, 128, 2, 8), (24, 128, 3, 16), (8, 128, 264, 8), (8, 128, 72, 16)])
def test_nothing_outside_the_outputs_is_written(C_, O_, B, PW, gpu_lib):
    """dw_base, dw_basis and the workspace each sit inside a larger buffer of a sentinel: every element of the two gradients is overwritten and equals the ops
    result, every guard region (around the workspace too) is intact."""
    from convkan_amd import ops
    from convkan_amd import _lib as L
    lib = L.load()
    torch.manual_seed(3)
    _, spec, wb, ws = _layer(C_, O_)
    x = torch.randn(B, C_, PW, PW, device="cuda")
    dz = torch.randn(B, O_, PW, PW, device="cuda")
    want = ops.kan_conv_bwd_weight_split(spec, x, dz)
    geom, basis, _ = ops._plan_cached(*ops._plan_key(spec, x.shape, O_))
    nbytes = lib.kan_split_bwd_weight_workspace_bytes(C.byref(geom), C.byref(basis))
    assert nbytes > 0 and nbytes % 16 == 0
    pad, sentinel = 1 << 16, 12345.0
    bigs = [torch.full((t.numel() + 2 * pad,), sentinel, device="cuda") for t in want]
    outs = [b[pad:pad + t.numel()] for b, t in zip(bigs, want)]
    wbig = torch.full((nbytes + 2 * pad,), 0x5A, device="cuda", dtype=torch.uint8)
    wsp = wbig[pad:pad + nbytes]
    L.check(lib.kan_conv_bwd_weight_split(ops._ptr(dz), ops._ptr(x), C.c_void_p(outs[0].data_ptr()), C.c_void_p(outs[1].data_ptr()), C.c_void_p(wsp.data_ptr()),
                                          C.byref(geom), C.byref(basis), ops._stream(x)), "kan_conv_bwd_weight_split")
    torch.cuda.synchronize()
    for big, out, t in zip(bigs, outs, want):
        assert bool((out != sentinel).all()) and torch.equal(out.view_as(t), t)
        assert bool((big[:pad] == sentinel).all()) and bool((big[pad + t.numel():] == sentinel).all())
    assert bool((wbig[:pad] == 0x5A).all()) and bool((wbig[pad + nbytes:] == 0x5A).all())


def test_split_bwd_weight_scope_is_enforced(gpu_lib):
    """The refusals of ops.kan_conv_bwd_data_split (test_gpu_split_bwd_data.py), for the weight gradient: KanConvError naming the split-precision scope."""
    import convkan_amd as K
    from convkan_amd import _lib as L
    from convkan_amd import ops
    silu = torch.nn.SiLU
    for layer, shape in ((K.KANConv2DLayer(16, 128, 3, padding=1, base_activation=silu), (2, 16, 4, 4)),                  # 4x4 planes
                         (K.KANConv2DLayer(16, 128, 3, padding=1, grid_size=8, base_activation=silu), (2, 16, 8, 8)),     # not the default spec
                         (K.KANConv2DLayer(16, 64, 3, padding=1, base_activation=silu), (2, 16, 8, 8)),                   # 64 outputs
                         (K.KANConv2DLayer(16, 128, 3, padding=1, base_activation=silu), (3, 16, 8, 8)),                  # odd batch
                         (K.KANConv2DLayer(16, 128, 3, padding=1), (2, 16, 8, 8))):                                       # GELU base branch
        layer = layer.cuda()
        x = torch.randn(*shape, device="cuda")
        dz = torch.randn(shape[0], layer.base_conv[0].weight.shape[0], shape[2], shape[3], device="cuda")
        with pytest.raises(L.KanConvError, match="split-precision"):
            ops.kan_conv_bwd_weight_split(layer.conv_spec(), x, dz)


def test_contexts_on_kan_vgg11(gpu_lib):
    """Inside ops.split_precision_backward_weight() one training step of KAN-VGG11 runs the split launch for exactly the layers of IN_CONTEXT (backward
    order).  A weight gradient feeds nothing else: logits and every other gradient stay bit-equal to the exact step, the six base / spline weight gradients
    of those layers move, within TOL_DW.  The decision is the forward's; split_precision_inference has no say in training; split_precision_backward() is the
    two backward contexts nested."""
    import convkan_amd as K
    from convkan_amd import ops
    from convkan_amd.models import vggkan
    torch.manual_seed(1)
    m = vggkan(3, 10, arch="VGG11", kan_conv="KAN", dropout_linear=0.0).cuda().train()
    x = torch.randn(8, 3, 32, 32, device="cuda")
    t = torch.randint(0, 10, (8,), device="cuda")
    in_out = {(s[1], {64: 128, 128: 256, 256: 256}[s[1]]) for s in IN_CONTEXT}
    ids = {}
    for mod in m.modules():
        if isinstance(mod, K.KANConv2DLayer) and (mod.base_conv[0].weight.shape[1], mod.base_conv[0].weight.shape[0]) in in_out:
            ids[id(mod.base_conv[0].weight)] = ids[id(mod.spline_conv[0].weight)] = True
    changed = [n for n, p in m.named_parameters() if id(p) in ids]
    assert len(changed) == 2 * len(IN_CONTEXT), changed
    with spies() as all_calls:
        calls = all_calls["kan_conv_bwd_weight_split"]
        y0, g0 = _vgg_step(m, x, t)
        assert calls == []
        with ops.split_precision_backward_weight():
            y1, g1 = _vgg_step(m, x, t)
        assert calls == IN_CONTEXT, calls
        assert torch.equal(y0, y1)
        others = [n for n in g0 if n not in changed]
        e_slopes = _same_but_slopes(g0, g1, others)
        print(f"[split bwd-weight KAN-VGG11 bs 8] PReLU slope gradients vs the exact step (atomic sums, judged together): {e_slopes:.1e}")
        assert all(bool(torch.isfinite(g1[n]).all()) for n in changed) and not all(torch.equal(g0[n], g1[n]) for n in changed)
        dist = {n: relerr(g1[n], g0[n]) for n in changed}
        print("[split bwd-weight KAN-VGG11 bs 8] weight-gradient distance from the exact step (max-normalised): " + "  ".join(f"{n} {e:.1e}" for n, e in dist.items()))
        assert all(e <= TOL_DW for e in dist.values()), dist
        n_calls = len(calls)
        with ops.split_precision_inference():                             # outside the context: the exact step
            y2, g2 = _vgg_step(m, x, t)
        assert len(calls) == n_calls and torch.equal(y0, y2)
        _same_but_slopes(g0, g2, list(g0))
        m.zero_grad(set_to_none=True)
        with ops.split_precision_backward_weight():                       # decided at forward time ...
            loss = torch.nn.functional.cross_entropy(m(x), t)
        loss.backward()                                                   # ... so a backward outside still runs the split kernel
        assert len(calls) == n_calls + len(IN_CONTEXT)
        assert all(torch.equal(g1[n], p.grad) for n, p in m.named_parameters() if p.numel() > 1)
        with ops.split_precision_backward():
            _, g3 = _vgg_step(m, x, t)
        with ops.split_precision_backward_data():
            with ops.split_precision_backward_weight():
                _, g4 = _vgg_step(m, x, t)
        assert len(calls) == n_calls + 3 * len(IN_CONTEXT)
        _same_but_slopes(g3, g4, list(g3))
        assert any(not torch.equal(g3[n], g1[n]) for n in g1 if n not in changed)      # and the input gradient did go split as well


def test_graphed_steps_inside_the_context_equal_eager_steps_bitwise(gpu_lib):
    """A GraphedStep recorded inside split_precision_backward(), FusedAdamW outside the graph, two batches: losses and weights equal two eager steps inside
    the context (the workspace is the graph pool's: stable addresses, no host sync), and differ from two exact steps."""
    import convkan_amd as K
    from convkan_amd import ops
    from convkan_amd.models import vggkan
    torch.manual_seed(7)
    base = vggkan(3, 10, arch="VGG11", kan_conv="KAN", dropout_linear=0.0).cuda().train()
    g = torch.Generator(device="cuda").manual_seed(3)
    batches = [(torch.randn(8, 3, 32, 32, device="cuda", generator=g), torch.randint(0, 10, (8,), device="cuda", generator=g)) for _ in range(2)]
    out = {}
    for mode in ("eager", "graph"):
        model = copy.deepcopy(base)
        opt = K.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
        losses = []
        if mode == "eager":
            with ops.split_precision_backward():
                for d, t in batches:
                    losses.append(float(K.train_step(model, d, t, opt)))
        else:
            with ops.split_precision_backward():
                step = K.GraphedStep(model, batches[0][0], batches[0][1])
            for d, t in batches:
                losses.append(float(step(d, t)))
                opt.step()
        torch.cuda.synchronize()
        out[mode] = (losses, {n: p.detach().clone() for n, p in model.named_parameters()})
    assert out["eager"][0] == out["graph"][0], (out["eager"][0], out["graph"][0])
    for n, a in out["eager"][1].items():
        assert torch.equal(a, out["graph"][1][n]), n
    model = copy.deepcopy(base)                                           # and the steps did take the split path: an exact pair of steps differs
    opt = K.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    for d, t in batches:
        K.train_step(model, d, t, opt)
    assert any(not torch.equal(p.detach(), out["eager"][1][n]) for n, p in model.named_parameters())


def test_gradient_sinks_receive_the_split_gradient(gpu_lib):
    """A sink registered on the layer's two weight Parameters (as parallel/dp.py registers its bucket slices) is written by the split launch: p.grad aliases
    the sink and equals it, exactly as on the exact path, and holds the split gradient (not the exact one)."""
    import convkan_amd as K
    from convkan_amd import ops
    torch.manual_seed(5)
    layer = K.KANConv2DLayer(16, 128, 3, padding=1, base_activation=torch.nn.SiLU).cuda().train()
    params = [layer.base_conv[0].weight, layer.spline_conv[0].weight]
    x = torch.randn(4, 16, 8, 8, device="cuda")
    dy = torch.randn(4, 128, 8, 8, device="cuda")
    calls = []
    orig = ops.kan_conv_bwd_weight_split
    ops.kan_conv_bwd_weight_split = lambda *a, **k: (calls.append(tuple(a[1].shape)), orig(*a, **k))[1]
    try:
        seen = {}
        for mode in ("plain", "exact", "split"):
            layer.zero_grad(set_to_none=True)
            sinks = [torch.full_like(p, 777.0) for p in params]
            if mode != "plain":
                for p, s in zip(params, sinks):
                    ops.GRAD_SINKS[id(p)] = ops.GradSink(weakref.ref(p), s)
            if mode == "split":
                with ops.split_precision_backward_weight():
                    layer(x).backward(dy)
            else:
                layer(x).backward(dy)
            torch.cuda.synchronize()
            seen[mode] = [(p.grad.data_ptr() == s.data_ptr(), torch.equal(p.grad, s), p.grad.detach().clone()) for p, s in zip(params, sinks)]
            for p in params:
                ops.GRAD_SINKS.pop(id(p), None)
        assert calls == [(4, 16, 8, 8)]
        for i in range(2):
            assert seen["exact"][i][1] and torch.equal(seen["exact"][i][2], seen["plain"][i][2])      # the exact path writes through
            assert seen["split"][i][0] == seen["exact"][i][0] and seen["split"][i][1] == seen["exact"][i][1]
            assert not torch.equal(seen["split"][i][2], seen["exact"][i][2]) and relerr(seen["split"][i][2], seen["exact"][i][2]) <= TOL_DW
    finally:
        ops.kan_conv_bwd_weight_split = orig
        for p in params:
            ops.GRAD_SINKS.pop(id(p), None)


def test_cut_weight_cache_entry_dies_with_its_weights(gpu_lib):
    """split_precision_backward() leans on the cut-weight cache of the bwd-data launch, keyed by weight addresses and version stamps.  A later model's weights
    can land on a dead model's addresses with equal stamps (fresh Parameters: version 0), and an eager step would then multiply the dead model's cut weights:
    the entry must go when its weights do."""
    import gc
    import convkan_amd as K
    from convkan_amd import ops
    layer = K.KANConv2DLayer(16, 128, 3, padding=1, base_activation=torch.nn.SiLU).cuda().train()
    x = torch.randn(2, 16, 8, 8, device="cuda", requires_grad=True)
    with ops.split_precision_backward():
        layer(x).sum().backward()
    key = (layer.base_conv[0].weight.data_ptr(), layer.spline_conv[0].weight.data_ptr(), x.device.index)
    assert key in ops._CUT_BWD_DATA.entries
    del layer
    gc.collect()
    assert key not in ops._CUT_BWD_DATA.entries

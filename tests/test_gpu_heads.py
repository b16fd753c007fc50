"""MLP KAN heads with one [I, O, degree + 1] coefficient tensor on the GPU: the [I][O][n] pack / unpack kernels bit for bit against the
conv-layout ones, every fixture of tests/golden/heads against the reference's fp64 pass, the L1-wrapped model, and a VGG with a ChebyKAN head."""
import ctypes as C

import pytest
import torch

from heads_cases import COEFFS, build_head, head_cases, load_head, state_dict_of
from helpers import TOL_DW, TOL_DX, TOL_Y, relerr

pytestmark = pytest.mark.gpu


def _tol(stated, d, key32, key64):
    """The project's one rule: max(stated, 4 x the fp32 reference's own distance from fp64 on that tensor)."""
    return max(stated, 4.0 * relerr(torch.from_numpy(d[key32]), torch.from_numpy(d[key64])))


def _check(what, got, d, key32, key64, stated):
    err, tol = relerr(got, torch.from_numpy(d[key64])), _tol(stated, d, key32, key64)
    print(f"{what}: error {err:.2e}  tolerance {tol:.1e}")
    assert err <= tol, (what, err, tol)


# ------------------------------------------------------------------------------------------- pack / unpack, exact
def _plan(K, I, O, n, dev, B=4):
    spec = K.LucasKANLayer(I, O, n - 1).conv_spec()                 # n = 13, 16: the recurrence coefficients travel as a device table
    geom, basis, plan = K.ops._plan_cached(*K.ops._plan_key(spec, (B, I, 1, 1), O))
    return geom, K.ops._with_table(basis, spec, dev), plan


@pytest.mark.parametrize("I,O,n", [(1, 1, 2), (7, 3, 4), (9, 130, 3), (300, 5, 4), (37, 257, 16), (130, 129, 13)])
def test_pack_and_unpack_match_the_conv_layout_kernels_bit_for_bit(gpu_lib, I, O, n):
    import convkan_amd as K
    lib, dev, P = gpu_lib, torch.device("cuda"), K.ops._ptr
    geom, basis, plan = _plan(K, I, O, n, dev)
    g, b, st = C.byref(geom), C.byref(basis), K.ops._stream(torch.empty(1, device=dev))
    coeffs = torch.randn(I, O, n, generator=torch.Generator().manual_seed(I * 1000 + O)).to(dev)
    permuted = coeffs.permute(1, 0, 2).reshape(O, I * n, 1, 1).contiguous()
    new = lambda nbytes: torch.full((nbytes // 4,), 123.0, device=dev)               # the same finite sentinel under both packers
    wp_a, wd_a, wp_b, wd_b, wp_c = (new(plan.packed_weight_bytes), new(plan.bwd_data_weight_bytes), new(plan.packed_weight_bytes),
                                    new(plan.bwd_data_weight_bytes), new(plan.packed_weight_bytes))
    K._lib.check(lib.kan_pack_weights(None, P(permuted), P(wp_a), P(wd_a), g, b, st), "kan_pack_weights")
    K._lib.check(lib.kan_pack_weights_iod(P(coeffs), P(wp_b), P(wd_b), g, b, st), "kan_pack_weights_iod")
    K._lib.check(lib.kan_pack_weights_iod(P(coeffs), P(wp_c), None, g, b, st), "kan_pack_weights_iod (wd = NULL)")
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(wp_a), bits(wp_b)) and torch.equal(bits(wd_a), bits(wd_b)) and torch.equal(bits(wp_a), bits(wp_c))
    assert bool((wp_a != 123.0).any())
    # unpack: random slabs, one clone per unpacker (the conv-layout one folds many slabs in place).  The batch size only sets the slab count:
    # 1; 11 = one round of eight running sums and a remainder; 16 = two rounds; 48 and up = folded into slab 0 first
    counts = []
    for B in (4, 2900, 4096, 65536):
        geom, basis, plan = _plan(K, I, O, n, dev, B)
        g, b = C.byref(geom), C.byref(basis)
        counts.append(plan.bwd_weight_splits)
        slabs = torch.randn(plan.bwd_weight_splits * plan.bwd_weight_slab_elems, generator=torch.Generator().manual_seed(O + B)).to(dev)
        s_a, s_b = slabs.clone(), slabs.clone()
        dw_a, dw_b = torch.full((O, I * n, 1, 1), 7.0, device=dev), torch.full((I, O, n), 7.0, device=dev)
        K._lib.check(lib.kan_unpack_wgrad(P(s_a), None, P(dw_a), g, b, st), "kan_unpack_wgrad")
        K._lib.check(lib.kan_unpack_wgrad_iod(P(s_b), P(dw_b), g, b, st), "kan_unpack_wgrad_iod")
        assert torch.equal(bits(dw_a.view(O, I, n).permute(1, 0, 2).contiguous()), bits(dw_b)), plan.bwd_weight_splits
        assert bool((dw_b != 7.0).all())
    assert counts[0] == 1 and 8 < counts[1] < 16 and counts[2] == 16 and counts[3] >= 32, counts


# ------------------------------------------------------------------------------------------- layers against the reference's fp64 pass
class _NoWeightCopies:
    """While active, torch.einsum raises, and Tensor.permute raises on a tensor as large as the layer's coefficients: the head's forward and
    backward must reach the kernels without a permuted or contracted copy of the weights."""

    def __init__(self, monkeypatch, numel):
        permute = torch.Tensor.permute

        def no_einsum(*a, **k):
            raise AssertionError("torch.einsum on the head's path")

        def guarded(t, *a, **k):
            if t.numel() >= numel:
                raise AssertionError(f"Tensor.permute of a weight-sized tensor {tuple(t.shape)} on the head's path")
            return permute(t, *a, **k)
        monkeypatch.setattr(torch, "einsum", no_einsum)
        monkeypatch.setattr(torch.Tensor, "permute", guarded)


@pytest.mark.parametrize("name", head_cases("layer"))
def test_layer_matches_the_reference_fp64_pass(gpu_lib, monkeypatch, name):
    d = load_head(name)
    c = d["cfg"]
    layer = build_head(c)
    layer.load_state_dict(state_dict_of(d), strict=True)
    layer = layer.cuda()
    key = COEFFS[c["family"]]
    x = torch.from_numpy(d["x"]).cuda().requires_grad_(True)
    with monkeypatch.context() as mp:
        _NoWeightCopies(mp, getattr(layer, key).numel())
        y = layer(x)
        y.backward(torch.from_numpy(d["g"]).cuda())
        torch.cuda.synchronize()
    assert tuple(y.shape) == (c["B"], c["O"])
    _check(f"{name} y", y, d, "y", "y64", TOL_Y)
    _check(f"{name} dx", x.grad, d, "dx", "dx64", TOL_DX)
    _check(f"{name} d {key}", getattr(layer, key).grad, d, "grad." + key, "grad64." + key, TOL_DW)
    if not d["dx64"].any():                     # Fibonacci degree 1, Gegenbauer alpha 0: the basis does not depend on x
        assert int(torch.count_nonzero(x.grad)) == 0


def test_forward_flattens_leading_dimensions(gpu_lib):
    d = load_head("hermite_deg3")
    layer = build_head(d["cfg"])
    layer.load_state_dict(state_dict_of(d))
    layer = layer.cuda()
    x = torch.from_numpy(d["x"]).cuda()
    with torch.no_grad():
        assert torch.equal(layer(x.reshape(5, 1, 7)), layer(x))


def test_l1_wrapped_model_matches_the_reference_gradients(gpu_lib):
    """mlp_lucaskan([6, 5, 3], l1_decay=0.01): the L1 wrapper of the first layer acts as the reference's does, so each gradient -- penalty
    included wherever the reference's hook adds it -- is the reference's."""
    d = load_head("lucas_mlp_l1")
    m = build_head(d["cfg"])
    m.load_state_dict(state_dict_of(d), strict=True)
    m = m.cuda()
    x = torch.from_numpy(d["x"]).cuda().requires_grad_(True)
    y = m(x)
    y.backward(torch.from_numpy(d["g"]).cuda())
    torch.cuda.synchronize()
    _check("mlp_l1 y", y, d, "y", "y64", TOL_Y)
    _check("mlp_l1 dx", x.grad, d, "dx", "dx64", TOL_DX)
    for n, p in m.named_parameters():
        _check(f"mlp_l1 d {n}", p.grad, d, "grad." + n, "grad64." + n, TOL_DW)


def test_vgg11_with_a_chebykan_head_trains(gpu_lib):
    import convkan_amd as K
    from convkan_amd.models import vggkan
    torch.manual_seed(0)
    m = vggkan(3, 10, arch="VGG11", classifier_type="KAN", kan_classifier="ChebyKAN").cuda()
    y = m(torch.randn(2, 3, 32, 32, device="cuda"))
    assert tuple(y.shape) == (2, 10)
    y.square().sum().backward()
    torch.cuda.synchronize()
    head = [(n, p) for n, p in m.classifier.named_parameters()]
    assert [n for n, _ in head] == ["1.layers.0.cheby_coeffs"] and isinstance(m.classifier[1], K.ChebyKAN)
    for n, p in head:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), n

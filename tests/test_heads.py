"""MLP KAN heads with one [I, O, degree + 1] coefficient tensor (ChebyKAN and the six recurrence families), host side: factory and
model structure against the reference's fixtures (tests/golden/heads), the coefficient tables against the reference's fp64 output,
and the two [I][O][n] entry points of the C ABI up to the point where they would launch."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

from conftest import ROOT
from heads_cases import COEFFS, KEYS, LAYER, REFUSED, basis_fp64, build_head, head_cases, load_head, state_dict_of


def test_factory_has_the_seven_heads_and_refuses_the_other_nine():
    import convkan_amd as K
    from convkan_amd.models import vggkan
    from heads_cases import FACTORY
    assert set(K.MLP_KAN_FACTORY) == {"KAN", *KEYS.values()}
    for fam, key in KEYS.items():
        assert K.MLP_KAN_FACTORY[key] is getattr(K, FACTORY[fam])
    assert len(REFUSED) == 9 and not set(REFUSED) & set(K.MLP_KAN_FACTORY)
    for name in REFUSED:
        with pytest.raises(NotImplementedError, match=name):
            vggkan(3, 10, arch="VGG11", classifier_type="KAN", kan_classifier=name)
    with pytest.raises(NotImplementedError):                    # the B-spline head keeps refusing l1_decay
        K.mlp_kan([4, 4], l1_decay=0.1)


@pytest.mark.parametrize("name", head_cases("layer"))
def test_layer_mirrors_the_reference(name):
    d = load_head(name)
    c = d["cfg"]
    layer = build_head(c)
    layer.load_state_dict(state_dict_of(d), strict=True)
    key = COEFFS[c["family"]]
    assert [n for n, _ in layer.named_parameters()] == [key]
    assert [n for n, _ in layer.named_buffers()] == (["arange"] if c["family"] == "cheby" else [])
    assert tuple(getattr(layer, key).shape) == (c["I"], c["O"], c["degree"] + 1)
    if c["family"] == "cheby":
        assert layer.arange.dtype == torch.int64 and torch.equal(layer.arange, torch.arange(c["degree"] + 1))
    with pytest.raises(Exception, match="no CPU fallback"):
        layer(torch.from_numpy(d["x"]))


def test_init_is_the_reference_normal():
    import convkan_amd as K
    torch.manual_seed(0)
    layer = K.LucasKANLayer(64, 48, 3)
    std = 1 / (64 * 4)
    assert abs(float(layer.lucas_coeffs.detach().std()) / std - 1) < 0.05 and abs(float(layer.lucas_coeffs.detach().mean())) < 0.05 * std


def test_model_fixture_structure_and_keys():
    import convkan_amd as K
    d = load_head("lucas_mlp_l1")
    m = build_head(d["cfg"])
    m.load_state_dict(state_dict_of(d), strict=True)
    assert list(m.state_dict()) == ["layers.0.module.lucas_coeffs", "layers.1.lucas_coeffs"]         # L1 wraps every layer but the last
    assert isinstance(m.layers[0], K.utils.regularization.L1) and m.layers[0].weight_decay == 0.01
    assert isinstance(m.layers[0].module, K.LucasKANLayer) and isinstance(m.layers[1], K.LucasKANLayer)
    assert m.polynomial_order == 3 and m.num_layers == 2
    kinds = [type(l).__name__ for l in K.mlp_gegenbauerkan([8, 16, 4], dropout=0.1, alpha_param=0.3).layers]
    assert kinds == ["Dropout", "GegenbauerKANLayer", "Dropout", "GegenbauerKANLayer"]
    assert [type(l).__name__ for l in K.mlp_chebykan([8, 16, 4], dropout=0.1, first_dropout=False).layers] == ["ChebyKANLayer", "Dropout", "ChebyKANLayer"]
    assert K.mlp_laguerrekan([4, 4], alpha=0.5).alpha == 0.5 and K.mlp_laguerrekan([4, 4], alpha=0.5).layers[0].alpha == 0.5


@pytest.mark.parametrize("name", head_cases("layer"))
def test_coefficient_table_reproduces_the_reference_fp64_output(name):
    """The table the layer hands to ConvSpec, run through the header's recurrence in fp64 and contracted with the fixture's coefficients, is the
    reference MLP layer's fp64 output: 1e-12 of the largest element (both are fp64 evaluations of the same polynomials)."""
    d = load_head(name)
    c = d["cfg"]
    layer = build_head(c)
    spec = layer.conv_spec()
    assert spec.w_layout == 1 and spec.act == -1 and spec.kernel == (1, 1) and spec.groups == 1 and spec.n_basis == c["degree"] + 1
    planes = basis_fp64(spec, torch.from_numpy(d["x"]))
    y = torch.einsum("bid,iod->bo", planes, torch.from_numpy(d["sd." + COEFFS[c["family"]]]).double())
    y64 = torch.from_numpy(d["y64"])
    err = float((y - y64).abs().max() / y64.abs().max())
    print(f"{name}: table vs reference fp64 {err:.2e}")
    assert err <= 1e-12, err


@pytest.mark.parametrize("fam", [f for f in LAYER if f != "cheby"])
def test_head_tables_are_the_conv_layers_tables(fam):
    """The reuse of poly_layers.py's `_coeffs` is by construction; this pins that a head and the conv layer of its family state one table."""
    import convkan_amd as K
    extra = {"gegenbauer": {"alpha_param": 0.7}, "laguerre": {"alpha": 0.5}}.get(fam, {})
    for degree in (1, 3, 12):
        head = getattr(K, LAYER[fam])(3, 2, degree, **extra)
        conv = getattr(K, LAYER[fam].replace("KANLayer", "KANConv2DLayer"))(3, 2, 1, degree, **extra)
        assert head.conv_spec().table == conv.conv_spec().table


def test_degree_limits():
    import convkan_amd as K
    with pytest.raises(ValueError):
        K.BesselKANLayer(4, 4, 0)
    K.ChebyKANLayer(4, 4, K._lib.KAN_MAX_PLANES - 1)
    with pytest.raises(NotImplementedError, match="KAN_MAX_PLANES = 16"):
        K.ChebyKANLayer(4, 4, K._lib.KAN_MAX_PLANES)
    assert K.ops._device_table(K.LucasKANLayer(4, 4, 11).conv_spec()) and not K.ops._device_table(K.LucasKANLayer(4, 4, 10).conv_spec())


def test_entry_points_declared_bound_and_exported():
    import convkan_amd as K
    K.build_library()
    header = open(os.path.join(ROOT, "include", "kanconv.h")).read()
    raw = C.CDLL(K._lib.LIB_PATH)
    for name in ("kan_pack_weights_iod", "kan_unpack_wgrad_iod"):
        assert re.search(r"\bint " + name + r"\s*\(", header) and name in K._lib.SIGNATURES and hasattr(raw, name)
    assert "w_layout" in K.ops.ConvSpec.__dataclass_fields__ and K.ops.ConvSpec.__dataclass_fields__["w_layout"].default == 0


def _geom_basis(K, kh=1, groups=1, act=-1):
    spec = K.LucasKANLayer(7, 3, 3).conv_spec()
    spec = K.ops.ConvSpec(**{**spec.__dict__, "kernel": (kh, kh), "padding": (kh // 2, kh // 2), "groups": groups, "act": act})
    g, b, _ = K.ops._plan_cached(*K.ops._plan_key(spec, (4, 7 * groups, 4, 4), 3))
    return g, b


def test_launchers_refuse_out_of_scope_calls_without_a_device():
    """Every refusal below is decided by host arithmetic before any launch; the pointers are never dereferenced."""
    import convkan_amd as K
    K.build_library()
    lib, p, nul = K._lib.load(), C.c_void_p(4096), C.c_void_p(0)
    cases = [(_geom_basis(K, kh=3), "1x1"), (_geom_basis(K, act=K._lib.ACT_SILU), "base branch"), (_geom_basis(K, groups=2), "one group")]
    for (g, b), msg in cases:
        assert lib.kan_pack_weights_iod(p, p, p, C.byref(g), C.byref(b), nul) < 0 and msg in lib.kan_last_error().decode()
        assert lib.kan_unpack_wgrad_iod(p, p, C.byref(g), C.byref(b), nul) < 0 and msg in lib.kan_last_error().decode()
    g, b = _geom_basis(K)
    assert lib.kan_pack_weights_iod(nul, p, p, C.byref(g), C.byref(b), nul) < 0 and "null" in lib.kan_last_error().decode()
    assert lib.kan_pack_weights_iod(p, nul, p, C.byref(g), C.byref(b), nul) < 0
    assert lib.kan_unpack_wgrad_iod(nul, p, C.byref(g), C.byref(b), nul) < 0 and "null" in lib.kan_last_error().decode()
    assert lib.kan_unpack_wgrad_iod(p, nul, C.byref(g), C.byref(b), nul) < 0
    assert lib.kan_pack_weights_iod(p, p, p, None, C.byref(b), nul) < 0 and lib.kan_unpack_wgrad_iod(p, p, C.byref(g), None, nul) < 0


def test_vgg_and_alexnet_build_with_the_new_heads():
    import convkan_amd as K
    from convkan_amd.models import alexnet_kan, vggkan
    for head, first in (("KAN", "1.layers.0.cheby_coeffs"), ("HiddenKAN", "0.layers.0.cheby_coeffs"), ("VGGKAN", "0.weight")):
        v = vggkan(3, 10, arch="VGG11", classifier_type=head, kan_classifier="ChebyKAN")
        names = [n for n, _ in v.classifier.named_parameters()]
        assert names[0] == first, (head, names)
        layers = [m for m in v.classifier.modules() if isinstance(m, K.ChebyKANLayer)]
        assert len(layers) == 1 and layers[0].degree == 3 and "CHEBYKAN" in v.name
    a = alexnet_kan(10, arch="small", classifier_type="KAN", kan_classifier="LucasKAN")
    names = [n for n, _ in a.classifier.named_parameters()]
    assert names[0] == "fc1.weight" and names[-1] == "kan_fc3.layers.0.lucas_coeffs", names
    assert isinstance(a.classifier.kan_fc3, K.LucasKAN) and not any(isinstance(m, nn.Dropout) for m in a.classifier.kan_fc3.layers)

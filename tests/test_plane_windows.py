"""CPU: plane windows -- any degree / grid size on launches of at most KAN_MAX_PLANES planes (layers/conv_layers.py `_HipLayer._conv_stage`).

Construction and state_dict parity above the old limits, the partition a layer cuts its planes into, the weight slicing of every
window scheme (fp64 torch on the oracle's basis functions: the sum over windows IS the conv over the whole basis), and the planner's
checks of the first-plane offset (`order = mode | first << 8`, include/kanconv.h)."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import convkan_amd as K
from convkan_amd import _lib as L
from convkan_amd import ops
from conftest import GOLDEN, load_golden
from helpers import build_layer
from oracle import kan_oracle as O

WINDOWS = os.path.join(GOLDEN, "windows")
FIXTURES = sorted(fn[:-4] for fn in os.listdir(WINDOWS) if fn.endswith(".npz"))


def load(name):
    return load_golden(os.path.join("windows", name))


def test_fixture_set_is_complete():
    want = {"fourier_grid8", "fourier_grid20_s2g2", "fourier_1d_grid9", "lucas_deg11", "lucas_deg16", "taylor_deg18", "gegenbauer_deg20_d2",
            "cheby_deg17", "jacobi_deg12", "legendre_deg32", "bersnstein_deg12", "rbf_grid20", "relu_g12k4", "bessel_deg12", "hermite_deg12"}
    assert want <= set(FIXTURES), want - set(FIXTURES)


# ------------------------------------------------------------------------------------------------------------------ 1. construction
def _grown(c, size=40):
    """The fixture's layer configuration at degree / grid_size `size`."""
    c = dict(c)
    if c["kind"] == "relu":
        c["extra"] = dict(c.get("extra", {}), g=size - 4, k=4)
    elif c["kind"] == "rbf":
        c["grid_size"] = size
    else:
        c["degree"] = size              # (FourierKAN fixtures carry grid_size as `degree`)
    return c


@pytest.mark.parametrize("name", FIXTURES)
def test_builds_with_reference_state_dict(name):
    d = load(name)
    layer = build_layer(d["cfg"])
    sd = {k[3:]: torch.from_numpy(v) for k, v in d.items() if k.startswith("sd.")}
    assert [(k, tuple(v.shape)) for k, v in layer.state_dict().items()] == [(k, tuple(v.shape)) for k, v in sd.items()]
    layer.load_state_dict(sd, strict=True)
    big = build_layer(_grown(d["cfg"]))
    assert list(big.state_dict().keys()) == list(sd.keys())               # no buffer of the device coefficient table, no window state
    spec = big.conv_spec()
    assert spec.first == 0 and spec.n_basis + int(spec.has_base) > L.KAN_MAX_PLANES and len(big._plane_windows()) >= 3


# ------------------------------------------------------------------------------------------------------------------ 2. partition
def _layers(size):
    return {
        "lucas": K.LucasKANConv2DLayer(3, 4, 3, degree=size), "bessel": K.BesselKANConv2DLayer(3, 4, 3, degree=size),
        "fibonacci": K.FibonacciKANConv2DLayer(3, 4, 3, degree=size), "hermite": K.HermiteKANConv2DLayer(3, 4, 3, degree=size),
        "gegenbauer": K.GegenbauerKANConv2DLayer(3, 4, 3, degree=size, alpha_param=0.5),
        "laguerre": K.LaguerreKANConv2DLayer(3, 4, 3, degree=size, alpha=1.0), "taylor": K.TaylorKANConv2DLayer(3, 4, 3, degree=size),
        "taylor_noact": K.TaylorKANConv2DLayer(3, 4, 3, degree=size, base_activation=None),
        "cheby": K.ChebyKANConv2DLayer(3, 4, 3, degree=size), "fourier": K.FourierKANConv2DLayer(3, 4, 3, grid_size=size),
        "fourier_1d": K.FourierKANConv1DLayer(3, 4, 3, grid_size=size),
        "jacobi": K.JacobiKANConv2DLayer(3, 4, 3, degree=size), "legendre": K.LegendreKANConv2DLayer(3, 4, 3, degree=size),
        "bersnstein": K.BersnsteinKANConv2DLayer(3, 4, 3, degree=size), "rbf": K.FastKANConv2DLayer(3, 4, 3, grid_size=size),
        "relu": K.ReLUKANConv2DLayer(3, 4, 3, g=size - 3, k=3), "bspline": K.KANConv2DLayer(3, 4, 3, grid_size=size),
    }


@pytest.mark.parametrize("size", [8, 16, 17, 33, 40])
def test_windows_partition_the_planes(size):
    for fam, layer in _layers(size).items():
        spec = layer.conv_spec()
        wins = layer._plane_windows()
        u = layer._window_unit
        n = spec.n_basis // u
        assert wins[0][1] == 0 and wins[-1][2] == n, fam
        assert all(a[2] == b[1] for a, b in zip(wins, wins[1:])), fam                    # [0, n) exactly once, in order
        for i, (ws, j0, j1, base) in enumerate(wins):
            assert j1 > j0 and ws.n_basis == u * (j1 - j0), fam
            assert ws.n_basis + int(ws.has_base) <= L.KAN_MAX_PLANES, fam                 # base included
            assert base == (i == 0 and spec.has_base) and ws.has_base == base, fam        # the base branch rides the first window only
            assert (ws.kernel, ws.stride, ws.padding, ws.dilation, ws.groups) == (spec.kernel, spec.stride, spec.padding, spec.dilation, spec.groups)
            if spec.kind in (L.BASIS_POLY, L.BASIS_CHEBY, L.BASIS_FOURIER):
                assert ws.first == j0 and ws.table == spec.table and ws.order == spec.order, fam
            else:
                assert ws.first == 0, fam
            if spec.kind == L.BASIS_BSPLINE:
                assert ws.table == spec.table[j0:j1 + spec.order + 1], fam
            if spec.kind == L.BASIS_RBF:
                assert ws.table == spec.table[j0:j1], fam
        if spec.kind == L.BASIS_FOURIER:
            # frequencies [f0, f1): the cos and the sin block of a window hold the same k; 7 frequencies beside the base plane, 8 otherwise
            assert [j1 - j0 for _, j0, j1, _ in wins[:-1]] == [7 if spec.has_base else 8] + [8] * (len(wins) - 2), fam
        if spec.n_basis + int(spec.has_base) <= L.KAN_MAX_PLANES:
            assert len(wins) == 1 and wins[0][0] == spec, fam                             # fits one launch: the layer's own spec, untouched


def test_window_width_is_a_class_attribute():
    assert K.LucasKANConv2DLayer.plane_window == L.KAN_MAX_PLANES
    layer = K.FourierKANConv2DLayer(3, 4, 3, grid_size=6)
    assert len(layer._plane_windows()) == 1
    layer.plane_window = 4
    assert [(j0, j1, b) for _, j0, j1, b in layer._plane_windows()] == [(0, 1, True), (1, 3, False), (3, 5, False), (5, 6, False)]


# ------------------------------------------------------------------------------------------------------------------ 3. slicing
def _sum_over_windows(layer, planes, ws, pick):
    """sum_w conv2d(pick(planes, j0, j1), window slice of ws) in fp64, against the conv over all planes ([B, C, n, H, W], channel c*n + j)."""
    n = planes.shape[2] // layer._window_unit
    whole = F.conv2d(planes.flatten(1, 2), ws, padding=1)
    parts = sum(F.conv2d(pick(planes, j0, j1).flatten(1, 2), layer._window_weights([ws], j0, j1, n)[0], padding=1)
                for _, j0, j1, _ in layer._plane_windows())
    assert len(layer._plane_windows()) >= 3
    err = float((parts - whole).abs().max() / whole.abs().max())
    assert err <= 1e-12, err


def _x(C_=3):
    return torch.randn(2, C_, 6, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(5))


def test_slicing_recurrence():
    layer = K.LucasKANConv2DLayer(3, 4, 3, degree=20).double()
    layer.plane_window = 6
    planes = O.poly_basis(_x(), "lucas", 20)
    _sum_over_windows(layer, planes, layer.poly_conv[0].weight.detach(), lambda p, j0, j1: p[:, :, j0:j1])


def test_slicing_fourier():
    G = 11
    layer = K.FourierKANConv2DLayer(3, 4, 3, grid_size=G).double()
    layer.plane_window = 7
    planes = O.fourier_basis(_x(), G)
    pick = lambda p, f0, f1: torch.cat((p[:, :, f0:f1], p[:, :, G + f0:G + f1]), dim=2)       # cos(k x), then sin(k x), k = f0+1 .. f1
    _sum_over_windows(layer, planes, layer.fourier_conv[0].weight.detach(), pick)


def test_slicing_plane_major_jacobi():
    from convkan_amd.layers.conv_layers import _channel_major
    layer = K.JacobiKANConv2DLayer(3, 4, 3, degree=18, a=1.0, b=0.5).double()
    layer.plane_window = 8
    x = _x()
    planes = O.poly_basis(x, "jacobi", 18, a=1.0, b=0.5)
    ws = _channel_major(layer.poly_weights.detach(), 19)[0]
    _sum_over_windows(layer, planes, ws, lambda p, j0, j1: p[:, :, j0:j1])
    # ... and the channel-major view is the reference's plane-major weight (k*C + c) re-indexed, not re-valued
    whole = F.conv2d(planes.transpose(1, 2).flatten(1, 2), layer.poly_weights.detach()[0], padding=1)
    assert torch.allclose(whole, F.conv2d(planes.flatten(1, 2), ws, padding=1), rtol=1e-12, atol=1e-12)


def test_slicing_relukan_phases():
    layer = K.ReLUKANConv2DLayer(3, 4, 3, g=14, k=4).double()
    layer.plane_window = 5
    with torch.no_grad():                                    # channel-distinct phases, as after training
        layer.phase_low.add_(0.05 * torch.randn(layer.phase_low.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(6)))
        layer.phase_high.add_(0.05 * torch.randn(layer.phase_high.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(7)))
    x = _x()
    planes = O.relukan_basis(x, layer.phase_low.detach(), layer.phase_high.detach(), layer.r)
    n = 18

    def pick(p, j0, j1):                                     # the window's planes from the window's phase slice alone
        q = O.relukan_basis(x, layer.phase_low.detach()[:, :, j0:j1], layer.phase_high.detach()[:, :, j0:j1], layer.r)
        assert torch.equal(q, p[:, :, j0:j1])
        return q
    assert planes.shape[2] == n
    _sum_over_windows(layer, planes, layer.relukan_conv[0].weight.detach(), pick)


# ------------------------------------------------------------------------------------------------------------------ 4. kan_plan
LUCAS = lambda n: (2.0, 1.0, 0.0) + (1.0, 0.0, 1.0) * (n - 2)


def _spec(kind, n, first=0, order=0, act=L.ACT_NONE, table=(), p0=0.0, p1=0.0):
    return ops.ConvSpec(kind=kind, n_basis=n, order=order, act=act, p0=p0, p1=p1, table=table, kernel=(3, 3), stride=(1, 1),
                        padding=(1, 1), dilation=(1, 1), first=first)


def _plan(spec, B=4, C_=6, H=8, O_=20):
    return ops._plan_cached(spec, B, C_, H, H, O_, C_, O_)[2]


@pytest.mark.parametrize("kind, n, kw", [
    (L.BASIS_POLY, 6, dict(order=1, act=L.ACT_GELU, table=LUCAS(30))), (L.BASIS_POLY, 4, dict(order=0, act=L.ACT_NONE, table=LUCAS(9))),
    (L.BASIS_CHEBY, 7, dict(p0=-0.99, p1=0.99)), (L.BASIS_FOURIER, 10, dict(act=L.ACT_SILU))])
def test_plan_takes_a_first_plane_offset(kind, n, kw):
    p0 = _plan(_spec(kind, n, **kw))
    for first in (1, 5, 19):
        if kind == L.BASIS_POLY and len(kw["table"]) < 3 * (first + n - 1):
            continue
        p = _plan(_spec(kind, n, first=first, **kw))
        assert (p.P, p.K, p.Kpad, p.Opad) == (p0.P, p0.K, p0.Kpad, p0.Opad)


def test_struct_packs_first_into_order():
    b = ops._basis_struct(_spec(L.BASIS_POLY, 4, first=9, order=1, table=LUCAS(13)))
    assert b.order == 1 | (9 << 8) and b.n_basis == 4 and not b.chan_table
    assert ops._basis_struct(_spec(L.BASIS_POLY, 4, order=1, table=LUCAS(4))).order == 1


@pytest.mark.parametrize("kind, n, kw", [
    (L.BASIS_BSPLINE, 8, dict(order=3, act=L.ACT_SILU, table=tuple(float(v) for v in torch.linspace(-2.2, 2.2, 12).tolist()))),
    (L.BASIS_RBF, 8, dict(act=L.ACT_SILU, p0=4 / 7, table=tuple(float(v) for v in torch.linspace(-2, 2, 8).tolist()))),
    (L.BASIS_RELU, 8, dict(act=L.ACT_SILU, p0=1.5625)), (L.BASIS_GRAM, 4, dict(act=L.ACT_SILU))])
def test_plan_rejects_an_offset_for_the_other_kinds(kind, n, kw):
    _plan(_spec(kind, n, **kw))
    with pytest.raises(L.KanConvError, match="first-plane offset"):
        _plan(_spec(kind, n, first=1, **kw))


def test_plan_rejects_negative_first_and_a_long_basis_without_table():
    with pytest.raises(L.KanConvError, match="negative first-plane offset"):
        _plan(_spec(L.BASIS_CHEBY, 4, first=-1, p0=-0.99, p1=0.99))
    lib = L.load()
    geom, _, plan = ops._plan_cached(_spec(L.BASIS_POLY, 4, order=1, table=LUCAS(4)), 4, 6, 8, 8, 20, 6, 20)
    for first, n, ok in ((0, 11, True), (7, 4, True), (8, 4, False), (0, 12, False)):
        b = ops._basis_struct(_spec(L.BASIS_POLY, n, first=first, order=1, table=LUCAS(first + n)))
        assert not b.chan_table
        rc = lib.kan_plan(C.byref(geom), C.byref(b), C.byref(L.KanPlan()))
        assert (rc == 0) == ok, (first, n)
        if not ok:
            assert b"chan_table" in lib.kan_last_error()
    # the host hands such a spec its coefficients as a device table (set per launch): the plan itself is made without a device
    assert _plan(_spec(L.BASIS_POLY, 12, order=1, act=L.ACT_GELU, table=LUCAS(12))).P == 13
    with pytest.raises(L.KanConvError, match="KAN_MAX_PLANES"):
        _plan(_spec(L.BASIS_POLY, 16, order=1, act=L.ACT_GELU, table=LUCAS(16)))


def test_windows_and_device_tables_run_the_generic_kernels():
    """A tail window of 4 planes is no degree-3 layer: the compile-time specs (halo / band routes) are for first == 0 and by-value tables."""
    kw = dict(order=1, act=L.ACT_GELU)
    fit = _plan(_spec(L.BASIS_POLY, 4, table=LUCAS(4), **kw), B=8, C_=16, H=8, O_=128)
    win = _plan(_spec(L.BASIS_POLY, 4, first=3, table=LUCAS(7), **kw), B=8, C_=16, H=8, O_=128)
    assert fit.fwd_halo == 1 and win.fwd_halo == 0 and (win.IPC, win.KC) != (fit.IPC, fit.KC)
    assert _plan(_spec(L.BASIS_CHEBY, 4, p0=-0.99, p1=0.99), B=8, C_=16, H=8, O_=128).fwd_halo == 1
    assert _plan(_spec(L.BASIS_CHEBY, 4, first=4, p0=-0.99, p1=0.99), B=8, C_=16, H=8, O_=128).fwd_halo == 0


# ------------------------------------------------------------------------------------------------------------------ 5. what still raises
def test_3d_layers_above_the_plane_limit_raise_at_construction():
    for build in (lambda: K.LucasKANConv3DLayer(3, 4, 3, degree=15), lambda: K.FourierKANConv3DLayer(3, 4, 3, grid_size=8),
                  lambda: K.ChebyKANConv3DLayer(3, 4, 3, degree=16), lambda: K.KANConv3DLayer(3, 4, 3, grid_size=13),
                  lambda: K.FastKANConv3DLayer(3, 4, 3, grid_size=16), lambda: K.TaylorKANConv3DLayer(3, 4, 3, degree=16)):
        with pytest.raises(NotImplementedError, match="KAN_MAX_PLANES = 16"):
            build()
    K.LucasKANConv3DLayer(3, 4, 3, degree=14)                # 16 planes with the base: one launch, coefficients as a device table
    K.FourierKANConv3DLayer(3, 4, 3, grid_size=7)
    K.TaylorKANConv3DLayer(3, 4, 3, degree=15)


def test_gram_keeps_its_degree_limit():
    K.GRAMKANConv2DLayer(3, 4, 3, degree=14)
    with pytest.raises(NotImplementedError):
        K.GRAMKANConv2DLayer(3, 4, 3, degree=15)

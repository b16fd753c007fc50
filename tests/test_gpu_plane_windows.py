"""GPU: plane windows -- layers above the one-launch plane limit against the reference's frozen vectors (tests/golden/windows/), the
bit-exact plane probe of the first-plane offset, forced windows on every kernel route the planner has for generic specs, and the
layers at or below the old limits left as they were.  Every test is a handful of launches on a few hundred pixels."""
import os

import pytest
import torch

import convkan_amd as K
from convkan_amd import _lib as L
from convkan_amd import ops
from conftest import GOLDEN, load_golden
from helpers import TOL_DW, TOL_DX, TOL_Y, build_layer, check_vs_oracle, relerr

pytestmark = pytest.mark.gpu

WINDOWS = os.path.join(GOLDEN, "windows")
FIXTURES = sorted(fn[:-4] for fn in os.listdir(WINDOWS) if fn.endswith(".npz"))


# ------------------------------------------------------------------------------------------------------------------ 1. fixtures
@pytest.mark.parametrize("name", FIXTURES)
def test_layer_above_the_limit_matches_reference(name, gpu_lib):
    """The comparison of test_gpu_golden.py (tolerance max(stated, 4 x the fp32 reference's own noise) per tensor), then the same layer
    against the fp64 oracle (helpers.check_vs_oracle: the same rule with the noise measured live)."""
    d = load_golden(os.path.join("windows", name))
    c = d["cfg"]
    layer = build_layer(c)
    layer.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in d.items() if k.startswith("sd.")}, strict=True)
    spec = layer.conv_spec()
    assert spec.n_basis + int(spec.has_base) > 11                    # above a limit of the parent: a device table, plane windows or both
    layer = layer.cuda().train()
    x = torch.from_numpy(d["x"]).cuda().requires_grad_(True)
    y = layer(x)
    assert tuple(y.shape) == d["y"].shape
    y.backward(torch.from_numpy(d["g"]).cuda())
    torch.cuda.synchronize()
    noise = d["noise"]

    def tol(key, base):
        return max(base, 4.0 * noise.get(key, 0.0))
    errs = {"y": (relerr(y, torch.from_numpy(d["y"])), tol("y", TOL_Y)), "dx": (relerr(x.grad, torch.from_numpy(d["dx"])), tol("dx", TOL_DX))}
    for n, p in layer.named_parameters():
        key = "grad." + n
        if key in d:
            assert p.grad is not None, n
            errs[n] = (relerr(p.grad, torch.from_numpy(d[key])), tol(key, TOL_DW if p.dim() == 4 else 2e-5))
        else:
            assert p.grad is None or not p.requires_grad or float(p.grad.abs().max()) == 0.0, n
    print(f"[windows] {name}: " + " ".join(f"{k}={v[0]:.2e}/{v[1]:.1e}" for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not v[0] <= v[1]}
    assert not bad, f"{name}: {bad}  (all: {errs})"
    errs = check_vs_oracle(layer.cpu(), c, torch.from_numpy(d["x"]), groups=c["groups"], tag=name)
    print(f"[windows] {name} vs fp64 oracle: " + " ".join(f"{k}={v[0]:.2e}/{v[1]:.1e}" for k, v in errs.items()))


# ------------------------------------------------------------------------------------------------------------------ 2. bit-exact plane probe
LUCAS13 = (2.0, 1.0, 0.0) + (1.0, 0.0, 1.0) * 11            # 13 planes: 36 coefficients, read from the device table
PROBES = {
    # kind -> (spec keywords of the FULL launch, planes of the full launch selected by a window that starts at `first`)
    "poly": (dict(kind=L.BASIS_POLY, n_basis=13, order=1, p0=0.0, p1=0.0, table=LUCAS13), lambda f: list(range(f, 13)), lambda f: 13 - f),
    "cheby": (dict(kind=L.BASIS_CHEBY, n_basis=16, order=0, p0=-0.99, p1=0.99, table=()), lambda f: list(range(f, 16)), lambda f: 16 - f),
    # G = 8 frequencies, no base: cos(k x) k = 1..8 in planes 0..7, sin(k x) in planes 8..15; `first` skips frequencies
    "fourier": (dict(kind=L.BASIS_FOURIER, n_basis=16, order=0, p0=0.0, p1=0.0, table=()),
                lambda f: list(range(f, 8)) + list(range(8 + f, 16)), lambda f: 2 * (8 - f)),
}
# first = 8 leaves a G = 8 Fourier basis no frequency at all (and a full spec of more frequencies does not fit one launch): its last case is 7
PROBE_FIRSTS = {"poly": (1, 5, 8), "cheby": (1, 5, 8), "fourier": (1, 5, 7)}


def _probe_spec(kw, **over):
    return ops.ConvSpec(act=L.ACT_NONE, kernel=(1, 1), stride=(1, 1), padding=(0, 0), dilation=(1, 1), **dict(kw, **over))


def _run(spec, x, w, dz):
    xg = x.clone().requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    z = ops.kan_conv(spec, xg, None, [], [wg])
    z.backward(dz)
    torch.cuda.synchronize()
    return z.detach(), xg.grad, wg.grad


@pytest.mark.parametrize("kind, first", [(k, f) for k in PROBES for f in PROBE_FIRSTS[k]])
def test_window_planes_are_the_full_launch_planes_bit_for_bit(kind, first, gpu_lib):
    """1x1 kernel, one input channel: with one-hot weights every output IS one plane (times 1.0, plus exact zeros), every dx one derivative
    plane times dz, every dW one plane times dz.  The window launch (first, n - first planes, identity weights) and the full launch
    (first = 0, n planes, the one-hot that selects the same planes) must agree to the bit: they run the same instructions for plane k."""
    kw, select, count = PROBES[kind]
    n, sel, m = kw["n_basis"], select(first), count(first)
    full = _probe_spec(kw)
    win = _probe_spec(kw, first=first, n_basis=m)
    gen = torch.Generator().manual_seed(11 + first)
    x = (torch.randn(2, 1, 4, 4, generator=gen) * 1.3).cuda()
    w_full = torch.zeros(m, n, 1, 1)
    w_full[torch.arange(m), torch.tensor(sel)] = 1.0
    w_win = torch.eye(m).view(m, m, 1, 1)
    for o in {0, m // 2, m - 1}:
        dz = torch.zeros(2, m, 4, 4)
        dz[:, o] = torch.randn(2, 4, 4, generator=gen)
        zf, dxf, _ = _run(full, x, w_full.cuda(), dz.cuda())
        zw, dxw, _ = _run(win, x, w_win.cuda(), dz.cuda())
        assert torch.isfinite(zf).all() and float(zf.abs().max()) > 0
        assert torch.equal(zw, zf), f"z differs by {float((zw - zf).abs().max()):.3e}"
        assert torch.equal(dxw, dxf), f"dx (output {o}) differs by {float((dxw - dxf).abs().max()):.3e}"
    # dW: one image, one non-zero dz pixel -- every entry is one plane value times one dz value
    x1 = x[:1].contiguous()
    dz = torch.zeros(1, m, 4, 4)
    dz[0, :, 2, 1] = torch.randn(m, generator=gen)
    _, _, dwf = _run(full, x1, w_full.cuda(), dz.cuda())
    _, _, dww = _run(win, x1, w_win.cuda(), dz.cuda())
    assert float(dww.abs().max()) > 0
    assert torch.equal(dww, dwf[:, sel]), f"dW differs by {float((dww - dwf[:, sel]).abs().max()):.3e}"
    if kind == "poly":
        assert ops._device_table(full) and ops._device_table(win) and (LUCAS13, x.device) in ops._TABLES


# ------------------------------------------------------------------------------------------------------------------ 3. routes
# Forced windows (plane_window = 4) on layers that fit one launch, on the smallest geometry that reaches each kernel family the planner has
# for GENERIC specs (run-time plane count: what a window with first > 0 always is).  The band and the expanded kernels are instantiated for
# compile-time specs only (csrc/kan_internal.h fast_spec), so on their geometries a window takes the planner's generic choice: the
# tap-major kernels on 64-output tiles, and the position-major tap-skipping launches of the tap-major kernels.
GEOMS = {
    "few_channels": dict(B=2, C=3, O=64, H=8, W=8, k=3, s=1, p=1, d=1, groups=1),       # 3 -> 64 on 8x8 (compile-time specs: band kernels)
    "small_planes": dict(B=16, C=16, O=128, H=4, W=4, k=3, s=1, p=1, d=1, groups=1),    # 16 -> 128 on 4x4, B = 16: position-major
    "tap_major": dict(B=2, C=8, O=8, H=6, W=6, k=3, s=2, p=1, d=1, groups=2),
    "depthwise": dict(B=2, C=4, O=4, H=6, W=6, k=3, s=1, p=1, d=1, groups=4),
}
FAMILIES = {"lucas": dict(kind="lucas", degree=9), "cheby": dict(kind="cheby", degree=9), "fourier": dict(kind="fourier", degree=6)}


@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_forced_windows_on_every_generic_route(fam, geom, gpu_lib):
    torch.manual_seed(3)
    c = dict(GEOMS[geom], **FAMILIES[fam])
    layer = build_layer(c)
    assert len(layer._plane_windows()) == 1
    layer.plane_window = 4
    wins = layer._plane_windows()
    assert len(wins) >= 3 and sum(w[0].first > 0 for w in wins) == len(wins) - 1
    G = c["groups"]
    for spec, _, _, _ in wins:
        if spec.first == 0:
            continue            # the first window IS a small layer of its family and may have a compile-time spec (ChebyKAN degree 3: band kernels)
        g_, _, plan = ops._plan_cached(spec, c["B"], c["C"] // G, c["H"], c["W"], c["O"] // G, c["C"], c["O"])
        flags = (plan.fwd_halo, plan.fwd_band, plan.fwd_expanded, plan.bwd_weight_halo, plan.bwd_weight_band, plan.bwd_weight_expanded, plan.e_pm_wanted)
        assert flags == (0,) * 7, flags                                      # no compile-time-spec route for a window
        direct = plan.bwd_data_weight_bytes == plan.packed_weight_bytes      # the direct depthwise kernels read ONE weight layout
        if geom == "few_channels":
            assert plan.Opad == 64 and not plan.x_pm_wanted and not direct   # tap-major kernels, 64-output tiles
        elif geom == "small_planes":
            assert plan.x_pm_wanted == 1 and plan.dz_pm_wanted == 1 and plan.bwd_weight_target > 0      # position-major, dead taps skipped
        elif geom == "tap_major":
            assert not plan.x_pm_wanted and not plan.dz_pm_wanted and not direct and g_.groups == 2
        else:
            assert direct and g_.C == 1 and plan.fwd_splits == 1             # direct depthwise kernels (the array form of the functors)
    x = torch.randn(c["B"], c["C"], c["H"], c["W"])
    check_vs_oracle(layer, c, x, groups=G, tag=f"{fam} {geom} windows of 4")


# ------------------------------------------------------------------------------------------------------------------ 4. untouched below the limits
# The plan of the layer's own spec on 16 -> 128 @ 8x8, B = 32, as the commit before plane windows gives it (recorded from a run of that
# commit): (P, IPC, KC, Kpad, fwd_splits, bwd_data_splits, bwd_weight_splits, fwd_halo, fwd_band, bwd_weight_halo, bwd_weight_band).
# IPC / KC / the halo and band flags are what the compile-time variant of the spec decides.
PARENT_PLANS = {
    "lucas3": (5, 2, 10, 720, 8, 9, 8, 1, 0, 0, 0),          # FAST_POLY4: pair order of the halo forward
    "fourier5": (11, 1, 12, 1728, 18, 9, 8, 0, 0, 0, 0),     # generic
    "cheby4": (5, 2, 10, 720, 8, 9, 32, 0, 1, 0, 1),         # FAST_CHEBY5: band kernels
    "bspline": (9, 2, 18, 1296, 8, 9, 32, 1, 0, 1, 0),       # FAST_BSPLINE_GELU: halo forward and weight gradient
}


def test_layers_below_the_limits_are_untouched(gpu_lib):
    layers = {"lucas3": K.LucasKANConv2DLayer(16, 128, 3, degree=3, padding=1), "fourier5": K.FourierKANConv2DLayer(16, 128, 3, grid_size=5, padding=1),
              "cheby4": K.ChebyKANConv2DLayer(16, 128, 3, degree=4, padding=1), "bspline": K.KANConv2DLayer(16, 128, 3, padding=1)}
    ops._TABLES.clear()
    for name, layer in layers.items():
        spec = layer.conv_spec()
        assert spec.first == 0 and not ops._device_table(spec)
        assert len(layer._plane_windows()) == 1 and layer._plane_windows()[0][0] == spec
        _, basis, p = ops._plan_cached(spec, 32, 16, 8, 8, 128, 16, 128)
        assert basis.order == spec.order and not basis.chan_table
        got = (p.P, p.IPC, p.KC, p.Kpad, p.fwd_splits, p.bwd_data_splits, p.bwd_weight_splits, p.fwd_halo, p.fwd_band, p.bwd_weight_halo, p.bwd_weight_band)
        assert got == PARENT_PLANS[name], (name, got)
        assert (p.x_pm_wanted, p.dz_pm_wanted, p.e_pm_wanted, p.fwd_expanded, p.bwd_weight_expanded, p.row_blocks) == (0,) * 6
        layer = layer.cuda()
        x = torch.randn(32, 16, 8, 8, device="cuda", requires_grad=True)
        layer(x).sum().backward()
    torch.cuda.synchronize()
    assert not ops._TABLES                                   # no device coefficient table was created for any of them

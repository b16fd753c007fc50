"""CPU: the host side of the OPT-IN split-precision weight gradient (kan_conv_bwd_weight_split) -- the two exports, the workspace size
against a restatement of the layout the header documents, refusals that need no device, and the arithmetic itself emulated in torch on real plane values (the
context switches: tests/test_split_host.py): three bf16 pieces per operand and the kernel's six products (summed smallest first) against fp64, next to the three-product form that is
NOT enough."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import convkan_amd as K
from convkan_amd import _lib as L
from conftest import ROOT
from split_cells import OUT_OF_SCOPE
from split_cells import geom_basis as _gb

NEW = ("kan_split_bwd_weight_workspace_bytes", "kan_conv_bwd_weight_split")


def test_two_symbols_declared_bound_and_exported():
    K.build_library()
    header = open(os.path.join(ROOT, "include", "kanconv.h")).read()
    declared = set(re.findall(r"\b(kan_[a-z_]+)\s*\(", header))
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(raw, name), name


@pytest.mark.parametrize("C_,O_,PW,B", [(8, 128, 8, 2), (16, 128, 8, 34), (64, 128, 16, 256), (128, 256, 8, 256), (256, 256, 8, 256), (24, 128, 16, 3), (8, 128, 16, 1)])
def test_workspace_bytes_restate_the_layout(C_, O_, PW, B):
    lib = L.load()
    g, b = _gb(C_, O_, PW, B=B)
    octets = -(-B // 8)                                      # images are the inner depth index: 8 per 16-byte chunk, the tail padded with zeros
    dzc = octets * PW * PW * 3 * O_ * 8 * 2                  # [octet][pixel][piece][o][8 bf16]
    units = octets * (1 if PW == 8 else 4)                   # depth units of 64 pixels x 8 images
    ks = min(32, -(-512 // (C_ * (O_ // 128))), units)       # depth splits: workgroups for two rounds of 256 CUs, at most one per unit
    part = ks * O_ * C_ * 81 * 4                             # [KS][O][C][9 planes x 9 taps] floats
    got = lib.kan_split_bwd_weight_workspace_bytes(C.byref(g), C.byref(b))
    assert got == dzc + part and got > 0
    assert lib.kan_split_supported(C.byref(g), C.byref(b)) == 1


def test_out_of_scope_and_null_pointers_are_refused_without_a_device():
    lib = L.load()
    fake = C.c_void_p(4096)                      # never dereferenced: the refusal is host arithmetic before any launch
    for kw in OUT_OF_SCOPE:
        g, b = _gb(**kw)
        assert lib.kan_split_bwd_weight_workspace_bytes(C.byref(g), C.byref(b)) == 0, kw
        assert lib.kan_conv_bwd_weight_split(fake, fake, fake, fake, fake, C.byref(g), C.byref(b), None) != 0, kw
        assert b"split-precision" in lib.kan_last_error()
    g, b = _gb(16, 128, 8)
    for hole in range(5):
        args = [fake] * 5
        args[hole] = None
        assert lib.kan_conv_bwd_weight_split(*args, C.byref(g), C.byref(b), None) != 0
        assert b"null pointer" in lib.kan_last_error()
    assert lib.kan_split_bwd_weight_workspace_bytes(None, None) == 0
    args = [fake] * 4 + [C.c_void_p(4096 + 8)]          # the header asks for a 16-byte aligned workspace (16-byte stores of the dz cut)
    assert lib.kan_conv_bwd_weight_split(*args, C.byref(g), C.byref(b), None) != 0
    assert b"16-byte aligned" in lib.kan_last_error()


def _cut3(v):
    """fp32 -> three bf16 pieces (round to nearest even), as split_pair / split3 of csrc/kan_split.hip; returned widened to fp32."""
    h = v.bfloat16().float()
    r = v - h
    m = r.bfloat16().float()
    lo = (r - m).bfloat16().float()
    return h, m, lo


@pytest.mark.parametrize("C_,O_,B,PW", [(8, 128, 2, 8), (16, 128, 1, 16), (8, 128, 34, 8)])
def test_six_products_reach_fp32_and_three_do_not(C_, O_, B, PW):
    """dW = wgrad(dz, planes(x)) over all 9 planes (SiLU + the eight cubic B-splines of the default grid), x = 1.5 randn.  The kernel's six products, summed
    smallest first, sit at the fp32 rounding floor (measured 1.6e-7 .. 4.0e-7 max-normalised against fp64); hi*hi + hi*mid + mid*hi alone stops at
    3.6 .. 5.5e-6.  Asserted: six <= 1e-6 < three."""
    from oracle import kan_oracle as O
    torch.manual_seed(C_ + PW + B)
    x = 1.5 * torch.randn(B, C_, PW, PW)
    dz = torch.randn(B, O_, PW, PW)
    knots = O.bspline_knots(5, 3, [-1, 1])
    planes = torch.cat([F.silu(x).unsqueeze(2), O.bspline_basis(x, knots, 3).permute(0, 1, 4, 2, 3)], dim=2).reshape(B, C_ * 9, PW, PW)
    # dW[o][k][r][t] = sum_b,h,w dz[b,o,h,w] E[b,k,h+r-1,w+t-1]: a convolution with the batch as the contracted channel axis
    wgrad = lambda e, d: F.conv2d(e.transpose(0, 1), d.transpose(0, 1), padding=1).transpose(0, 1)
    ref = wgrad(planes.double(), dz.double())
    assert tuple(ref.shape) == (O_, C_ * 9, 3, 3)
    (dh, dm, dl), (eh, em, el) = _cut3(dz), _cut3(planes)
    # A = dz, B = plane values; the kernel's order: lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi
    six = wgrad(eh, dl)
    for d, e in ((dh, el), (dm, em), (dm, eh), (dh, em), (dh, eh)):
        six = six + wgrad(e, d)
    three = wgrad(em, dh) + wgrad(eh, dm) + wgrad(eh, dh)
    scale = float(ref.abs().max())
    e6 = float((six.double() - ref).abs().max()) / scale
    e3 = float((three.double() - ref).abs().max()) / scale
    print(f"[split bwd-weight emulation {C_}->{O_} @{PW}x{PW} B={B}] six products {e6:.2e}  three products {e3:.2e}")
    assert e6 <= 1e-6 < e3, (e6, e3)

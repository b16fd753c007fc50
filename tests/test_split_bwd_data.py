"""CPU: the host side of the OPT-IN split-precision input gradient (kan_conv_bwd_data_split) -- the three exports, the byte count of
the cut weights against a restatement of their layout, refusals that need no device, and the arithmetic itself emulated in torch (the context switch:
tests/test_split_host.py):
three bf16 pieces per operand and the kernel's six products (summed smallest first) against fp64, next to the three-product form that is NOT enough."""
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

NEW = ("kan_split_bwd_data_weight_bytes", "kan_split_pack_weights_bwd_data", "kan_conv_bwd_data_split")


def test_three_symbols_declared_bound_and_exported():
    K.build_library()
    header = open(os.path.join(ROOT, "include", "kanconv.h")).read()
    declared = set(re.findall(r"\b(kan_[a-z_]+)\s*\(", header))
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(raw, name), name


@pytest.mark.parametrize("C_,O_,PW", [(8, 128, 8), (16, 128, 8), (64, 128, 16), (256, 256, 8)])
def test_cut_weight_bytes_restate_the_layout(C_, O_, PW):
    lib = L.load()
    g, b = _gb(C_, O_, PW)
    row_tiles = -(-C_ // 14)                    # 128 rows = two 64-row halves of 7 channels x 9 planes
    steps = (O_ // 16) * 9                      # per 16 output channels: 9 taps, each one 16-deep step (two o-octets)
    want = row_tiles * steps * 3 * 2 * 128 * 8 * 2      # [row tile][step][piece][k-half][row][8 bf16]
    assert lib.kan_split_bwd_data_weight_bytes(C.byref(g), C.byref(b)) == want
    assert lib.kan_split_supported(C.byref(g), C.byref(b)) == 1


def test_out_of_scope_and_null_pointers_are_refused_without_a_device():
    lib = L.load()
    fake = C.c_void_p(4096)                      # never dereferenced: the refusal is host arithmetic before any launch
    for kw in OUT_OF_SCOPE:
        g, b = _gb(**kw)
        assert lib.kan_split_bwd_data_weight_bytes(C.byref(g), C.byref(b)) == 0, kw
        assert lib.kan_split_pack_weights_bwd_data(fake, fake, fake, C.byref(g), C.byref(b), None) != 0, kw
        assert b"split-precision" in lib.kan_last_error()
        assert lib.kan_conv_bwd_data_split(fake, fake, fake, fake, C.byref(g), C.byref(b), None) != 0, kw
        assert b"split-precision" in lib.kan_last_error()
    g, b = _gb(16, 128, 8)
    for hole in range(3):
        args = [fake] * 3
        args[hole] = None
        assert lib.kan_split_pack_weights_bwd_data(*args, C.byref(g), C.byref(b), None) != 0
        assert b"null pointer" in lib.kan_last_error()
    for hole in range(4):
        args = [fake] * 4
        args[hole] = None
        assert lib.kan_conv_bwd_data_split(*args, C.byref(g), C.byref(b), None) != 0
        assert b"null pointer" in lib.kan_last_error()
    assert lib.kan_split_bwd_data_weight_bytes(None, None) == 0


def _cut3(v):
    """fp32 -> three bf16 pieces (round to nearest even), as split_pair / split3 of csrc/kan_split.hip; returned widened to fp32."""
    h = v.bfloat16().float()
    r = v - h
    m = r.bfloat16().float()
    lo = (r - m).bfloat16().float()
    return h, m, lo


@pytest.mark.parametrize("C_,O_,B,PW", [(8, 128, 2, 8), (16, 256, 2, 8), (16, 128, 1, 16)])
def test_six_products_reach_fp32_and_three_do_not(C_, O_, B, PW):
    """G = dgrad(dz, W) over all 9 planes.  The kernel's six products, summed smallest first, sit at the fp32 rounding floor (measured 1.2e-7 .. 2.3e-7
    max-normalised against fp64); hi*hi + hi*mid + mid*hi alone stops at 4 .. 5.5e-6.  Asserted: six <= 1e-6 < three -- the six products are needed, and the
    arithmetic leaves a factor of ten under TOL_DX = 1e-5."""
    torch.manual_seed(C_ + PW)
    dz = torch.randn(B, O_, PW, PW)
    w = torch.randn(O_, C_ * 9, 3, 3) / (C_ * 9) ** 0.5
    ref = F.conv_transpose2d(dz.double(), w.double(), padding=1)
    (dh, dm, dl), (wh, wm, wl) = _cut3(dz), _cut3(w)
    prod = lambda a, b_: F.conv_transpose2d(a, b_, padding=1)
    # A = weights, B = dz; the kernel's order: lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi
    six = prod(dh, wl)
    for a, b_ in ((dl, wh), (dm, wm), (dh, wm), (dm, wh), (dh, wh)):
        six = six + prod(a, b_)
    three = prod(dh, wm) + prod(dm, wh) + prod(dh, wh)
    scale = float(ref.abs().max())
    e6 = float((six.double() - ref).abs().max()) / scale
    e3 = float((three.double() - ref).abs().max()) / scale
    print(f"[split bwd-data emulation {C_}->{O_} @{PW}x{PW} B={B}] six products {e6:.2e}  three products {e3:.2e}")
    assert e6 <= 1e-6 < e3, (e6, e3)

"""Shared by test_heads.py (CPU) and test_gpu_heads.py: the fixtures of tests/golden/heads (make_golden_heads.py), the modules they
describe, and an fp64 evaluation of a layer's basis straight from the coefficient table it hands to ConvSpec."""
import json
import os

import numpy as np
import torch

from conftest import GOLDEN

HEADS = os.path.join(GOLDEN, "heads")
LAYER = {"cheby": "ChebyKANLayer", "bessel": "BesselKANLayer", "fibonacci": "FibonacciKANLayer", "gegenbauer": "GegenbauerKANLayer",
         "hermite": "HermiteKANLayer", "laguerre": "LaguerreKANLayer", "lucas": "LucasKANLayer"}
FACTORY = {"cheby": "mlp_chebykan", "bessel": "mlp_besselkan", "fibonacci": "mlp_fibonaccikan", "gegenbauer": "mlp_gegenbauerkan",
           "hermite": "mlp_hermitekan", "laguerre": "mlp_laguerrekan", "lucas": "mlp_lucaskan"}
KEYS = {"cheby": "ChebyKAN", "bessel": "BesselKAN", "fibonacci": "FibonacciKAN", "gegenbauer": "GegenbauerKAN", "hermite": "HermiteKAN",
        "laguerre": "LaguerreKAN", "lucas": "LucasKAN"}
COEFFS = {"cheby": "cheby_coeffs", "bessel": "bessel_coeffs", "fibonacci": "fib_coeffs", "gegenbauer": "gegenbauer_coeffs",
          "hermite": "hermite_coeffs", "laguerre": "laguerre_coeffs", "lucas": "lucas_coeffs"}
REFUSED = ("FastKAN", "LegendreKAN", "BersnsteinKAN", "JacobiKAN", "GRAMKAN", "FourierKAN", "ReLUKAN", "TaylorKAN", "WavKAN")


def head_cases(kind=None):
    names = sorted(fn[:-4] for fn in os.listdir(HEADS) if fn.endswith(".npz"))
    return [n for n in names if kind is None or (n.endswith("_mlp_l1") == (kind == "model"))]


_CACHE = {}


def load_head(name):
    """The fixture as {key: array}, cfg decoded; loaded once and shared (callers do not modify it)."""
    if name not in _CACHE:
        d = dict(np.load(os.path.join(HEADS, name + ".npz")))
        d["cfg"] = json.loads(bytes(d["cfg"]).decode())
        _CACHE[name] = d
    return _CACHE[name]


def build_head(cfg):
    """This package's module for a fixture's cfg, with default-initialised parameters."""
    import convkan_amd as K
    if cfg["kind"] == "model":
        return getattr(K, FACTORY[cfg["family"]])(cfg["layers_hidden"], l1_decay=cfg["l1_decay"], degree=cfg["degree"], **cfg["extra"])
    return getattr(K, LAYER[cfg["family"]])(cfg["I"], cfg["O"], cfg["degree"], **cfg["extra"])


def state_dict_of(d):
    return {k[3:]: torch.from_numpy(v) for k, v in d.items() if k.startswith("sd.")}


def basis_fp64(spec, x):
    """[B, I, n] planes of `spec` at x in fp64, by the definitions of include/kanconv.h: Chebyshev T_k = cos(k acos(clamp(tanh x, p0, p1)));
    Poly T_0 = c0, T_1 = a1 t + b1, T_k = (A_k t + B_k) T_{k-1} + C_k T_{k-2} on t = tanh x, the table entries as the layer states them (Python floats: the kernels get
    their fp32 roundings)."""
    import convkan_amd as K
    t = torch.tanh(x.double())
    if spec.kind == K._lib.BASIS_CHEBY:
        th = torch.acos(t.clamp(spec.p0, spec.p1))
        return torch.stack([torch.cos(k * th) for k in range(spec.n_basis)], dim=-1)
    assert spec.kind == K._lib.BASIS_POLY and spec.order == 1
    tab = list(spec.table)
    planes = [torch.full_like(t, tab[0]), tab[1] * t + tab[2]]
    for k in range(2, spec.n_basis):
        a, b, c = tab[3 * k - 3: 3 * k]
        planes.append((a * t + b) * planes[-1] + c * planes[-2])
    return torch.stack(planes[:spec.n_basis], dim=-1)

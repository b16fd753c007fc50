"""MLP KAN heads with one coefficient tensor: ChebyKAN and the six three-term-recurrence families.

  reference                                              this file
  layers/cheby_kan_layers.py:5-38        ChebyKANLayer        ChebyKANLayer
  layers/bessel_kan_layers.py:8-37       BesselKANLayer       BesselKANLayer
  layers/fibonacci_kan_layers.py:8-39    FibonacciKANLayer    FibonacciKANLayer
  layers/gegenbauer_kan_layers.py:7-33   GegenbauerKANLayer   GegenbauerKANLayer
  layers/hermite_kan_layers.py:7-29      HermiteKANLayer      HermiteKANLayer
  layers/laguerre_kan_layers.py:7-37     LaguerreKANLayer     LaguerreKANLayer
  layers/lucas_kan_layers.py:8-39        LucasKANLayer        LucasKANLayer
  models/kans.py:58-105, 153-222, 250-272, 329-401, 505-542   the seven models and their mlp_* factories

All seven compute  y = einsum('bid,iod->bo', basis_d(tanh x), coeffs[I, O, degree + 1])  with no base branch, norm or bias: the conv
stage of the HIP kernels on a [B, I, 1, 1] view with a 1x1 kernel (as KANLayer, mlp_layers.py), the basis evaluated in the kernels
(KAN_BASIS_CHEBY / KAN_BASIS_POLY with act = KAN_ACT_NONE).  The coefficient tensor keeps the reference's input-major layout, name and
state_dict key; `ConvSpec.w_layout = W_IOD` makes the conv op pack it and return its gradient in that layout (kan_pack_weights_iod /
kan_unpack_wgrad_iod), so no permuted copy of a head's weights is ever made.

One launch holds KAN_MAX_PLANES planes, so degree + 1 <= 16 (plane windows for heads are not built); 12 planes and up carry the
recurrence coefficients as a device table, as the conv layers do.  CPU tensors raise: there is no fallback.
"""
from __future__ import annotations

from typing import List

import numpy as np
import torch
import torch.nn as nn

from .. import _lib as L
from .. import ops
from ..utils.regularization import L1
from .poly_layers import (BesselKANConvNDLayer, FibonacciKANConvNDLayer, GegenbauerKANConvNDLayer, HermiteKANConvNDLayer,
                          LaguerreKANConvNDLayer, LucasKANConvNDLayer, _table)


class _CoeffKANLayer(nn.Module):
    """Shared body: one parameter `<_coeffs_name>` [input_dim, output_dim, degree + 1], init normal_(0, 1 / (input_dim (degree + 1)))."""
    _coeffs_name = ""

    def _make_coeffs(self, input_dim: int, output_dim: int, degree: int) -> None:
        if degree < 1:
            raise ValueError(f"{type(self).__name__} on the HIP path needs degree >= 1, got {degree}")
        if degree + 1 > L.KAN_MAX_PLANES:
            raise NotImplementedError(f"{type(self).__name__}: degree + 1 = {degree + 1} planes exceed KAN_MAX_PLANES = {L.KAN_MAX_PLANES}, the most one "
                                      f"launch holds (degree <= {L.KAN_MAX_PLANES - 1}); plane windows are not built for the MLP heads")
        self._io = (input_dim, output_dim)
        coeffs = nn.Parameter(torch.empty(input_dim, output_dim, degree + 1))
        nn.init.normal_(coeffs, mean=0.0, std=1 / (input_dim * (degree + 1)))
        setattr(self, self._coeffs_name, coeffs)

    def _coeffs(self):
        """(c0, a1, b1, [(A_k, B_k, C_k), k = 2..degree]) of T_0 = c0, T_1 = a1 t + b1, T_k = (A_k t + B_k) T_{k-1} + C_k T_{k-2}."""
        raise NotImplementedError

    def _basis_kw(self) -> dict:
        n = self.degree + 1
        return dict(kind=L.BASIS_POLY, n_basis=n, order=1, act=L.ACT_NONE, p0=0.0, p1=0.0, table=_table(self._coeffs(), n))

    def conv_spec(self) -> ops.ConvSpec:
        return ops.ConvSpec(**self._basis_kw(), kernel=(1, 1), stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1, w_layout=ops.W_IOD)

    def forward(self, x):
        i, o = self._io
        x = x.reshape(-1, i)
        z = ops.kan_conv(self.conv_spec(), x.reshape(x.shape[0], i, 1, 1), None, [], [getattr(self, self._coeffs_name)])
        return z.view(-1, o)


class ChebyKANLayer(_CoeffKANLayer):
    """T_k(t) = cos(k acos(clamp(t, -1 + 1e-7, 1 - 1e-7))), t = tanh x  (cheby_kan_layers.py:22-32); `arange` is a buffer there, so it is one here."""
    _coeffs_name = "cheby_coeffs"

    def __init__(self, input_dim: int, output_dim: int, degree: int):
        super().__init__()
        self.input_dim, self.output_dim, self.degree = input_dim, output_dim, degree
        self.epsilon = 1e-7
        self._make_coeffs(input_dim, output_dim, degree)
        self.register_buffer("arange", torch.arange(0, degree + 1, 1))

    def _basis_kw(self):
        lo, hi = float(np.float32(-1 + self.epsilon)), float(np.float32(1 - self.epsilon))     # torch.clamp casts its Python-float bounds to fp32
        return dict(kind=L.BASIS_CHEBY, n_basis=self.degree + 1, order=0, act=L.ACT_NONE, p0=lo, p1=hi, table=())


# The six recurrences below are the ones the conv classes of the same families run (poly_layers.py), so their coefficient tables are reused;
# tests/test_heads.py evaluates each table in fp64 against the reference MLP layer's own output.
class BesselKANLayer(_CoeffKANLayer):
    """y_0 = 1, y_1 = t + 1, y_i = (2i - 1) t y_{i-1} + y_{i-2}  (bessel_kan_layers.py:28-32)."""
    _coeffs_name = "bessel_coeffs"
    _coeffs = BesselKANConvNDLayer._coeffs

    def __init__(self, input_dim, output_dim, degree):
        super().__init__()
        self.input_dim, self.output_dim, self.degree = input_dim, output_dim, degree
        self._make_coeffs(input_dim, output_dim, degree)


class FibonacciKANLayer(_CoeffKANLayer):
    """F_0 = 0, F_1 = 1, F_i = t F_{i-1} + F_{i-2}  (fibonacci_kan_layers.py:24-31).  At degree 1 the basis does not depend on x: dx is zero."""
    _coeffs_name = "fib_coeffs"
    _coeffs = FibonacciKANConvNDLayer._coeffs

    def __init__(self, input_dim, output_dim, degree):
        super().__init__()
        self.input_dim, self.output_dim, self.degree = input_dim, output_dim, degree
        self._make_coeffs(input_dim, output_dim, degree)


class GegenbauerKANLayer(_CoeffKANLayer):
    """C_0 = 1, C_1 = 2 a t, (n + 1) C_{n+1} = 2 (n + a) t C_n - (n + 2a - 1) C_{n-1}  (gegenbauer_kan_layers.py:23-30).  With the models'
    default a = 0 every plane above the first is zero, as in the reference."""
    _coeffs_name = "gegenbauer_coeffs"
    _coeffs = GegenbauerKANConvNDLayer._coeffs

    def __init__(self, input_dim, output_dim, degree, alpha_param):
        super().__init__()
        self.input_dim, self.output_dim, self.degree, self.alpha_param = input_dim, output_dim, degree, alpha_param
        self._make_coeffs(input_dim, output_dim, degree)


class HermiteKANLayer(_CoeffKANLayer):
    """H_0 = 1, H_1 = 2t, H_i = 2t H_{i-1} - 2 (i - 1) H_{i-2}  (hermite_kan_layers.py:22-26; the attribute is `out_dim` there)."""
    _coeffs_name = "hermite_coeffs"
    _coeffs = HermiteKANConvNDLayer._coeffs

    def __init__(self, input_dim, output_dim, degree):
        super().__init__()
        self.input_dim, self.out_dim, self.degree = input_dim, output_dim, degree
        self._make_coeffs(input_dim, output_dim, degree)


class LaguerreKANLayer(_CoeffKANLayer):
    """L_0 = 1, L_1 = 1 + a - t, k L_k = (2 (k - 1) + 1 + a - t) L_{k-1} - (k - 1 + a) L_{k-2}  (laguerre_kan_layers.py:22-30)."""
    _coeffs_name = "laguerre_coeffs"
    _coeffs = LaguerreKANConvNDLayer._coeffs

    def __init__(self, input_dim, output_dim, degree, alpha):
        super().__init__()
        self.input_dim, self.output_dim, self.degree, self.alpha = input_dim, output_dim, degree, alpha
        self._make_coeffs(input_dim, output_dim, degree)


class LucasKANLayer(_CoeffKANLayer):
    """L_0 = 2, L_1 = t, L_i = t L_{i-1} + L_{i-2}  (lucas_kan_layers.py:24-31)."""
    _coeffs_name = "lucas_coeffs"
    _coeffs = LucasKANConvNDLayer._coeffs

    def __init__(self, input_dim, output_dim, degree):
        super().__init__()
        self.input_dim, self.output_dim, self.degree = input_dim, output_dim, degree
        self._make_coeffs(input_dim, output_dim, degree)


# ------------------------------------------------------------------------------------------- models
class _CoeffKAN(nn.Module):
    """Stack of one family's layers as models/kans.py builds it: an optional first Dropout, every layer but the last wrapped in
    utils.regularization.L1 when l1_decay > 0, a Dropout after every layer but the last."""
    _layer = None

    def _stack(self, layers_hidden, dropout, l1_decay, degree, first_dropout, *layer_args):
        self.layers_hidden, self.polynomial_order = layers_hidden, degree
        self.layers = nn.ModuleList([])
        self.num_layers = len(layers_hidden[:-1])
        if dropout > 0 and first_dropout:
            self.layers.append(nn.Dropout(p=dropout))
        for i, (fin, fout) in enumerate(zip(layers_hidden[:-1], layers_hidden[1:])):
            layer, last = self._layer(fin, fout, degree, *layer_args), i == self.num_layers - 1
            self.layers.append(L1(layer, l1_decay) if l1_decay > 0 and not last else layer)
            if dropout > 0 and not last:
                self.layers.append(nn.Dropout(p=dropout))

    def forward(self, x):
        for layer in self.layers:
            x = layer(x)
        return x


class _DegreeKAN(_CoeffKAN):
    def __init__(self, layers_hidden, dropout: float = 0.0, l1_decay: float = 0.0, degree: int = 3, first_dropout: bool = True, **kwargs):
        super().__init__()
        self._stack(layers_hidden, dropout, l1_decay, degree, first_dropout)


class ChebyKAN(_DegreeKAN):
    _layer = ChebyKANLayer


class BesselKAN(_DegreeKAN):
    _layer = BesselKANLayer


class FibonacciKAN(_DegreeKAN):
    _layer = FibonacciKANLayer


class HermiteKAN(_DegreeKAN):
    _layer = HermiteKANLayer


class LucasKAN(_DegreeKAN):
    _layer = LucasKANLayer


class GegenbauerKAN(_CoeffKAN):
    _layer = GegenbauerKANLayer

    def __init__(self, layers_hidden, dropout: float = 0.0, l1_decay: float = 0.0, degree: int = 3, alpha_param: float = 0.0,
                 first_dropout: bool = True, **kwargs):
        super().__init__()
        self._stack(layers_hidden, dropout, l1_decay, degree, first_dropout, alpha_param)


class LaguerreKAN(_CoeffKAN):
    _layer = LaguerreKANLayer

    def __init__(self, layers_hidden, dropout: float = 0.0, l1_decay: float = 0.0, degree: int = 3, alpha: float = 0.0,
                 first_dropout: bool = True, **kwargs):
        super().__init__()
        self.alpha = alpha
        self._stack(layers_hidden, dropout, l1_decay, degree, first_dropout, alpha)


def mlp_chebykan(layers_hidden: List[int], dropout: float = 0.0, degree: int = 3, l1_decay: float = 0.0, first_dropout: bool = True) -> ChebyKAN:
    return ChebyKAN(layers_hidden, dropout=dropout, degree=degree, l1_decay=l1_decay, first_dropout=first_dropout)


def mlp_besselkan(layers_hidden: List[int], dropout: float = 0.0, degree: int = 3, l1_decay: float = 0.0, first_dropout: bool = True) -> BesselKAN:
    return BesselKAN(layers_hidden, dropout=dropout, degree=degree, l1_decay=l1_decay, first_dropout=first_dropout)


def mlp_fibonaccikan(layers_hidden: List[int], dropout: float = 0.0, degree: int = 3, l1_decay: float = 0.0,
                     first_dropout: bool = True) -> FibonacciKAN:
    return FibonacciKAN(layers_hidden, dropout=dropout, degree=degree, l1_decay=l1_decay, first_dropout=first_dropout)


def mlp_gegenbauerkan(layers_hidden: List[int], dropout: float = 0.0, degree: int = 3, l1_decay: float = 0.0, alpha_param: float = 0.0,
                      first_dropout: bool = True) -> GegenbauerKAN:
    return GegenbauerKAN(layers_hidden, dropout=dropout, degree=degree, l1_decay=l1_decay, alpha_param=alpha_param, first_dropout=first_dropout)


def mlp_hermitekan(layers_hidden: List[int], dropout: float = 0.0, degree: int = 3, l1_decay: float = 0.0, first_dropout: bool = True) -> HermiteKAN:
    return HermiteKAN(layers_hidden, dropout=dropout, degree=degree, l1_decay=l1_decay, first_dropout=first_dropout)


def mlp_laguerrekan(layers_hidden: List[int], dropout: float = 0.0, degree: int = 3, l1_decay: float = 0.0, alpha: float = 0.0,
                    first_dropout: bool = True) -> LaguerreKAN:
    return LaguerreKAN(layers_hidden, dropout=dropout, degree=degree, l1_decay=l1_decay, alpha=alpha, first_dropout=first_dropout)


def mlp_lucaskan(layers_hidden: List[int], dropout: float = 0.0, degree: int = 3, l1_decay: float = 0.0, first_dropout: bool = True) -> LucasKAN:
    return LucasKAN(layers_hidden, dropout=dropout, degree=degree, l1_decay=l1_decay, first_dropout=first_dropout)


HEAD_FACTORY = {"ChebyKAN": mlp_chebykan, "BesselKAN": mlp_besselkan, "FibonacciKAN": mlp_fibonaccikan, "GegenbauerKAN": mlp_gegenbauerkan,
                "HermiteKAN": mlp_hermitekan, "LaguerreKAN": mlp_laguerrekan, "LucasKAN": mlp_lucaskan}

"""Drop-in conv-KAN layers: same constructor signatures, attribute names, parameter order and
state_dict keys as the reference classes, with forward/backward on the libkanconv HIP kernels.

  reference class                                   this file
  layers/kan_layers.py:116-258  KANConvNDLayer       KANConvNDLayer
  layers/kan_layers.py:274-284  KANConv2DLayer       KANConv2DLayer
  layers/fast_kan_layers.py:34-120 / :137-148        FastKANConvNDLayer / FastKANConv2DLayer
  layers/cheby_kan_layers.py:39-111 / :124-131       ChebyKANConvNDLayer / ChebyKANConv2DLayer
  utils/utils.py:19-33          RadialBasisFunction  RadialBasisFunction

The ``nn.Conv2d`` children are weight holders only (their forward is never called): keeping them
preserves ``state_dict`` keys (``base_conv.0.weight`` ...), lets ``load_state_dict`` move weights
between this package and the reference in both directions, and keeps callers that walk
``.modules()`` for ``nn.Conv2d`` (models/kan_alexnet.py:236-241) working.

The 2-D layers are the hot path.  The 1-D shims (KANConv1DLayer, FastKANConv1DLayer, ChebyKANConv1DLayer:
kan_layers.py:287-297, fast_kan_layers.py:151-162, cheby_kan_layers.py:134-141) run on the same kernels by viewing
[B, C, L] as [B, C, 1, L] with a (1, k) kernel; the 3-D shims (kan_layers.py:261-271 and siblings) run one 2-D launch set per
depth tap (conv3d_stage).
"""
from __future__ import annotations

from inspect import signature
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib as L
from .. import ops


def _pair(v):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"expected an int or a pair, got {v!r}")
        return int(v[0]), int(v[1])
    return int(v), int(v)


_ACT_CODES = {nn.Identity: L.ACT_IDENTITY, nn.SiLU: L.ACT_SILU, nn.ReLU: L.ACT_RELU, nn.Tanh: L.ACT_TANH, nn.Sigmoid: L.ACT_SIGMOID}


def _act_code(module: nn.Module, host_ok: bool = False) -> int:
    """Map the instantiated ``base_activation`` module to a kernel activation id.  A module without a device functor is
    applied by the host (``_HipLayer._base_input``) where the layer supports that (`host_ok`): the kernels then see the
    activated tensor as their base-branch input with the identity functor, and the raw input as the basis tensor."""
    if type(module) is nn.GELU:
        return L.ACT_GELU_TANH if getattr(module, "approximate", "none") == "tanh" else L.ACT_GELU
    code = _ACT_CODES.get(type(module))
    if code is None:
        if host_ok:
            return L.ACT_IDENTITY
        raise NotImplementedError(
            f"base_activation {type(module).__name__} has no HIP functor yet (supported: Identity/None, GELU, SiLU, ReLU, Tanh, Sigmoid)")
    return code


def _host_applied(module: nn.Module) -> bool:
    return type(module) is not nn.GELU and type(module) not in _ACT_CODES


def _unfused_pool(y, pool):
    """max_pool2d for the `pool` argument of the layers' forward: True = (2, 2), or a (kernel, stride) pair."""
    k, st = (2, 2) if pool is True else (int(pool[0]), int(pool[1]))
    return F.max_pool2d(y, k, st)


def _dropout2d(p: float, ndim: int = 2):
    if p <= 0:
        return None
    return nn.Dropout1d(p=p) if ndim == 1 else nn.Dropout3d(p=p) if ndim == 3 else nn.Dropout2d(p=p)


def _check_groups(groups, input_dim, output_dim):
    # kan_layers.py:148-153 (same messages in the sibling classes)
    if groups <= 0:
        raise ValueError('groups must be a positive integer')
    if input_dim % groups != 0:
        raise ValueError('input_dim must be divisible by groups')
    if output_dim % groups != 0:
        raise ValueError('output_dim must be divisible by groups')


def _filter_norm_kwargs(norm_class, norm_kwargs):
    valid = signature(norm_class).parameters          # kan_layers.py:178-179
    return {k: v for k, v in norm_kwargs.items() if k in valid}


def _fusable_instnorm(mods) -> bool:
    """True when every per-group norm is a plain InstanceNorm1d/2d (instance statistics in train and eval)."""
    return all(type(m) in (nn.InstanceNorm2d, nn.InstanceNorm1d) and not m.track_running_stats for m in mods)


def _fusable_batchnorm(mods) -> bool:
    """True when every per-group norm is a plain BatchNorm1d/2d/3d whose momentum is a number (None, the cumulative average, stays with
    torch) and the groups share eps, momentum, affine and track_running_stats: the BatchNorm kernels then run all groups in one launch."""
    def key(m):
        return m.eps, m.momentum, m.affine, m.track_running_stats
    return all(type(m) in (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d) and type(m.momentum) in (int, float) and key(m) == key(mods[0]) and
               m.track_running_stats == (m.running_mean is not None) for m in mods)


def _batch_stats(mods, training: bool) -> ops.BatchStats:
    """The `bn` argument of the norm ops for the per-group BatchNorm modules: running buffers of all groups concatenated (the buffers
    themselves for one group), or None without running statistics."""
    def cat(name):
        if not mods[0].track_running_stats:
            return None
        return getattr(mods[0], name) if len(mods) == 1 else torch.cat([getattr(m, name) for m in mods])
    return ops.BatchStats(cat("running_mean"), cat("running_var"), float(mods[0].momentum), training)


def _commit_stats(mods, bn: ops.BatchStats) -> None:
    """After a launch with `bn`: what nn.BatchNorm's forward does to its buffers in training mode -- the new running values back into each
    group's module (one group: the kernel wrote them in place) and the batch counter, a torch in-place add (graph capture records it)."""
    if not bn.training or bn.running_mean is None:
        return
    for g, m in enumerate(mods):
        if len(mods) > 1:
            m.running_mean.copy_(bn.running_mean.view(len(mods), -1)[g])
            m.running_var.copy_(bn.running_var.view(len(mods), -1)[g])
        m.num_batches_tracked.add_(1)


def _batch_norm(mods, z, training: bool):
    """The BatchNorm kernel alone over a [B, C, H, W] tensor, all groups in one launch (`_fusable_batchnorm(mods)` holds)."""
    bn = _batch_stats(mods, training)
    y = ops.batch_norm(z, *_gamma_beta(mods), bn.running_mean, bn.running_var, training, bn.momentum, mods[0].eps)
    _commit_stats(mods, bn)
    return y


def _need_conv2d(conv_class, ndim, allow_3d: bool = False):
    ok = ((nn.Conv2d, 2), (nn.Conv1d, 1)) + (((nn.Conv3d, 3),) if allow_3d else ())
    if (conv_class, ndim) not in ok:
        raise NotImplementedError("this layer is built for " + ("1-D, 2-D and 3-D" if allow_3d else "1-D and 2-D") + " on the HIP path")


def _triple(v):
    if isinstance(v, (tuple, list)):
        if len(v) != 3:
            raise ValueError(f"expected an int or a triple, got {v!r}")
        return int(v[0]), int(v[1]), int(v[2])
    return int(v), int(v), int(v)


def conv3d_stage(basis_kw, kernel_size, stride, padding, dilation, groups, x, xn, w_base, w_basis):
    """The fused conv stage for 3-D layers (kan_layers.py:261-271 and the sibling 3-D shims), on the 2-D kernels.

    A 3-D cross-correlation is a sum over the kd depth taps of 2-D ones: output slice `do` takes, for tap `td`, the 2-D
    conv stage of input slice `di = do*sd - pd + td*dd` with the kernel slice W[:, :, td] -- and nothing where `di` falls into
    the depth padding, which is exactly the reference's zero padding of the EXPANDED operand.  So each depth tap is one
    launch set of the 2-D kernels over the batch of all (image, valid depth slice) pairs; torch only gathers the slices and
    sums the kd partial results.  x: [B, C, D, H, W]; weights per group [Og, Cg(*n), kd, kh, kw]."""
    (kd, kh, kw), (sd, sh, sw), (pd, ph, pw), (dd, dh, dw) = _triple(kernel_size), _triple(stride), _triple(padding), _triple(dilation)
    if x.dim() != 5:
        raise ValueError(f"expected [B, C, D, H, W] input for a 3-D layer, got shape {tuple(x.shape)}")
    B, C, D, H, W = x.shape
    Do = (D + 2 * pd - dd * (kd - 1) - 1) // sd + 1
    if Do <= 0:
        raise L.KanConvError(f"empty output depth for input depth {D}")
    spec = ops.ConvSpec(kernel=(kh, kw), stride=(sh, sw), padding=(ph, pw), dilation=(dh, dw), groups=groups, **basis_kw)
    z = None
    for td in range(kd):
        dos = [o for o in range(Do) if 0 <= o * sd - pd + td * dd < D]
        if not dos:
            continue
        d0, n = dos[0] * sd - pd + td * dd, len(dos)              # valid outputs are consecutive; their inputs step by sd

        def gather(t):
            return t[:, :, d0:d0 + (n - 1) * sd + 1:sd].permute(0, 2, 1, 3, 4).reshape(B * n, C, H, W)
        z2 = ops.kan_conv(spec, gather(x), gather(xn) if xn is not None else None,
                          [w[:, :, td] for w in w_base], [w[:, :, td] for w in w_basis])
        z2 = z2.view(B, n, *z2.shape[1:]).permute(0, 2, 1, 3, 4)                      # [B, O, n, Ho, Wo]
        z2 = F.pad(z2, (0, 0, 0, 0, dos[0], Do - dos[0] - n))
        z = z2 if z is None else z + z2
    if z is None:                                                 # every tap of every output lies in the depth padding: all zeros
        ho, wo = spec.out_hw(H, W)
        z = x.new_zeros((B, w_basis[0].shape[0] * groups, Do, ho, wo))
        z = z + 0.0 * (x.sum() + sum(w.sum() for w in list(w_base) + list(w_basis)))      # zero gradients, as autograd gives the reference
    return z


def _norm_affine(mods):
    """Per-group lists (gammas, betas) of the norm modules, or (None, None): the form `ops.kan_conv_in_prelu` takes."""
    if mods[0].affine:
        return [m.weight for m in mods], [m.bias for m in mods]
    return None, None


def _gamma_beta(mods):
    """(gamma, beta) of all groups concatenated, or (None, None): the form `ops.instance_norm` takes."""
    gam, bet = _norm_affine(mods)
    return (torch.cat(gam), torch.cat(bet)) if gam is not None else (None, None)


def _channel_major(poly_weights, n):
    """Per-group views of a plane-major ``poly_weights`` [G, O/G, n * C/G, k, k] (channel index j*C + c) in the kernels'
    channel-major order (c*n + j); autograd carries the gradient back."""
    G, og, cn, k = poly_weights.shape[:4]
    return [poly_weights[g].view(og, n, cn // n, k, k).transpose(1, 2).reshape(og, cn, k, k) for g in range(G)]


def _norm3d(mods, prelus, z, og):
    """Per-group norm (+ PReLU) of a [B, O, D, H, W] tensor: plain InstanceNorm3d / BatchNorm3d run on the norm kernels with the
    volume as one plane; anything else is the caller's own module."""
    B, O, Dz, Hz, Wz = z.shape
    if all(type(m) is nn.InstanceNorm3d and not m.track_running_stats for m in mods):
        y = ops.instance_norm(z.reshape(B, O, Dz * Hz, Wz), *_gamma_beta(mods), eps=mods[0].eps).view(B, O, Dz, Hz, Wz)
        parts = [y[:, g * og:(g + 1) * og] for g in range(len(mods))]
    elif _fusable_batchnorm(mods):
        y = _batch_norm(mods, z.reshape(B, O, Dz * Hz, Wz), mods[0].training).view(B, O, Dz, Hz, Wz)
        parts = [y[:, g * og:(g + 1) * og] for g in range(len(mods))]
    else:
        parts = [mods[g](z[:, g * og:(g + 1) * og]) for g in range(len(mods))]
    if prelus is not None:
        parts = [prelus[g](p) for g, p in enumerate(parts)]
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)


def _one(v):
    if isinstance(v, (tuple, list)):
        if len(v) != 1:
            raise ValueError(f"expected an int or a 1-tuple, got {v!r}")
        return int(v[0])
    return int(v)


class _HipLayer(nn.Module):
    """Shared plumbing.  1-D layers (ndim == 1) are lifted to 2-D: x [B,C,L] -> [B,C,1,L], weights [O,C,k] -> [O,C,1,k]
    (views), kernel (1,k), stride (1,s), padding (0,p), dilation (1,d); InstanceNorm1d over L == InstanceNorm2d over 1 x L."""

    def _spec(self, **kw) -> ops.ConvSpec:
        if getattr(self, "ndim", 2) == 1:
            return ops.ConvSpec(kernel=(1, _one(self.kernel_size)), stride=(1, _one(self.stride)), padding=(0, _one(self.padding)),
                                dilation=(1, _one(self.dilation)), groups=self.groups, **kw)
        return ops.ConvSpec(kernel=_pair(self.kernel_size), stride=_pair(self.stride), padding=_pair(self.padding),
                            dilation=_pair(self.dilation), groups=self.groups, **kw)

    def _lift(self, x):
        if getattr(self, "ndim", 2) == 1:
            if x.dim() != 3:
                raise ValueError(f"expected [B, C, L] input for a 1-D layer, got shape {tuple(x.shape)}")
            return x.unsqueeze(2)
        return x

    def _lower(self, y):
        return y.squeeze(2) if getattr(self, "ndim", 2) == 1 else y

    def _w(self, convs):
        return [m.weight.unsqueeze(2) for m in convs] if getattr(self, "ndim", 2) == 1 else [m.weight for m in convs]

    pool_types = ()     # the one statement of which layers take `forward(x, pool=)`, and in which form: see _FusedTailLayer

    def takes_pool(self, pool) -> bool:
        """Whether the models hand this layer the MaxPool2d that follows it as `forward(x, pool=pool)`: True for
        MaxPool2d(2, 2) (models/kan_vgg.py), a (kernel, stride) tuple (models/kan_alexnet.py)."""
        return getattr(self, "ndim", 2) == 2 and isinstance(pool, self.pool_types)

    def conv_spec(self) -> ops.ConvSpec:
        return self._spec(**self._basis_kw())

    # ---- plane windows: any degree / grid size on launches of at most KAN_MAX_PLANES planes
    plane_window = L.KAN_MAX_PLANES     # planes per launch, base included (a test lowers it to force windows on a layer that fits one launch)
    _window_unit = 1                    # planes per window index (FourierKAN: 2, a cos and a sin plane per frequency)

    def _check_planes_3d(self):
        """3-D layers run one launch set per depth tap (conv3d_stage) and have no window loop: above the plane limit they raise here."""
        kw = self._basis_kw()
        planes = kw["n_basis"] + int(kw["act"] != L.ACT_NONE)
        if getattr(self, "ndim", 2) == 3 and planes > L.KAN_MAX_PLANES:
            raise NotImplementedError(f"{planes} planes per channel exceed KAN_MAX_PLANES = {L.KAN_MAX_PLANES}: 3-D layers have no plane windows "
                                      "(the 1-D and 2-D layers take any degree / grid size)")

    def _window_kw(self, kw, j0, j1, base):
        """The basis description of window [j0, j1) of the layer's `_basis_kw()`: how a family starts in the middle.  Recurrence families and
        ChebyKAN: the kernels run the recurrence from 0 and emit from plane `first` on; the coefficient table stays whole."""
        return dict(kw, first=j0, n_basis=j1 - j0, act=kw["act"] if base else L.ACT_NONE)

    def _window_weights(self, ws, j0, j1, n):
        """Basis weights of window [j0, j1) out of n: per-group [O, C*n, ...] (channel index c*n + j) -> [O, C*(j1 - j0), ...]."""
        return [w.reshape(w.shape[0], w.shape[1] // n, n, *w.shape[2:])[:, :, j0:j1].reshape(w.shape[0], -1, *w.shape[2:]) for w in ws]

    def _plane_windows(self):
        """The library holds at most KAN_MAX_PLANES = 16 planes per channel in one launch; the reference takes any degree / grid_size.
        The conv stage is linear in the planes, so a layer of more planes runs one launch set per window of <= `plane_window` planes
        (the first carries the base branch) and sums the results: [(spec, j0, j1, with_base), ...], [j0, j1) in window units."""
        kw = self._basis_kw()
        u = self._window_unit
        n, has_act = kw["n_basis"] // u, kw["act"] != L.ACT_NONE
        out, j0 = [], 0
        while j0 < n:
            base = j0 == 0 and has_act
            j1 = min(n, j0 + max(1, (self.plane_window - int(base)) // u))
            out.append((self._spec(**self._window_kw(kw, j0, j1, base)), j0, j1, base))
            j0 = j1
        return out

    def _conv_stage(self, spec, xa, xb, wb, ws, phases=None):
        """The conv stage of a (lifted) layer: one launch set, or -- more planes than one launch holds -- the sum over plane windows
        (differentiable: autograd routes the gradient of each weight / phase slice back into its Parameter).  `xb`: the basis tensor where
        it is not `xa` (host-applied activation, FastKAN's normalised input, Legendre's x_n): a window without the base branch reads it alone."""
        def stage(sp, x, xn, w_base, w_basis, ph):
            if ph is None:
                return ops.kan_conv(sp, x, xn, w_base, w_basis)
            return ops.kan_conv_phased(sp, x, ph, w_base, w_basis, xn=xn)
        if spec.n_basis + int(spec.has_base) <= self.plane_window:
            return stage(spec, xa, xb, wb, ws, phases)
        n, z = spec.n_basis // self._window_unit, None
        for wspec, j0, j1, base in self._plane_windows():
            part = stage(wspec, xa if base else (xb if xb is not None else xa), xb if base else None, wb if base else [],
                         self._window_weights(ws, j0, j1, n), phases[:, :, j0:j1].contiguous() if phases is not None else None)
            z = part if z is None else z + part
        return z

    def _build(self, conv_class, norm_class, cg, og, basis=None, planes=0, prelus=False, norm_dim=None, plane_major=0):
        """The per-group module lists, created and initialised in the order every family's reference constructor uses (a seeded
        construction draws the same weights): ``base_conv``, the basis convs `planes * cg -> og` under the attribute name `basis`,
        ``layer_norm`` over `norm_dim` (default `og`) channels, ``prelus``, a plane-major ``poly_weights`` of `plane_major` planes
        (drawn here, initialised by the caller); then the Kaiming init of the base and the basis convs."""
        def convs(cin):
            return nn.ModuleList([conv_class(cin, og, self.kernel_size, self.stride, self.padding, self.dilation, groups=1, bias=False)
                                  for _ in range(self.groups)])
        self.base_conv = convs(cg)
        if basis is not None:
            setattr(self, basis, convs(planes * cg))
        self.layer_norm = nn.ModuleList([norm_class(og if norm_dim is None else norm_dim, **_filter_norm_kwargs(norm_class, self.norm_kwargs))
                                         for _ in range(self.groups)])
        if prelus:
            self.prelus = nn.ModuleList([nn.PReLU() for _ in range(self.groups)])
        if plane_major:
            self.poly_weights = nn.Parameter(torch.randn(self.groups, og, cg * plane_major, *([self.kernel_size] * self.ndim)))
        for conv in [*self.base_conv, *(getattr(self, basis) if basis is not None else ())]:
            nn.init.kaiming_uniform_(conv.weight, nonlinearity='linear')

    def _base_input(self, x):
        """(base-branch tensor, basis tensor or None): `(act(x), x)` when the host applies the activation (no device functor
        for this module; the kernels run their two-input form with the identity functor), else `(x, None)`."""
        if _host_applied(self.base_activation):
            return self.base_activation(x), x
        return x, None

    def _norm_act(self, z):
        """Tail of the 'norm, then activation' layers (Jacobi, Legendre, Bersnstein, ReLU-KAN, GRAM) for the (lifted) pre-norm
        tensor: the InstanceNorm / BatchNorm kernel, or the caller's own norm modules on the layer's own rank (nn.LayerNorm over the
        flattened group), then ``base_activation``."""
        mods = self.layer_norm
        if _fusable_instnorm(mods):
            y = self._lower(ops.instance_norm(z, *_gamma_beta(mods), eps=mods[0].eps))
        elif _fusable_batchnorm(mods):
            y = self._lower(_batch_norm(mods, z.contiguous(), self.training))
        else:
            z = self._lower(z)
            og = z.shape[1] // self.groups
            parts = []
            for g, norm in enumerate(mods):
                zg = z[:, g * og:(g + 1) * og]
                parts.append(norm(zg.reshape(zg.shape[0], -1)).view(zg.shape) if isinstance(norm, nn.LayerNorm) else norm(zg))
            y = torch.cat(parts, dim=1)
        return self.base_activation(y)


class _FusedTailLayer(_HipLayer):
    """The one forward of the layers shaped  y = Dropout([PReLU](norm(conv stage)))  -- B-spline, the recurrence families,
    FourierKAN, ChebyKAN.  A subclass gives `_basis_kw()`, the attribute name of its basis-conv list (`_basis`) and whether
    it has a base branch with PReLUs (`_has_base`; ChebyKAN has neither)."""
    _basis = "poly_conv"
    _has_base = True
    pool_types = (bool, tuple)

    def _norm_prelu(self, z):
        """Un-fused tail for the (lifted) [B, O, H, W] pre-norm tensor: the InstanceNorm / BatchNorm kernel (or the caller's own norm
        modules on the layer's own rank), then PReLU where the layer has them.  Returns the tensor in the layer's rank."""
        mods, og = self.layer_norm, z.shape[1] // self.groups
        if _fusable_instnorm(mods) or _fusable_batchnorm(mods):
            n = ops.instance_norm(z.contiguous(), *_gamma_beta(mods), eps=mods[0].eps) if _fusable_instnorm(mods) else _batch_norm(mods, z.contiguous(), self.training)
            n = self._lower(n)
            parts = [n[:, g * og:(g + 1) * og] for g in range(self.groups)]
        else:
            z = self._lower(z)
            parts = [mods[g](z[:, g * og:(g + 1) * og]) for g in range(self.groups)]
        if self._has_base:
            parts = [self.prelus[g](t) for g, t in enumerate(parts)]
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)

    def _forward3d(self, x):
        """[B, C, D, H, W] layers (the ...KANConv3DLayer shims of the reference): each depth tap is one launch set of the 2-D
        kernels, on the same basis description as conv_spec()."""
        xa, xb = self._base_input(x) if self._has_base else (x, None)
        z = conv3d_stage(self._basis_kw(), self.kernel_size, self.stride, self.padding, self.dilation, self.groups, xa, xb,
                         [m.weight for m in self.base_conv] if self._has_base else [], [m.weight for m in getattr(self, self._basis)])
        y = _norm3d(self.layer_norm, self.prelus if self._has_base else None, z, self.output_dim // self.groups)
        return self.dropout(y) if self.dropout is not None else y

    def forward(self, x, pool=False):
        """`pool` (not part of the reference signature) returns max_pool2d(layer(x), ...): True for a layer that is followed by
        MaxPool2d(2, 2) (models/kan_vgg.py), `(k, s)` for a general MaxPool2d(k, s) without padding (models/kan_alexnet.py:
        (3, 2)).  Where the tail is fused and `ops.pool_fusable`, the pooling is done inside the InstanceNorm(+PReLU) kernels."""
        if self.ndim == 3:
            if pool:
                raise NotImplementedError("pool is a 2-D fusion")
            return self._forward3d(x)
        spec = self.conv_spec()
        x = self._lift(x)
        wb = self._w(self.base_conv) if self._has_base else []
        ws = self._w(getattr(self, self._basis))
        prelus = [m.weight for m in self.prelus] if self._has_base else None
        xa, xb = self._base_input(x) if self._has_base else (x, None)      # (act(x), x) when the host applies the activation
        windowed = spec.n_basis + int(spec.has_base) > self.plane_window    # more planes than one launch holds: _HipLayer._conv_stage
        mods = self.layer_norm
        bnorm = _fusable_batchnorm(mods) and ops.fits_one_launch(spec, x, ws)      # (batch statistics cannot be cut into runs of images)
        if not windowed and xb is None and (_fusable_instnorm(mods) or bnorm) and all(p.numel() == 1 for p in prelus or ()):
            gam, bet = _norm_affine(mods)
            bn = _batch_stats(mods, self.training) if bnorm else None
            fused_pool = bool(pool) and self.ndim == 2 and self.dropout is None and ops.pool_fusable(pool, *spec.out_hw(x.shape[2], x.shape[3]), batchnorm=bnorm)
            y = ops.kan_conv_in_prelu(spec, x, wb, ws, gam, bet, prelus, eps=mods[0].eps, pool=pool if fused_pool else False, bn=bn)
            if bnorm:
                _commit_stats(mods, bn)
            if fused_pool:
                return y
            y = self._lower(y)
        else:
            # other norm classes (e.g. LayerNorm, GroupNorm), a host-applied activation or plane windows: HIP conv stage, then the un-fused tail
            y = self._norm_prelu(self._conv_stage(spec, xa, xb, wb, ws))
        if self.dropout is not None:
            y = self.dropout(y)
        return _unfused_pool(y, pool) if pool else y


# =========================================================================================== B-spline
class KANConvNDLayer(_FusedTailLayer):
    _basis = "spline_conv"

    def __init__(self, conv_class, norm_class, input_dim, output_dim, spline_order, kernel_size,
                 groups=1, padding=0, stride=1, dilation=1,
                 ndim: int = 2, grid_size=5, base_activation=nn.GELU, grid_range=[-1, 1], dropout=0.0,
                 **norm_kwargs):
        super().__init__()
        _need_conv2d(conv_class, ndim, allow_3d=True)
        self.input_dim, self.output_dim = input_dim, output_dim
        self.spline_order, self.kernel_size = spline_order, kernel_size
        self.padding, self.stride, self.dilation, self.groups, self.ndim = padding, stride, dilation, groups, ndim
        self.grid_size = grid_size
        self.base_activation = base_activation() if base_activation is not None else nn.Identity()
        self.grid_range = grid_range
        self.norm_kwargs = norm_kwargs
        self.dropout = _dropout2d(dropout, ndim)
        _check_groups(groups, input_dim, output_dim)
        self.input_dim_group, self.output_dim_group = input_dim // groups, output_dim // groups
        self._build(conv_class, norm_class, self.input_dim_group, self.output_dim_group, "spline_conv", grid_size + spline_order, prelus=True)
        h = (self.grid_range[1] - self.grid_range[0]) / grid_size
        # plain attribute, not a buffer: absent from state_dict exactly as in kan_layers.py:184-190
        self.grid = torch.linspace(self.grid_range[0] - h * spline_order, self.grid_range[1] + h * spline_order,
                                   grid_size + 2 * spline_order + 1, dtype=torch.float32)
        self._act_code = _act_code(self.base_activation, host_ok=True)
        self._check_planes_3d()

    def _basis_kw(self):
        return dict(kind=L.BASIS_BSPLINE, n_basis=self.grid_size + self.spline_order, order=self.spline_order,
                    act=self._act_code, p0=0.0, p1=0.0, table=tuple(float(v) for v in self.grid.tolist()))

    def _window_kw(self, kw, j0, j1, base):
        """B-spline basis j is a function of knots j .. j + order + 1 alone, so bases [j0, j1) of this layer ARE the bases of a B-spline
        layer built on knots[j0 : j1 + order + 1] (kan_layers.py:117-131 takes any grid_size): a window is a slice of the knots."""
        return dict(kw, n_basis=j1 - j0, act=kw["act"] if base else L.ACT_NONE, table=kw["table"][j0:j1 + self.spline_order + 1])


class KANConv3DLayer(KANConvNDLayer):
    def __init__(self, input_dim, output_dim, kernel_size, spline_order=3, groups=1, padding=0, stride=1, dilation=1,
                 grid_size=5, base_activation=nn.GELU, grid_range=[-1, 1], dropout=0.0, norm_layer=nn.InstanceNorm3d,
                 **norm_kwargs):
        super().__init__(nn.Conv3d, norm_layer, input_dim, output_dim, spline_order, kernel_size,
                         groups=groups, padding=padding, stride=stride, dilation=dilation, ndim=3,
                         grid_size=grid_size, base_activation=base_activation, grid_range=grid_range, dropout=dropout, **norm_kwargs)


class KANConv1DLayer(KANConvNDLayer):
    def __init__(self, input_dim, output_dim, kernel_size, spline_order=3, groups=1, padding=0, stride=1, dilation=1,
                 grid_size=5, base_activation=nn.GELU, grid_range=[-1, 1], dropout=0.0, norm_layer=nn.InstanceNorm1d,
                 **norm_kwargs):
        super().__init__(nn.Conv1d, norm_layer, input_dim, output_dim, spline_order, kernel_size,
                         groups=groups, padding=padding, stride=stride, dilation=dilation, ndim=1,
                         grid_size=grid_size, base_activation=base_activation, grid_range=grid_range, dropout=dropout,
                         **norm_kwargs)


class KANConv2DLayer(KANConvNDLayer):
    def __init__(self, input_dim, output_dim, kernel_size, spline_order=3, groups=1, padding=0, stride=1, dilation=1,
                 grid_size=5, base_activation=nn.GELU, grid_range=[-1, 1], dropout=0.0, norm_layer=nn.InstanceNorm2d,
                 **norm_kwargs):
        super().__init__(nn.Conv2d, norm_layer, input_dim, output_dim, spline_order, kernel_size,
                         groups=groups, padding=padding, stride=stride, dilation=dilation, ndim=2,
                         grid_size=grid_size, base_activation=base_activation, grid_range=grid_range, dropout=dropout,
                         **norm_kwargs)


# =========================================================================================== FastKAN
class RadialBasisFunction(nn.Module):
    """Parameter holder mirroring utils/utils.py:19-33 (state_dict key ``rbf.grid``)."""

    def __init__(self, grid_min: float = -2., grid_max: float = 2., num_grids: int = 8, denominator: Optional[float] = None):
        super().__init__()
        self.grid = nn.Parameter(torch.linspace(grid_min, grid_max, num_grids), requires_grad=False)
        self.denominator = denominator or (grid_max - grid_min) / (num_grids - 1)


class FastKANConvNDLayer(_HipLayer):
    def __init__(self, conv_class, norm_class, input_dim, output_dim, kernel_size,
                 groups=1, padding=0, stride=1, dilation=1,
                 ndim: int = 2, grid_size=8, base_activation=nn.SiLU, grid_range=[-2, 2], dropout=0.0, **norm_kwargs):
        super().__init__()
        _need_conv2d(conv_class, ndim, allow_3d=True)
        self.input_dim, self.output_dim, self.kernel_size = input_dim, output_dim, kernel_size
        self.padding, self.stride, self.dilation, self.groups, self.ndim = padding, stride, dilation, groups, ndim
        self.grid_size = grid_size
        self.base_activation = base_activation() if base_activation is not None else nn.Identity()
        self.grid_range = grid_range
        self.norm_kwargs = norm_kwargs
        _check_groups(groups, input_dim, output_dim)
        cg, og = input_dim // groups, output_dim // groups
        self._build(conv_class, norm_class, cg, og, "spline_conv", grid_size, norm_dim=cg)       # the norm is on the INPUT of the RBFs
        self.rbf = RadialBasisFunction(grid_range[0], grid_range[1], grid_size)
        self.dropout = _dropout2d(dropout, ndim)
        self._act_code = _act_code(self.base_activation, host_ok=True)
        self._centres = tuple(float(v) for v in self.rbf.grid.detach().tolist())
        self._check_planes_3d()

    def _window_kw(self, kw, j0, j1, base):
        """A FastKAN window is a slice of the centres (the denominator is the layer's)."""
        return dict(kw, n_basis=j1 - j0, act=kw["act"] if base else L.ACT_NONE, table=kw["table"][j0:j1])

    def _basis_kw(self):
        return dict(kind=L.BASIS_RBF, n_basis=self.grid_size, order=0, act=self._act_code, p0=float(self.rbf.denominator), p1=0.0,
                    table=self._centres)

    def _forward3d(self, x):
        xs = self.dropout(x) if self.dropout is not None else x
        cg = self.input_dim // self.groups
        if all(type(m) is nn.InstanceNorm3d and not m.track_running_stats for m in self.layer_norm):
            B, C, D, H, W = xs.shape
            xn = ops.instance_norm(xs.reshape(B, C, D * H, W), *_gamma_beta(self.layer_norm), eps=self.layer_norm[0].eps).view(B, C, D, H, W)
        elif _fusable_batchnorm(self.layer_norm):
            B, C, D, H, W = xs.shape
            xn = _batch_norm(self.layer_norm, xs.reshape(B, C, D * H, W), self.training).view(B, C, D, H, W)
        else:
            xn = torch.cat([self.layer_norm[g](xs[:, g * cg:(g + 1) * cg]) for g in range(self.groups)], dim=1)
        return conv3d_stage(self._basis_kw(), self.kernel_size, self.stride, self.padding, self.dilation, self.groups, self._base_input(x)[0], xn,
                            [m.weight for m in self.base_conv], [m.weight for m in self.spline_conv])

    def forward(self, x):
        if self.ndim == 3:
            return self._forward3d(x)
        # fast_kan_layers.py:100-111: the base branch sees raw x; the RBFs see norm(dropout(x))
        xs = self.dropout(x) if self.dropout is not None else x
        cg = self.input_dim // self.groups
        if _fusable_instnorm(self.layer_norm):
            xn = self._lift(xs) if xs.dim() == 3 else xs
            xn = ops.instance_norm(xn.contiguous(), *_gamma_beta(self.layer_norm), eps=self.layer_norm[0].eps)
        elif _fusable_batchnorm(self.layer_norm):
            xn = _batch_norm(self.layer_norm, (self._lift(xs) if xs.dim() == 3 else xs).contiguous(), self.training)
        else:
            xn = self._lift(torch.cat([self.layer_norm[g](xs[:, g * cg:(g + 1) * cg]) for g in range(self.groups)], dim=1))
        return self._lower(self._conv_stage(self.conv_spec(), self._lift(self._base_input(x)[0]), xn, self._w(self.base_conv), self._w(self.spline_conv)))


class FastKANConv1DLayer(FastKANConvNDLayer):
    def __init__(self, input_dim, output_dim, kernel_size, groups=1, padding=0, stride=1, dilation=1,
                 grid_size=8, base_activation=nn.SiLU, grid_range=[-2, 2], dropout=0.0,
                 norm_layer=nn.InstanceNorm1d, **norm_kwargs):
        super().__init__(nn.Conv1d, norm_layer, input_dim, output_dim, kernel_size,
                         groups=groups, padding=padding, stride=stride, dilation=dilation, ndim=1,
                         grid_size=grid_size, base_activation=base_activation, grid_range=grid_range,
                         dropout=dropout, **norm_kwargs)


class FastKANConv3DLayer(FastKANConvNDLayer):
    def __init__(self, input_dim, output_dim, kernel_size, groups=1, padding=0, stride=1, dilation=1,
                 grid_size=8, base_activation=nn.SiLU, grid_range=[-2, 2], dropout=0.0,
                 norm_layer=nn.InstanceNorm3d, **norm_kwargs):
        super().__init__(nn.Conv3d, norm_layer, input_dim, output_dim, kernel_size,
                         groups=groups, padding=padding, stride=stride, dilation=dilation, ndim=3,
                         grid_size=grid_size, base_activation=base_activation, grid_range=grid_range,
                         dropout=dropout, **norm_kwargs)


class FastKANConv2DLayer(FastKANConvNDLayer):
    def __init__(self, input_dim, output_dim, kernel_size, groups=1, padding=0, stride=1, dilation=1,
                 grid_size=8, base_activation=nn.SiLU, grid_range=[-2, 2], dropout=0.0,
                 norm_layer=nn.InstanceNorm2d, **norm_kwargs):
        super().__init__(nn.Conv2d, norm_layer, input_dim, output_dim, kernel_size,
                         groups=groups, padding=padding, stride=stride, dilation=dilation, ndim=2,
                         grid_size=grid_size, base_activation=base_activation, grid_range=grid_range,
                         dropout=dropout, **norm_kwargs)


# =========================================================================================== ChebyKAN
class ChebyKANConvNDLayer(_FusedTailLayer):
    _has_base = False                                   # cheby_kan_layers.py:39-111: no base branch, no PReLU
    pool_types = (tuple,)                               # models/kan_alexnet.py fuses its MaxPool2d(3, 2); models/kan_vgg.py leaves ChebyKAN un-fused

    def __init__(self, conv_class, norm_layer, input_dim, output_dim, degree, kernel_size,
                 groups=1, padding=0, stride=1, dilation=1, ndim: int = 2, dropout=0.0, **norm_kwargs):
        super().__init__()
        _need_conv2d(conv_class, ndim, allow_3d=True)
        self.input_dim, self.output_dim, self.degree, self.kernel_size = input_dim, output_dim, degree, kernel_size
        self.padding, self.stride, self.dilation, self.groups, self.ndim = padding, stride, dilation, groups, ndim
        self.norm_kwargs = norm_kwargs
        self.epsilon = 1e-7
        self.dropout = _dropout2d(dropout, ndim)
        _check_groups(groups, input_dim, output_dim)
        og = output_dim // groups
        self.layer_norm = nn.ModuleList([norm_layer(og, **_filter_norm_kwargs(norm_layer, norm_kwargs)) for _ in range(groups)])
        self.poly_conv = nn.ModuleList([conv_class((degree + 1) * input_dim // groups, og, kernel_size, stride, padding, dilation,
                                                   groups=1, bias=False) for _ in range(groups)])
        self.register_buffer("arange", torch.arange(0, degree + 1, 1).view(1, 1, -1, *([1] * ndim)))    # cheby_kan_layers.py:85-86
        for conv in self.poly_conv:
            # cheby_kan_layers.py:88-90 (normal_ first, then overwritten; `**` requires an int kernel_size, as there)
            nn.init.normal_(conv.weight, mean=0.0, std=1 / (input_dim * (degree + 1) * kernel_size ** ndim))
            nn.init.kaiming_normal_(conv.weight, mode='fan_in', nonlinearity='relu')
        self._check_planes_3d()

    def _basis_kw(self):
        lo = float(np.float32(-1 + self.epsilon))       # torch.clamp casts its Python-float bounds to fp32
        hi = float(np.float32(1 - self.epsilon))
        return dict(kind=L.BASIS_CHEBY, n_basis=self.degree + 1, order=0, act=L.ACT_NONE, p0=lo, p1=hi, table=())


class ChebyKANConv1DLayer(ChebyKANConvNDLayer):
    def __init__(self, input_dim, output_dim, kernel_size, degree=3, groups=1, padding=0, stride=1, dilation=1,
                 dropout=0.0, norm_layer=nn.InstanceNorm1d, **norm_kwargs):
        super().__init__(nn.Conv1d, norm_layer, input_dim, output_dim, degree, kernel_size,
                         groups=groups, padding=padding, stride=stride, dilation=dilation, ndim=1, dropout=dropout, **norm_kwargs)


class ChebyKANConv3DLayer(ChebyKANConvNDLayer):
    def __init__(self, input_dim, output_dim, kernel_size, degree=3, groups=1, padding=0, stride=1, dilation=1,
                 dropout=0.0, norm_layer=nn.InstanceNorm3d, **norm_kwargs):
        super().__init__(nn.Conv3d, norm_layer, input_dim, output_dim, degree, kernel_size,
                         groups=groups, padding=padding, stride=stride, dilation=dilation, ndim=3, dropout=dropout, **norm_kwargs)


class ChebyKANConv2DLayer(ChebyKANConvNDLayer):
    def __init__(self, input_dim, output_dim, kernel_size, degree=3, groups=1, padding=0, stride=1, dilation=1,
                 dropout=0.0, norm_layer=nn.InstanceNorm2d, **norm_kwargs):
        super().__init__(nn.Conv2d, norm_layer, input_dim, output_dim, degree, kernel_size,
                         groups=groups, padding=padding, stride=stride, dilation=dilation, ndim=2, dropout=dropout, **norm_kwargs)


__all__ = ["KANConvNDLayer", "KANConv2DLayer", "KANConv1DLayer", "KANConv3DLayer", "FastKANConv3DLayer", "ChebyKANConv3DLayer", "FastKANConvNDLayer", "FastKANConv2DLayer", "FastKANConv1DLayer",
           "ChebyKANConvNDLayer", "ChebyKANConv2DLayer", "ChebyKANConv1DLayer", "RadialBasisFunction"]
_ = F

"""Autograd operators over the libkanconv C ABI.

Two differentiable entry points, both launching only hand-written HIP kernels:

* ``kan_conv``           -- the fused "expand to basis planes + convolve" stage
                            (reference: kan_layers.py:199-239, fast_kan_layers.py:103-109,
                            cheby_kan_layers.py:93-97).
* ``kan_conv_in_prelu``  -- the same followed by InstanceNorm2d [+ PReLU]
                            (kan_layers.py:241-243, cheby_kan_layers.py:98).
* ``instance_norm``      -- InstanceNorm2d alone (fast_kan_layers.py:106, norm on the input).
* ``batch_norm``         -- BatchNorm2d alone; ``kan_conv_in_prelu(..., bn=)`` is the fused tail of a layer built with
                            ``norm_layer=BatchNorm2d`` (train.py:67-68: the default of the reference's training script).
* ``cross_entropy``      -- the criterion (generic_train.py:26) with the counters of the test metrics (evaluations.py:131-151)
                            accumulated on the device.
* ``prepare_batch``      -- one batch from a device-resident uint8 dataset: gather, crop with zero padding, flip, ToTensor, Normalize
                            (utils/dataloader.py:56-90) and the labels, in one launch.
* ``prepare_resized_batch`` -- the same for the loader's ImageNet branch (:26-54): Resize, a crop box, Resize of the box (PIL's 8-bit bilinear
                            bytes), flip, Grayscale(3), ToTensor, Normalize, in one launch.

All tensors are fp32, NCHW, on a ROCm device.  Groups (kan_layers.py:249-258 loops over them in
Python) run inside the SAME launches (KanGeom.groups; the group index is folded into the grid):
the per-group weights are stacked once per call, activations are never copied or concatenated.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import weakref
from collections import OrderedDict
from dataclasses import dataclass, replace
from functools import lru_cache, partial, wraps
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _lib as L


@dataclass(frozen=True)
class ConvSpec:
    """Static description of one layer's conv stage (hashable: used as a plan-cache key)."""
    kind: int
    n_basis: int
    order: int
    act: int                      # L.ACT_NONE => no base branch
    p0: float
    p1: float
    table: Tuple[float, ...]
    kernel: Tuple[int, int]
    stride: Tuple[int, int]
    padding: Tuple[int, int]
    dilation: Tuple[int, int]
    groups: int = 1
    first: int = 0                # plane window of a Poly / Cheby / Fourier basis: the family's index of the first plane (frequency) emitted
    w_layout: int = 0             # 0: the reference's conv weights [O, C*n, kh, kw] (+ base weights); W_IOD: ONE coefficient tensor [I, O, n]
                                  # (the MLP KAN heads: 1x1 kernel, one group, no base branch), packed / unpacked by the *_iod kernels

    @property
    def has_base(self) -> bool:
        return self.act != L.ACT_NONE

    def out_hw(self, H: int, W: int) -> Tuple[int, int]:
        (kh, kw), (sh, sw), (ph, pw), (dh, dw) = self.kernel, self.stride, self.padding, self.dilation
        return (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1


W_IOD = 1


def _outputs(spec: ConvSpec, w_basis: Sequence[torch.Tensor]) -> int:
    """Output channels of the conv stage, all groups."""
    return w_basis[0].shape[1] if spec.w_layout == W_IOD else sum(w.shape[0] for w in w_basis)


def _device_table(spec: ConvSpec) -> bool:
    """A recurrence (Poly) basis whose coefficients do not fit the by-value table: the kernels read them from device memory."""
    return spec.kind == L.BASIS_POLY and len(spec.table) > L.KAN_MAX_TABLE


def _basis_struct(spec: ConvSpec) -> L.KanBasis:
    b = L.KanBasis()
    b.kind, b.n_basis, b.act, b.p0, b.p1 = spec.kind, spec.n_basis, spec.act, spec.p0, spec.p1
    b.order = spec.order | (spec.first << 8)          # KAN_ORDER_PACK (include/kanconv.h)
    if _device_table(spec):
        return b                                      # chan_table is set per call (_with_table)
    if len(spec.table) > L.KAN_MAX_TABLE:
        raise L.KanConvError(f"basis table of {len(spec.table)} entries exceeds KAN_MAX_TABLE={L.KAN_MAX_TABLE}")
    for i, v in enumerate(spec.table):
        b.table[i] = v
    return b


@lru_cache(maxsize=512)
def _plan_cached(spec: ConvSpec, B: int, Cg: int, H: int, W: int, Og: int, C_total: int, O_total: int):
    Ho, Wo = spec.out_hw(H, W)
    if Ho <= 0 or Wo <= 0:
        raise L.KanConvError(f"empty output ({Ho}x{Wo}) for input {H}x{W}")
    g = L.KanGeom()
    g.B, g.C, g.H, g.W, g.O, g.Ho, g.Wo = B, Cg, H, W, Og, Ho, Wo
    (g.kh, g.kw), (g.sh, g.sw), (g.ph, g.pw), (g.dh, g.dw) = spec.kernel, spec.stride, spec.padding, spec.dilation
    g.x_bstride, g.y_bstride = C_total * H * W, O_total * Ho * Wo
    g.groups = spec.groups
    b = _basis_struct(spec)
    p = L.KanPlan()
    bp = b
    if _device_table(spec):
        # the plan is pure host arithmetic and keyed by the spec alone, not the device: it sees a stand-in for the table pointer that
        # every launch sets on its own copy (_with_table); the cached struct keeps NULL, which the launchers' checks reject
        bp = L.KanBasis.from_buffer_copy(b)
        bp.chan_table = 1
    L.check(L.load().kan_plan(C.byref(g), C.byref(bp), C.byref(p)), "kan_plan")
    p.pos8_bw_slabs = L.load().kan_bwd_weight_rowgroup_slabs(C.byref(g), C.byref(bp))      # slabs of kan_conv_bwd_weight_rowgroups (0: not offered)
    p.tile_orders = L.load().kan_tile_orders(C.byref(g), C.byref(bp))      # the launchers' pixel order inside a tile: not a KanPlan field (kanconv.h)
    return g, b, p


def _plan_key(spec: ConvSpec, shape, Og: int) -> tuple:
    """The `_plan_cached` arguments of a conv stage over an NCHW input of `shape` with `Og` outputs per group."""
    B, Ct, H, W = shape
    return (spec, B, Ct // spec.groups, H, W, Og, Ct, Og * spec.groups)


def _with_phases(basis: L.KanBasis, phases: Optional[torch.Tensor], mode: int = 0) -> L.KanBasis:
    """Per-call copy of a cached basis struct carrying the device pointer of the ReLU-KAN phase table and the plane mode."""
    if phases is None:
        return basis
    b = L.KanBasis.from_buffer_copy(basis)
    b.chan_table, b.order = phases.data_ptr(), mode
    return b


_TABLES: "dict[tuple, torch.Tensor]" = {}           # (coefficient table, device) -> fp32 device tensor; the cache keeps it alive


def _with_table(basis: L.KanBasis, spec: ConvSpec, device) -> L.KanBasis:
    """Per-call copy of a cached basis struct carrying the device pointer of a long recurrence-coefficient table
    ([c0, a1, b1, A_2, B_2, C_2, ...], padded to 3 floats per plane).  Not a module buffer: state_dict() keys stay the reference's."""
    if not _device_table(spec):
        return basis
    key = (spec.table, torch.device(device))
    t = _TABLES.get(key)
    if t is None:
        t = _TABLES[key] = torch.tensor(list(spec.table) + [0.0] * 3, dtype=torch.float32, device=device)
    b = L.KanBasis.from_buffer_copy(basis)
    b.chan_table = t.data_ptr()
    return b


def _ptr(t: Optional[torch.Tensor], offset: int = 0) -> C.c_void_p:
    if t is None:
        return C.c_void_p(0)
    return C.c_void_p(t.data_ptr() + 4 * offset)


def _stream(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _dense(t: torch.Tensor) -> torch.Tensor:
    """`t` itself when it is contiguous and starts on a 16-byte boundary, else a copy that is (torch's allocator hands out 256-byte aligned blocks).
    What the kernels may assume of every activation and incoming-gradient pointer: the library picks its 8- and 16-byte
    routes from the pointers it is given (the norm kernels' float2 variants, the quadrant forward), so a view that starts 4 bytes into its storage
    would take another kernel than the same values in a tensor of their own; after this it takes the same one."""
    t = t.contiguous()
    return t.clone() if t.data_ptr() & 15 else t


def _require(t: torch.Tensor, name: str, align: bool = True) -> torch.Tensor:
    """`t` as the kernels read it: on a ROCm device, fp32, contiguous and (`align`) 16-byte aligned -- refused or copied on the host, before any launch.
    `align=False`: the conv weights, whose alignment `_pack` itself looks at (a copy here would hide the Parameter the cache is keyed by)."""
    if not isinstance(t, torch.Tensor):
        raise L.KanConvError(f"{name} must be a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise L.KanConvError(f"{name} is on {t.device}: this path runs only on a ROCm device (MI355X); there is no CPU fallback")
    if t.dtype != torch.float32:
        raise L.KanConvError(f"{name} must be float32, got {t.dtype}")
    return _dense(t) if align else t.contiguous()


def _split_weights(spec: ConvSpec, weights: Sequence[torch.Tensor]):
    G = spec.groups
    if spec.has_base:
        return list(weights[:G]), list(weights[G:2 * G])
    return [None] * G, list(weights[:G])


# --------------------------------------------------------------------------------------- optional kernel timing
# bench.py sets PROFILE to a list; each conv-kernel launch then appends a KernelSample with HIP events recorded on the
# launch stream (torch's current stream is the stream handed to the C ABI).
PROFILE: Optional[list] = None


@dataclass
class KernelSample:
    name: str                 # kernel family + output-tile tag
    flops: float              # dense algorithmic FLOPs of the launch
    executed: float           # FLOPs the MFMA pipe really runs: structural zeros skipped by position-major launches removed
    layer: str                # "C->O@HxW kKxK" of the launch
    start: "torch.cuda.Event"
    end: "torch.cuda.Event"


def _launch(sample, t: torch.Tensor, fn) -> None:
    """Run one conv-kernel launch; `sample` = (name, flops, executed, layer) from `_sample`."""
    name, flops, executed, layer = sample
    if PROFILE is None:
        L.check(fn(), name)
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.current_stream(t.device)
    e0.record(stream)
    L.check(fn(), name)
    e1.record(stream)
    PROFILE.append(KernelSample(name, flops, executed, layer, e0, e1))


def _conv_flops(geom, plan) -> float:
    """Dense algorithmic FLOPs of one conv-stage launch: 2*B*O*Ho*Wo*C*P*kh*kw per group."""
    return 2.0 * geom.B * geom.O * geom.Ho * geom.Wo * geom.C * plan.P * geom.kh * geom.kw * max(1, geom.groups)


@lru_cache(maxsize=256)
def _live_fraction(which: str, H: int, W: int, Ho: int, Wo: int, kh: int, kw: int, sh: int, sw: int, ph: int, pw: int, dh: int, dw: int) -> float:
    """Share of the (position, tap) products that touch a real input pixel (the rest multiply zero padding).  The
    position-major launches skip exactly those (kanconv.hip: live_taps_out / live_taps_in / live_positions_for_tap)."""
    live = 0
    for ho in range(Ho):
        for wo in range(Wo):
            for r in range(kh):
                for t in range(kw):
                    hi, wi = ho * sh - ph + r * dh, wo * sw - pw + t * dw
                    live += 0 <= hi < H and 0 <= wi < W
    return live / float(Ho * Wo * kh * kw)


_ROW_BLOCK_BIT = {"fwd": 1, "bwd_data": 2, "bwd_weight": 0}          # KanPlan.row_blocks: which launches run row-ordered 4x4 blocks


def _quadrant_order(geom, plan, which: str) -> bool:
    """The launch runs quadrant tiles (32 images x a 2x2 quadrant of a 4x4 plane) instead of row blocks: the planner's predicate restated
    (kan_plan.hip, plan_conv: `c.quad_fwd = rowblk_fwd && g->B % 32 == 0`; the forward only: bwd-data has its own predicate, `_quadrant_bwd_data`, as it also needs dz_pm).  The launcher also wants an 8-byte aligned
    output, which every torch allocation is."""
    return which == "fwd" and bool(plan.row_blocks & 1) and geom.B % 32 == 0


def _quadrant_bwd_data(geom, plan, have_dz_pm: bool) -> bool:
    """bwd-data runs quadrant tiles fed from the position-major copy of dz (kan_plan.hip, plan_conv: `c.quad_bd`; the launcher takes them when it is given
    dz_pm and a single input tensor -- `_conv_backward` builds dz_pm only without xn): exactly the live (position, tap) blocks are issued."""
    return bool(have_dz_pm) and bool(plan.row_blocks & 2) and bool(getattr(plan, "tile_orders", 0) & L.ORDER_QUAD_BWD_DATA)


def _row_blocks8_forward(geom, plan) -> bool:
    """The forward runs half-plane row-block tiles on 8x8 planes (4 images x 4 rows; kan_plan.hip, plan_conv: `c.rowblk8_fwd`): the block of the plane's
    first / last row is skipped under the tap row that leaves the plane, 1/12 of the MFMA work.  `plan.row_blocks` stays 0 for these geometries."""
    return geom.H == 8 and geom.W == 8 and bool(getattr(plan, "tile_orders", 0) & L.ORDER_ROWBLK8_FWD)


def _pos8_bwd_data(geom, plan) -> bool:
    """bwd-data on 8x8 planes can run tiles of 32 images x 4 columns of a plane row fed from dz_pm (kan_plan.hip, plan_conv: `c.pos8_bd`): exactly the 484 of
    576 (position, tap) blocks with a source are issued.  `plan.dz_pm_wanted` stays 0 for these layers; `_conv_backward` builds the copy where this holds."""
    return bool(getattr(plan, "tile_orders", 0) & L.ORDER_POS8_BWD_DATA)


def _pos8_bwd_weight(geom, plan) -> bool:
    """The weight gradient on 8x8 planes has an entry of its own that issues exactly the 484 of 576 (position, tap) blocks with a source
    (kan_conv_bwd_weight_rowgroups; kan_plan.hip: `c.pos8_bw`), with its own slab count: `plan` stays the other route's."""
    return bool(getattr(plan, "tile_orders", 0) & L.ORDER_POS8_BWD_WEIGHT)


def _executed_flops(geom, plan, which: str, have_dz_pm: bool = False) -> float:
    """Dense count minus the dead (position, tap) products a position-major launch skips (plan.*_target > 0 marks one)."""
    target = {"fwd": plan.fwd_target, "bwd_data": plan.bwd_data_target, "bwd_weight": plan.bwd_weight_target}[which]
    dense = _conv_flops(geom, plan)
    g = geom
    if target <= 0:
        # row-ordered 4x4 launches skip the blocks of the first / last row under the tap row that leaves the plane: 2/3 * 1/4 of the work;
        # the quadrant order skips exactly the dead (position, tap) blocks
        if _quadrant_order(geom, plan, which) or (which == "bwd_data" and _quadrant_bwd_data(geom, plan, have_dz_pm)):
            return dense * _live_fraction(which, g.H, g.W, g.Ho, g.Wo, g.kh, g.kw, g.sh, g.sw, g.ph, g.pw, g.dh, g.dw)
        if plan.row_blocks & _ROW_BLOCK_BIT[which]:
            return dense * (5.0 / 6.0)
        if which == "fwd" and _row_blocks8_forward(geom, plan):
            return dense * (11.0 / 12.0)
        if which == "bwd_data" and have_dz_pm and _pos8_bwd_data(geom, plan):
            return dense * (484.0 / 576.0)
        return dense
    return dense * _live_fraction(which, g.H, g.W, g.Ho, g.Wo, g.kh, g.kw, g.sh, g.sw, g.ph, g.pw, g.dh, g.dw)


def _layer_tag(geom) -> str:
    return f"{geom.C * max(1, geom.groups)}->{geom.O * max(1, geom.groups)}@{geom.H}x{geom.W} k{geom.kh}x{geom.kw}"


def _sample(which: str, geom, plan, pm: bool, two: bool = False, expanded: bool = False):
    """THE place that names a launch: the (name, flops, executed, layer) arguments of `_launch` for the launch the caller makes.
    `which`: "fwd" | "bwd_weight" | "bwd_data"; `pm`: the position-major copies that launch can take were passed; `two`: a second
    input (xn) was passed (the halo weight gradient then is not run); `expanded`: it is the expanded-operand (DMA) entry point."""
    tile = "128" if plan.Opad % 128 == 0 else "64"
    if which == "bwd_data":
        name = "k_conv_bwd_data"
    elif expanded:
        name = f"k_conv_{which}_pmdma/o{tile}"
    elif plan.fwd_band if which == "fwd" else plan.bwd_weight_band:
        # band kernel tiles: 128 outputs where they fit, 192 for exactly 192, else 64 (kan_direct.hip); the weight gradient takes the
        # band route only where the forward does (kan_plan.hip: band_bw implies band), so one tag rule serves both
        name = f"k_band_{which}/o" + ("128" if plan.Opad % 128 == 0 else "192" if plan.Opad == 192 else "64")
    else:
        halo = plan.fwd_halo if which == "fwd" else (plan.bwd_weight_halo and not two)
        name = f"k_conv_{which}{'_halo' if halo else ''}/o{tile}"
    # zero products are skipped by the expanded launches, by launches that got their position-major copies, and by the row-ordered 4x4 ones
    skips = expanded or pm or bool(plan.row_blocks & _ROW_BLOCK_BIT[which]) or (which == "fwd" and _row_blocks8_forward(geom, plan))
    dense = _conv_flops(geom, plan)
    return name, dense, _executed_flops(geom, plan, which, pm) if skips else dense, _layer_tag(geom)


# --------------------------------------------------------------------------------------- raw stages
def _position_major(t: torch.Tensor, ch_off: int, Cn: int) -> torch.Tensor:
    """[Cn*H*W][B] copy of channels [ch_off, ch_off+Cn) of an NCHW tensor (kan_position_major)."""
    B, Ct, H, W = t.shape
    out = torch.empty(Cn * H * W * B, device=t.device, dtype=torch.float32)
    L.check(L.load().kan_position_major(_ptr(t, ch_off * H * W), _ptr(out), B, Cn, H * W, Ct * H * W, _stream(t)), "kan_position_major")
    return out


def _stack(ws: Sequence[Optional[torch.Tensor]]) -> Optional[torch.Tensor]:
    """Per-group weights -> one [G, ...] block (a view for G == 1)."""
    if ws[0] is None:
        return None
    return ws[0].unsqueeze(0) if len(ws) == 1 else torch.stack(list(ws))


# --------------------------------------------------------------------------------------- persistent packed weights
# The kernels read the weights in two GEMM layouts (wp forward, wd bwd-data) that only change when the weights do.  Single-group
# layers keep both layouts alive between calls and re-pack on demand:
#   * host side, a change of tensor identity, storage address or autograd version counter (every in-place op, optimizer step,
#     load_state_dict; FusedAdamW bumps the counters of the parameters it updates through raw pointers) forces a re-pack;
#   * device side, every call fingerprints the reference-layout weights (kan_pack_weights_cached: one pass over the bytes,
#     ~20 us for an 85 MB layer) and the pack kernels return at once when the fingerprint equals the previous call's.  This is
#     what catches writes the version counter cannot see -- `p.data.mul_()`, `dist.broadcast(p.data)`, EMA idioms, any
#     raw-pointer writer.  KAN_PACK_SAMPLE=n (> 1) fingerprints every n-th group of four elements instead of all of them.
# KAN_PACK_CACHE=0 disables the cache (pack on every call); otherwise it is the number of (layer, packed layout) entries kept (LRU),
# bounded in bytes as well by KAN_PACK_CACHE_BYTES (default 16 GiB of the 288 GB).  An entry is keyed by what FIXES the packed layouts
# (channels, outputs, planes, kernel, step shape, halo pair order) -- not by batch size or resolution, so a last partial batch, another
# evaluation batch size or variable-size inputs share one copy of each layer's layouts instead of adding ~0.66 GB per shape for KAN-VGG11.
_PACKED: "OrderedDict[tuple, PackedWeights]" = OrderedDict()
_PACK_CACHE_MAX = int(os.environ.get("KAN_PACK_CACHE", "256"))
_PACK_CACHE_BYTES = int(os.environ.get("KAN_PACK_CACHE_BYTES", str(16 << 30)))
_PACK_SAMPLE = max(1, int(os.environ.get("KAN_PACK_SAMPLE", "1")))
# How often the device-side fingerprint runs for a layer whose HOST stamps (tensor identity, address, version counter) have not moved:
# 1 = on every call (332 MB of weight reads + two early-exit pack launches per KAN-VGG11 step: 0.19 ms of 15.4); N = on every N-th call --
# a write the version counters cannot see (`p.data.mul_()`, a raw copy into the storage) is then picked up at the next verification at the
# latest, and at once after `weights_changed()`; 0 = never (stamps only).  Every write autograd / the optimizers can see (in-place ops,
# load_state_dict, torch.optim, FusedAdamW) moves a stamp and re-packs on the next call whatever this is set to.
_PACK_VERIFY_EVERY = int(os.environ.get("KAN_PACK_VERIFY_EVERY", "16"))
_EPOCH = 0
PACK_STATS = {"calls": 0, "forced": 0, "skipped": 0}  # host-side counters (tests, tools)


_ALWAYS_PACK = False


@contextlib.contextmanager
def always_pack():
    """Inside: every conv stage packs its weights unconditionally (the pack kernels are enqueued whatever the host-side stamps say).  For code that
    RECORDS launches for later replay -- a HIP graph (`train.GraphedStep`): the decision "weights unchanged, skip the pack" is taken on the host at
    record time and would be frozen into the graph, so a replay after an optimizer step would multiply stale layouts."""
    global _ALWAYS_PACK
    prev, _ALWAYS_PACK = _ALWAYS_PACK, True
    try:
        yield
    finally:
        _ALWAYS_PACK = prev


# --------------------------------------------------------------------------------------- opt-in split precision
# Three conv launches have a split-precision twin in csrc/kan_split.hip: the forward, the input gradient, the weight gradient.  Everything the host adds
# to them is in this section: ONE switch record and the six public contexts that set its fields, ONE scope rule, ONE cut-weight cache class (an
# instance per launch that reads cut weights), the three public entry points, and ONE per-stage decision that both autograd Functions take.
@dataclass(frozen=True)
class SplitMode:
    """Which launches of the layers in scope run in split precision.  Immutable: a context swaps the whole record and puts back the one it found."""
    inference: bool = False       # the forward of a fused stage, under no_grad only
    fwd: bool = False             # the forward, in any grad mode
    bwd_data: bool = False        # the input gradient
    bwd_weight: bool = False      # the weight gradients


_SPLIT = SplitMode()


@contextlib.contextmanager
def _split(**on):
    """Inside: `_SPLIT` with the named fields True, every other field as found; on exit, the record that was found."""
    global _SPLIT
    prev, _SPLIT = _SPLIT, replace(_SPLIT, **on)
    try:
        yield
    finally:
        _SPLIT = prev


def split_precision_inference():
    """OPT-IN, inference only: inside, a fused conv + InstanceNorm + PReLU stage whose inputs need no gradient (torch.no_grad() / eval serving) and whose
    geometry is in scope of `kan_conv_fwd_split` (default B-spline spec on 8x8 / 16x16 planes, 3x3 / stride 1 / pad 1, one group, C % 8 == 0, O % 128 == 0,
    even batch on 8x8) runs its conv stage in split precision (3 x bf16 pieces, six bf16 MFMA products; ~4e-6 of the largest pre-norm value from the exact result, 1.7x
    faster).  Everything else -- every other layer, and every training step -- stays on exact fp32 MFMA.  Never on by default."""
    return _split(inference=True)


def split_precision_forward():
    """OPT-IN, training and inference: inside, a conv stage (`kan_conv`, `kan_conv_in_prelu`) in scope of `kan_conv_fwd_split` (one group, base branch, no
    second input, no phases, no plane windows, `kan_split_supported`: default B-spline spec on 8x8 / 16x16 planes, 3x3 / stride 1 / pad 1, C % 8 == 0,
    O % 128 == 0, even batch on 8x8) runs its FORWARD in split precision (3 x bf16 pieces, six bf16 MFMA products), with grad mode on or off.  Its backward
    stays the exact one -- the forward hands it what it needs -- unless the backward contexts are entered too (`split_precision_training`).  Every other
    layer stays on exact fp32 MFMA.  Never on by default."""
    return _split(fwd=True)


def split_precision_backward_data():
    """OPT-IN, training: a conv autograd Function whose FORWARD runs inside with grad mode on (the decision is taken there, as autocast takes it), whose
    input needs a gradient and whose stage is in scope of `kan_conv_bwd_data_split` (one group, base branch, no second input, no phases, no plane
    windows, `kan_split_supported`: default B-spline spec on 8x8 / 16x16 planes, 3x3 / stride 1 / pad 1, C % 8 == 0, O % 128 == 0, even batch on 8x8)
    computes its INPUT gradient in split precision (3 x bf16 pieces, six bf16 MFMA products).  The forward, the weight gradient and every other layer
    stay on exact fp32 MFMA.  Never on by default."""
    return _split(bwd_data=True)


def split_precision_backward_weight():
    """OPT-IN, training: a conv autograd Function whose FORWARD runs inside (the decision is taken there and carried on the autograd node, so a backward
    run outside still takes it), whose weights need a gradient and whose stage is in scope of `kan_conv_bwd_weight_split` (one group, base branch, no
    second input, no phases, no plane windows, `kan_split_supported`: default B-spline spec on 8x8 / 16x16 planes, 3x3 / stride 1 / pad 1, C % 8 == 0,
    O % 128 == 0, even batch on 8x8) computes its WEIGHT gradient in split precision (3 x bf16 pieces, six bf16 MFMA products), straight into the tensors
    the exact path would fill (GRAD_SINKS included).  The forward, the input gradient and every other layer stay on exact fp32 MFMA.  Never on by default."""
    return _split(bwd_weight=True)


def split_precision_backward():
    """`split_precision_backward_data` and `split_precision_backward_weight` at once: the whole backward of the layers in scope."""
    return _split(bwd_data=True, bwd_weight=True)


def split_precision_training():
    """`split_precision_forward`, `split_precision_backward_data` and `split_precision_backward_weight` at once: all three conv launches of the layers in
    scope, for a training step run inside (`train.train_step(..., split_precision=True)`).  `split_precision_inference` is a switch of its own."""
    return _split(fwd=True, bwd_data=True, bwd_weight=True)


# THE sentence that states the scope (every refusal quotes it), and THE rule (every launch asks it).
_SPLIT_SCOPE = ("default B-spline spec (grid 5, order 3, SiLU base branch), 8x8 or 16x16 planes, 3x3 / stride 1 / pad 1, one group, no second input, no phases, "
                "no plane window, C % 8 == 0, O % 128 == 0, even batch on 8x8 planes")


def _split_scope(spec: ConvSpec, x: torch.Tensor, xn, phases, Og: int):
    """(geom, basis) of a stage the split-precision launches take, None for every other: the host conditions, then the library's (`kan_split_supported`).
    Each launch then asks its own byte count, which is 0 where that launch is over its size limit."""
    if spec.groups != 1 or not spec.has_base or xn is not None or phases is not None or x.dim() != 4 or spec.first or spec.w_layout == W_IOD:
        return None
    geom, basis, _ = _plan_cached(*_plan_key(spec, x.shape, Og))
    return (geom, basis) if L.load().kan_split_supported(C.byref(geom), C.byref(basis)) else None


def _split_launch(which: str, nbytes_export: str, spec: ConvSpec, x: torch.Tensor, Og: Optional[int] = None, dz: Optional[torch.Tensor] = None):
    """(geom, basis, byte count of `nbytes_export`) for a public entry point, or its refusal: the stage out of scope or over the launch's size limit, or
    (the two backward launches, which take the output count from it) a `dz` that is not the stage's output gradient."""
    if dz is not None:
        if x.dim() != 4 or dz.dim() != 4:
            raise L.KanConvError(f"split-precision {which}: NCHW x and dz, got {tuple(x.shape)} and {tuple(dz.shape)}")
        Og = dz.shape[1]
    scope = _split_scope(spec, x, None, None, Og)
    nbytes = _split_bytes(nbytes_export, *scope) if scope is not None else 0
    if not nbytes:
        raise L.KanConvError(f"split-precision {which}: {_SPLIT_SCOPE} only")
    geom, basis = scope
    if dz is not None and tuple(dz.shape) != (geom.B, Og, geom.Ho, geom.Wo):
        raise L.KanConvError(f"split-precision {which}: dz {tuple(dz.shape)} != {(geom.B, Og, geom.Ho, geom.Wo)}")
    return geom, basis, nbytes


def _split_bytes(nbytes_export: str, geom, basis) -> int:
    """A launch's own byte-count export: 0 where it does not take the stage (out of scope, or over its size limit)."""
    return getattr(L.load(), nbytes_export)(C.byref(geom), C.byref(basis))


def _cut_weights(nbytes_export: str, pack_export: str, geom, basis, w_base: torch.Tensor, w_basis: torch.Tensor, buf: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The weights cut into bf16 pieces by `pack_export`, into `buf` (allocated when None)."""
    if buf is None:
        buf = torch.empty(_split_bytes(nbytes_export, geom, basis), device=w_base.device, dtype=torch.uint8)
    L.check(getattr(L.load(), pack_export)(_ptr(w_base), _ptr(w_basis), C.c_void_p(buf.data_ptr()), C.byref(geom), C.byref(basis), _stream(w_base)), pack_export)
    return buf


_cut_weights_fwd = partial(_cut_weights, "kan_split_weight_bytes", "kan_split_pack_weights")
_cut_weights_bwd_data = partial(_cut_weights, "kan_split_bwd_data_weight_bytes", "kan_split_pack_weights_bwd_data")


class CutWeightCache:
    """The cut weights of one split-precision launch, per weight pair.  `nbytes(geom, basis)`: the size of the cut (0: the launch does not take the stage);
    `pack(geom, basis, w_base, w_basis, buf)`: the cut, into `buf`.  ONE buffer per pair: re-cut in place when a version stamp of the two owners or the
    `weights_changed()` epoch moved and, under `always_pack` (a recorded step), unconditionally -- a replay cuts the weights as they are then, into the
    address it was recorded with; reallocated only when its size is wrong.  At most `bound` pairs, the least recently used goes first."""

    def __init__(self, nbytes, pack, bound: int = 16):
        self.nbytes, self.pack, self.bound = nbytes, pack, bound
        self.entries: "OrderedDict" = OrderedDict()      # (weight addresses, device index) -> (version stamps and epoch, cut weights)

    def get(self, geom, basis, wb: torch.Tensor, ws: torch.Tensor) -> Optional[torch.Tensor]:
        nbytes = self.nbytes(geom, basis)
        if not nbytes:
            return None
        key = (wb.data_ptr(), ws.data_ptr(), wb.device.index)
        stamps = (_owner(wb)._version, _owner(ws)._version, _EPOCH)
        ent = self.entries.get(key)
        if ent is None:                                     # drop the entry when a weight tensor dies: another model's weights may get the same addresses and stamps
            for o in (_owner(wb), _owner(ws)):
                weakref.finalize(o, self.entries.pop, key, None)
        buf = ent[1] if ent is not None and ent[1].numel() == nbytes else None
        if buf is None or ent[0] != stamps or _ALWAYS_PACK:
            if buf is None:
                buf = torch.empty(nbytes, device=wb.device, dtype=torch.uint8)
            self.pack(geom, basis, wb, ws, buf)
        self.entries[key] = (stamps, buf)
        self.entries.move_to_end(key)
        while len(self.entries) > self.bound:
            self.entries.popitem(last=False)
        return buf


_CUT_FWD = CutWeightCache(partial(_split_bytes, "kan_split_weight_bytes"), _cut_weights_fwd)
_CUT_BWD_DATA = CutWeightCache(partial(_split_bytes, "kan_split_bwd_data_weight_bytes"), _cut_weights_bwd_data)


def _split_fwd_keeps(spec: ConvSpec, x: torch.Tensor, w_base, w_basis, exact_x: bool, exact_w: bool):
    """(wd, x_pm, plan): what a split-precision forward hands an EXACT backward, without the exact forward launch -- the bwd-data weight layout from `_pack`
    when an exact input gradient will run, the position-major x where the plan wants it when an exact weight gradient will.  With both gradients split
    (or not needed) nothing is packed."""
    plan_key = _plan_key(spec, x.shape, w_basis[0].shape[0])
    geom, basis, plan = _plan_cached(*plan_key)
    wd = x_pm = None
    if exact_x:
        _, wd = _pack(L.load(), spec, geom, basis, plan, plan_key, w_base, w_basis, True, None, x.device, _stream(x))      # (B-spline: no device table)
    if exact_w and plan.x_pm_wanted:
        x_pm = _position_major(x, 0, x.shape[1])
    return wd, x_pm, plan


class SplitStage(NamedTuple):
    """What `_split_decision` settled for one conv stage."""
    z: Optional[torch.Tensor] = None          # [B, O, H, W] pre-norm values of the split-precision forward, which has then run; None: the exact forward is due
    wcd: Optional[torch.Tensor] = None        # cut weights for kan_conv_bwd_data_split; None: the input gradient is the exact one
    dw_split: bool = False                    # the weight gradients come from kan_conv_bwd_weight_split


_NOTHING_SPLIT = SplitStage()


def _split_decision(spec: ConvSpec, x: torch.Tensor, xn, phases, w_base, w_basis, want_fwd: bool, need_dgrad: bool, need_w: bool) -> SplitStage:
    """Which of a stage's three conv launches run in split precision, taken in the autograd forward (as autocast takes its own) and carried on the node, so a
    backward run outside the contexts still follows it.  `want_fwd`: the caller saw `split_precision_forward` (or `split_precision_inference` under no_grad);
    `need_dgrad` / `need_w` come from ctx.needs_input_grad: False whenever the caller's grad mode is off.  With no switch on it returns before any plan
    lookup or library call.  The three public entry points are reached through the module globals (the tests' spies replace them)."""
    want_x, want_w = _SPLIT.bwd_data and need_dgrad, _SPLIT.bwd_weight and need_w
    if not (want_fwd or want_x or want_w):
        return _NOTHING_SPLIT
    scope = _split_scope(spec, x, xn, phases, w_basis[0].shape[0])
    if scope is None:
        return _NOTHING_SPLIT
    geom, basis = scope
    wb, ws = w_base[0], w_basis[0]
    wcd = _CUT_BWD_DATA.get(geom, basis, wb, ws) if want_x else None
    dw_split = bool(want_w and _split_bytes("kan_split_bwd_weight_workspace_bytes", geom, basis) > 0)
    wc = _CUT_FWD.get(geom, basis, wb, ws) if want_fwd else None
    z = kan_conv_fwd_split(spec, x, wb, ws, wc)[0] if wc is not None else None
    return SplitStage(z, wcd, dw_split)


def _conv_forward_or_split(spec: ConvSpec, x, xn, phases, w_base, w_basis, want_fwd: bool, need_dgrad: bool, need_w: bool):
    """The forward of a conv stage under `_split_decision`.  Returns (z_slabs [S,B,O,Ho,Wo], (bwd-data weight layout or None, position-major x or None), plan,
    the SplitStage): after a split-precision forward (one slab) the pair holds what the EXACT launches of the backward will read, no more."""
    split = _split_decision(spec, x, xn, phases, w_base, w_basis, want_fwd, need_dgrad, need_w)
    if split.z is None:
        zs, packed, _, _, plan = _conv_forward(spec, x, xn, w_base, w_basis, need_dgrad, phases)
        return zs, packed, plan, split
    wd, x_pm, plan = _split_fwd_keeps(spec, x, w_base, w_basis, need_dgrad and split.wcd is None, need_w and not split.dw_split)
    return split.z.unsqueeze(0), (wd, x_pm), plan, split


def kan_conv_fwd_split(spec: ConvSpec, x: torch.Tensor, w_base: torch.Tensor, w_basis: torch.Tensor, wc: Optional[torch.Tensor] = None):
    """OPT-IN split-precision conv stage (forward only, no autograd; kanconv.h `kan_conv_fwd_split`): the fp32 result of `kan_conv` to ~4e-6 of its largest
    element, through 3 x bf16 pieces and six bf16 MFMA products per k-block.  The layers take it only inside `split_precision_inference` /
    `split_precision_forward`; scope: `_SPLIT_SCOPE` (raises KanConvError otherwise).  Returns (z, wc): pass `wc` back while the weights are unchanged to
    skip the cut (0.05 ms at 256 -> 256)."""
    lib = L.load()
    x, w_base, w_basis = _require(x, "x"), _require(w_base, "w_base"), _require(w_basis, "w_basis")
    Ot = w_basis.shape[0]
    geom, basis, _ = _split_launch("forward", "kan_split_weight_bytes", spec, x, Ot)
    with torch.cuda.device(x.device):
        if wc is None:
            wc = _cut_weights_fwd(geom, basis, w_base, w_basis)
        z = torch.empty((geom.B, Ot, geom.H, geom.W), device=x.device, dtype=torch.float32)
        L.check(lib.kan_conv_fwd_split(_ptr(x), C.c_void_p(wc.data_ptr()), _ptr(z), C.byref(geom), C.byref(basis), _stream(x)), "kan_conv_fwd_split")
    return z, wc


def kan_conv_bwd_data_split(spec: ConvSpec, x: torch.Tensor, dz: torch.Tensor, w_base: Optional[torch.Tensor], w_basis: Optional[torch.Tensor],
                            wcd: Optional[torch.Tensor] = None):
    """OPT-IN split-precision input gradient of the conv stage (no autograd; kanconv.h `kan_conv_bwd_data_split`): what the backward of `kan_conv` returns for
    x, through 3 x bf16 pieces of dz and the weights and six bf16 MFMA products per k-block; the derivative planes are the exact kernel's.  Scope: that of
    `kan_conv_fwd_split` (raises KanConvError otherwise).  Returns (dx, wcd): pass `wcd` back while the weights are unchanged to skip the cut (the
    weights may then be None)."""
    lib = L.load()
    x, dz = _require(x, "x"), _require(dz, "dz")
    geom, basis, nbytes = _split_launch("bwd-data", "kan_split_bwd_data_weight_bytes", spec, x, dz=dz)
    with torch.cuda.device(x.device):
        if wcd is None:
            wcd = _cut_weights_bwd_data(geom, basis, _require(w_base, "w_base"), _require(w_basis, "w_basis"))
        elif wcd.numel() != nbytes or wcd.dtype != torch.uint8 or wcd.device != x.device:
            raise L.KanConvError(f"split-precision bwd-data: wcd must hold {nbytes} bytes on {x.device}")
        dx = torch.empty_like(x)
        L.check(lib.kan_conv_bwd_data_split(_ptr(dz), _ptr(x), C.c_void_p(wcd.data_ptr()), _ptr(dx), C.byref(geom), C.byref(basis), _stream(x)), "kan_conv_bwd_data_split")
    return dx, wcd


def kan_conv_bwd_weight_split(spec: ConvSpec, x: torch.Tensor, dz: torch.Tensor, out=None):
    """OPT-IN split-precision weight gradient of the conv stage (no autograd; kanconv.h `kan_conv_bwd_weight_split`): what the backward of `kan_conv` returns
    for the base / spline weights, through 3 x bf16 pieces of the plane values (the exact kernel's) and of dz and six bf16 MFMA products per k-block.  Scope:
    that of `kan_conv_fwd_split` (raises KanConvError otherwise).  Returns (dw_base [O, C, 3, 3], dw_basis [O, C * 8, 3, 3]); `out`: a pair of contiguous
    fp32 tensors of those shapes to write into.  The workspace (cut dz + depth-split partial sums) comes from torch's allocator on the current stream."""
    lib = L.load()
    x, dz = _require(x, "x"), _require(dz, "dz")
    geom, basis, nbytes = _split_launch("bwd-weight", "kan_split_bwd_weight_workspace_bytes", spec, x, dz=dz)
    Ot, Ct = dz.shape[1], x.shape[1]
    shapes = ((Ot, Ct, 3, 3), (Ot, Ct * spec.n_basis, 3, 3))
    with torch.cuda.device(x.device):
        if out is None:
            out = tuple(torch.empty(sh, device=x.device, dtype=torch.float32) for sh in shapes)
        elif any(tuple(t.shape) != sh or t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous() for t, sh in zip(out, shapes)):
            raise L.KanConvError(f"split-precision bwd-weight: out must be contiguous fp32 tensors {shapes} on {x.device}")
        ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
        L.check(lib.kan_conv_bwd_weight_split(_ptr(dz), _ptr(x), _ptr(out[0]), _ptr(out[1]), C.c_void_p(ws.data_ptr()), C.byref(geom), C.byref(basis), _stream(x)),
                "kan_conv_bwd_weight_split")
    return out[0], out[1]


def weights_changed() -> None:
    """Tell the packed-weight cache that weights may have been written through a path the version counters cannot see (`.data` ops,
    `dist.broadcast(p.data)`, raw-pointer kernels): every layer fingerprints its weights on its next call."""
    global _EPOCH
    _EPOCH += 1


class PackedWeights:
    __slots__ = ("wp", "wd", "ring", "cur", "stamps", "epoch", "unverified")

    def __init__(self):
        self.wp = self.wd = self.ring = None
        self.cur, self.stamps = 0, None
        self.epoch, self.unverified = -1, 0           # weights_changed() epoch of the last device-side check; calls since then

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.wp, self.wd) if t is not None)


def _layout_key(spec: "ConvSpec", geom, plan) -> tuple:
    """What the packed layouts wp / wd depend on (kanconv.hip: wp_row, k_pack_bwd_data): the per-group channel / output counts, the
    step shape (IPC, KC), the padded dims, and whether the forward uses the halo kernels' pair order.  B, H, W enter only through those."""
    return (spec, geom.C, geom.O, plan.P, plan.IPC, plan.KC, plan.Kpad, plan.Opad, plan.fwd_halo, plan.fwd_band, plan.packed_weight_bytes, plan.bwd_data_weight_bytes)


@lru_cache(maxsize=512)
def _cacheable(plan_key) -> bool:
    geom, basis, _ = _plan_cached(*plan_key)
    return bool(L.load().kan_pack_cacheable(C.byref(geom), C.byref(basis)))


def _owner(w: torch.Tensor) -> torch.Tensor:
    """The tensor that owns the storage (1-D layers hand in `weight.unsqueeze(2)` views, fresh objects on every call)."""
    return w._base if w._base is not None else w


def _packed_entry(key, owners):
    ent = _PACKED.get(key)
    if ent is None:
        ent = PackedWeights()
        _PACKED[key] = ent
        for o in owners:                              # drop the layouts when a weight tensor dies
            weakref.finalize(o, _PACKED.pop, key, None)
        while len(_PACKED) > _PACK_CACHE_MAX or (len(_PACKED) > 1 and sum(e.nbytes() for e in _PACKED.values()) > _PACK_CACHE_BYTES):
            _PACKED.popitem(last=False)
    else:
        _PACKED.move_to_end(key)
    return ent


def _pack(lib, spec, geom, basis, plan, plan_key, w_base, w_basis, need_dgrad, phases, device, st):
    """Returns (wp, wd or None): packed afresh, or the layer's persistent layouts brought up to date."""
    def fresh():
        wp = torch.empty(plan.packed_weight_bytes // 4, device=device, dtype=torch.float32)
        wd = torch.empty(plan.bwd_data_weight_bytes // 4, device=device, dtype=torch.float32) if need_dgrad else None
        wb_all, ws_all = _stack(w_base), _stack(w_basis)          # keep the stacked copies alive until the pack is enqueued
        L.check(lib.kan_pack_weights(_ptr(wb_all), _ptr(ws_all), _ptr(wp), _ptr(wd), C.byref(geom), C.byref(basis), st), "kan_pack_weights")
        return wp, wd
    if spec.w_layout == W_IOD:
        # packed afresh on every call: no _PACKED entry, no fingerprint ring (caching this layout is not built yet)
        wp = torch.empty(plan.packed_weight_bytes // 4, device=device, dtype=torch.float32)
        wd = torch.empty(plan.bwd_data_weight_bytes // 4, device=device, dtype=torch.float32) if need_dgrad else None
        L.check(lib.kan_pack_weights_iod(_ptr(w_basis[0]), _ptr(wp), _ptr(wd), C.byref(geom), C.byref(basis), st), "kan_pack_weights_iod")
        return wp, wd
    if _PACK_CACHE_MAX <= 0 or spec.groups != 1 or phases is not None or not _cacheable(plan_key):
        return fresh()
    ws, wb = w_basis[0], w_base[0]
    if (ws.data_ptr() | (wb.data_ptr() if wb is not None else 0)) & 15:
        return fresh()
    owners = [_owner(w) for w in (wb, ws) if w is not None]
    if not all(o.is_leaf for o in owners):            # a per-call temporary of the autograd graph (weight slices made contiguous, re-ordered
        return fresh()                                # plane-major weights): an entry would be built and dropped on every call
    ent = _packed_entry((_layout_key(spec, geom, plan), device.index) + tuple(id(o) for o in owners), owners)
    stamps = [(w.data_ptr(), o._version, tuple(w.shape)) for w, o in zip((w for w in (wb, ws) if w is not None), owners)]
    force = _ALWAYS_PACK or ent.wp is None or ent.stamps != stamps or (need_dgrad and ent.wd is None)
    if ent.wp is None:
        ent.wp = torch.empty(plan.packed_weight_bytes // 4, device=device, dtype=torch.float32)
        ent.ring = torch.zeros(L.KAN_FP_WORDS, device=device, dtype=torch.int64)
    if need_dgrad and ent.wd is None:
        ent.wd = torch.empty(plan.bwd_data_weight_bytes // 4, device=device, dtype=torch.float32)
    if not force and ent.epoch == _EPOCH and _PACK_VERIFY_EVERY != 1 and (_PACK_VERIFY_EVERY == 0 or ent.unverified + 1 < _PACK_VERIFY_EVERY):
        ent.unverified += 1                           # host stamps unchanged and verified recently: no fingerprint, no pack launch
        PACK_STATS["skipped"] += 1
        return ent.wp, (ent.wd if need_dgrad else None)
    ent.epoch, ent.unverified = _EPOCH, 0
    if force:                                         # a graph that saved the old layouts must not be differentiated any more:
        for t in (ent.wp, ent.wd):                    # autograd's saved-tensor version check raises, as it would for the weights
            if t is not None:
                torch.autograd.graph.increment_version(t)
    # once the bwd-data layout exists it is kept in step with wp on every call (a call that skipped it could re-pack wp alone)
    L.check(lib.kan_pack_weights_cached(_ptr(wb), _ptr(ws), _ptr(ent.wp), _ptr(ent.wd), C.byref(geom), C.byref(basis),
                                        C.c_void_p(ent.ring.data_ptr()), ent.cur, int(force), _PACK_SAMPLE, st), "kan_pack_weights_cached")
    PACK_STATS["calls"] += 1
    PACK_STATS["forced"] += int(force)
    ent.cur = (ent.cur + 1) % 3
    ent.stamps = stamps
    return ent.wp, (ent.wd if need_dgrad else None)


def _conv_forward(spec: ConvSpec, x, xn, w_base, w_basis, need_dgrad: bool = True, phases=None):
    """Returns (z_slabs [S,B,O,Ho,Wo], (bwd-data weight layout or None, position-major x or None), geom, basis, plan)."""
    lib = L.load()
    Ct = x.shape[1]
    plan_key = _plan_key(spec, x.shape, _outputs(spec, w_basis) // spec.groups)
    geom, basis, plan = _plan_cached(*plan_key)
    basis = _with_table(_with_phases(basis, phases), spec, x.device)
    st = _stream(x)
    z = torch.empty((plan.fwd_splits, geom.B, geom.O * spec.groups, geom.Ho, geom.Wo), device=x.device, dtype=torch.float32)
    wp, wd = _pack(lib, spec, geom, basis, plan, plan_key, w_base, w_basis, need_dgrad, phases, x.device, st)
    if plan.fwd_expanded and xn is None:
        # small padded planes: the expanded position-major operand (kept for the weight gradient), DMA + MFMA forward
        e_pm = _expand_pm(x, geom, basis, plan, st)
        _launch(_sample("fwd", geom, plan, True, expanded=True), x,
                lambda: lib.kan_conv_fwd_expanded(_ptr(e_pm), _ptr(wp), _ptr(z), C.byref(geom), C.byref(basis), st))
        # what the backward keeps: the expanded copy (its weight gradient reads it), or -- when that launch still runs the
        # tap-major position-major kernel -- the plain copy it needs
        return z, (wd, _position_major(x, 0, Ct) if plan.x_pm_wanted else e_pm), geom, basis, plan
    x_pm = _position_major(x, 0, Ct) if (plan.x_pm_wanted and xn is None) else None
    _launch(_sample("fwd", geom, plan, x_pm is not None, xn is not None), x,
            lambda: lib.kan_conv_fwd(_ptr(x), _ptr(xn if xn is not None else x), _ptr(wp), _ptr(z), C.byref(geom), C.byref(basis),
                                     _ptr(x_pm), st))
    return z, (wd, x_pm), geom, basis, plan


def _expand_pm(x, geom, basis, plan, st):
    e_pm = torch.empty(plan.e_pm_elems, device=x.device, dtype=torch.float32)
    L.check(L.load().kan_position_major_expanded(_ptr(x), _ptr(e_pm), C.byref(geom), C.byref(basis), st), "kan_position_major_expanded")
    return e_pm


# --------------------------------------------------------------------------------------- gradient sinks (data parallel)
# parallel/dp.py registers, per weight Parameter, the slice of its all-reduce bucket.  The weight-gradient unpack kernel
# then writes the reference-layout gradient straight into the bucket and autograd adopts that view as .grad: the copy
# "gradient -> bucket" (332 MB read + write per KAN-VGG11 step) disappears.  Single-group layers only (grouped layers
# stack their per-group gradients in one tensor and keep the copy).
class GradSink:
    """One registered sink: `view` is the bucket slice shaped like the Parameter.  `used` is set when a launch has written
    through it and cleared by the reducer's finish(): a Parameter that feeds TWO graph nodes of one backward pass (a shared
    layer) must not have both nodes write the same buffer -- autograd would then sum two aliases of the last gradient."""
    __slots__ = ("ref", "view", "used")

    def __init__(self, ref, view):
        self.ref, self.view, self.used = ref, view, False


GRAD_SINKS: "dict[int, GradSink]" = {}             # id(Parameter) -> its sink


def _sink_for(wid, shape, device):
    ent = GRAD_SINKS.get(wid) if wid is not None else None
    if ent is None or ent.used:
        return None
    p, t = ent.ref(), ent.view
    # only a FIRST gradient may be written in place: with .grad already set autograd accumulates, and the sink would
    # have overwritten the running sum
    if p is None or p.grad is not None or tuple(t.shape) != tuple(shape) or t.device != device or not t.is_contiguous():
        return None
    ent.used = True
    return t


def _conv_backward(spec: ConvSpec, x, xn, packed, dz, need_x: bool, need_xn: bool, need_w: bool, phases=None, mode: int = 0, wids=None, dparams=None, wcd=None, dw_split: bool = False):
    """dz: [B,O,Ho,Wo] contiguous.  Returns (dx, dxn, dw_base list, dw_basis list) -- per-group views of stacked gradients.
    `wids`: ids of the (base, basis) weight Parameters of a single-group layer, for GRAD_SINKS.
    `wcd`, `dw_split`: the forward's SplitStage fields (`_split_decision`): dx comes from kan_conv_bwd_data_split iff `wcd` is given, the weight gradients
    from kan_conv_bwd_weight_split iff `dw_split`."""
    lib = L.load()
    B, Ct, H, W = x.shape
    G = spec.groups
    Cg = Ct // G
    Ot = dz.shape[1]
    Og = Ot // G
    geom, basis, plan = _plan_cached(*_plan_key(spec, x.shape, Og))
    basis = _with_table(_with_phases(basis, phases, mode), spec, x.device)
    kh, kw = spec.kernel
    st = _stream(x)
    xs = xn if xn is not None else x
    wd, x_pm = packed
    dw_base: List[Optional[torch.Tensor]] = [None] * G
    dw_basis: List[Optional[torch.Tensor]] = [None] * G
    split_w = need_w and dw_split                        # which launches run in split precision ...
    split_x = need_x and wcd is not None
    exact_w = need_w and not split_w                     # ... and which exact ones are left: only they read dz_pm
    exact_x = (need_x or need_xn) and not split_x
    # ... or exact bwd-data alone, on the 8x8 planes whose row-segment tiles are fed from it (the copy's time is inside the step)
    dz_pm = _position_major(dz, 0, Ot) if (xn is None and ((plan.dz_pm_wanted and (exact_w or exact_x)) or (exact_x and _pos8_bwd_data(geom, plan)))) else None
    if split_w:                                          # opt-in split-precision weight gradient: no packed slabs, no unpack; same tensors, same sinks
        sb, ss = (_sink_for(wids[0], (Og, Cg, kh, kw), x.device), _sink_for(wids[1], (Og, Cg * spec.n_basis, kh, kw), x.device)) if wids else (None, None)
        dwb = sb if sb is not None else torch.empty((Og, Cg, kh, kw), device=x.device, dtype=torch.float32)
        dws = ss if ss is not None else torch.empty((Og, Cg * spec.n_basis, kh, kw), device=x.device, dtype=torch.float32)
        kan_conv_bwd_weight_split(spec, x, dz, out=(dwb, dws))
        dw_base, dw_basis = list(dwb.unsqueeze(0).unbind(0)), list(dws.unsqueeze(0).unbind(0))       # views, as the exact path returns them
    elif exact_w:
        pos8 = xn is None and spec.w_layout != W_IOD and _pos8_bwd_weight(geom, plan)
        slabs = plan.pos8_bw_slabs * G * plan.K * plan.Opad if pos8 else plan.bwd_weight_splits * plan.bwd_weight_slab_elems
        dwp = torch.empty(slabs, device=x.device, dtype=torch.float32)
        if pos8:
            name, dense, _, tag = _sample("bwd_weight", geom, plan, False)
            _launch(("k_conv_bwd_weight_pos8/" + name.split("/")[1], dense, dense * (484.0 / 576.0), tag), x,
                    lambda: lib.kan_conv_bwd_weight_rowgroups(_ptr(dz), _ptr(x), _ptr(dwp), C.byref(geom), C.byref(basis), st))
        elif plan.bwd_weight_expanded and xn is None and dz_pm is not None:
            # small padded planes: expanded position-major operand, DMA + MFMA weight gradient (kanconv.h)
            e_pm = x_pm if (plan.fwd_expanded and not plan.x_pm_wanted and x_pm is not None and mode == 0) else _expand_pm(x, geom, basis, plan, st)   # the forward's copy, if it kept one (value planes only)
            _launch(_sample("bwd_weight", geom, plan, True, expanded=True), x,
                    lambda: lib.kan_conv_bwd_weight_expanded(_ptr(dz_pm), _ptr(e_pm), _ptr(dwp), C.byref(geom), C.byref(basis), st))
        else:
            _launch(_sample("bwd_weight", geom, plan, x_pm is not None and dz_pm is not None, xn is not None), x,
                    lambda: lib.kan_conv_bwd_weight(_ptr(dz), _ptr(x), _ptr(xs), _ptr(dwp), C.byref(geom), C.byref(basis), _ptr(x_pm),
                                                    _ptr(dz_pm), st))
        if spec.w_layout == W_IOD:                      # the gradient lands in the coefficients' own [I, O, n] layout; no GRAD_SINKS write-through
            dco = torch.empty((Cg, Og, spec.n_basis), device=x.device, dtype=torch.float32)
            L.check(lib.kan_unpack_wgrad_iod(_ptr(dwp), _ptr(dco), C.byref(geom), C.byref(basis), st), "kan_unpack_wgrad_iod")
            dw_basis = [dco]
        else:
            sb = _sink_for(wids[0], (Og, Cg, kh, kw), x.device) if (wids and G == 1 and spec.has_base) else None
            ss = _sink_for(wids[1], (Og, Cg * spec.n_basis, kh, kw), x.device) if (wids and G == 1) else None
            dwb = (sb.unsqueeze(0) if sb is not None else
                   torch.empty((G, Og, Cg, kh, kw), device=x.device, dtype=torch.float32)) if spec.has_base else None
            dws = ss.unsqueeze(0) if ss is not None else torch.empty((G, Og, Cg * spec.n_basis, kh, kw), device=x.device, dtype=torch.float32)
            unpack = lib.kan_unpack_wgrad_rowgroups if pos8 else lib.kan_unpack_wgrad
            L.check(unpack(_ptr(dwp), _ptr(dwb), _ptr(dws), C.byref(geom), C.byref(basis), st), "kan_unpack_wgrad")
            dw_basis = list(dws.unbind(0))
            if spec.has_base:
                dw_base = list(dwb.unbind(0))
    dx = dxn = None
    if split_x:                                          # opt-in split-precision input gradient: one slab, no reduce
        dx, _ = kan_conv_bwd_data_split(spec, x, dz, None, None, wcd)
    elif exact_x:
        S = plan.bwd_data_splits
        separate = xn is not None
        dxs = torch.empty((S, B, Ct, H, W), device=x.device, dtype=torch.float32)
        dxns = torch.empty_like(dxs) if separate else None
        head, tail = (_ptr(dz), _ptr(x), _ptr(xs), _ptr(wd), _ptr(dxs), _ptr(dxns)), (C.byref(geom), C.byref(basis), _ptr(dz_pm), st)
        _launch(_sample("bwd_data", geom, plan, dz_pm is not None), x,
                (lambda: lib.kan_conv_bwd_data(*head, *tail)) if dparams is None else
                (lambda: lib.kan_conv_bwd_data_params(*head, _ptr(dparams), *tail)))
        dx, dxn = _sum_slabs(dxs, B, Ct, H * W), (_sum_slabs(dxns, B, Ct, H * W) if separate else None)
    return dx, dxn, dw_base, dw_basis


def _sum_slabs(slabs: torch.Tensor, B: int, Cn: int, HW: int) -> torch.Tensor:
    """[S,B,Cn,...] partial slabs -> their sum (kan_slab_reduce); S == 1 is a view."""
    if slabs.shape[0] == 1:
        return slabs[0]
    out = torch.empty_like(slabs[0])
    L.check(L.load().kan_slab_reduce(_ptr(slabs), slabs.shape[0], slabs[0].numel(), _ptr(out), B, Cn, HW, Cn * HW, _stream(slabs)),
            "kan_slab_reduce")
    return out


def _flat_grads(spec: ConvSpec, dw_base, dw_basis):
    return tuple(dw_base) + tuple(dw_basis) if spec.has_base else tuple(dw_basis)


# --------------------------------------------------------------------------------------- autograd
def _save(ctx, **named) -> None:
    """save_for_backward of the tensors that are not None, remembered by name (`_saved` returns them)."""
    ctx.saved_names = tuple(k for k, t in named.items() if t is not None)
    ctx.save_for_backward(*(t for t in named.values() if t is not None))


def _once(backward):
    """`once_differentiable` for the backwards of this module, which run raw kernels: differentiating what they return raises torch's
    once-differentiable error instead of silently treating it as a constant.  torch's decorator attaches that error only when an incoming gradient
    carries a graph; under create_graph=True (grad mode is then on in here) with plain incoming gradients -- `autograd.grad(y.sum(), x, create_graph=True)`,
    the gradient-penalty idiom -- the returned gradients would carry no graph and a penalty term added to a loss would contribute nothing, with no
    error.  So in that case the incoming gradients are made to require one."""
    inner = once_differentiable(backward)

    @wraps(backward)
    def wrapper(ctx, *grads):
        if torch.is_grad_enabled() and not any(g is not None and g.requires_grad for g in grads):
            grads = tuple(g.detach().requires_grad_(True) if g is not None else None for g in grads)
        return inner(ctx, *grads)
    return wrapper


def _asked(ctx, grads: tuple) -> tuple:
    """What a backward returns: `grads` with None in every position whose input did not ask for a gradient (ctx.needs_input_grad) -- a kernel that fills
    several gradients at once (the norm parameters, the wavelet parameters, all weight groups) hands back only those that were asked for."""
    return tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad))


def _saved(ctx, *names):
    """The tensors `_save` kept under `names` (None for one that was None), in that order."""
    kept = dict(zip(ctx.saved_names, ctx.saved_tensors))
    return tuple(kept.get(n) for n in names)


def _is_depthwise(spec: ConvSpec, x, w_basis) -> bool:
    """Layers the library runs on its direct depthwise kernels (C = 1 per group, O <= 2, <= 9 taps): no G tile, no epilogue accumulation."""
    return x.shape[1] // spec.groups == 1 and w_basis[0].shape[0] <= 2 and spec.kernel[0] * spec.kernel[1] <= 9


class _KanConv(torch.autograd.Function):
    """z = conv stage.  args: spec, split, x, xn (or None: the basis reads x), phases (or None), *[w_base_g...], *[w_basis_g...]

    `split`: run the forward in split precision where `kan_conv_fwd_split` takes it (`split_precision_forward`); the backward gets what an exact one needs.
    `xn`: a second input -- x feeds the base branch (a host-applied base activation: x = act(input)), xn the basis.
    `phases`: the parameter table of a basis with trainable per-channel parameters, [Cg, 2, n] (phase_low, phase_high per channel) for ReLU-KAN
    (relu_kan_layers.py:118-136), [n] recurrence coefficients for Gram.
    d phase[c][m][j] = sum_{b,pixel} G_{c,j} * d basis_j / d phase_m, where G = dgrad(dz, W_basis) is never materialised:
    the sum is regrouped as  sum_{group,o,tap} W_basis[o][c*n+j][tap] * wgrad(d basis / d phase_m, dz)[o][c*n+j][tap],
    i.e. the weight-gradient kernel run on the parameter-derivative planes, contracted with the weights."""

    @staticmethod
    def forward(ctx, spec: ConvSpec, split: bool, x, xn, phases, *weights):
        x = _require(x, "x")
        xn = _require(xn, "xn") if xn is not None else None
        weights = [_require(w, "weight", align=False) for w in weights]
        w_base, w_basis = _split_weights(spec, weights)
        if spec.w_layout == W_IOD:
            want = (x.shape[1], w_basis[0].shape[1] if w_basis[0].dim() == 3 else -1, spec.n_basis)
            if len(weights) != 1 or tuple(w_basis[0].shape) != want or spec.groups != 1 or spec.kernel != (1, 1) or spec.has_base or phases is not None:
                raise L.KanConvError(f"w_layout = W_IOD takes one [inputs, outputs, n_basis] coefficient tensor, a 1x1 kernel, one group and no base branch; "
                                     f"got {[tuple(w.shape) for w in weights]} for input {tuple(x.shape)}, n_basis {spec.n_basis}")
        if phases is not None:
            phases = _require(phases, "phases")
            want = (x.shape[1] // spec.groups, 2, spec.n_basis) if spec.kind == L.BASIS_RELU else (spec.n_basis,)
            if tuple(phases.shape) != want:
                raise L.KanConvError(f"parameter table {tuple(phases.shape)} != {want} for basis kind {spec.kind}")
        need_dgrad = bool(ctx.needs_input_grad[2] or (xn is not None and ctx.needs_input_grad[3]))         # (0: spec, 1: split, 2: x, 3: xn, 4: phases, 5...: weights)
        need_w = any(ctx.needs_input_grad[5:])
        with torch.cuda.device(x.device):
            zs, (wd, x_pm), _, stage = _conv_forward_or_split(spec, x, xn, phases, w_base, w_basis, split, need_dgrad, need_w)
            z = _sum_slabs(zs, zs.shape[1], zs.shape[2], zs.shape[3] * zs.shape[4])
        ctx.spec, ctx.wsplit = spec, stage.dw_split
        # the basis weights are kept only for the parameter gradient (their version counters are then checked in the backward)
        kept_w = {f"w_basis{g}": w for g, w in enumerate(w_basis)} if phases is not None else {}
        _save(ctx, x=x, xn=xn, phases=phases, wd=wd, x_pm=x_pm, wcd=stage.wcd, **kept_w)
        return z

    @staticmethod
    @_once
    def backward(ctx, dz):
        spec, G = ctx.spec, ctx.spec.groups
        x, xn, phases, wd, x_pm, wcd, *w_basis = _saved(ctx, "x", "xn", "phases", "wd", "x_pm", "wcd", *(f"w_basis{g}" for g in range(G)))
        packed = (wd, x_pm)
        need_x, need_xn = ctx.needs_input_grad[2], xn is not None and ctx.needs_input_grad[3]
        need_p, need_w = ctx.needs_input_grad[4], any(ctx.needs_input_grad[5:])
        dz = _dense(dz)
        dph = None
        with torch.cuda.device(x.device):
            # ReLU-KAN / Gram: when the input gradient is computed anyway, its launch also accumulates the parameter gradients from the same G tiles
            # (kan_conv_bwd_data_params); otherwise (first layer of a model, depthwise groups) two more weight-gradient passes deliver them
            in_epilogue = need_p and (need_x or need_xn) and not _is_depthwise(spec, x, w_basis)
            dpar = None
            if in_epilogue:                                    # ReLU-KAN: [Cg, 2, n] directly; Gram: 64 slot rows of partial sums
                dpar = torch.zeros_like(phases) if spec.kind == L.BASIS_RELU else phases.new_zeros((64, spec.n_basis))
            dx, dxn, dwb, dws = _conv_backward(spec, x, xn, packed, dz, need_x, need_xn, need_w, phases, dparams=dpar, wcd=wcd, dw_split=ctx.wsplit)
            if in_epilogue:
                dph = dpar if spec.kind == L.BASIS_RELU else dpar.sum(dim=0)
            if need_p and not in_epilogue:
                Cg, n = x.shape[1] // G, spec.n_basis
                W = torch.stack(list(w_basis)).view(G, -1, Cg, n, spec.kernel[0] * spec.kernel[1])

                def factor(mode):                               # wgrad of the parameter-derivative planes, times the weights
                    _, _, _, dwm = _conv_backward(spec, x, xn, packed, dz, False, False, True, phases, mode)
                    return W * torch.stack(list(dwm)).view_as(W)
                if spec.kind == L.BASIS_RELU:                  # per-channel phases [Cg, 2, n]
                    dph = torch.stack([factor(mode).sum(dim=(0, 1, 4)) for mode in (1, 2)], dim=1)
                else:                                          # Gram: layer-global coefficients c_2..c_degree (entries 0, 1 unused)
                    dph = torch.zeros_like(phases)
                    for mode in range(1, n - 1):
                        dph[mode + 1] = factor(mode).sum()
        return _asked(ctx, (None, None, dx, dxn, dph) + _flat_grads(spec, dwb, dws))


def _cat(ts: Sequence[Optional[torch.Tensor]]) -> Optional[torch.Tensor]:
    """Per-group vectors -> one contiguous vector (the tensor itself for one group)."""
    if ts[0] is None:
        return None
    return ts[0] if len(ts) == 1 else torch.cat([t.reshape(-1) for t in ts])


# --------------------------------------------------------------------------------------- InstanceNorm / BatchNorm [+ PReLU] [+ max-pool] launchers
# The only callers of the six kan_instnorm_prelu* and the two kan_batchnorm_prelu* entry points.  `pool`: False | True (= MaxPool2d(2, 2), the
# register-resident kernels, even planes only) | (k, s) (= MaxPool2d(k, s), the generic kernels); `groups` > 1: one PReLU slope per C / groups channels.
@dataclass(frozen=True, eq=False)
class BatchStats:
    """What turns a norm launch into a BatchNorm one (`bn=`): the [C] running buffers (None: track_running_stats=False), the momentum of
    their update and the module's training flag.  The kernels update the buffers in place."""
    running_mean: Optional[torch.Tensor]
    running_var: Optional[torch.Tensor]
    momentum: float
    training: bool

    @property
    def batch(self) -> bool:
        """The statistics are the batch's (torch: training, or no running statistics to use instead)."""
        return self.training or self.running_mean is None


def _bn_workspace(B: int, Ct: int, device) -> torch.Tensor:
    return torch.empty(L.load().kan_batchnorm_workspace_bytes(B, Ct), device=device, dtype=torch.uint8)


def _pool_mode(pool, Ho: int, Wo: int):
    """(2, 2) on an even plane runs the register-resident 2x2 kernels."""
    return True if pool == (2, 2) and pool_fusable(True, Ho, Wo) else pool


def _norm_fwd(zs, slab_elems: int, gamma, beta, slope, eps: float, groups: int = 1, pool=False, *, bn: Optional[BatchStats] = None):
    """zs: [S, B, C, H, W] partial slabs `slab_elems` apart, or one [B, C, H, W] tensor.  Returns (y, z, mean, rstd, pidx): z the summed
    pre-norm values (slab 0 itself when there is one slab, else a tensor of their own, so that the S-slab buffer can be freed), pidx the
    uint8 argmax of each pool window (None without a pool).  `bn`: BatchNorm instead of InstanceNorm -- mean and rstd are then [C]."""
    lib = L.load()
    S, z = (1, zs) if zs.dim() == 4 else (zs.shape[0], zs[0])
    B, Ct, Ho, Wo = z.shape
    if z.numel() == 0:                                  # refused here, not by an empty grid (the conv stages stop in kan_plan, the loss at B < 1)
        raise L.KanConvError(f"the norm kernels take a non-empty tensor, got {tuple(z.shape)}")
    HW, span, st = Ho * Wo, (Ct // groups if groups > 1 else 0), _stream(zs)
    mean = torch.empty(B * Ct if bn is None else Ct, device=zs.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    if S > 1:
        z = torch.empty_like(z)
    pool = _pool_mode(pool, Ho, Wo)
    if bn is not None:
        if isinstance(pool, tuple) or (pool and not pool_fusable(True, Ho, Wo)):
            raise L.KanConvError(f"the BatchNorm kernels fuse MaxPool2d(2, 2) on even planes only, got pool {pool!r} on {Ho}x{Wo}")
        if bn.training and B * HW < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(z.shape)}")
        for t in (bn.running_mean, bn.running_var):
            if t is not None and (_require(t, "running statistics") is not t or t.numel() != Ct):
                raise L.KanConvError(f"running statistics must be contiguous, 16-byte aligned [{Ct}] tensors (the kernels update them in place)")
        y = torch.empty((B, Ct, Ho // 2, Wo // 2) if pool else z.shape, device=zs.device, dtype=torch.float32)
        pidx = torch.empty(y.shape, device=zs.device, dtype=torch.uint8) if pool else None
        L.check(lib.kan_batchnorm_prelu_fwd(_ptr(zs), S, slab_elems, _ptr(z), _ptr(gamma), _ptr(beta), _ptr(slope), _ptr(y),
                                            C.c_void_p(pidx.data_ptr() if pool else 0), _ptr(mean), _ptr(rstd), _ptr(bn.running_mean), _ptr(bn.running_var),
                                            C.c_void_p(_bn_workspace(B, Ct, zs.device).data_ptr()), B, Ct, Ho, Wo, Ct * HW, eps, bn.momentum, span,
                                            int(bn.training), st), "kan_batchnorm_prelu_fwd")
        return y, z, mean, rstd, pidx
    if not pool:
        y = torch.empty_like(z)
        L.check(lib.kan_instnorm_prelu_fwd(_ptr(zs), S, slab_elems, _ptr(z), _ptr(gamma), _ptr(beta), _ptr(slope), _ptr(y), _ptr(mean), _ptr(rstd),
                                           B, Ct, HW, Ct * HW, eps, span, st), "kan_instnorm_prelu_fwd")
        return y, z, mean, rstd, None
    pk, ps = pool if isinstance(pool, tuple) else (2, 2)
    if pool is True:
        if not pool_fusable(True, Ho, Wo):
            raise L.KanConvError(f"fused 2x2 max-pool needs an even plane, got {Ho}x{Wo}")
    elif Ho < pk or Wo < pk:
        raise L.KanConvError(f"fused {pk}x{pk} max-pool on a {Ho}x{Wo} plane")
    y = torch.empty((B, Ct, (Ho - pk) // ps + 1, (Wo - pk) // ps + 1), device=zs.device, dtype=torch.float32)
    pidx = torch.empty(y.shape, device=zs.device, dtype=torch.uint8)
    head = (_ptr(zs), S, slab_elems, _ptr(z), _ptr(gamma), _ptr(beta), _ptr(slope), _ptr(y), C.c_void_p(pidx.data_ptr()), _ptr(mean), _ptr(rstd),
            B, Ct, Ho, Wo, Ct * HW, eps, span)
    if pool is True:                                 # the full-size y is never written
        L.check(lib.kan_instnorm_prelu_pool_fwd(*head, st), "kan_instnorm_prelu_pool_fwd")
    else:                                            # overlapping windows allowed (the AlexNet pattern 3, 2)
        L.check(lib.kan_instnorm_prelu_poolk_fwd(*head, pk, ps, st), "kan_instnorm_prelu_poolk_fwd")
    return y, z, mean, rstd, pidx


def _norm_bwd(dy, z, mean, rstd, gamma, beta, slope, pidx, groups: int = 1, pool=False, *, bn: Optional[BatchStats] = None):
    """Backward of `_norm_fwd` from what it returned.  Returns (dz, dgamma, dbeta, dslope), None for a parameter that is None."""
    lib = L.load()
    dy = _dense(dy)
    B, Ct, Ho, Wo = z.shape
    HW, span, st = Ho * Wo, (Ct // groups if groups > 1 else 0), _stream(z)
    dz = torch.empty_like(z)
    dgam, dbet, dslo = ((torch.zeros_like if bn is None else torch.empty_like)(t) if t is not None else None for t in (gamma, beta, slope))
    pool = _pool_mode(pool, Ho, Wo)
    if bn is not None:                                  # (the parameter gradients are written, not accumulated)
        L.check(lib.kan_batchnorm_prelu_bwd(_ptr(dy), C.c_void_p(pidx.data_ptr() if pidx is not None else 0), _ptr(z), _ptr(mean), _ptr(rstd), _ptr(gamma),
                                            _ptr(beta), _ptr(slope), _ptr(dz), _ptr(dgam), _ptr(dbet), _ptr(dslo),
                                            C.c_void_p(_bn_workspace(B, Ct, z.device).data_ptr()), B, Ct, Ho, Wo, Ct * HW, span, int(bn.batch), st),
                "kan_batchnorm_prelu_bwd")
        return dz, dgam, dbet, dslo
    if not pool:
        L.check(lib.kan_instnorm_prelu_bwd(_ptr(dy), _ptr(z), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(slope), _ptr(dz),
                                           _ptr(dgam), _ptr(dbet), _ptr(dslo), B, Ct, HW, Ct * HW, span, st), "kan_instnorm_prelu_bwd")
        return dz, dgam, dbet, dslo
    head = (_ptr(dy), C.c_void_p(pidx.data_ptr()), _ptr(z), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(slope), _ptr(dz),
            _ptr(dgam), _ptr(dbet), _ptr(dslo), B, Ct, Ho, Wo, Ct * HW, span)
    if pool is True:
        L.check(lib.kan_instnorm_prelu_pool_bwd(*head, st), "kan_instnorm_prelu_pool_bwd")
    else:
        L.check(lib.kan_instnorm_prelu_poolk_bwd(*head, pool[0], pool[1], st), "kan_instnorm_prelu_poolk_bwd")
    return dz, dgam, dbet, dslo


class _KanConvInPrelu(torch.autograd.Function):
    """y = [MaxPool2d]([PReLU](InstanceNorm(conv stage))), or BatchNorm in its place.
    args: spec, eps, use_affine, use_prelu, pool, split, bn, x, *[w_base_g], *[w_basis_g], *[gamma_g], *[beta_g], *[prelu_g]
    `split`: run the conv stage in split precision where `kan_conv_fwd_split` takes it (`split_precision_inference` under no_grad, `split_precision_forward`
    in any grad mode); the backward gets what an exact one needs (`_split_fwd_keeps`).
    `bn`: None, or the BatchStats of a BatchNorm tail (running buffers of all groups concatenated)."""

    @staticmethod
    def forward(ctx, spec: ConvSpec, eps: float, use_affine: bool, use_prelu: bool, pool, split: bool, bn, x, *params):
        x = _require(x, "x")
        G = spec.groups
        nw = G * (2 if spec.has_base else 1)
        params = [_require(p, "parameter", align=i >= nw) for i, p in enumerate(params)]
        w_base, w_basis = _split_weights(spec, params[:nw])
        rest = params[nw:]
        gammas = rest[:G] if use_affine else [None] * G
        betas = rest[G:2 * G] if use_affine else [None] * G
        prelus = rest[2 * G * int(use_affine):] if use_prelu else [None] * G
        if use_prelu and any(p.numel() != 1 for p in prelus):
            raise L.KanConvError("only scalar-slope PReLU (nn.PReLU()) is supported, as in kan_layers.py:182")
        with torch.cuda.device(x.device):
            need_x, need_w = bool(ctx.needs_input_grad[7]), any(ctx.needs_input_grad[8:8 + nw])
            zs, (wd, x_pm), plan, stage = _conv_forward_or_split(spec, x, None, None, w_base, w_basis, split, need_x, need_w)
            # all groups in one launch: per-channel gamma/beta concatenated, one PReLU slope per Og channels
            gamma, beta, slope = _cat(gammas), _cat(betas), _cat(prelus)
            y, z, mean, rstd, pidx = _norm_fwd(zs, plan.fwd_slab_elems, gamma, beta, slope, eps, G, pool, bn=bn)
        ctx.spec, ctx.pool, ctx.bn, ctx.wsplit = spec, pool, bn, stage.dw_split
        ctx.wids = (id(w_base[0]) if spec.has_base else None, id(w_basis[0])) if G == 1 else None
        _save(ctx, x=x, z=z, mean=mean, rstd=rstd, wd=wd, x_pm=x_pm, gamma=gamma, beta=beta, slope=slope, pidx=pidx, wcd=stage.wcd)
        return y

    @staticmethod
    @_once
    def backward(ctx, dy):
        spec, G = ctx.spec, ctx.spec.groups
        x, z, mean, rstd, wd, x_pm, gamma, beta, slope, pidx, wcd = _saved(ctx, "x", "z", "mean", "rstd", "wd", "x_pm", "gamma", "beta", "slope", "pidx", "wcd")
        with torch.cuda.device(x.device):
            dz, dgam, dbet, dpre = _norm_bwd(dy, z, mean, rstd, gamma, beta, slope, pidx, G, ctx.pool, bn=ctx.bn)
            nw = G * (2 if spec.has_base else 1)
            need_x = ctx.needs_input_grad[7]
            need_w = any(ctx.needs_input_grad[8:8 + nw])
            dx, _, dwb, dws = _conv_backward(spec, x, None, (wd, x_pm), dz, need_x, False, need_w, wids=ctx.wids, wcd=wcd, dw_split=ctx.wsplit)
        grads = _flat_grads(spec, dwb, dws)
        if gamma is not None:
            grads += tuple(dgam.view(G, -1).unbind(0)) + tuple(dbet.view(G, -1).unbind(0))
        if slope is not None:
            grads += tuple(dpre.view(G, 1).unbind(0))
        return _asked(ctx, (None, None, None, None, None, None, None, dx) + grads)


class _InstanceNorm(torch.autograd.Function):
    """InstanceNorm2d over NCHW, or BatchNorm2d when `bn` is a BatchStats (args: x, gamma|None, beta|None, eps, bn|None)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps: float, bn=None):
        x = _require(x, "x")
        if x.dim() != 4:
            raise L.KanConvError(f"the norm ops take an NCHW tensor, got {tuple(x.shape)}")
        # the public `instance_norm` / `batch_norm`: gamma and beta are the caller's tensors, validated like every other one (a strided view would be
        # read as if it were dense, an fp64 one as fp32, a host address handed to a kernel, a short one read past its end)
        gamma = _require(gamma, "gamma") if gamma is not None else None
        beta = _require(beta, "beta") if beta is not None else None
        for t, n in ((gamma, "gamma"), (beta, "beta")):
            if t is not None and (t.device != x.device or t.numel() != x.shape[1]):
                raise L.KanConvError(f"{n} must hold {x.shape[1]} values on {x.device}, got {tuple(t.shape)} on {t.device}")
        with torch.cuda.device(x.device):
            y, _, mean, rstd, _ = _norm_fwd(x, 0, gamma, beta, None, eps, bn=bn)
        ctx.bn = bn
        _save(ctx, x=x, mean=mean, rstd=rstd, gamma=gamma, beta=beta)
        return y

    @staticmethod
    @_once
    def backward(ctx, dy):
        x, mean, rstd, gamma, beta = _saved(ctx, "x", "mean", "rstd", "gamma", "beta")
        with torch.cuda.device(x.device):
            dx, dg, db, _ = _norm_bwd(dy, x, mean, rstd, gamma, beta, None, None, bn=ctx.bn)
        return _asked(ctx, (dx, dg, db, None, None))


# --------------------------------------------------------------------------------------- Wav-KAN wavelet stage
class _WavStage(torch.autograd.Function):
    """u = sum_{c, taps} w[o, c, tap] * psi((x - trans[o, c]) / scale[o, c]) for one group (wav_kan_layers.py:186-217 and the two
    'fast' variants), on the direct kernels of csrc/wavkan.inc.  x: [B, C, H, W] contiguous; scale, trans: [O, C]; w: [O, C, kh, kw]."""

    @staticmethod
    def _geom(wavelet, x, w, stride, padding, dilation):
        B, Cn, H, W = x.shape
        O, _, kh, kw = w.shape
        Ho = (H + 2 * padding[0] - dilation[0] * (kh - 1) - 1) // stride[0] + 1
        Wo = (W + 2 * padding[1] - dilation[1] * (kw - 1) - 1) // stride[1] + 1
        if Ho <= 0 or Wo <= 0:
            raise L.KanConvError(f"empty output ({Ho}x{Wo}) for input {H}x{W}")
        return L.KanWavGeom(B, Cn, H, W, O, Ho, Wo, kh, kw, stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1],
                            int(wavelet), Cn * H * W, O * Ho * Wo)

    @staticmethod
    def forward(ctx, wavelet, stride, padding, dilation, x, scale, trans, w):
        lib = L.load()
        x, scale, trans, w = (_require(t, n) for t, n in ((x, "x"), (scale, "scale"), (trans, "translation"), (w, "wavelet weights")))
        if x.dim() != 4 or w.dim() != 4 or x.numel() == 0:
            raise L.KanConvError(f"the wavelet stage takes a non-empty NCHW input and [O, C, kh, kw] weights, got {tuple(x.shape)} and {tuple(w.shape)}")
        if scale.shape != (w.shape[0], w.shape[1]) or trans.shape != scale.shape or w.shape[1] != x.shape[1]:
            raise L.KanConvError(f"wavelet parameter shapes {tuple(scale.shape)}, {tuple(trans.shape)}, {tuple(w.shape)} do not match input {tuple(x.shape)}")
        geom = _WavStage._geom(wavelet, x, w, stride, padding, dilation)
        u = torch.empty((geom.B, geom.O, geom.Ho, geom.Wo), device=x.device, dtype=torch.float32)
        L.check(lib.kan_wav_fwd(_ptr(x), _ptr(scale), _ptr(trans), _ptr(w), _ptr(u), C.byref(geom), _stream(x)), "kan_wav_fwd")
        ctx.save_for_backward(x, scale, trans, w)
        ctx.geom = geom
        return u

    @staticmethod
    @_once
    def backward(ctx, du):
        lib = L.load()
        x, scale, trans, w = ctx.saved_tensors
        geom = ctx.geom
        du = _dense(du)
        st = _stream(x)
        dx = dscale = dtrans = dw = None
        if ctx.needs_input_grad[4]:
            dx = torch.empty_like(x)
            L.check(lib.kan_wav_bwd_input(_ptr(du), _ptr(x), _ptr(scale), _ptr(trans), _ptr(w), _ptr(dx), C.byref(geom), st), "kan_wav_bwd_input")
        if any(ctx.needs_input_grad[5:8]):
            ws = torch.empty((lib.kan_wav_param_workspace(C.byref(geom)),), device=x.device, dtype=torch.float32)
            dw, dscale, dtrans = torch.empty_like(w), torch.empty_like(scale), torch.empty_like(trans)
            L.check(lib.kan_wav_bwd_params(_ptr(du), _ptr(x), _ptr(scale), _ptr(trans), _ptr(w), _ptr(dw), _ptr(dscale), _ptr(dtrans), _ptr(ws),
                                           C.byref(geom), st), "kan_wav_bwd_params")
        return _asked(ctx, (None, None, None, None, dx, dscale, dtrans, dw))


def wav_stage(wavelet: int, x: torch.Tensor, scale: torch.Tensor, trans: torch.Tensor, w: torch.Tensor, stride, padding, dilation) -> torch.Tensor:
    return _WavStage.apply(int(wavelet), tuple(stride), tuple(padding), tuple(dilation), x, scale, trans, w)


# --------------------------------------------------------------------------------------- public API
# The kernels address activations with 32-bit byte offsets (buffer loads), so one launch takes tensors below 2 GiB.  Every op
# on this path is independent per image (conv, per-(image, channel) InstanceNorm, PReLU, pooling), so a larger batch is cut
# into the fewest equal-ish runs of whole images that fit and the results are concatenated; autograd sums the weight gradients.
MAX_TENSOR_BYTES = (1 << 31) - 1


def _image_runs(spec: ConvSpec, x: torch.Tensor, out_channels: int) -> Optional[int]:
    """Images per launch if the batch has to be cut (None: it fits)."""
    B, C, H, W = x.shape
    Ho, Wo = spec.out_hw(H, W)
    per_image = 4 * max(C * H * W, out_channels * Ho * Wo)
    if B * per_image <= MAX_TENSOR_BYTES:
        return None
    if per_image > MAX_TENSOR_BYTES:
        raise L.KanConvError(f"one image's activations ({per_image} bytes) exceed the {MAX_TENSOR_BYTES}-byte launch limit")
    fit = MAX_TENSOR_BYTES // per_image               # images one launch can take; equal-ish runs of at most that many
    runs = -(-B // fit)
    return -(-B // runs)


def fits_one_launch(spec: ConvSpec, x: torch.Tensor, w_basis: Sequence[torch.Tensor]) -> bool:
    """The conv stage runs as one launch set, not once per run of images (what a fused BatchNorm tail needs)."""
    return _image_runs(spec, x, _outputs(spec, w_basis)) is None


def _apply(stage, spec: ConvSpec, x, xn, w_base, w_basis, extra=()) -> torch.Tensor:
    """Body of the public entry points: stage(x, xn, *flattened weight lists, *extra), once, or once per run of whole images."""
    ws = (list(w_base) if spec.has_base else []) + list(w_basis) + list(extra)
    n = _image_runs(spec, x, _outputs(spec, w_basis))
    if n is None:
        return stage(x, xn, *ws)
    xs = x.split(n)
    xns = xn.split(n) if xn is not None else [None] * len(xs)
    return torch.cat([stage(a.contiguous(), b.contiguous() if b is not None else None, *ws) for a, b in zip(xs, xns)])


def kan_conv(spec: ConvSpec, x: torch.Tensor, xn: Optional[torch.Tensor], w_base: Sequence[torch.Tensor],
             w_basis: Sequence[torch.Tensor]) -> torch.Tensor:
    split = _SPLIT.fwd                                  # opt-in split-precision forward: decided here, where the caller's flags are visible; each run of images decides its scope
    return _apply(lambda a, b, *ws: _KanConv.apply(spec, split, a, b, None, *ws), spec, x, xn, w_base, w_basis)


def kan_conv_phased(spec: ConvSpec, x: torch.Tensor, phases: torch.Tensor, w_base: Sequence[torch.Tensor],
                    w_basis: Sequence[torch.Tensor], xn: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Conv stage of a basis with trainable parameters held in device memory, differentiable in them: ReLU-KAN
    (`phases` = [channels per group, 2, n_basis]: low, high) or Gram (`phases` = [n_basis] recurrence coefficients c_k)."""
    return _apply(lambda a, b, *ws: _KanConv.apply(spec, False, a, b, phases, *ws), spec, x, xn, w_base, w_basis)


def pool_fusable(pool, ho: int, wo: int, batchnorm: bool = False) -> bool:
    """THE rule for whether the InstanceNorm(+PReLU) kernels can apply the max-pool `pool` to a ho x wo plane: a (k, s) window always
    (the generic kernels), True = MaxPool2d(2, 2) only on an even plane (the register-resident 2x2 kernels).  The layers ask before they
    request a fused pool; `_norm_fwd` refuses a request that breaks it.  `batchnorm`: the BatchNorm kernels, which fuse MaxPool2d(2, 2)
    on an even plane and nothing else."""
    even = ho % 2 == 0 and wo % 2 == 0
    if batchnorm:
        return even and (pool is True or tuple(pool) == (2, 2))
    return pool is not True or even


def _norm_pool(pool):
    """False | True (= the even-plane 2x2 kernels) | a (k, s) tuple."""
    if pool is True or not pool:
        return bool(pool)
    k, st = int(pool[0]), int(pool[1])
    if not (2 <= k <= 15 and 1 <= st <= k):
        raise L.KanConvError(f"fused max-pool takes 2 <= kernel <= 15 and 1 <= stride <= kernel, got {pool!r}")
    return (k, st)


def kan_conv_in_prelu(spec: ConvSpec, x: torch.Tensor, w_base: Sequence[torch.Tensor], w_basis: Sequence[torch.Tensor],
                      gammas: Optional[Sequence[torch.Tensor]], betas: Optional[Sequence[torch.Tensor]],
                      prelus: Optional[Sequence[torch.Tensor]], eps: float = 1e-5, pool=False, bn: Optional[BatchStats] = None) -> torch.Tensor:
    """`pool=True` additionally applies MaxPool2d(kernel 2, stride 2) inside the same kernels (even output planes only); `pool=(k, s)` a general
    MaxPool2d(k, s) without padding (overlapping windows allowed: the AlexNet pattern (3, 2)).  `bn`: the norm is BatchNorm2d (per-rank batch
    statistics; 2x2 pool on even planes only) -- its statistics span the batch, so the call must fit one launch (`fits_one_launch`)."""
    pool = _norm_pool(pool)
    if bn is not None and not fits_one_launch(spec, x, w_basis):
        raise L.KanConvError("a BatchNorm tail cannot be cut into runs of images: run kan_conv, then batch_norm")
    # opt-in split-precision forward, decided where the caller's grad mode and flags are visible: the inference switch under no_grad only, the forward switch always
    split = _SPLIT.fwd or (_SPLIT.inference and not torch.is_grad_enabled())
    aff = gammas is not None
    extra = (list(gammas) + list(betas) if aff else []) + (list(prelus) if prelus is not None else [])
    return _apply(lambda a, _, *ps: _KanConvInPrelu.apply(spec, float(eps), aff, prelus is not None, pool, split, bn, a, *ps),
                  spec, x, None, w_base, w_basis, extra)


def instance_norm(x: torch.Tensor, gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None, eps: float = 1e-5):
    return _InstanceNorm.apply(x, gamma, beta, float(eps), None)


def batch_norm(x: torch.Tensor, gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None,
               running_mean: Optional[torch.Tensor] = None, running_var: Optional[torch.Tensor] = None, training: bool = True,
               momentum: float = 0.1, eps: float = 1e-5):
    """BatchNorm2d over NCHW with this rank's batch statistics (F.batch_norm's semantics: the running buffers are updated in place when
    training, used when not; without them the batch statistics serve both modes).  Raises ValueError for one value per channel in training."""
    return _InstanceNorm.apply(x, gamma, beta, float(eps), BatchStats(running_mean, running_var, float(momentum), bool(training)))


# --------------------------------------------------------------------------------------- cross-entropy loss and test metrics
class _CrossEntropy(torch.autograd.Function):
    """loss = mean_b (lse[b] - logits[b, target[b]]) on the kernels of csrc/kan_loss.hip (generic_train.py:26's criterion, mean reduction);
    ``metrics``: None or the int64 counter buffer of ``ClassMetrics``, which the same launches add to.  The upstream gradient stays on the device."""

    @staticmethod
    def forward(ctx, logits, target, metrics):
        lib = L.load()
        logits = _require(logits, "logits")
        if torch.cuda.is_current_stream_capturing():
            raise L.KanConvError("cross_entropy is not recorded into a HIP graph (train.GraphedStep): keep torch's criterion inside a recorded step")
        if logits.dim() != 2 or target.shape != logits.shape[:1]:
            raise L.KanConvError(f"cross_entropy takes logits [B, C] and target [B], got {tuple(logits.shape)} and {tuple(target.shape)}")
        if target.device != logits.device or target.dtype != torch.int64:
            raise L.KanConvError(f"target must be int64 on {logits.device}, got {target.dtype} on {target.device}")
        target = target.contiguous()
        B, Cn = logits.shape
        if metrics is not None and (metrics.device != logits.device or metrics.dtype != torch.int64 or not metrics.is_contiguous()
                                    or metrics.numel() * 8 != lib.kan_xent_metrics_bytes(Cn)):
            raise L.KanConvError(f"metrics buffer does not fit {Cn} classes on {logits.device}: build it with ClassMetrics({Cn}, device)")
        loss = torch.empty((), device=logits.device, dtype=torch.float32)
        lse = torch.empty((B,), device=logits.device, dtype=torch.float32)
        ws = torch.empty((max(int(lib.kan_xent_workspace_bytes(B)), 4) // 4,), device=logits.device, dtype=torch.int32)
        L.check(lib.kan_xent_fwd(_ptr(logits), _ptr(target), B, Cn, _ptr(loss), _ptr(lse), _ptr(metrics), _ptr(ws), _stream(logits)), "kan_xent_fwd")
        ctx.save_for_backward(logits, target, lse)
        return loss

    @staticmethod
    @_once
    def backward(ctx, g):
        lib = L.load()
        logits, target, lse = ctx.saved_tensors
        g = _require(g, "grad of the loss").reshape(1)
        dlogits = torch.empty_like(logits)
        L.check(lib.kan_xent_bwd(_ptr(logits), _ptr(target), _ptr(lse), _ptr(g), _ptr(dlogits), logits.shape[0], logits.shape[1], _stream(logits)),
                "kan_xent_bwd")
        return _asked(ctx, (dlogits, None, None))


def cross_entropy(logits: torch.Tensor, target: torch.Tensor, metrics=None) -> torch.Tensor:
    """Mean cross-entropy of fp32 ``logits`` [B, C] against int64 ``target`` [B] (a device scalar).  ``metrics``: a ``ClassMetrics`` (or its
    buffer); every call then adds this batch's loss, predictions (lowest index among the maxima, as torch.max) and per-class counts to it on
    the device -- no host read.  A target outside [0, C) adds nothing, gets a zero gradient row and is reported by ``ClassMetrics.result()``."""
    return _CrossEntropy.apply(logits, target, getattr(metrics, "buffer", metrics))


# --------------------------------------------------------------------------------------- the non-finite probe
def count_nonfinite(t: torch.Tensor, record: torch.Tensor, tick: torch.Tensor) -> None:
    """Add the number of NaN / +inf / -inf elements of fp32 ``t`` to ``record`` -- three int64 on ``t``'s device, [elements, first_tick, last_tick] --
    with one launch of csrc/kan_guard.hip on the current stream; ``tick`` (one int64 on the device, read by the kernel) is what first_tick / last_tick
    are set to when the launch finds something.  No autograd, no host read, nothing returned; usable while the stream is capturing.  A tensor that
    is not contiguous is counted through a dense copy.  What ``AnomalyProbe`` launches per slot (the reference's counterpart: train.py:431)."""
    if not isinstance(t, torch.Tensor):
        raise L.KanConvError(f"count_nonfinite takes a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise L.KanConvError(f"the tensor is on {t.device}: this path runs only on a ROCm device (MI355X); there is no CPU fallback")
    if t.dtype != torch.float32:
        raise L.KanConvError(f"count_nonfinite takes float32, got {t.dtype}")
    for name, b, n in (("record", record, 3), ("tick", tick, 1)):
        if not (isinstance(b, torch.Tensor) and b.dtype == torch.int64 and b.device == t.device and b.numel() == n and b.is_contiguous()):
            raise L.KanConvError(f"count_nonfinite: {name} must be {n} contiguous int64 on {t.device}")
    if t.numel() == 0:                                                     # (an empty tensor has no address to hand over)
        return
    t = t.detach().contiguous()
    L.check(L.load().kan_nonfinite_count(C.c_void_p(t.data_ptr()), t.numel(), C.c_void_p(tick.data_ptr()), C.c_void_p(record.data_ptr()), _stream(t)),
            "kan_nonfinite_count")


# --------------------------------------------------------------------------------------- batches from a device-resident uint8 dataset
def prepare_batch(images: torch.Tensor, table: torch.Tensor, out_hw, mean, std, labels: Optional[torch.Tensor] = None,
                  channels_last: bool = True, out=None):
    """One batch of a uint8 dataset that lives on the device, in one launch of csrc/kan_feed.hip and with no host read: the transforms of
    utils/dataloader.py:56-90 (``RandomCrop(S, padding=p)``, ``RandomHorizontalFlip``, ``ToTensor``, ``Normalize``) and the DataLoader's batching.

    ``images``: uint8 [N, H, W, C] (``channels_last``, CIFAR's layout) or [N, C, H, W] (SVHN's; MNIST's [N, H, W] counts as C = 1 either way);
    ``table``: int32 [B, 4], rows (index, top, left, flip) with top / left in unpadded source coordinates (negative: zero padding of the raw
    bytes, so a padded pixel comes out as (0 - mean) / std); ``out_hw``: (Ho, Wo); ``mean`` / ``std``: C floats; ``labels``: int64 [N] or None.
    Returns (data fp32 [B, C, Ho, Wo], target int64 [B] or None).  ``out=(data, target)`` writes into given tensors (``GraphedStep``'s
    ``step.data`` / ``step.target``) and returns them.  A row whose index is outside [0, N) gets an all-zero image and target -1
    (``ClassMetrics.result()`` reports it).  No autograd: images carry no gradient."""
    lib = L.load()
    if not (isinstance(images, torch.Tensor) and isinstance(table, torch.Tensor)):
        raise L.KanConvError("prepare_batch takes tensors for images and table")
    if images.dtype != torch.uint8 or not images.is_contiguous():
        raise L.KanConvError(f"images must be contiguous uint8, got {images.dtype}{'' if images.is_contiguous() else ', not contiguous'}")
    if images.dim() == 3:
        N, H, W = images.shape
        Cn = 1
    elif images.dim() == 4:
        N, H, W, Cn = images.shape if channels_last else (images.shape[0], images.shape[2], images.shape[3], images.shape[1])
    else:
        raise L.KanConvError(f"images must be [N, H, W, C], [N, C, H, W] or [N, H, W], got {tuple(images.shape)}")
    if min(N, H, W, Cn) < 1:
        raise L.KanConvError(f"images are empty: {tuple(images.shape)}")
    if Cn > 4:
        raise L.KanConvError(f"at most 4 channels, got {Cn} ({'channels_last' if channels_last else 'channels first'} {tuple(images.shape)})")
    limit = int(lib.kan_feed_max_image_bytes())
    if H * W * Cn > limit:
        raise L.KanConvError(f"an image of {H} x {W} x {Cn} = {H * W * Cn} bytes is above the {limit} bytes this kernel stages")
    if table.device != images.device or table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != 4 or table.shape[0] < 1 \
            or not table.is_contiguous():
        raise L.KanConvError(f"table must be contiguous int32 [B, 4] on {images.device}, got {table.dtype} {tuple(table.shape)} on {table.device}")
    B = table.shape[0]
    Ho, Wo = (int(v) for v in out_hw)
    if Ho < 1 or Wo < 1:
        raise L.KanConvError(f"out_hw must be positive, got {(Ho, Wo)}")
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != Cn or len(std) != Cn:
        raise L.KanConvError(f"mean and std must hold {Cn} values, got {len(mean)} and {len(std)}")
    if labels is not None and (labels.device != images.device or labels.dtype != torch.int64 or labels.shape != (N,) or not labels.is_contiguous()):
        raise L.KanConvError(f"labels must be contiguous int64 [{N}] on {images.device}, got {labels.dtype} {tuple(labels.shape)} on {labels.device}")
    if not images.is_cuda:                                   # after the checks that need no device, so those speak on any tensor
        raise L.KanConvError(f"images are on {images.device}: this path runs only on a ROCm device (MI355X); there is no CPU fallback")
    if out is not None:
        data, target = out
        if data.device != images.device or data.dtype != torch.float32 or tuple(data.shape) != (B, Cn, Ho, Wo) or not data.is_contiguous():
            raise L.KanConvError(f"out data must be contiguous float32 {(B, Cn, Ho, Wo)} on {images.device}, got {data.dtype} {tuple(data.shape)}")
        if (target is None) != (labels is None):
            raise L.KanConvError("out target is given exactly when labels are")
        if target is not None and (target.device != images.device or target.dtype != torch.int64 or tuple(target.shape) != (B,)
                                   or not target.is_contiguous()):
            raise L.KanConvError(f"out target must be contiguous int64 {(B,)} on {images.device}, got {target.dtype} {tuple(target.shape)}")
    else:
        data = torch.empty((B, Cn, Ho, Wo), device=images.device, dtype=torch.float32)
        target = torch.empty((B,), device=images.device, dtype=torch.int64) if labels is not None else None
    fl = C.c_float * Cn
    L.check(lib.kan_feed_batch(_ptr(images), _ptr(labels), _ptr(table), N, B, Cn, H, W, Ho, Wo, 1 if channels_last else 0, fl(*mean), fl(*std),
                               _ptr(data), _ptr(target), _stream(images)), "kan_feed_batch")
    return data, target


def prepare_resized_batch(images: torch.Tensor, table: torch.Tensor, resize, out_hw, mean, std, labels: Optional[torch.Tensor] = None,
                          channels_last: bool = True, out_channels: Optional[int] = None, coeffs=None, out=None):
    """``prepare_batch`` for the loader's ImageNet branch (utils/dataloader.py:26-54), in one launch of csrc/kan_feed_resize.hip and with no
    host read: ``Resize`` of the whole image to ``resize`` = (Rh, Rw) (an int follows ``Resize(int)``; None: the image's own size), the crop
    box of each row, ``Resize`` of the box to ``out_hw``, flip, ``Grayscale(3)`` when ``out_channels`` is 3 on one-channel images, ``ToTensor``,
    ``Normalize`` -- with the bytes of PIL's 8-bit bilinear resampling (``data.resample_coeffs``).

    ``table``: int32 [B, 6], rows (index, top, left, h, w, flip), the box in stage-1 (Rh x Rw) coordinates; ``mean`` / ``std``: ``out_channels``
    floats (default: the images' C); ``coeffs``: the ``data.ResizeTables`` of this geometry on the images' device (``data.resize_tables``; built
    and uploaded here when None -- a loop passes its own, as ``ResizedDeviceBatches`` does).  Returns (data fp32 [B, out_channels, Ho, Wo],
    target int64 [B] or None); ``out=(data, target)`` writes into given tensors.  A row whose index is outside [0, N) or whose box is not inside
    the stage-1 image with h, w >= 1 gets an all-zero image and target -1.  No autograd: images carry no gradient."""
    lib = L.load()
    if not (isinstance(images, torch.Tensor) and isinstance(table, torch.Tensor)):
        raise L.KanConvError("prepare_resized_batch takes tensors for images and table")
    if images.dtype != torch.uint8 or not images.is_contiguous():
        raise L.KanConvError(f"images must be contiguous uint8, got {images.dtype}{'' if images.is_contiguous() else ', not contiguous'}")
    if images.dim() == 3:
        N, H, W = images.shape
        Cn = 1
    elif images.dim() == 4:
        N, H, W, Cn = images.shape if channels_last else (images.shape[0], images.shape[2], images.shape[3], images.shape[1])
    else:
        raise L.KanConvError(f"images must be [N, H, W, C], [N, C, H, W] or [N, H, W], got {tuple(images.shape)}")
    if min(N, H, W, Cn) < 1:
        raise L.KanConvError(f"images are empty: {tuple(images.shape)}")
    if Cn > 4:
        raise L.KanConvError(f"at most 4 channels, got {Cn} ({'channels_last' if channels_last else 'channels first'} {tuple(images.shape)})")
    limit = int(lib.kan_feed_max_image_bytes())
    if H * W * Cn > limit:
        raise L.KanConvError(f"an image of {H} x {W} x {Cn} = {H * W * Cn} bytes is above the {limit} bytes this kernel stages")
    if table.device != images.device or table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != 6 or table.shape[0] < 1 \
            or not table.is_contiguous():
        raise L.KanConvError(f"table must be contiguous int32 [B, 6] on {images.device}, got {table.dtype} {tuple(table.shape)} on {table.device}")
    B = table.shape[0]
    from . import data as D                                  # data imports this module
    Rh, Rw = D.resized_hw(H, W, resize)
    Ho, Wo = (int(v) for v in out_hw)
    if Rh < 1 or Rw < 1:
        raise L.KanConvError(f"resize must be positive, got {(Rh, Rw)}")
    if Ho < 1 or Wo < 1:
        raise L.KanConvError(f"out_hw must be positive, got {(Ho, Wo)}")
    OC = Cn if out_channels is None else int(out_channels)
    if OC != Cn and not (OC == 3 and Cn == 1):
        raise L.KanConvError(f"out_channels is the images' {Cn}, or 3 for one-channel images, got {OC}")
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != OC or len(std) != OC:
        raise L.KanConvError(f"mean and std must hold {OC} values, got {len(mean)} and {len(std)}")
    if labels is not None and (labels.device != images.device or labels.dtype != torch.int64 or labels.shape != (N,) or not labels.is_contiguous()):
        raise L.KanConvError(f"labels must be contiguous int64 [{N}] on {images.device}, got {labels.dtype} {tuple(labels.shape)} on {labels.device}")
    if coeffs is not None:
        if not isinstance(coeffs, D.ResizeTables) or coeffs.geometry != (H, W, Rh, Rw, Ho, Wo) or coeffs.device != images.device:
            raise L.KanConvError(f"coeffs must be the data.ResizeTables of {(H, W, Rh, Rw, Ho, Wo)} on {images.device}, got "
                                 f"{getattr(coeffs, 'geometry', type(coeffs).__name__)} on {getattr(coeffs, 'device', None)}")
        kmax = int(lib.kan_feed_resize_max_ksize())
        if max(coeffs.ksize) > kmax:
            raise L.KanConvError(f"a resampling pass of {max(coeffs.ksize)} taps is above the {kmax} this kernel's tiles are sized for")
    if not images.is_cuda:                                   # after the checks that need no device, so those speak on any tensor
        raise L.KanConvError(f"images are on {images.device}: this path runs only on a ROCm device (MI355X); there is no CPU fallback")
    if out is not None:
        data, target = out
        if data.device != images.device or data.dtype != torch.float32 or tuple(data.shape) != (B, OC, Ho, Wo) or not data.is_contiguous():
            raise L.KanConvError(f"out data must be contiguous float32 {(B, OC, Ho, Wo)} on {images.device}, got {data.dtype} {tuple(data.shape)}")
        if (target is None) != (labels is None):
            raise L.KanConvError("out target is given exactly when labels are")
        if target is not None and (target.device != images.device or target.dtype != torch.int64 or tuple(target.shape) != (B,)
                                   or not target.is_contiguous()):
            raise L.KanConvError(f"out target must be contiguous int64 {(B,)} on {images.device}, got {target.dtype} {tuple(target.shape)}")
    else:
        data = torch.empty((B, OC, Ho, Wo), device=images.device, dtype=torch.float32)
        target = torch.empty((B,), device=images.device, dtype=torch.int64) if labels is not None else None
    if coeffs is None:
        coeffs = D.resize_tables(H, W, Rh, Rw, Ho, Wo, device=images.device)
    fl = C.c_float * OC
    (k1x, k1y, k2x, k2y), ks = coeffs.tables, coeffs.ksize
    L.check(lib.kan_feed_resize_batch(_ptr(images), _ptr(labels), _ptr(table), N, B, Cn, H, W, Rh, Rw, Ho, Wo, 1 if channels_last else 0, OC,
                                      _ptr(k1x), ks[0], _ptr(k1y), ks[1], _ptr(k2x), ks[2], _ptr(k2y), ks[3], fl(*mean), fl(*std), _ptr(data),
                                      _ptr(target), _stream(images)), "kan_feed_resize_batch")
    return data, target
